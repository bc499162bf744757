"""The bf16 inference MLP -- k_mlp_pp<W, false> behind pnr_mlp_forward, what every bf16 render and the benchmark's frames run, and
the lock-step k_mlp_fused<PNR_PREC_BF16, W, 1, 8, 2> under desc.schedule = 1 -- layer by layer against float64.  The kernels save no
activations, so they read out their own internals: the probe networks of tests/_mlp_probe_bf16.py (pinned on the CPU by
test_mlp_probe_bf16.py) return every region as the next Linear reads it, bit for bit, and the forward half of the training check
(tests/_mlp_ref.check_forward) runs on them: the identity columns of EX are bf16 of c_oracle.points bit for bit, every band inside
E_j, every X_l, F, G, SH_* inside [RNE(r64 - delta), RNE(r64 + delta)], every raw row inside C_ACC K u m + ulp of float64 on the
kernel's own input region.  The fused plans 1 and 2, k_mlp_pp_sigma and k_mlp_pp_field are tied to this raw bit for bit elsewhere
(test_gpu_stages.py, test_gpu_fused_sweep.py, test_gpu_field_query.py).  SURVEY.md 8a row a5.

Every call goes through the C entry point.  rays, z and raw are interior views of ONE allocation filled with a sentinel, a guard on
both sides (behind raw at least one whole channel row); after each launch the guards are intact and no sentinel is left inside raw.
Every launch is made twice, with the default schedule and with schedule = 1: the two kernels agree bit for bit, raw and every probe
read-out included.

Cases: the 15 geometries of the training sweep plus D = 16 and D = 2 at W = 256, S = 287, every region (G included) and every raw
row; n_sem = every value 1 ... 256 x n_inst 0 / 1 / 33, and n_inst in 13 values up to 256 x n_sem 0 / 1 / 45 / 256 (516 channels),
at both head depths and both widths on a D = 3 trunk at S = 33 (a full tile plus one sample), head_tap = "feature" at two widths per
depth: every chunk count of pp_layer_out's stream through the three LDS slots and every boundary of store_raw_block's
`u < n_out - 4 hi`; the region that feeds the heads is read out once per trunk and tap (and per *.0 Linear at depth 2), every real
launch's rgb and sigma equal that launch's bit for bit, and every logit row is checked against float64 on it.  S = every value
1 ... 257, 383 ... 385, 511 ... 513 and N = 1 ... 257 at R = 3 on the benched 8 x 256 network and on 3 x 128; four raw layouts at a
300-logit network bit for bit; >= 3 grid-stride passes plus a ragged tail against slice launches and a repeat bit for bit; zeroed
rows, large weights, far points, near == far, n_rays = 0; NaN / Inf / d = 0 rays isolated from their neighbours.

Ties at the head-width cases: pnr_mlp_forward_train's raw equals the inference raw bit for bit at all 3312 of them -- the training
FORWARD refuses no head width up to 256 + 256 (only pnr_mlp_backward and pnr_mlp_wgrad refuse heads wider than 64:
test_gpu_mlp_sweep.py::test_backward_refuses_heads_wider_than_64) --, and pnr_mlp_query_supported says yes to every one of them:
pnr_mlp_query's sigma and logits at ops.points equal the raw rows bit for bit at 3292 (the seven (n_sem, n_inst) pairs
test_gpu_field_query.py has are left to it).

Worst error / bound an MI355X gave over this file (PNR_SWEEP_REPORT=<file.json> adds them to that file under "infer bf16: ...").
For bf16 outputs: the worst |r64 - midpoint| / delta among values that were not RNE(r64) ('-': every value was RNE(r64)); for
fp32 outputs the worst |kernel - r64| / bound.  The bounds are derived (tests/_mlp_ref.py header); this table is a record, not an
assertion.

  quantity                         bound                                         MI355X worst / bound
  gamma(x): identity columns of EX bf16 of c_oracle.points, bit for bit          -
  gamma(x): bands of EX            RNE interval of E_j = 8 u, 4 E_j + 2 u ...     0.018
  gamma(d): ED                     the same with the 8 u direction term          - (every value was RNE(r64))
  X_l                              RNE interval of delta = C_ACC K u m           0.12
  F, G, SH_sem, SH_inst            the same                                      0.0026, 0.0012, 0.0024, 0.0017
  raw (rgb, sigma, logits)         C_ACC K u m + ulp                             0.018
  schedule 1 == default, training forward == inference, field query == raw rows, layouts, slices, repeat: bit for bit
The slowest test took 3.9 s (the grid-stride case: 196,725 samples on 256 CUs), the whole file 48 s.
"""
import ctypes
import json
import os

import pytest
import torch

import _mlp_probe_bf16 as pb
import _mlp_ref as mr
from _arena import SENTINEL
from panopticnerf_amd import ops
from test_gpu_mlp_fp32_infer_sweep import Launch
from test_gpu_mlp_sweep import GEOMS, _big_weights, _far_rays, _zero_rows

pytestmark = pytest.mark.gpu

_REPORT = os.environ.get("PNR_SWEEP_REPORT")
_WORST = {}
_TIES = {"training forward": 0, "field query": 0}      # head-width cases compared bit for bit
_IMAGES = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("infer bf16, worst error / bound:", {k: "%.3g" % v for k, v in sorted(_WORST.items())}, _TIES)
    if _REPORT:
        out = {}
        if os.path.exists(_REPORT):
            with open(_REPORT) as f:
                out = json.load(f)
        out.update({"infer bf16: " + k: _WORST[k] for k in sorted(_WORST)})
        out.update({"infer bf16: " + k: v for k, v in _TIES.items()})
        with open(_REPORT, "w") as f:
            json.dump(out, f, indent=1)


@pytest.fixture(autouse=True)
def _after_each_test():
    yield
    _IMAGES.clear()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:           # a device error fails every later launch too: stop here
        pytest.exit("the GPU reported an error, nothing more is launched: %s" % e, returncode=3)


def _with(desc, **fields):
    d = ops.MlpDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc), ctypes.sizeof(d))
    for k, v in fields.items():
        setattr(d, k, v)
    return d


class Launch16(Launch):
    """Launch with the descriptor's schedule set, and the packed images cached per (descriptor, parameter tensors): the schedules,
    the ties and repeated inputs share one image.  The cache keeps the tensors alive, so an id names one tensor."""

    def __init__(self, dev, layout="channel", pad=24, schedule=0):
        super().__init__(dev, layout, pad)
        self.schedule = schedule

    def image(self, desc, params):
        key = (bytes(_with(desc, schedule=0)), tuple((k, id(params[k]), params[k]._version) for k in sorted(params)))
        if key not in _IMAGES:
            img = ops.pack_mlp(desc, params)
            if desc.plan == 0:
                pb.assert_pp_takes(img, pb.geom_of(desc))
            _IMAGES[key] = (img.to(self.dev), list(params.values()))
        return _IMAGES[key][0]

    def __call__(self, desc, params, rays, z, n_rays=None):
        return super().__call__(_with(desc, schedule=self.schedule), params, rays, z, n_rays)


class Both:
    """every launch with the default schedule (k_mlp_pp) and with schedule = 1 (k_mlp_fused<bf16>): bit for bit the same raw"""

    def __init__(self, dev, layout="channel", pad=24):
        self.pp, self.ls = Launch16(dev, layout, pad, 0), Launch16(dev, layout, pad, 1)

    def __call__(self, desc, params, rays, z, n_rays=None):
        a, b = self.pp(desc, params, rays, z, n_rays), self.ls(desc, params, rays, z, n_rays)
        if not torch.equal(a, b):
            self.pp.bad.append("launch %d: schedule 1 differs from the default in %d elements" % (self.pp.calls, int((a != b).sum())))
        return a

    @property
    def bad(self):
        return self.pp.bad + self.ls.bad

    @property
    def calls(self):
        return self.pp.calls + self.ls.calls


def _note(rep):
    for k, v in rep.worst.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)


def check(dev, case, launch=None, real=None):
    """the whole case: every region read out, every region and every raw row checked"""
    launch = Both(dev) if launch is None else launch
    rep = mr.Report()
    X, real = pb.check(rep, launch, case["desc"], case["params"], case["rays"], case["z"], real=real)
    _note(rep)
    print({k: "%.3g" % v for k, v in rep.worst.items()}, "%d launches" % launch.calls)
    assert not launch.bad, launch.bad[:8]
    rep.check()
    return X, real


# --------------------------------------------------------------------------------------------------------- geometries
MORE = [(16, 256, 7, 5, 3, "trunk", 2, 10, 4), (2, 256, 0, 5, 3, "feature", 1, 10, 4)]


@pytest.mark.parametrize("geom", GEOMS + MORE, ids=lambda g: pb.GEOM_ID % g)
def test_every_geometry_at_287_samples(dev, geom):
    case = pb.make_case(geom, 7, 41, seed=(GEOMS + MORE).index(geom))
    X, _ = check(dev, case)
    want = {"EX", "ED", "F", "G"} | {"X%d" % (l + 1) for l in range(geom[0])}
    if geom[6] == 2:
        want |= ({"SH_sem"} if geom[3] else set()) | ({"SH_inst"} if geom[4] else set())
    assert set(X) == want


# -------------------------------------------------------------------------------------------------------- head widths
HEAD_R, HEAD_N = 3, 11                          # S = 33: one full 32-sample tile plus one sample
FIELD_QUERY_HAS = {(0, 0), (45, 32), (45, 0), (0, 32), (19, 8), (96, 0), (33, 33)}       # test_gpu_field_query.py's HEADS
FEATURE_TOO = (37, 200)                         # the two widths per depth that also run with head_tap = "feature"


def _trunk3(W, C, K, tap, depth):
    return (3, W, 1, C, K, tap, depth, 10, 4)


def _is_head(name):
    return name.startswith(("semantic_linears", "instance_linears"))


class HeadSweep:
    """one D = 3 trunk of width W (the parameters of seed 3 in front of the heads): the region the heads read is read out once per
    tap, SH_* once per *.0 Linear; every case's rgb / sigma must be those launches', and its logits are checked on them"""

    def __init__(self, dev, W):
        self.dev, self.W, self.launch, self.tapx, self.sh = dev, W, Both(dev), {}, {}
        base = pb.make_case(_trunk3(W, 0, 0, "trunk", 1), HEAD_R, HEAD_N, seed=3)
        self.trunk, self.rays, self.z = base["params"], base["rays"], base["z"]
        self.rays_d, self.z_d = self.rays.to(dev), self.z.to(dev)
        self.pts_d = ops.points(self.rays_d, self.z_d).reshape(-1, 3).contiguous()

    def tap_region(self, case):
        tap = case["geom"][5]
        if tap not in self.tapx:
            X, rgbs = pb.read_out(self.launch, case["desc"], case["params"], self.rays, self.z, need={"F" if tap == "feature" else "X3"})
            self.tapx[tap] = (X, rgbs)
        return self.tapx[tap]

    def hidden_regions(self, case):
        """SH_* of the case's own *.0 Linears (depth 2), read out once per distinct Linear"""
        p, X, need = case["params"], {}, {}
        for nm, _, _, sh in pb.m32.heads(case["desc"]):
            key = (case["geom"][5], nm, p[nm + ".0.weight"].numpy().tobytes(), p[nm + ".0.bias"].numpy().tobytes())
            if key in self.sh:
                X[sh] = self.sh[key]
            else:
                need[sh] = key
        if need:
            got, rgbs = pb.read_out(self.launch, case["desc"], p, self.rays, self.z, need=set(need))
            assert torch.equal(rgbs, self.tap_region(case)[1])
            for sh, key in need.items():
                X[sh] = self.sh[key] = got[sh]
        return X

    def run(self, C, K, tap, depth):
        geom = _trunk3(self.W, C, K, tap, depth)
        case = pb.make_case(geom, HEAD_R, HEAD_N, seed=3)
        desc, params = case["desc"], case["params"]
        assert all(torch.equal(v, params[k]) for k, v in self.trunk.items()) and torch.equal(case["z"], self.z)
        pb.assert_normal(desc, params, self.rays, self.z)
        real = self.launch(desc, params, self.rays, self.z)
        Xt, rgbs = self.tap_region(case)
        assert torch.equal(real[:, :4], rgbs), ("rgb / sigma differ from the read-out launch's", C, K, tap, depth)
        X = dict(Xt)
        if depth == 2:
            X.update(self.hidden_regions(case))
        rep = mr.Report()
        pb.check_regions(rep, desc, params, self.rays, self.z, X, real, regions=[k for k in X if k.startswith("SH_")],
                         parts=[k[:-7] for k in params if _is_head(k) and k.endswith(".weight")])
        _note(rep)
        assert not self.launch.bad, (self.launch.bad[:8], C, K, tap, depth)
        assert not rep.fails, (C, K, tap, depth, rep.fails[:8])
        self.ties(case, real)

    def ties(self, case, real):
        """the training forward takes every head width (a refusal is an error here); so does the field query"""
        desc, params = case["desc"], case["params"]
        raw_t, _ = ops.mlp_forward_train(desc, self.launch.pp.image(desc, params), self.rays_d, self.z_d)
        _TIES["training forward"] += 1
        assert torch.equal(raw_t.t(), real), ("the training forward's raw differs from the inference raw", case["geom"])
        C, K = desc.n_sem, desc.n_inst
        if (C, K) in FIELD_QUERY_HAS:
            return
        assert ops.field_query_supported(desc), case["geom"]
        _TIES["field query"] += 1
        d4 = _with(desc, plan=4)
        out = ops.mlp_query(d4, self.launch.pp.image(d4, params), self.pts_d, want=("sigma", "logits"))
        assert torch.equal(out["sigma"], real[:, 3]), ("pnr_mlp_query's sigma differs from the raw row", case["geom"])
        if C:
            assert torch.equal(out["sem_logits"].t(), real[:, 4:4 + C]), ("pnr_mlp_query's semantic logits", case["geom"])
        if K:
            assert torch.equal(out["inst_logits"].t(), real[:, 4 + C:4 + C + K]), ("pnr_mlp_query's instance logits", case["geom"])


@pytest.mark.parametrize("W", [128, 256])
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("n_inst", [0, 1, 33])
@pytest.mark.parametrize("n_sem_from", [1, 129])
def test_every_semantic_width(dev, n_sem_from, n_inst, depth, W):
    """n_sem = 1 ... 256 (two halves): one to eight 32-row chunks of the semantic head through the three weight slots, the stream
    wrapping back to chunk 0 at every position, every `u < n_out - 4 hi`, with no instance head, one row, or a block and a row behind"""
    sweep = HeadSweep(dev, W)
    for n_sem in range(n_sem_from, n_sem_from + 128):
        for tap in ("trunk", "feature") if n_sem in FEATURE_TOO else ("trunk",):
            sweep.run(n_sem, n_inst, tap, depth)


N_INST = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 255, 256]


@pytest.mark.parametrize("W", [128, 256])
@pytest.mark.parametrize("depth", [1, 2])
def test_instance_widths_behind_four_semantic_widths(dev, depth, W):
    """the instance head's rows behind no semantic head, one row, 45 rows and 256 (256 + 256: 516 channels)"""
    sweep = HeadSweep(dev, W)
    for n_sem in (0, 1, 45, 256):
        for n_inst in N_INST:
            for tap in ("trunk", "feature") if n_inst in (33, 256) and n_sem == 45 else ("trunk",):
                sweep.run(n_sem, n_inst, tap, depth)


# -------------------------------------------------------------------------------------------------------------- sizes
BIG = (8, 256, 4, 45, 32, "trunk", 2, 10, 4)
SMALL = (3, 128, 1, 5, 3, "feature", 1, 10, 4)
S_LIST = list(range(1, 258)) + [383, 384, 385, 511, 512, 513]
COUNTS = {"S_low": [(1, S) for S in S_LIST[:130]], "S_high": [(1, S) for S in S_LIST[130:]],
          "N_low": [(3, N) for N in range(1, 130)], "N_high": [(3, N) for N in range(130, 258)]}


@pytest.mark.parametrize("which", sorted(COUNTS))
@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["8x256", "3x128"])
def test_every_sample_count(dev, geom, which):
    """S across the 32-sample tile, one and two 256-sample groups and a second wave group without a valid sample; N across the magic
    division by N (N = 1 included).  sigma and the logits on the kernel's own tap region (and SH_* at depth 2) at every count"""
    first = pb.make_case(geom, 1, 1, seed=5)
    desc, params = first["desc"], first["params"]
    tap = "F" if geom[5] == "feature" else "X%d" % geom[0]
    need = {tap, "X%d" % geom[0]} | ({"SH_sem", "SH_inst"} if geom[6] == 2 else set())
    plist = pb.probes(desc, params, need)
    launch, net = Both(dev), mr.Net(desc, params, dev)
    for R, N in COUNTS[which]:
        c = pb.make_case(geom, R, N, seed=5, params=params)
        pb.assert_normal(desc, params, c["rays"], c["z"])
        real = launch(desc, params, c["rays"], c["z"])
        X, _ = pb.read_out(launch, desc, params, c["rays"], c["z"], real=real, probe_list=plist)
        rep = mr.Report()
        pb.check_regions(rep, desc, params, c["rays"], c["z"], X, real, regions=[k for k in X if k.startswith("SH_")],
                         parts=[nm for nm, _, _, _ in net.raw_parts() if nm != "rgb_linear"], net=net)
        _note(rep)
        assert not launch.bad, (launch.bad[:8], R, N)
        assert not rep.fails, (R, N, rep.fails[:8])


@pytest.mark.parametrize("S", [1, 31, 33, 255, 257, 513])
@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["8x256", "3x128"])
def test_every_region_at_six_sample_counts(dev, geom, S):
    check(dev, pb.make_case(geom, 1, S, seed=6))


# ------------------------------------------------------------------------------------------------------------ layouts
WIDE300 = (3, 128, 1, 200, 100, "trunk", 1, 10, 4)


def test_four_raw_layouts_are_bit_identical(dev):
    """channel-major dense, with the default pad (ops.RAW_PAD), with a pad of 6 floats (channel rows not 16-byte aligned), and
    sample-major, at 300 logits; the sample-major launcher then reads every region out"""
    case = pb.make_case(WIDE300, 7, 41, seed=7)
    ls = [Both(dev, "channel", 0), Both(dev, "channel", ops.RAW_PAD), Both(dev, "channel", 6), Both(dev, "sample")]
    raws = [l(case["desc"], case["params"], case["rays"], case["z"]) for l in ls]
    assert not sum((l.bad for l in ls), [])
    assert all(torch.equal(raws[0], r) for r in raws[1:])
    check(dev, case, launch=ls[3], real=raws[3])


# -------------------------------------------------------------------------------------------------------- grid stride
def test_three_grid_stride_passes_equal_slice_launches(dev):
    """launch_pp's grid is min(groups, CUs) workgroups of 256 samples: S >= 3 x 256 x CUs + 77 gives every workgroup three full
    passes and some a ragged fourth, the weight stream wrapping each time.  The big launch equals launches over three ray slices and a
    repeat of itself bit for bit, the lock-step kernel agrees, and sigma and the 103 logits of every sample are checked on X_3"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    N = 61
    R = -(-(3 * 256 * cus + 77) // N)
    case = pb.make_case((3, 128, 1, 70, 33, "trunk", 1, 10, 4), R, N, seed=8)
    assert case["S"] >= 3 * 256 * cus + 77
    desc, params, rays, z = case["desc"], case["params"], case["rays"], case["z"]
    pb.assert_normal(desc, params, rays, z)
    both = Both(dev)
    launch = both.pp
    big = both(desc, params, rays, z)
    again = launch(desc, params, rays, z)
    assert not both.bad and torch.equal(big, again)
    for r0, r1 in ((0, R // 3), (R // 3, 2 * R // 3 + 1), (2 * R // 3 + 1, R)):
        part = launch(desc, params, rays[r0:r1], z[r0:r1])
        assert torch.equal(part, big[r0 * N:r1 * N]), (r0, r1)
    X, _ = pb.read_out(launch, desc, params, rays, z, need={"X3"}, real=big)
    assert not both.bad, both.bad[:8]
    net, rep, step = mr.Net(desc, params, dev), mr.Report(), 1 << 15
    for s0 in range(0, case["S"], step):
        mr.check_forward(rep, net, {"X3": X["X3"][s0:s0 + step].double()}, big[s0:s0 + step], regions=[],
                         parts=["alpha_linear", "semantic_linears.0", "instance_linears.0"])
    _note(rep)
    rep.check()


# -------------------------------------------------------------------------------------------------------- edge inputs
def _edge_case(edge):
    kw = {"zero_rows": dict(params_fn=_zero_rows), "big_weights": dict(params_fn=_big_weights), "far_points": dict(rays_z=_far_rays()),
          "near_equals_far": dict(near=2.0, far=2.0)}[edge]
    return pb.make_case(BIG, 7, 41, seed=5, **kw)


@pytest.mark.parametrize("edge", ["zero_rows", "big_weights", "far_points", "near_equals_far"])
def test_edge_inputs(dev, edge):
    """the training sweep's edge inputs: zeroed rows and tiny negative pre-activations, trunk weights x 6.5 (activations ~1e4), points
    up to 200 m with p = 0 and axis-aligned directions; and every sample of a ray at one depth"""
    case = _edge_case(edge)
    X, _ = check(dev, case)
    if edge == "zero_rows":
        assert (X["X3"][:, 0:8] == 0).all() and (X["X4"][:, 9:12] == 0).all() and (X["SH_sem"][:, 1] == 0).all()
    if edge == "big_weights":
        assert X["X8"].abs().max() > 3e3
    if edge == "far_points":
        assert X["EX"][:, :3].abs().max() > 100 and (X["EX"][:24 * 3:24, :3] == 0).all()
    if edge == "near_equals_far":
        assert (case["z"] == 2.0).all()


@pytest.mark.parametrize("schedule", [0, 1])
def test_zero_rays_writes_nothing(dev, schedule):
    case = pb.make_case(BIG, 7, 41, seed=7)
    launch = Launch16(dev, schedule=schedule)
    launch(case["desc"], case["params"], case["rays"], case["z"], n_rays=0)
    assert not launch.bad
    ar = launch.arena
    assert bool((ar.view("raw") == SENTINEL).all()) and ar.guards_intact()


# ---------------------------------------------------------------------------------------------------------- isolation
@pytest.mark.parametrize("schedule", [0, 1])
def test_non_finite_rays_do_not_touch_their_neighbours(dev, schedule):
    """rays with a NaN origin, an Inf origin and d = 0 in the middle of a 32-sample tile and at its ends (N = 1: ray = sample; N = 3:
    a bad ray straddles a tile boundary): every other ray's rows are the bits of the launch without them.  (The bad rays' own rows
    are not asserted.)"""
    for N, bad in ((1, (0, 15, 31, 32, 63, 64, 95)), (3, (10, 21, 31))):
        case = pb.make_case((3, 128, 1, 5, 3, "trunk", 2, 10, 4), 96 // N, N, seed=16)
        desc, params, rays, z = case["desc"], case["params"], case["rays"], case["z"]
        launch = Launch16(dev, schedule=schedule)
        clean = launch(desc, params, rays, z)
        dirty_rays = rays.clone()
        for i, r in enumerate(bad):
            if i % 3 == 0:
                dirty_rays[r, 0] = float("nan")
            elif i % 3 == 1:
                dirty_rays[r, 1] = float("inf")
            else:
                dirty_rays[r, 3:6] = 0.0
        dirty = launch(desc, params, dirty_rays, z)
        assert not launch.bad, launch.bad
        keep = torch.ones(case["R"], dtype=torch.bool)
        keep[list(bad)] = False
        keep = keep.repeat_interleave(N).to(dev)
        assert torch.isfinite(clean).all() and torch.equal(dirty[keep], clean[keep])
