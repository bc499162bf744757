"""The fp32 inference MLP (k_mlp_fused<PNR_PREC_FP32, W, 1, 4, 1> behind pnr_mlp_forward: what every fp32 render runs) layer by
layer against float64.  The kernel saves no activations, so it reads out its own internals: the probe networks of
tests/_mlp_probe.py (pinned on the CPU by test_mlp_probe.py) return every region of the acts layout bit for bit, and the
layer-local check of tests/_mlp32_ref.py runs on them: identity columns of gamma(x) bit for bit, every band against float64 sin /
cos of the kernel's own argument, every X, F, SH and raw row inside C_ACC (K + 2) u m + ulp of float64 on the kernel's own input
region.  G is read out at every geometry: the two-step rgb bound of _mlp_probe.py, which needs no G, is 1.3 ... 4.5 x the old
bar 1e-4 max(1, |rgb|) at some of them (test_mlp_probe.py), so it is kept only where sizes and edge inputs vary.  SURVEY.md 8a
row a5.

Every call goes through the C entry point.  rays, z and raw are interior views of ONE allocation filled with a sentinel, a guard
on both sides (behind raw at least one whole channel row: "the channel behind the last"); after each launch the guards are
intact and no sentinel is left inside the output.

Cases: the 14 geometries of the fp32 training sweep plus D = 16 and D = 2 at W = 256, S = 287; n_sem 1 ... 256 x n_inst 0 / 1 /
33 at both head depths and both widths (every boundary of store_raw_block's `u < n_out - 4 hi` and of the 32-row block loop);
S = 1 ... 257 and N = 1 ... 257 at an 8 x 256 and a 3 x 128 network; three raw layouts bit for bit; >= 3 trips of the persistent
loop against slice launches bit for bit; far points, a dead layer, weights x 64, near == far, n_rays = 0; NaN / Inf / d = 0 rays
isolated from their neighbours.

The fmaf chain: with EX, X_1 and X_2 read out exactly, pts_linears.0 and a hidden layer restated in numpy float32 in the kernel's
order (the bias first, then per lane-vector slot v the k-slots (hi = 0, v), (hi = 1, v) of pnr_mlp_layout.h, one fused
multiply-add each: _mlp_probe.layer32).  An MI355X gave 0 of 36,736 differing elements of X_1 and 0 of 36,736 of X_2 (on the
CPU the ascending-k chain of _mlp32_ref.forward32 differs from this restatement in 14,286 and 15,290 elements: the count tells
the orders apart): test_the_fmaf_chain asserts equality, which pins the sentence "bit-for-bit an fmaf chain" in pnr_mlp.hip's
header together with the order.

Worst error / bound an MI355X gave over this file (PNR_SWEEP_REPORT=<file.json> adds them to that file under "infer: ...").  The
bounds are derived, not measured, except the trig row: this kernel calls libm's sincosf, whose error nothing in the project fixes.
Its worst |kernel - float64| over this file, far points included, is 6.88e-8 (1.15 u), below _mlp32_ref.TRIG_MEASURED = 6.96e-8
of k_f32_inputs: _mlp32_ref.TRIG_BOUND is kept.

  quantity                         bound                                         MI355X worst / bound
  gamma: identity columns of EX    bit for bit                                   -
  gamma: identity columns of ED    8 u relative                                  0.26
  gamma: sin / cos bands           TRIG_BOUND = 2.78e-7 (_mlp32_ref)              0.25 (worst |kernel - float64| 6.88e-8 = 1.15 u)
  X, F, G, SH, raw                 C_ACC (K + 2) u m + ulp                       0.20 (X; raw 0.043, F 0.021, SH 0.017, G 0.015)
  rgb without G (two-step)         |W_rgb| E_G + f32_bound(...)                  0.0008
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _mlp32_ref as m32
import _mlp_probe as mp
from _arena import GUARD, SENTINEL, Arena
from oracle import c_oracle as co
from oracle import torch_oracle as to
from panopticnerf_amd import _lib, ops
from test_gpu_mlp_fp32_sweep import GEOMS, _ID, _rays

pytestmark = pytest.mark.gpu

TRIG_BOUND = m32.TRIG_BOUND     # the measured worst of this file is below TRIG_MEASURED (module docstring)

_REPORT = os.environ.get("PNR_SWEEP_REPORT")
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _REPORT:
        out = {}
        if os.path.exists(_REPORT):
            with open(_REPORT) as f:
                out = json.load(f)
        out.update({"infer: " + k: _WORST[k] for k in sorted(_WORST)})
        out["infer: trig_bound"] = TRIG_BOUND
        with open(_REPORT, "w") as f:
            json.dump(out, f, indent=1)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class Launch:
    """launch(desc, params, rays, z) -> raw (S, ch) through pnr_mlp_forward on guarded buffers.  layout: 'channel' (channel-major,
    channel stride S + pad) or 'sample' (raw_stride_s = channels, raw_stride_c = 1)"""

    def __init__(self, dev, layout="channel", pad=24):
        self.dev, self.layout, self.pad, self.bad, self.calls, self.arena = dev, layout, pad, [], 0, None

    def image(self, desc, params):
        """the packed image on the device (a subclass may cache it)"""
        return ops.pack_mlp(desc, params).to(self.dev)

    def __call__(self, desc, params, rays, z, n_rays=None):
        lib = _lib.load()
        R, N = z.shape
        S, ch = R * N, 4 + desc.n_sem + desc.n_inst
        if self.layout == "channel":
            ss, sc = 1, S + self.pad
            n_raw, g_raw = ch * sc, max(GUARD, sc)
        else:
            ss, sc = ch, 1
            n_raw, g_raw = S * ch, max(GUARD, ch)
        self.arena = ar = Arena(self.dev, [("rays", 8 * R, GUARD), ("z", S, GUARD), ("raw", n_raw, g_raw)])
        ar.view("rays").copy_(rays.reshape(-1).to(self.dev))
        ar.view("z").copy_(z.reshape(-1).to(self.dev))
        img = self.image(desc, params)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.pnr_mlp_forward(ctypes.byref(desc), _p(img), _p(ar.view("rays")), _p(ar.view("z")), R if n_rays is None else n_rays, N,
                                       _p(ar.view("raw")), ss, sc, stream), "pnr_mlp_forward")
        torch.cuda.synchronize()
        self.calls += 1
        raw = ar.view("raw").as_strided((S, ch), (ss, sc))
        if not ar.guards_intact():
            self.bad.append("launch %d: a guard was written" % self.calls)
        if (R if n_rays is None else n_rays) and (raw == SENTINEL).any():
            self.bad.append("launch %d: %d elements of raw never written" % (self.calls, int((raw == SENTINEL).sum())))
        return raw


def make_case(geom, R, N, seed=0, near=0.5, far=8.0):
    """geom = (D, W, skip, xyz_L, dir_L, n_sem, n_inst, head_tap, head_depth)"""
    D, W, skip, Lx, Ld, C, K, tap, depth = geom
    cfg = to.mlp_config(D=D, W=W, skips=(skip,) if skip >= 0 else (), xyz_L=Lx, dir_L=Ld, n_sem=C, n_inst=K, head_W=W // 2,
                        head_tap=tap, head_depth=depth)
    rng = np.random.default_rng(seed + 11)
    rays = _rays(rng, R, near=near, far=far)
    z = co.stratified(rays, N, t_rand=rng.random((R, N)).astype(np.float32))
    return dict(desc=ops.make_desc(D, W, skip, Lx, Ld, C, K, W // 2, "fp32", tap, depth), params=to.init_params(cfg, seed=seed),
                rays=torch.from_numpy(rays), z=torch.from_numpy(z), S=R * N, R=R, N=N)


def check(dev, case, launch=None, **kw):
    launch = Launch(dev) if launch is None else launch
    rep = m32.Report()
    X, real = mp.check(rep, launch, case["desc"], case["params"], case["rays"], case["z"], trig_bound=TRIG_BOUND, **kw)
    for k, v in rep.worst.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    print({k: "%.3g" % v for k, v in rep.worst.items()}, "%d launches" % launch.calls)
    assert not launch.bad, launch.bad[:8]
    rep.check()
    return X, real


# --------------------------------------------------------------------------------------------------------- geometries
MORE = [(16, 256, 7, 10, 4, 5, 3, "trunk", 2), (2, 256, 0, 10, 4, 5, 3, "feature", 1)]


@pytest.mark.parametrize("geom", GEOMS + MORE, ids=_ID)
def test_every_geometry_at_287_samples(dev, geom):
    case = make_case(geom, 7, 41, seed=(GEOMS + MORE).index(geom))
    check(dev, case, full_G=True)


# -------------------------------------------------------------------------------------------------------- head widths
N_SEM = [1, 3, 4, 5, 28, 31, 32, 33, 36, 63, 64, 65, 127, 128, 129, 255, 256]


@pytest.mark.parametrize("W", [128, 256])
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("n_sem", N_SEM)
def test_head_widths_around_every_block_boundary(dev, n_sem, depth, W):
    """store_raw_block stores row u of a 32-row block iff u < n_out - 4 hi: every n_sem with n_inst 0 / 1 / 33 behind it (a row stored
    one block or one channel off lands in the other head, in the guard behind the last channel, or leaves a sentinel)"""
    for n_inst in (0, 1, 33):
        case = make_case((3, W, 1, 10, 4, n_sem, n_inst, "trunk" if n_sem & 1 else "feature", depth), 3, 23, seed=n_sem)
        only = {nm + sfx for nm, _, _, _ in m32.heads(case["desc"]) for sfx in ((".0", ".1") if depth == 2 else (".0",))}
        check(dev, case, only=only)


# -------------------------------------------------------------------------------------------------------------- sizes
BIG = (8, 256, 4, 10, 4, 45, 32, "trunk", 2)
SMALL = (3, 128, 1, 10, 4, 5, 3, "feature", 1)
COUNTS = [(S, 1) for S in (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)] + [(R, N) for N in (7, 37, 64, 192, 257) for R in (1, 3)]


@pytest.mark.parametrize("RN", COUNTS, ids=lambda rn: "R%d_N%d" % rn)
@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["8x256", "3x128"])
def test_sample_counts_around_the_tile_and_the_group(dev, geom, RN):
    """S across the 32-sample tile and the 128-sample group; N across the magic division by N (N = 1 included)"""
    check(dev, make_case(geom, *RN, seed=5))


# ------------------------------------------------------------------------------------------------------------ layouts
def test_three_raw_layouts_are_bit_identical(dev):
    """channel-major with a 16-byte aligned padded stride (S + 25 = 312), with a stride that is not (S + 24 = 311), sample-major"""
    case = make_case(BIG, 7, 41, seed=7)
    la, lb, lc = Launch(dev, "channel", 25), Launch(dev, "channel", 24), Launch(dev, "sample")
    a, b, c = (l(case["desc"], case["params"], case["rays"], case["z"]) for l in (la, lb, lc))
    assert not la.bad + lb.bad + lc.bad
    assert torch.equal(a, b) and torch.equal(a, c)
    check(dev, case, launch=lc)


# ---------------------------------------------------------------------------------------------------- persistent loop
def test_three_trips_of_the_persistent_loop_equal_slice_launches(dev):
    """launch_mlp caps the grid at CU count x 4 workgroups of 128 samples: S >= 3 x that + 77 makes every workgroup take at least
    three trips whatever the occupancy, the weight stream wrapping each time.  The big launch equals slice launches of <= 4096
    samples and a repeat of itself bit for bit; one slice of the middle is checked layer by layer."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    N = 61
    R = -(-(3 * cus * 4 * 128 + 77) // N)
    case = make_case((8, 256, 4, 10, 4, 3, 2, "trunk", 2), R, N, seed=8)
    assert case["S"] >= 3 * cus * 4 * 128 + 77
    desc, params, rays, z = case["desc"], case["params"], case["rays"], case["z"]
    launch = Launch(dev)
    big = launch(desc, params, rays, z)
    again = launch(desc, params, rays, z)
    assert not launch.bad and torch.equal(big, again)
    step = 4096 // N
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        part = launch(desc, params, rays[r0:r1], z[r0:r1])
        assert torch.equal(part, big[r0 * N:r1 * N]), (r0, r1)
    assert not launch.bad, launch.bad[:8]
    r0 = (R // 2) // step * step                     # a slice whose samples a second or third trip evaluated in the big launch
    sl = dict(case, rays=rays[r0:r0 + 5], z=z[r0:r0 + 5], R=5, S=5 * N)
    check(dev, sl, real=big[r0 * N:(r0 + 5) * N].clone())


# -------------------------------------------------------------------------------------------------------- edge inputs
EDGE = (3, 128, 1, 10, 4, 5, 3, "trunk", 2)


def test_far_points_at_band_9(dev):
    """|p| up to ~1e3: arguments of the top band reach 2^9 x 1e3 (libm's sincosf reduces them: the trig row includes this case)"""
    case = make_case(EDGE, 7, 41, seed=13, far=1e3)
    X, _ = check(dev, case)
    assert X["EX"][:, :3].abs().max() > 500


def test_far_points_with_unused_bands(dev):
    """|p| ~ 1e6 at xyz_L = 4: the kernel still runs sincosf for bands 4 ... 9 (arguments up to 5e8) against zero weights"""
    case = make_case((3, 128, 1, 4, 4, 5, 3, "feature", 2), 7, 41, seed=14, far=1e6)
    X, _ = check(dev, case)
    assert X["EX"][:, :3].abs().max() > 5e5


def test_a_dead_layer(dev):
    """pts_linears.1's bias at -1e4: X_2 = 0 everywhere and everything behind it is its bias chain"""
    case = make_case((3, 128, -1, 10, 4, 5, 3, "trunk", 2), 7, 41, seed=11)
    case["params"]["pts_linears.1.bias"].fill_(-1e4)
    X, _ = check(dev, case)
    assert not X["X2"].any()


def test_weights_times_64(dev):
    """every weight matrix x 64 (activations grow to 64^5): the bounds scale with m"""
    case = make_case((3, 128, 1, 10, 4, 5, 3, "feature", 2), 7, 41, seed=12)
    for k, v in case["params"].items():
        if k.endswith(".weight"):
            v.mul_(64.0)
    check(dev, case)


def test_near_equals_far(dev):
    case = make_case(EDGE, 7, 41, seed=15, near=2.0, far=2.0)
    assert (case["z"] == 2.0).all()
    check(dev, case)


def test_zero_rays_writes_nothing(dev):
    case = make_case(EDGE, 7, 41, seed=7)
    launch = Launch(dev)
    launch(case["desc"], case["params"], case["rays"], case["z"], n_rays=0)
    assert not launch.bad
    ar = launch.arena
    assert bool((ar.view("raw") == SENTINEL).all()) and ar.guards_intact()


# ---------------------------------------------------------------------------------------------------------- isolation
def test_non_finite_rays_do_not_touch_their_neighbours(dev):
    """rays with a NaN origin, an Inf origin and d = 0 in the middle of a 32-sample tile and at its ends (N = 1: ray = sample; N = 3:
    a bad ray straddles a tile boundary): every other ray's rows are the bits of the launch without them.  (The bad rays' own rows
    are not asserted: the kernel's ReLU is fmaxf, which turns a NaN pre-activation into 0, so they come out finite.)"""
    for N, bad in ((1, (0, 15, 31, 32, 63, 64, 95)), (3, (10, 21, 31))):
        case = make_case((3, 128, 1, 10, 4, 5, 3, "trunk", 2), 96 // N, N, seed=16)
        desc, params, rays, z = case["desc"], case["params"], case["rays"], case["z"]
        launch = Launch(dev)
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


# -------------------------------------------------------------------------------------------------------- fmaf chain
def test_the_fmaf_chain(dev):
    """pnr_mlp.hip's header: the fp32 path is "bit-for-bit an fmaf chain".  pts_linears.0 from the kernel's EX and pts_linears.1 from
    its X_1, restated as fmaf chains in the kernel's order (_mlp_probe.layer32), against the kernel's X_1 and X_2."""
    case = make_case((3, 128, -1, 10, 4, 0, 0, "trunk", 2), 7, 41, seed=17)
    desc, params = case["desc"], case["params"]
    launch = Launch(dev)
    X = mp.read_out(launch, mp.probes(desc, params, need={"EX", "X1", "X2"}), case["rays"], case["z"])
    assert not launch.bad
    X = {k: v.cpu().numpy() for k, v in X.items()}
    p = {k: v.numpy() for k, v in params.items()}
    x1 = mp.layer32([(X["EX"], mp.kernel_order("gx", 10))], p["pts_linears.0.weight"], p["pts_linears.0.bias"])
    x2 = mp.layer32([(X["X1"], mp.kernel_order("feat", width=128))], p["pts_linears.1.weight"], p["pts_linears.1.bias"])
    d1, d2 = int((x1 != X["X1"]).sum()), int((x2 != X["X2"]).sum())
    print("fmaf chain: %d of %d elements of X_1 differ, %d of %d of X_2" % (d1, x1.size, d2, x2.size))
    _WORST["fmaf chain: differing elements of X_1"], _WORST["fmaf chain: differing elements of X_2"] = d1, d2
    assert d1 == 0 and d2 == 0
