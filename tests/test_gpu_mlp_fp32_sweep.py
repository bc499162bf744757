"""The fp32 parity mode of the training MLP (pnr_mlp_forward_train_fp32, pnr_mlp_backward_fp32: k_f32_inputs, k_f32_gemm with
and without its split over the reduction, k_f32_slab_sum, k_f32_colsum) per element against the float64 reference of
tests/_mlp32_ref.py, whose docstring derives every bound: each saved activation and raw row layer by layer from the kernel's own
saved inputs, each weight and bias gradient from d_raw and the saved activations.  SURVEY.md 8a row a9.

Every call goes through the C entry points.  raw, acts, d_raw, the workspace (exactly pnr_mlp_backward_fp32_workspace_bytes long)
and every gradient are interior views of ONE allocation filled with a sentinel; each has a guard on both sides, checked after
every call, and no sentinel may be left inside an output.  The guard behind the workspace is at least as long as the overrun of
the library before the head_depth-1 Linears were counted in the workspace size (_mlp32_ref.parent_workspace_bytes).

Cases: 14 geometries at S = 287 (W 128 / 256, D 2 / 3 / 8, skip -1 / 0 / D - 2 / 4, xyz_L 0 / 4 / 10, dir_L 0 / 4, heads from
(0, 0) to (64, 65), (130, 0) and, for head_depth 1 at W = 128, (200, 0) and (0, 256); every head_tap x head_depth); S = 1, 63, 64,
65, 2047, 2048, 2049, 4101 (one, two and three slabs of 2048, a second slab of one sample) at an 8 x 256 and a 3 x 128 network;
d_raw zero outside the last slab / the last 64-row tile; raw and d_raw strides; slices, repeat calls, n_rays = 0; zero d_raw, a
dead layer, weights x 64, far points.

Worst error / bound an MI355X gave over this file (PNR_SWEEP_REPORT=<file.json> writes them).  The bounds are derived, not
measured, except the trig row: nothing in the project fixes the error of the device's sinf / cosf, so its bound is 4 x the
measured worst |kernel - float64| (floored at 2 u = 1.19e-7, and below test_embed's 2e-6).

  quantity                         bound                                         MI355X worst / bound
  gamma: identity columns of EX    bit for bit                                   -
  gamma: identity columns of ED    8 u relative                                  0.20
  gamma: sin / cos bands           TRIG_BOUND = 2.78e-7 = 4 x 6.96e-8            0.25 (worst |kernel - float64| 6.96e-8 = 1.17 u)
  X, F, G, SH, raw                 C_ACC (K + 2) u m + ulp                       0.20 (X; raw 0.023)
  dW, db of the output Linears     C_ACC (min(S, 2048) + n_slab) u A + ulp       0.17
  dW, db of every other Linear     C_ACC (P + min(S, 2048) + n_slab) u A + ulp   0.19
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _mlp32_ref as m32
from _arena import GUARD, SENTINEL, Arena as _Arena
from oracle import c_oracle as co
from oracle import torch_oracle as to
from panopticnerf_amd import _lib, ops

pytestmark = pytest.mark.gpu

_REPORT = os.environ.get("PNR_SWEEP_REPORT")
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _REPORT:
        out = {k: _WORST[k] for k in sorted(_WORST)}
        out.update(trig_measured_in_ref=m32.TRIG_MEASURED, trig_bound=m32.TRIG_BOUND)
        with open(_REPORT, "w") as f:
            json.dump(out, f, indent=1)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _rays(rng, R, near=0.5, far=8.0):
    o = rng.normal(0, 1, (R, 3)) + np.array([0, 1.5, 0])
    d = rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])
    return np.concatenate([o, d, np.full((R, 1), near), np.full((R, 1), far)], 1).astype(np.float32)


def make_case(geom, R, N, seed=0, far=8.0):
    """geom = (D, W, skip, xyz_L, dir_L, n_sem, n_inst, head_tap, head_depth)"""
    D, W, skip, Lx, Ld, C, K, tap, depth = geom
    cfg = to.mlp_config(D=D, W=W, skips=(skip,) if skip >= 0 else (), xyz_L=Lx, dir_L=Ld, n_sem=C, n_inst=K, head_W=W // 2,
                        head_tap=tap, head_depth=depth)
    rng = np.random.default_rng(seed + 11)
    rays = _rays(rng, R, far=far)
    z = co.stratified(rays, N, t_rand=rng.random((R, N)).astype(np.float32))
    return dict(desc=ops.make_desc(D, W, skip, Lx, Ld, C, K, W // 2, "fp32", tap, depth), params=to.init_params(cfg, seed=seed),
                rays=torch.from_numpy(rays), z=torch.from_numpy(z), S=R * N, R=R, N=N,
                d_raw=torch.from_numpy(rng.normal(size=(R * N, 4 + C + K)).astype(np.float32)))


class Run:
    """forward (and backward) of one case through the C entry points on guarded buffers.  raw_layout: 'channel' (channel-major,
    channel stride S + 24) or 'sample' (sample-major: raw_stride_s = channels, raw_stride_c = 1); d_pad: extra floats of d_raw's
    channel stride, NaN-filled."""

    def __init__(self, dev, case, d_raw=None, raw_layout="channel", d_pad=0, backward=True, n_rays=None):
        lib = _lib.load()
        desc, S, R, N = case["desc"], case["S"], case["R"], case["N"]
        ch = 4 + desc.n_sem + desc.n_inst
        self.params = {k: v.to(dev) for k, v in case["params"].items()}
        n_acts = int(lib.pnr_mlp_fp32_acts_floats(ctypes.byref(desc), S))
        ws_bytes = int(lib.pnr_mlp_backward_fp32_workspace_bytes(ctypes.byref(desc), S))
        assert n_acts == m32.acts_regions(desc, S)[1] and ws_bytes == m32.workspace_bytes(desc, S) and ws_bytes % 4 == 0
        ws_guard = max(GUARD, (ws_bytes - m32.parent_workspace_bytes(desc, S)) // 4 + GUARD)
        raw_sc = S + 24 if raw_layout == "channel" else 1
        ds = S + d_pad
        sizes = [("raw", ch * (S + 24) if raw_layout == "channel" else ch * S, GUARD), ("acts", n_acts, GUARD), ("d_raw", ch * ds, GUARD),
                 ("ws", ws_bytes // 4, ws_guard)] + [("g:" + k, v.numel(), GUARD) for k, v in self.params.items()]
        self.arena = ar = _Arena(dev, sizes)
        self.bad = []
        rays, z = case["rays"].to(dev), case["z"].to(dev)
        P, keep = ops._param_struct(desc, self.params, dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nr = R if n_rays is None else n_rays
        _lib.check(lib.pnr_mlp_forward_train_fp32(ctypes.byref(desc), ctypes.byref(P), _p(rays), _p(z), nr, N, _p(ar.view("raw")),
                                                  1 if raw_layout == "channel" else ch, raw_sc, _p(ar.view("acts")), stream),
                   "pnr_mlp_forward_train_fp32")
        torch.cuda.synchronize()
        self.acts = ar.view("acts")
        self.raw = ar.view("raw").as_strided((S, ch), (1, raw_sc) if raw_layout == "channel" else (ch, 1))      # (S, ch) view
        self._after("forward", [("raw", self.raw), ("acts", self.acts)], nr)
        self.grads = {k: ar.view("g:" + k).view(v.shape) for k, v in self.params.items()}
        if not backward:
            return
        d_raw = case["d_raw"] if d_raw is None else d_raw
        self.d_raw = d_raw.to(dev)
        ar.view("d_raw").fill_(float("nan"))
        ar.view("d_raw").as_strided((ch, S), (ds, 1)).copy_(self.d_raw.t())
        G, keep2 = ops._param_struct(desc, self.grads, dev)
        assert {t.data_ptr() for t in keep2 if isinstance(t, torch.Tensor)} == {t.data_ptr() for t in self.grads.values()}      # in place, no copies
        _lib.check(lib.pnr_mlp_backward_fp32(ctypes.byref(desc), ctypes.byref(P), _p(ar.view("d_raw")), ds, _p(self.acts), nr, N,
                                             ctypes.byref(G), _p(ar.view("ws")), stream), "pnr_mlp_backward_fp32")
        torch.cuda.synchronize()
        self._after("backward", list(self.grads.items()), nr)

    def _after(self, what, outputs, n_rays):
        if not self.arena.guards_intact():
            self.bad.append("%s: a guard was written" % what)
        if n_rays:
            self.bad += ["%s: %d elements of %s never written" % (what, int((t == SENTINEL).sum()), k) for k, t in outputs
                         if (t == SENTINEL).any()]


def check(dev, case, run, backward=True):
    rep = m32.Report()
    m32.check_forward(rep, case["desc"], run.params, case["rays"], case["z"], run.raw, run.acts)
    if backward:
        m32.check_backward(rep, case["desc"], run.params, run.acts, run.d_raw, run.grads, case["S"])
    for k, v in rep.worst.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    print({k: "%.3g" % v for k, v in rep.worst.items()})
    assert not run.bad, run.bad
    rep.check()


# --------------------------------------------------------------------------------------------------------- geometries
GEOMS = [  # D, W, skip, xyz_L, dir_L, n_sem, n_inst, head_tap, head_depth
    (2, 128, -1, 0, 0, 0, 0, "trunk", 2),
    (2, 128, 0, 4, 0, 1, 0, "trunk", 2),
    (3, 128, 1, 10, 4, 0, 1, "feature", 2),
    (3, 128, -1, 10, 4, 200, 0, "trunk", 1),             # a head_depth-1 Linear wider than the trunk: the workspace's widest launch
    (3, 128, 0, 10, 0, 0, 256, "feature", 1),
    (8, 256, 4, 10, 4, 45, 32, "trunk", 2),
    (8, 256, 4, 10, 4, 45, 32, "feature", 2),
    (8, 256, 4, 10, 4, 45, 32, "trunk", 1),
    (8, 256, 4, 10, 4, 45, 32, "feature", 1),
    (8, 256, 6, 4, 4, 64, 65, "trunk", 2),
    (8, 128, 0, 10, 4, 130, 0, "feature", 2),
    (3, 256, 1, 0, 4, 64, 65, "feature", 1),
    (2, 256, -1, 4, 0, 130, 0, "trunk", 1),
    (8, 128, 4, 0, 0, 1, 0, "feature", 1),
]
_ID = lambda g: "D%d_W%d_s%d_L%d_%d_C%d_K%d_%s%d" % g       # noqa: E731


@pytest.mark.parametrize("geom", GEOMS, ids=_ID)
def test_every_geometry_at_287_samples(dev, geom):
    case = make_case(geom, 7, 41, seed=GEOMS.index(geom))
    check(dev, case, Run(dev, case))


BIG = (8, 256, 4, 10, 4, 45, 32, "trunk", 2)
SMALL = (3, 128, 1, 10, 4, 5, 200, "feature", 1)        # three slabs of a 200-row head gradient
COUNTS = [(1, 1), (3, 21), (8, 8), (5, 13), (23, 89), (32, 64), (3, 683), (3, 1367)]      # S = 1, 63, 64, 65, 2047, 2048, 2049, 4101


@pytest.mark.parametrize("RN", COUNTS, ids=lambda rn: "S%d" % (rn[0] * rn[1]))
@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["8x256", "3x128"])
def test_sample_counts_around_the_tile_and_the_slab(dev, geom, RN):
    case = make_case(geom, *RN, seed=5)
    check(dev, case, Run(dev, case))


@pytest.mark.parametrize("kind", ["slab", "tile"])
@pytest.mark.parametrize("RN", [(3, 683), (3, 1367), (14, 151)], ids=lambda rn: "S%d" % (rn[0] * rn[1]))
@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["8x256", "3x128"])
def test_d_raw_localised_in_the_tail(dev, geom, RN, kind):
    """d_raw zero outside the last slab / outside its last 64-row tile (the same rows at S = 2049 and 4101, 66 and 2 rows at
    S = 2114): A holds those samples only, so a lost, doubled or misplaced tail is far above the bound"""
    case = make_case(geom, *RN, seed=6)
    d_raw = m32.localise(case["d_raw"], kind)
    assert 0 < int((d_raw != 0).any(1).sum()) <= (m32.KSLAB if kind == "slab" else 64)
    check(dev, case, Run(dev, case, d_raw=d_raw))


# ------------------------------------------------------------------------------------------------------------ strides
STRIDE_GEOM = (3, 128, 1, 10, 4, 5, 3, "trunk", 2)


def test_raw_channel_major_and_sample_major_are_bit_identical(dev):
    case = make_case(STRIDE_GEOM, 7, 41, seed=7)
    a = Run(dev, case, raw_layout="channel", backward=False)
    b = Run(dev, case, raw_layout="sample", backward=False)
    check(dev, case, b, backward=False)
    assert not a.bad and torch.equal(a.raw, b.raw) and torch.equal(a.acts, b.acts)


def test_padded_d_raw_with_nan_in_the_padding(dev):
    """channel stride S + 77, NaN between the channels: every gradient finite and the bits of the dense run"""
    case = make_case(STRIDE_GEOM, 7, 41, seed=7)
    a, b = Run(dev, case), Run(dev, case, d_pad=77)
    check(dev, case, b)
    assert not a.bad
    for k in a.grads:
        assert torch.isfinite(b.grads[k]).all() and torch.equal(a.grads[k], b.grads[k]), k


# --------------------------------------------------------------------------------------------------------- properties
def test_forward_of_ray_slices_equals_the_big_launch(dev):
    """rows are independent: two launches over rays 0 .. 2 and 3 .. 6 give the big launch's raw rows and acts rows bit for bit"""
    case = make_case(BIG, 7, 41, seed=8)
    big = Run(dev, case, backward=False)
    assert not big.bad
    Xb = m32.read_acts(case["desc"], case["S"], big.acts)
    for r0, r1 in ((0, 3), (3, 7)):
        part = dict(case, rays=case["rays"][r0:r1], z=case["z"][r0:r1], R=r1 - r0, S=(r1 - r0) * 41)
        run = Run(dev, part, backward=False)
        assert not run.bad and torch.equal(run.raw, big.raw[r0 * 41:r1 * 41])
        for nm, x in m32.read_acts(case["desc"], part["S"], run.acts).items():
            assert torch.equal(x, Xb[nm][r0 * 41:r1 * 41]), nm


def test_two_backward_calls_are_bit_identical(dev):
    """deterministic reductions (include/pnr.h), three slabs"""
    case = make_case(SMALL, 3, 1367, seed=9)
    a, b = Run(dev, case), Run(dev, case)
    assert not a.bad + b.bad
    for k in a.grads:
        assert torch.equal(a.grads[k], b.grads[k]), k


def test_zero_rays_is_a_no_op(dev):
    case = make_case(STRIDE_GEOM, 7, 41, seed=7)
    run = Run(dev, case, n_rays=0, backward=False)
    assert run.arena.untouched()
    lib, desc = _lib.load(), case["desc"]
    P, keep = ops._param_struct(desc, run.params, dev)
    G, keep2 = ops._param_struct(desc, run.grads, dev)
    ar = run.arena
    _lib.check(lib.pnr_mlp_backward_fp32(ctypes.byref(desc), ctypes.byref(P), _p(ar.view("d_raw")), case["S"], _p(ar.view("acts")), 0, 41,
                                         ctypes.byref(G), _p(ar.view("ws")), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "pnr_mlp_backward_fp32")
    torch.cuda.synchronize()
    assert ar.untouched()


# -------------------------------------------------------------------------------------------------------- edge inputs
def test_zero_d_raw_gives_exactly_zero_gradients(dev):
    case = make_case(STRIDE_GEOM, 7, 41, seed=10)
    run = Run(dev, case, d_raw=torch.zeros_like(case["d_raw"]))
    assert not run.bad
    for k, g in run.grads.items():
        assert not g.any(), k


def test_a_dead_layer_gives_exactly_zero_upstream_gradients(dev):
    """pts_linears.1's bias at -1e4: X_2 = 0 everywhere, so every gate of dY_1 is shut: the gradients of pts_linears.0 and .1 and
    the weight gradient of pts_linears.2 (its input is X_2) are exactly 0; its bias gradient is not"""
    case = make_case((3, 128, -1, 10, 4, 5, 3, "trunk", 2), 7, 41, seed=11)
    case["params"]["pts_linears.1.bias"].fill_(-1e4)
    run = Run(dev, case)
    check(dev, case, run)
    assert not m32.read_acts(case["desc"], case["S"], run.acts)["X2"].any()
    for k in ("pts_linears.0.weight", "pts_linears.0.bias", "pts_linears.1.weight", "pts_linears.1.bias", "pts_linears.2.weight"):
        assert not run.grads[k].any(), k
    assert run.grads["pts_linears.2.bias"].any()


def test_weights_times_64(dev):
    """every weight matrix x 64 (activations grow to 64^5): the bounds scale with m and A"""
    case = make_case((3, 128, 1, 10, 4, 5, 3, "feature", 2), 7, 41, seed=12)
    for k, v in case["params"].items():
        if k.endswith(".weight"):
            v.mul_(64.0)
    check(dev, case, Run(dev, case))


def test_far_points_at_band_9(dev):
    """depths up to 120: arguments of the top band reach 2^9 x 150 (the device sinf / cosf reduce them exactly enough: the trig row
    of the table includes this case)"""
    case = make_case((3, 128, 1, 10, 4, 5, 3, "trunk", 2), 7, 41, seed=13, far=120.0)
    run = Run(dev, case)
    assert m32.read_acts(case["desc"], case["S"], run.acts)["EX"][:, :3].abs().max() > 60
    check(dev, case, run)
