"""Compositing forward (pnr_composite: k_composite, k_composite2) and backward (pnr_composite_backward3: k_composite_bwd) against
the float64 reference of tests/_composite_ref.py, at every admissible sample count, at head widths that hit every batching tail,
at edge inputs, and across several passes of the grid-stride loop.  SURVEY.md 8a rows a6, a9.

Error = max |kernel - ref64| / scale over the rays, per output map or per channel row of d_raw; scale = max(1, max |ref64|) over
that ray's values of the map (of the row), far for depth.  Two exceptions keep the older global scale, each pinned by a strict
xfail test that shows the per-ray gap: the semantic / instance maps of the edge rays whose logits are all +-80
(test_edge_logit_rays_per_ray_gap), and the d_sigma row at N <= 12 (test_small_N_d_sigma_per_ray_gap).  Each (kernel, quantity) has one bound on error / scale: 4x the worst value measured on an MI355X over this whole file (`worst`),
floored at 1e-6, and never looser than the suite's older bars (1e-4 for forward maps, 2e-4 for d_raw).  Inputs are seeded and
the kernels are deterministic, so the errors repeat exactly; the margin is for compiler changes.  `fp32 torch` is the same
oracle graph run in float32 against ref64, for context only (not asserted).  PNR_SWEEP_REPORT=<file.json> makes a run write
the worst errors it saw (both columns), which is how this table was made.

Measured on an MI355X (ROCm 7.0, this file at R = 157 and the grid-stride cases), error / scale:

  kernel           quantity      worst      fp32 torch  bound
  k_composite      rgb           5.25e-07   3.46e-07    2.1e-06
  k_composite      depth         8.55e-07   2.80e-07    3.4e-06
  k_composite      acc           7.84e-07   3.61e-07    3.1e-06
  k_composite      weights       1.02e-06   5.14e-07    4.0e-06
  k_composite      semantic      1.22e-06   8.31e-07    4.8e-06
  k_composite      instance      1.51e-06   6.33e-07    6.0e-06
  k_composite      fix_semantic  9.67e-07   4.83e-07    3.8e-06
  k_composite      fix_instance  1.11e-06   4.79e-07    4.4e-06
  k_composite2     rgb           2.45e-07   2.54e-07    1.0e-06 (floor)
  k_composite2     depth         2.75e-07   2.06e-07    1.0e-06 (floor)
  k_composite2     acc           2.42e-07   2.35e-07    1.0e-06 (floor)
  k_composite2     weights       3.14e-07   2.36e-07    1.2e-06
  k_composite2     semantic      3.57e-07   3.57e-07    1.4e-06
  k_composite2     instance      3.40e-07   3.49e-07    1.3e-06
  k_composite2     fix_semantic  3.10e-07   2.19e-07    1.2e-06
  k_composite2     fix_instance  2.71e-07   1.71e-07    1.0e-06 (floor)
  k_composite_bwd  d_rgb         4.08e-07   1.69e-07    1.6e-06
  k_composite_bwd  d_sigma       8.75e-07   4.21e-07    3.4e-06
  k_composite_bwd  d_sem         1.40e-06   5.74e-07    5.6e-06
  k_composite_bwd  d_inst        1.40e-06   6.27e-07    5.6e-06
"""
import json
import os

import numpy as np
import pytest
import torch

import _composite_ref as cref
from panopticnerf_amd import ops

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

NEAR, FAR = 0.5, 60.0
R_SWEEP = 157               # ragged: not a multiple of any rays-per-wave (64 / SUB = 1 .. 64, 8 for k_composite2)
ALL_N = list(range(4, 257, 4))
HIST_LDS = 48 * 1024        # the launcher's LDS budget for the fixed-field histograms

FWD_MAPS = ("rgb", "depth", "acc", "weights", "semantic", "instance", "fix_semantic", "fix_instance")
BWD_ROWS = ("d_rgb", "d_sigma", "d_sem", "d_inst")
BOUND = {   # (kernel, quantity) -> bound on error / scale: the table above
    ("k_composite", "rgb"): 2.1e-6, ("k_composite", "depth"): 3.4e-6, ("k_composite", "acc"): 3.1e-6,
    ("k_composite", "weights"): 4.0e-6, ("k_composite", "semantic"): 4.8e-6, ("k_composite", "instance"): 6.0e-6,
    ("k_composite", "fix_semantic"): 3.8e-6, ("k_composite", "fix_instance"): 4.4e-6,
    ("k_composite2", "rgb"): 1.0e-6, ("k_composite2", "depth"): 1.0e-6, ("k_composite2", "acc"): 1.0e-6,
    ("k_composite2", "weights"): 1.2e-6, ("k_composite2", "semantic"): 1.4e-6, ("k_composite2", "instance"): 1.3e-6,
    ("k_composite2", "fix_semantic"): 1.2e-6, ("k_composite2", "fix_instance"): 1.0e-6,
    ("k_composite_bwd", "d_rgb"): 1.6e-6, ("k_composite_bwd", "d_sigma"): 3.4e-6, ("k_composite_bwd", "d_sem"): 5.6e-6,
    ("k_composite_bwd", "d_inst"): 5.6e-6,
}
assert set(BOUND) == {(k, q) for k in ("k_composite", "k_composite2") for q in FWD_MAPS} | {("k_composite_bwd", q) for q in BWD_ROWS}

_REPORT = os.environ.get("PNR_SWEEP_REPORT")
_WORST, _WORST32 = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _REPORT:
        rows = [{"kernel": k, "quantity": q, "worst": _WORST.get((k, q)), "fp32_torch": _WORST32.get((k, q)), "bound": b}
                for (k, q), b in sorted(BOUND.items())]
        with open(_REPORT, "w") as f:
            json.dump(rows, f, indent=1)


def _sub(N):
    s = 1
    while s < N // 4:
        s <<= 1
    return s


def fwd_kernel(N, C, K, want_fix, channel_major=True):
    """Which forward kernel pnr_composite launches, and whether it keeps the fixed fields in its LDS histogram (composite_impl's
    rule): k_composite2 for channel-major images with 32 < N <= 64, else k_composite with SUB = pow2ceil(N / 4) lanes per ray."""
    if channel_major and 32 < N <= 64 and (not want_fix or 4 * 8 * (C + K) * 4 <= HIST_LDS):
        return "k_composite2", want_fix
    rpw = 64 // _sub(N)
    return "k_composite", want_fix and 4 * rpw * (C + K) * 4 <= HIST_LDS


def rays_per_wave(kernel, N):
    return 8 if kernel == "k_composite2" else 64 // _sub(N)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _inputs(seed, R, N, C, K, edge=False):
    """Seeded float32 inputs, sample-major raw (R, N, 4+C+K).  Directions are non-unit; sigma is scaled per ray so that some
    rays stay translucent to the last sample (its 1e10 interval matters) and some go opaque.  edge=True adds, in
    separate rays: an opaque sample early on (sigma 1e3), an empty ray (sigma + noise < 0 everywhere), runs of equal z,
    logits of +-80, and labels -1, -7 and >= n everywhere."""
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 1, (R, 3)) + np.array([0, 1.5, 0])
    d = (rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])) * rng.uniform(0.5, 2.0, (R, 1))
    rays = np.concatenate([o, d, np.full((R, 1), NEAR), np.full((R, 1), FAR)], 1).astype(np.float32)
    z = (NEAR + (FAR - NEAR) * (np.arange(N) + rng.random((R, N))) / N).astype(np.float32)
    raw = rng.normal(0, 1, (R, N, 4 + C + K)).astype(np.float32)
    raw[..., 3] = rng.normal(0.0, 0.05, (R, N)) * rng.uniform(0.2, 3.0, (R, 1))
    noise = rng.normal(0, 0.02, (R, N)).astype(np.float32)
    ls = rng.integers(-1, max(C, 1), (R, N)).astype(np.int32)
    li = rng.integers(-1, max(K, 1), (R, N)).astype(np.int32)
    if edge:
        raw[0, min(1, N - 1), 3] = 1e3                           # opaque after one early sample
        raw[1, :, 3] = -1.0                                      # empty: sigma + noise < 0
        for r in range(2, R, 3):                                 # runs of equal z (dist = 0), order kept
            for i in range(1, N):
                if rng.random() < 0.4:
                    z[r, i] = z[r, i - 1]
        big = rng.choice(np.array([-80.0, 80.0], np.float32), (R, N, C + K))
        raw[4::5, :, 4:] = big[4::5]                             # logits of +-80
        ls = rng.choice(np.array([-7, -1, C, C + 3] + list(range(C)), np.int32), (R, N))
        li = rng.choice(np.array([-7, -1, K, K + 3] + list(range(K)), np.int32), (R, N))
    return raw, z, rays, noise, ls, li


def _grads(seed, R, N, C, K):
    rng = np.random.default_rng(seed + 1000)
    shapes = {"rgb": (R, 3), "depth": (R,), "acc": (R,), "semantic": (R, C), "instance": (R, K), "weights": (R, N),
              "fix_semantic": (R, C), "fix_instance": (R, K)}
    g = {k: torch.tensor(rng.normal(size=s).astype(np.float32)) for k, s in shapes.items() if int(np.prod(s))}
    g["depth"] = g["depth"] * 0.1
    return g


def _cm(raw, dev):
    """sample-major (R, N, ch) numpy -> dense channel-major (ch, R*N) on the device"""
    R, N, ch = raw.shape
    return torch.tensor(np.ascontiguousarray(raw.reshape(R * N, ch).T)).to(dev)


def _g(x, dev):
    return None if x is None else torch.as_tensor(x).to(dev).contiguous()


# ------------------------------------------------------------------------------------------------------------------ checks
def _note(table, key, v):
    table[key] = max(table.get(key, 0.0), v)


def _ray_scale(k, v, logit_rays=None):
    """per-ray scale of a map (R, ...): max(1, max |ref64[ray]|), FAR for depth.  logit_rays (edge inputs: rays whose logits are all
    +-80): their semantic / instance maps keep the map's global scale -- see test_edge_logit_rays_per_ray_gap"""
    if k == "depth":
        return torch.full((v.shape[0],), FAR, dtype=torch.float64)
    s = v.reshape(v.shape[0], -1).abs().amax(1).clamp(min=1.0)
    if logit_rays is not None and k in ("semantic", "instance"):
        s[logit_rays] = max(1.0, v.abs().max().item())
    return s


def check_fwd(kernel, out, ref, what, ref32=None, logit_rays=None):
    assert set(out) == set(ref), (what, sorted(out), sorted(ref))
    for k, v in ref.items():
        if v.numel() == 0:
            continue
        R = v.shape[0]
        scale = _ray_scale(k, v, logit_rays)
        v = v.reshape(R, -1)
        e = ((out[k].detach().cpu().double().reshape(R, -1) - v).abs().amax(1) / scale).max().item()
        _note(_WORST, (kernel, k), e)
        if ref32 is not None:
            _note(_WORST32, (kernel, k), ((ref32[k].double().reshape(R, -1) - v).abs().amax(1) / scale).max().item())
        assert e <= BOUND[(kernel, k)], (what, kernel, k, e, BOUND[(kernel, k)])


def _row_kind(c, C):
    return BWD_ROWS[0] if c < 3 else BWD_ROWS[1] if c == 3 else BWD_ROWS[2] if c < 4 + C else BWD_ROWS[3]


SIGMA_GAP_N = 12          # see test_small_N_d_sigma_per_ray_gap


def check_bwd(d_raw, ref, C, N, what, ref32=None):
    got = d_raw.detach().cpu().double()
    assert got.shape == ref.shape, what
    ch = ref.shape[0]
    per_ray = lambda x: x.reshape(ch, -1, N)                        # noqa: E731  (channel row, ray, sample)
    scale = per_ray(ref).abs().amax(2).clamp(min=1.0)               # per channel row and ray
    if N <= SIGMA_GAP_N:                                            # the d_sigma row keeps its global scale: test_small_N_d_sigma_per_ray_gap
        scale[3] = max(1.0, ref[3].abs().max().item())
    err = ((per_ray(got) - per_ray(ref)).abs().amax(2) / scale).amax(1)
    e32 = ((per_ray(ref32.double()) - per_ray(ref)).abs().amax(2) / scale).amax(1) if ref32 is not None else None
    for c in range(ref.shape[0]):
        key = ("k_composite_bwd", _row_kind(c, C))
        _note(_WORST, key, err[c].item())
        if e32 is not None:
            _note(_WORST32, key, e32[c].item())
    bad = [(c, err[c].item()) for c in range(ref.shape[0]) if err[c].item() > BOUND[("k_composite_bwd", _row_kind(c, C))]]
    assert not bad, (what, bad[:8])


def run_fwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, white, what, layouts=(True, False), logit_rays=None):
    """pnr_composite on a channel-major (True) and / or a sample-major (False) copy of raw, each against forward64; returns
    the kernel's maps per layout"""
    R, N = z.shape
    ref = cref.forward64(raw, z, rays, C, K, noise, ls, li, sem_mode, white)
    ref32 = cref.forward64(raw, z, rays, C, K, noise, ls, li, sem_mode, white, dtype=torch.float32) if _REPORT else None
    outs = {}
    for cm in layouts:
        rg = _cm(raw, dev) if cm else torch.tensor(raw).to(dev)
        outs[cm] = ops.composite(rg, _g(z, dev), _g(rays, dev), C, K, cm, _g(noise, dev), _g(ls, dev), _g(li, dev), sem_mode, white)
        kernel, _ = fwd_kernel(N, C, K, ls is not None or li is not None, cm)
        check_fwd(kernel, outs[cm], ref, f"{what} channel_major={cm}", ref32, logit_rays)
    return outs


def run_bwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, grads, ce_sem, ce_inst, what):
    """one pnr_composite_backward3 call against backward64; returns d_raw"""
    dt = lambda v: None if v is None else torch.tensor([v], dtype=torch.float32, device=dev)   # noqa: E731
    d = ops.composite_backward(_cm(raw, dev), _g(z, dev), _g(rays, dev), C, K, {k: v.to(dev) for k, v in grads.items()},
                               _g(noise, dev), _g(ls, dev), _g(li, dev), dt(ce_sem), dt(ce_inst), sem_mode)
    ref = cref.backward64(raw, z, rays, C, K, grads, noise, ls, li, ce_sem or 0.0, ce_inst or 0.0, sem_mode)
    ref32 = (cref.backward64(raw, z, rays, C, K, grads, noise, ls, li, ce_sem or 0.0, ce_inst or 0.0, sem_mode, torch.float32)
             if _REPORT else None)
    check_bwd(d, ref, C, z.shape[1], what, ref32)
    return d


def test_kernel_selection_rule():
    """what the sweep assumes about composite_impl's dispatch (CPU-side arithmetic only, but the module is GPU-marked)"""
    assert fwd_kernel(44, 7, 5, True) == ("k_composite2", True)
    assert fwd_kernel(44, 7, 5, True, channel_major=False) == ("k_composite", True)
    assert fwd_kernel(4, 45, 32, True) == ("k_composite", False)
    assert fwd_kernel(4, 24, 24, True) == ("k_composite", True)
    assert fwd_kernel(8, 100, 28, True) == ("k_composite", False)
    # test_head_widths reaches the use_hist = 0 fallback (fixed fields by group_sum) of k_composite: N = 4 at 45 / 32, ...
    fallback = [(n, c, k) for n in WIDTH_N for c, k in WIDTHS if c + k and not fwd_kernel(n, c, k, True)[1]]
    assert fallback == [(4, 45, 32), (4, 100, 28), (8, 100, 28)], fallback
    assert [rays_per_wave("k_composite", n) for n in (4, 8, 12, 20, 36, 68, 132)] == [64, 32, 16, 8, 4, 2, 1]


# ------------------------------------------------------------------------------------------------------------------ a. forward, every N
@pytest.mark.parametrize("N", ALL_N)
def test_forward_every_N(dev, N):
    C, K = 7, 5
    raw, z, rays, noise, ls, li = _inputs(N, R_SWEEP, N, C, K)
    for sem_mode in (0, 1):
        for white in (False, True):
            run_fwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, white, f"N={N} sm={sem_mode} wb={white}")


# ------------------------------------------------------------------------------------------------------------------ b. backward, every N
CE_SEM, CE_INST = 0.013, 0.007
SOLO_N = [4, 8, 12, 28, 60, 100, 252]       # one N per sub-width SUB = 1, 2, 4, 8, 16, 32, 64


@pytest.mark.parametrize("N", ALL_N)
def test_backward_every_N(dev, N):
    C, K = 7, 5
    raw, z, rays, noise, ls, li = _inputs(N + 1, R_SWEEP, N, C, K)
    grads = _grads(N, R_SWEEP, N, C, K)
    for sem_mode in (0, 1):
        run_bwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, grads, CE_SEM, CE_INST, f"N={N} sm={sem_mode} all sources")
    if N not in SOLO_N:
        return
    # each source alone, every other one passed as NULL (labels only where the source reads them)
    for sem_mode in (0, 1):
        for k in cref.GRAD_KEYS:
            lab = k.startswith("fix_")
            run_bwd(dev, raw, z, rays, noise, ls if lab else None, li if lab else None, C, K, sem_mode, {k: grads[k]}, None, None,
                    f"N={N} sm={sem_mode} only {k}")
        run_bwd(dev, raw, z, rays, noise, ls, None, C, K, sem_mode, {}, CE_SEM, None, f"N={N} sm={sem_mode} only ce_sem")
        run_bwd(dev, raw, z, rays, None, None, li, C, K, sem_mode, {}, None, CE_INST, f"N={N} sm={sem_mode} only ce_inst")


# ------------------------------------------------------------------------------------------------------------------ c. head widths
WIDTH_N = [4, 8, 12, 16, 28, 32, 36, 44, 60, 64, 68, 100, 132, 192, 252, 256]
WIDTHS = [(0, 0), (1, 0), (0, 1), (1, 1), (3, 2), (9, 7), (45, 32), (100, 28)]


@pytest.mark.parametrize("N", WIDTH_N)
def test_head_widths(dev, N):
    """C mod CB / BWD_PB != 0, C < CB, C = 1 in softmax mode (probability 1, gradient 0), no heads at all, and at N <= 8 the
    widths whose LDS histogram would not fit (use_hist = 0: the group_sum fallback)"""
    R = R_SWEEP if N <= 128 else 61
    for C, K in WIDTHS:
        raw, z, rays, noise, ls, li = _inputs(1000 * C + 10 * K + N, R, N, C, K)
        grads = _grads(N + C, R, N, C, K)
        for sem_mode in (0, 1):
            run_fwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, sem_mode == 1, f"N={N} C={C} K={K} sm={sem_mode}")
            d = run_bwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, grads, CE_SEM, CE_INST, f"N={N} C={C} K={K} sm={sem_mode}")
            if sem_mode == 1 and C == 1:        # softmax of one logit: the composited-map gradient vanishes, only CE remains
                dce = run_bwd(dev, raw, z, rays, noise, ls, li, C, K, 1, {"semantic": grads["semantic"]}, None, None, "C=1 softmax")
                assert (dce[4] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ d. edge inputs
EDGE_N = [4, 8, 28, 36, 44, 64, 100, 192, 256]
LOGIT_RAYS = slice(4, None, 5)      # the edge rays whose logits are all +-80 (_inputs)


@pytest.mark.parametrize("N", EDGE_N)
def test_edge_inputs(dev, N):
    C, K = 7, 5
    raw, z, rays, noise, ls, li = _inputs(5 * N + 3, R_SWEEP, N, C, K, edge=True)
    assert ((raw[1, :, 3] + noise[1]) < 0).all() and (np.diff(z, axis=1) == 0).any()
    grads = _grads(N, R_SWEEP, N, C, K)
    ign_s = np.where((ls >= 0) & (ls < C), ls, -1).astype(np.int32)      # the same labels with every ignored one as -1
    ign_i = np.where((li >= 0) & (li < K), li, -1).astype(np.int32)
    for sem_mode in (0, 1):
        for white in (False, True):
            outs = run_fwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, white, f"edge N={N} sm={sem_mode} wb={white}",
                           logit_rays=LOGIT_RAYS)
            for cm, out in outs.items():
                what = f"edge N={N} sm={sem_mode} wb={white} cm={cm}"
                assert out["acc"][1].item() == 0.0 and (out["weights"][1] == 0).all(), what           # the empty ray
                assert (out["rgb"][1] == (1.0 if white else 0.0)).all(), what
                rg = _cm(raw, dev) if cm else torch.tensor(raw).to(dev)
                clean = ops.composite(rg, _g(z, dev), _g(rays, dev), C, K, cm, _g(noise, dev), _g(ign_s, dev), _g(ign_i, dev),
                                      sem_mode, white)
                for k in ("fix_semantic", "fix_instance"):                                          # ignored labels add nothing
                    assert torch.equal(out[k], clean[k]), (what, k)
        d = run_bwd(dev, raw, z, rays, noise, ls, li, C, K, sem_mode, grads, CE_SEM, CE_INST, f"edge N={N} sm={sem_mode}")
        d_clean = ops.composite_backward(_cm(raw, dev), _g(z, dev), _g(rays, dev), C, K, {k: v.to(dev) for k, v in grads.items()},
                                         _g(noise, dev), _g(ign_s, dev), _g(ign_i, dev), torch.tensor([CE_SEM], device=dev),
                                         torch.tensor([CE_INST], device=dev), sem_mode)
        assert torch.equal(d, d_clean), f"edge N={N} sm={sem_mode}: ignored labels changed d_raw"


@pytest.mark.xfail(strict=True, reason="known gap, kept for a follow-up: on rays whose logits are all +-80, k_composite's semantic "
                   "map misses its bound under the per-ray scale (7.8e-6 against 4.8e-6 at N = 256; the float32 torch graph: 2.0e-5)")
def test_edge_logit_rays_per_ray_gap(dev):
    """What the LOGIT_RAYS exception of test_edge_inputs leaves out.  On these rays a map of sum_i w_i v_i with v = +-80 cancels to
    a few units, so an fp32 rounding of the weights (relative ~1e-7 after 256 transmittance factors) costs 80 x that against a
    scale of a few: the per-ray error is bounded by max |v| sum_i w_i, not by the map's size.  Strict: the day the kernel meets the
    per-ray bound here, this test fails and the exception goes."""
    N, C, K = 256, 7, 5
    raw, z, rays, noise, ls, li = _inputs(5 * N + 3, R_SWEEP, N, C, K, edge=True)
    ref = cref.forward64(raw, z, rays, C, K, noise, ls, li, 0, False)["semantic"][LOGIT_RAYS]
    out = ops.composite(_cm(raw, dev), _g(z, dev), _g(rays, dev), C, K, True, _g(noise, dev), _g(ls, dev), _g(li, dev), 0, False)
    got = out["semantic"].cpu().double()[LOGIT_RAYS]
    e = float(((got - ref).abs().amax(1) / ref.abs().amax(1).clamp(min=1.0)).max())
    assert e <= BOUND[("k_composite", "semantic")], e


@pytest.mark.xfail(strict=True, reason="known gap, kept for a follow-up: at N <= 12, k_composite_bwd's d_sigma misses its bound under the "
                   "per-ray scale (up to 2.8e-5 against 3.4e-6; the float32 torch graph: 3.9e-6)")
def test_small_N_d_sigma_per_ray_gap(dev):
    """What the SIGMA_GAP_N exception of check_bwd leaves out.  d_sigma = delta (1 - alpha) (G T - S / (1 - alpha + 1e-10)): at
    N <= 12 the intervals delta are tens of units, and k_composite_bwd forms 1 - alpha, T and the suffix sums S in fp32, so one
    rounding of 1 - alpha (an ulp of 1) and of the cancelling difference are multiplied by delta.  Against a ray's own d_sigma
    scale that is up to 2.8e-5 (the float32 torch graph, whose autograd takes d alpha / d sigma from exp directly: 3.9e-6).
    Taking the factor from exp and the sums in double meets the bound, but changes the rounding of every training step, and the
    chaotic fp32-mode student of test_gpu_convergence.py then lands outside its gate: that change needs its own pull request.
    Strict: the day the kernel meets the per-ray bound here, this test fails and the exception goes."""
    N, C, K = 4, 7, 5
    raw, z, rays, noise, ls, li = _inputs(N + 1, R_SWEEP, N, C, K)
    grads = _grads(N, R_SWEEP, N, C, K)
    dt = lambda v: torch.tensor([v], dtype=torch.float32, device=dev)   # noqa: E731
    d = ops.composite_backward(_cm(raw, dev), _g(z, dev), _g(rays, dev), C, K, {k: v.to(dev) for k, v in grads.items()},
                               _g(noise, dev), _g(ls, dev), _g(li, dev), dt(CE_SEM), dt(CE_INST), 0)
    ref = cref.backward64(raw, z, rays, C, K, grads, noise, ls, li, CE_SEM, CE_INST, 0)[3].reshape(-1, N)
    got = d[3].detach().cpu().double().reshape(-1, N)
    e = float(((got - ref).abs().amax(1) / ref.abs().amax(1).clamp(min=1.0)).max())
    assert e <= BOUND[("k_composite_bwd", "d_sigma")], e


# ------------------------------------------------------------------------------------------------------------------ e. grid-stride loop
def _big_inputs(dev, R, N, C, K, seed):
    """device-side inputs for a launch of several grid-stride passes (same distributions as _inputs)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    o = torch.randn((R, 3), generator=g, device=dev)
    d = (torch.randn((R, 3), generator=g, device=dev) * 0.3 + torch.tensor([0.0, 0.0, 1.0], device=dev))
    d = d * (0.5 + 1.5 * torch.rand((R, 1), generator=g, device=dev))
    rays = torch.cat([o, d, torch.full((R, 1), NEAR, device=dev), torch.full((R, 1), FAR, device=dev)], 1).contiguous()
    t = (torch.arange(N, device=dev, dtype=torch.float32) + torch.rand((R, N), generator=g, device=dev)) / N
    z = (NEAR + (FAR - NEAR) * t).contiguous()
    raw = torch.randn((4 + C + K, R * N), generator=g, device=dev)
    raw[3] = (torch.randn((R, N), generator=g, device=dev) * 0.05 * (0.2 + 2.8 * torch.rand((R, 1), generator=g, device=dev))).reshape(-1)
    noise = (torch.randn((R, N), generator=g, device=dev) * 0.02).contiguous()
    ls = torch.randint(-1, C, (R, N), generator=g, device=dev, dtype=torch.int32)
    li = torch.randint(-1, K, (R, N), generator=g, device=dev, dtype=torch.int32)
    return raw, z, rays, noise, ls, li


def _grid_R(dev, kernel, N):
    """Both kernels cap their grid at 8 workgroups of 4 waves per CU and grid-stride over the remaining ray groups, a group
    being rays_per_wave(N) rays.  cap = CUs x 8 x 4 waves, so R = (3 cap + cap / 3) x rays_per_wave + rays_per_wave / 2 + 1
    rays make every launch take 3 full passes and a partial fourth, with a ragged last group."""
    cap = torch.cuda.get_device_properties(dev).multi_processor_count * 8 * 4
    rpw = rays_per_wave(kernel, N)
    return (3 * cap + cap // 3) * rpw + rpw // 2 + 1, cap


def _slices(R):
    n = min(777, R // 3)
    return [(0, n), (R // 2 - 301, R // 2 - 301 + n), (R - n, R)]


def _sample_rays(R):
    return np.sort(np.random.default_rng(R).choice(R, min(R, 512), replace=False))


@pytest.mark.parametrize("kernel,N", [("k_composite", 4), ("k_composite", 192), ("k_composite2", 44)])
def test_forward_grid_stride(dev, kernel, N):
    C, K = 2, 1
    R, cap = _grid_R(dev, kernel, N)
    assert fwd_kernel(N, C, K, True)[0] == kernel
    raw, z, rays, noise, ls, li = _big_inputs(dev, R, N, C, K, N)
    full = ops.composite(raw, z, rays, C, K, True, noise, ls, li)
    for a, b in _slices(R):
        part = ops.composite(raw[:, a * N:b * N], z[a:b], rays[a:b], C, K, True, noise[a:b].contiguous(), ls[a:b].contiguous(),
                             li[a:b].contiguous())
        for k in full:
            assert torch.equal(full[k][a:b], part[k]), (kernel, N, R, (a, b), k)
    idx = torch.tensor(_sample_rays(R), device=dev)
    s_raw = raw.reshape(-1, R, N)[:, idx].permute(1, 2, 0).cpu().numpy()
    ref = cref.forward64(s_raw, z[idx], rays[idx], C, K, noise[idx], ls[idx], li[idx])
    check_fwd(kernel, {k: v[idx] for k, v in full.items()}, ref, f"grid-stride {kernel} N={N} R={R}")


@pytest.mark.parametrize("N", [4, 44, 192])
def test_backward_grid_stride(dev, N):
    C, K = 2, 1
    R, cap = _grid_R(dev, "k_composite_bwd", N)
    raw, z, rays, noise, ls, li = _big_inputs(dev, R, N, C, K, N + 1)
    g = torch.Generator(device=dev).manual_seed(N)
    shapes = {"rgb": (R, 3), "depth": (R,), "acc": (R,), "semantic": (R, C), "instance": (R, K), "weights": (R, N),
              "fix_semantic": (R, C), "fix_instance": (R, K)}
    grads = {k: torch.randn(s, generator=g, device=dev) for k, s in shapes.items()}
    ce_s, ce_i = torch.tensor([CE_SEM], device=dev), torch.tensor([CE_INST], device=dev)
    full = ops.composite_backward(raw, z, rays, C, K, grads, noise, ls, li, ce_s, ce_i)
    for a, b in _slices(R):
        part = ops.composite_backward(raw[:, a * N:b * N].contiguous(), z[a:b], rays[a:b], C, K,
                                      {k: v[a:b].contiguous() for k, v in grads.items()}, noise[a:b].contiguous(),
                                      ls[a:b].contiguous(), li[a:b].contiguous(), ce_s, ce_i)
        assert torch.equal(full[:, a * N:b * N], part), (N, R, (a, b))
    idx = torch.tensor(_sample_rays(R), device=dev)
    s_raw = raw.reshape(-1, R, N)[:, idx].permute(1, 2, 0).cpu().numpy()
    ref = cref.backward64(s_raw, z[idx], rays[idx], C, K, {k: v[idx] for k, v in grads.items()}, noise[idx], ls[idx], li[idx],
                          CE_SEM, CE_INST)
    check_bwd(full.reshape(-1, R, N)[:, idx].reshape(4 + C + K, -1), ref, C, N, f"grid-stride bwd N={N} R={R}")
