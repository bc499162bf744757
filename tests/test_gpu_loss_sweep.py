"""The loss wrapper (pnr_losses: k_loss_count, k_loss_maps, k_loss_final; pnr_ce3d: k_ce3d, k_ce3d_final) against the float64
reference of tests/_loss_ref.py: at every class count 1 .. 130 (the 16 lanes of a ray stride over the classes), at every small
ray count, around every edge of the two-stage reductions, across three trips of the grid-stride and lane-strided loops, under a
common shift of the logits, at edge labels / logits / probabilities / depth targets, and for every subset of the map and gradient
pointers of the C entry point.  SURVEY.md 8f rank 1.

Every call goes through the C entry point with caller-owned buffers: each gradient buffer, losses_out, out2 and the workspace
(exactly pnr_*_workspace_bytes long) sits between guards, gradients are pre-filled with a sentinel, and every case checks that
the guards are intact and that no sentinel is left inside (ops.losses hands the kernel torch.empty buffers: a row the kernel
forgets is garbage in the backward pass).

Bounds: k * u * cond per element, u = 2^-24, cond from the float64 reference (the forms and their reasons are in the docstring of
_loss_ref.py), never looser than test_gpu_losses.py's bars.  k is fixed on the CPU, from the reference alone: rho is the worst
error / (u * cond) of the numpy float32 restatement of the kernels' op order (losses32 / ce3d32) and of the torch oracle's graph
run in float32, against float64, over the whole case list of this file (tests/test_loss_ref.py recomputes it);
k = max(4, ceil(4 rho)), the factor 4 being the project's margin for the device's expf / logf and fma contraction.  A mean's
bound is the mean of its rays' bounds plus k_sum u |term| (k_sum: the roundings on the longest path of the reduction); `mean`,
`total` and `ce3d mean` below are error / bound, so their k is 1.  The *_ray rows are observable on the GPU only where one ray
(sample) is labelled, so that the mean is its value.  The GPU column is context: the worst ratio an MI355X gave over this file
(PNR_SWEEP_REPORT=<file.json> writes it); it does not set k.

  quantity     cond                                           rho     k    MI355X
  ce_ray       max(1, log den + (mx - x_label))               3.10    13   1.17
  ce_grad      s (p_c (1 + |x_c - mx|) + [c = label])         6.30    26   5.81
  nll_ray      max(1, |log(p + eps)|)                         2.35    10   2.12
  nll_grad     |g|                                            2.63    11   2.52
  rgb_ray      the value                                      4.22    17   -  (its mean divides by 3)
  rgb_grad     |g|                                            2.76    12   2.76
  depth_ray    the value                                      2.93    12   1.60
  depth_grad   |g| (depth_l2); L1: bit for bit                2.53    11   2.53
  ce3d_ray     max(1, log den + (mx - x_label))               10.70   43   1.07
  mean         (its bound)                                    0.16    1    0.22
  total        (its bound)                                    0.11    1    0.09
  ce3d mean    (its bound)                                    0.07    1    0.03

ce3d_ray's rho is the largest because k_ce3d adds the n terms of its denominator one after the other (the online form), where
ce_row's 16 lanes split them: the error of log den grows with n (rho is reached at n around 100).

Shift invariance.  Until this file existed ce_row and k_ce3d returned (mx + logf(den)) - x_label, which rounds at the size of
mx: off by up to |mx| 2^-25 under a common offset of the logits (3e-5 at 1000, 1e-3 at 30000) while the value itself is a few
units.  On that order the shift cases below failed on an MI355X, and only they: a mean up to 1235 times its bound, one sample of
pnr_ce3d at an offset of 3e4 wrong by 9.5e-4; both kernels now return logf(den) + (mx - x_label).  The gradients use x - mx and never had the defect.

Not tested: non-finite logits (a -inf first logit turns k_ce3d's online form into NaN: -inf - -inf)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _loss_ref as lr
from panopticnerf_amd import _lib

pytestmark = pytest.mark.gpu

CASES = lr.loss_cases()
CE3D_CASES = lr.ce3d_cases()
SENTINEL = np.float32(-7.5e33)
GUARD = 64                      # elements on each side of every buffer

_REPORT = os.environ.get("PNR_SWEEP_REPORT")
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _REPORT:
        with open(_REPORT, "w") as f:
            json.dump({k: _WORST[k] for k in sorted(_WORST)}, f, indent=1)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class _Guarded:
    """a device buffer of `shape` between two guards, everything pre-filled with the sentinel (bytes 0xA5 for raw bytes)"""

    def __init__(self, dev, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.fill = 0xA5 if dtype == torch.uint8 else float(SENTINEL)
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, device=dev, dtype=dtype)
        self.view = self.buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all() and (self.buf[GUARD + self.n:] == self.fill).all())

    def numpy(self):
        return self.view.cpu().numpy().reshape(self.shape)


def run_losses(dev, maps, tg, C, K, l2=False, prob=False, want="all"):
    """pnr_losses through the C entry point.  maps: the maps to pass (others NULL); want: 'all', 'none' or the keys whose gradient is
    asked for.  Returns ({losses, grads} as numpy, list of structural failures)."""
    lib = _lib.load()
    R = next(iter(tg.values())).shape[0]
    d = {k: torch.tensor(v).to(dev).contiguous() for k, v in maps.items()}
    t = {k: torch.tensor(v).to(dev).contiguous() for k, v in tg.items()}
    want = set(maps) if want == "all" else set() if want == "none" else set(want)
    g = {k: _Guarded(dev, maps[k].shape) for k in want}
    out = _Guarded(dev, (8,))
    ws = _Guarded(dev, (int(lib.pnr_losses_workspace_bytes(R)),), torch.uint8)
    cfg = _lib.LossCfg(*(float(lr.WEIGHTS[k]) for k in lr.KEYS), int(bool(l2)), float(lr.FIX_EPS), int(bool(prob)))
    gp = lambda k: _p(g[k].view) if k in g else _p(None)    # noqa: E731
    rc = lib.pnr_losses(ctypes.byref(cfg), R, int(C), int(K), *(_p(d.get(k)) for k in lr.KEYS), _p(t.get("rgb")), _p(t.get("depth")),
                        _p(t.get("semantic")), _p(t.get("instance")), _p(out.view), *(gp(k) for k in lr.KEYS), _p(ws.view),
                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "pnr_losses")
    torch.cuda.synchronize()
    bad = [f"guard of {k} touched" for k, b in list(g.items()) + [("losses_out", out), ("workspace", ws)] if not b.guards_intact()]
    got = {"losses": out.numpy(), "grads": {k: b.numpy() for k, b in g.items()}}
    bad += [f"g_{k}: {int((v == SENTINEL).sum())} elements never written" for k, v in got["grads"].items() if (v == SENTINEL).any()]
    return got, bad


def check_losses(dev, case, maps=None, tg=None, present=None, want="all"):
    """one case against losses64: every gradient element, every term, the total, the exact entries, the structure"""
    if maps is None:
        maps, tg = lr.loss_inputs(case)
    if present is not None:
        maps = {k: v for k, v in maps.items() if k in present}
    got, bad = run_losses(dev, maps, tg, case["C"], case["K"], case["l2"], case["prob"], want)
    if maps:
        ref = lr.losses64(maps, tg, lr.WEIGHTS, case["C"], case["K"], case["l2"], lr.FIX_EPS, case["prob"])
        bad += lr.violations(got, ref, exact=True)
        lr.worst(got, ref, _WORST, exact=True)
        for i, k in enumerate(lr.KEYS):                      # one labelled ray: the mean is the ray's own value
            if k in ref["per_ray"] and ref["n"][k] == 1 and np.count_nonzero(ref["unit_ray"][k]) == 1:
                q = ref["kind"][k] + "_ray"
                _WORST[q] = max(_WORST.get(q, 0.0), abs(float(got["losses"][i]) - ref["losses"][i]) / ref["unit_ray"][k].sum())
    elif got["losses"].any():
        bad.append(f"no map at all, yet losses_out = {got['losses']}")
    return got, [f"{case['id']}: {b}" for b in bad]


def _run_group(dev, pick):
    bad = []
    for case in CASES:
        if pick(case):
            bad += check_losses(dev, case)[1]
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------------------ pnr_losses
@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("prob", [False, True])
def test_losses_every_class_count(dev, l2, prob):
    """C = 1 .. 130, K cycling through {0, 1, 15, 16, 17, 33}, R = 157 (the last block holds 13 rays)"""
    _run_group(dev, lambda c: c["group"] == "sweep" and c["l2"] == l2 and c["prob"] == prob)


def test_losses_every_small_ray_count(dev):
    """R = 1 .. 17: a term is one ray or a few, so the per-ray bound bites"""
    _run_group(dev, lambda c: c["group"] == "smallR")


def test_losses_around_each_reduction_edge(dev):
    """255 .. 257, 1023 .. 1025 (64 block partials: the width of k_loss_final), 4097 (5 trips of its lane loop)"""
    _run_group(dev, lambda c: c["group"] == "Redge")


def test_losses_three_trips_of_the_counting_loop(dev):
    """R = 3 * 262144 + 77: k_loss_count's 1024 x 256 grid strides three times; the counts are verified exactly through the
    gradients they divide (L1 depth gradient, fixed-field gradient at fl(p + eps) == 1: bit for bit)"""
    case = next(c for c in CASES if c["group"] == "big")
    maps, tg = lr.loss_inputs(case)
    ref = lr.losses64(maps, tg, lr.WEIGHTS, case["C"], case["K"])
    assert min(ref["counts"].values()) > 2 * 262144 and ref["exact"]["depth"][0].all()
    assert ref["exact"]["fix_semantic"][0].sum() == ref["counts"]["semantic"] and ref["exact"]["fix_instance"][0].sum() == ref["counts"]["instance"]
    got, bad = check_losses(dev, case, maps, tg)
    assert not bad, "\n".join(bad)


def test_losses_shift_invariance(dev):
    """a common offset of 0, +-80, +-1e3, 3e4 on each ray's logits (exact in float32 on the cases' logit grid): the values stay
    inside the shift-invariant bound, the gradients are those of the unshifted rows"""
    _run_group(dev, lambda c: c["group"] in ("shiftmix", "shift"))
    case = next(c for c in CASES if c["id"] == "shift30000-C45-R157")
    g1 = check_losses(dev, case)[0]["grads"]
    g0 = check_losses(dev, dict(case, offset=None))[0]["grads"]      # same seed (the id), no offset: x - mx is the same float
    assert all(np.array_equal(g1[k], g0[k]) for k in ("semantic", "instance"))


def test_losses_edge_inputs(dev):
    """labels -1, -7, n, n + 5, 255, INT_MAX, INT_MIN; logits all equal, +-80, one dominant class; probabilities 0, 1 and 1 - eps;
    depth targets 0, -0.0, negative, NaN; depth == depth_gt; rgb == rgb_gt; a batch without a label; a batch without a depth"""
    _run_group(dev, lambda c: c["group"] == "edge")


def test_losses_every_subset_of_pointers(dev):
    """All 64 subsets of the six maps x gradients for all / none / every other one: requested gradients fully written (ignored
    rays exactly 0: their bound is 0), nothing else touched, absent terms 0, losses_out[7] = 0, the same losses bits with and
    without gradients, the same bits from a second call."""
    case = next(c for c in CASES if c["id"] == "edge-l20-p0")
    maps, tg = lr.loss_inputs(case)
    bad = []
    for mask in range(64):
        present = [k for i, k in enumerate(lr.KEYS) if mask >> i & 1]
        res = {}
        for mode, want in (("all", "all"), ("none", "none"), ("alt", present[::2])):
            res[mode], b = check_losses(dev, case, maps, tg, present, want)
            bad += [f"subset {mask:06b} grads {mode}: {x}" for x in b]
            if set(res[mode]["grads"]) != (set(present) if mode == "all" else set(want) if mode == "alt" else set()):
                bad.append(f"subset {mask:06b}: wrong gradient set")
        again = check_losses(dev, case, maps, tg, present, "all")[0]
        for mode in ("none", "alt"):
            if res[mode]["losses"].tobytes() != res["all"]["losses"].tobytes():
                bad.append(f"subset {mask:06b}: losses differ between gradients all and {mode}")
        for k in present[::2]:
            if res["alt"]["grads"][k].tobytes() != res["all"]["grads"][k].tobytes():
                bad.append(f"subset {mask:06b}: g_{k} differs between gradients all and alt")
        if again["losses"].tobytes() != res["all"]["losses"].tobytes() or any(again["grads"][k].tobytes() != res["all"]["grads"][k].tobytes() for k in present):
            bad.append(f"subset {mask:06b}: a second call gives other bits")
        for i, k in enumerate(lr.KEYS):
            if k not in present and res["all"]["losses"][i] != 0:
                bad.append(f"subset {mask:06b}: absent term {k} = {res['all']['losses'][i]}")
        if res["all"]["losses"][7] != 0:
            bad.append(f"subset {mask:06b}: losses_out[7] = {res['all']['losses'][7]}")
    assert not bad, "\n".join(bad[:40])


def test_losses_targets_may_be_null(dev):
    """a NULL target switches its terms off like a NULL map (rgb_gt, depth_gt; the label targets must come with their maps)"""
    case = next(c for c in CASES if c["id"] == "Redge-257")
    maps, tg = lr.loss_inputs(case)
    for drop in ("rgb", "depth"):
        t = {k: v for k, v in tg.items() if k != drop}
        got, bad = run_losses(dev, maps, t, case["C"], case["K"], want=[k for k in maps if k != drop])
        ref = lr.losses64({k: v for k, v in maps.items() if k != drop}, t, lr.WEIGHTS, case["C"], case["K"])
        assert not bad + lr.violations(got, ref, exact=True) and got["losses"][lr.KEYS.index(drop)] == 0, drop


# -------------------------------------------------------------------------------------------------------------- pnr_ce3d
def run_ce3d(dev, x, lab, fc):
    """pnr_ce3d on a channel-major buffer with a padded stride (S + 24), NaN in the padding and in every channel outside
    [fc, fc + n): a finite result never read them"""
    lib = _lib.load()
    S, n = x.shape
    sc = S + 24
    buf = np.full((fc + n + 3, sc), np.nan, np.float32)
    buf[fc:fc + n, :S] = x.T
    raw, label = torch.tensor(buf).to(dev), torch.tensor(lab).to(dev)
    out = _Guarded(dev, (2,))
    ws = _Guarded(dev, (int(lib.pnr_ce3d_workspace_bytes(S)),), torch.uint8)
    _lib.check(lib.pnr_ce3d(_p(raw), sc, int(fc), int(n), _p(label), S, _p(out.view), _p(ws.view),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pnr_ce3d")
    torch.cuda.synchronize()
    bad = [f"guard of {k} touched" for k, b in (("out2", out), ("workspace", ws)) if not b.guards_intact()]
    return out.numpy(), bad


def _run_ce3d_group(dev, pick):
    bad = []
    for case in CE3D_CASES:
        if not pick(case):
            continue
        x, lab = lr.ce3d_inputs(case)
        got, b = run_ce3d(dev, x, lab, case["fc"])
        ref = lr.ce3d64(x.T, 0, case["n"], lab)
        b += lr.ce3d_violations(got[0], got[1], ref)
        if got[1] != np.float32(ref["count"]) or (ref["count"] == 0 and got[0] != 0):
            b.append(f"(mean, count) = {got}")
        if ref["count"]:
            _WORST["ce3d_mean"] = max(_WORST.get("ce3d_mean", 0.0), abs(float(got[0]) - ref["mean"]) / ref["bound"])
        if ref["count"] == 1:
            _WORST["ce3d_ray"] = max(_WORST.get("ce3d_ray", 0.0), abs(float(got[0]) - ref["mean"]) / ref["unit"].sum())
        bad += [f"{case['id']}: {v}" for v in b]
    assert not bad, "\n".join(bad[:40])


def test_ce3d_every_class_count(dev):
    """n = 1 .. 130 at S = 1000, first_channel 0, 4 and 4 + n"""
    _run_ce3d_group(dev, lambda c: c["group"] == "sweep")


def test_ce3d_sample_counts(dev):
    """S = 1, 63 .. 65, 255 .. 257, 64 * 256 + 1 (65 partials), 3 * 64 * 256 + 5 (four trips of the final's lane loop)"""
    _run_ce3d_group(dev, lambda c: c["group"] == "S")


def test_ce3d_one_labelled_sample_and_row_shapes(dev):
    """one labelled sample among unlabelled ones (the mean is its value); rows ascending (the rescale branch at every step),
    descending (never), all equal"""
    _run_ce3d_group(dev, lambda c: c["group"] in ("one", "rows"))


def test_ce3d_shift_invariance_and_labels(dev):
    """the offsets of the loss cases; labels -1, -7, n, n + 5, 255, INT_MAX, INT_MIN; no labelled sample gives (0, 0)"""
    _run_ce3d_group(dev, lambda c: c["group"] in ("shift", "labels"))
