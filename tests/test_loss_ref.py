"""CPU checks of the float64 loss reference (tests/_loss_ref.py) that tests/test_gpu_loss_sweep.py compares pnr_losses and pnr_ce3d
with: hand-made answers, agreement with the torch oracle in float64 (autograd) and with finite differences, corrupted variants
that must leave the bounds, and the float32 restatements, which must sit at no more than a quarter of every bound."""
import math

import numpy as np
import pytest
import torch

import _loss_ref as lr
from oracle import torch_oracle as to

W32 = {k: float(np.float32(v)) for k, v in lr.WEIGHTS.items()}
EPS32 = float(np.float32(lr.FIX_EPS))
CASES = lr.loss_cases()
CE3D_CASES = lr.ce3d_cases()
BY_ID = {c["id"]: c for c in CASES}


def _ref(case, **kw):
    maps, tg = lr.loss_inputs(case)
    return maps, tg, lr.losses64(maps, tg, lr.WEIGHTS, case["C"], case["K"], case["l2"], lr.FIX_EPS, case["prob"], **kw)


def _torch(case, maps, tg, dtype):
    """the torch oracle's graph with autograd -> {losses, grads} in _loss_ref's layout"""
    leaf = {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in maps.items()}
    t = {k: torch.tensor(v) if v.dtype == np.int32 else torch.tensor(v).to(dtype) for k, v in tg.items()}
    terms, total = to.losses(leaf, t, W32, case["C"], case["K"], case["l2"], EPS32, case["prob"])
    if isinstance(total, torch.Tensor) and total.requires_grad:
        total.backward()
    out = np.zeros(8)
    for i, k in enumerate(lr.KEYS):
        if k in terms:
            out[i] = float(terms[k].detach())
    out[6] = float(total.detach()) if isinstance(total, torch.Tensor) else float(total)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in leaf.items()}
    return {"losses": out, "grads": grads}


# --------------------------------------------------------------------------------------------------------- closed forms
def test_case_list_covers_what_the_sweep_promises():
    sweep = [c for c in CASES if c["group"] == "sweep"]
    assert {(c["C"], c["l2"], c["prob"]) for c in sweep} == {(C, a, b) for C in range(1, 131) for a in (0, 1) for b in (0, 1)}
    assert {c["K"] for c in sweep} == {0, 1, 15, 16, 17, 33}
    assert {c["R"] for c in CASES if c["group"] == "smallR"} == set(range(1, 18))
    assert lr.R_BIG >= 3 * 1024 * 256 and -(-(-(-4097 // 16)) // 64) >= 3
    assert len({c["id"] for c in CASES}) == len(CASES) and len({c["id"] for c in CE3D_CASES}) == len(CE3D_CASES)
    assert {c["n"] for c in CE3D_CASES if c["group"] == "sweep"} == set(range(1, 131))
    # the offsets are exact in float32 on the logit grid: the shifted row IS the row plus the offset
    x, _ = lr.ce3d_inputs(next(c for c in CE3D_CASES if c["id"] == "shift30000-n45"))
    x0, _ = lr.ce3d_inputs(dict(next(c for c in CE3D_CASES if c["id"] == "shift30000-n45"), offset=None))
    assert np.array_equal(x.astype(np.float64) - 3e4, x0.astype(np.float64))
    assert np.float32(np.float32(1) - np.float32(lr.FIX_EPS)) + np.float32(lr.FIX_EPS) == np.float32(1)     # the planted p


@pytest.mark.parametrize("C", [1, 2, 16, 17, 45, 130])
def test_uniform_logits_give_log_C(C):
    R = 5
    ref = lr.losses64({"semantic": np.full((R, C), 3.25, np.float32)}, {"semantic": np.arange(R, dtype=np.int32) % C},
                      {"semantic": 1.0}, C, 0)
    assert np.allclose(ref["per_ray"]["semantic"], math.log(C), atol=1e-14) and abs(ref["losses"][2] - math.log(C)) < 1e-14
    assert ref["counts"]["semantic"] == R and (C > 1 or (ref["losses"][2] == 0 and np.all(ref["grads"]["semantic"] == 0)))
    c3 = lr.ce3d64(np.full((C + 2, R), 3.25), 1, C, np.arange(R) % C)
    assert abs(c3["mean"] - math.log(C)) < 1e-14 and c3["count"] == R


def test_probability_maps_closed_forms():
    C, eps = 4, EPS32
    p = np.zeros((3, C), np.float32)
    p[0, 2] = 1.0                                         # one-hot on the label: -log(1 + eps)
    p[1, 3] = 1.0                                         # zero probability on the label (1): -log(eps)
    lab = np.array([2, 1, -1], np.int32)
    for key in ("fix_semantic", "semantic"):
        ref = lr.losses64({key: p}, {"semantic": lab}, {key: 0.5}, C, 0, maps_are_prob=True)
        assert np.allclose(ref["per_ray"][key], [-math.log(1 + eps), -math.log(eps), 0.0], atol=1e-15)
        g = np.zeros((3, C))
        g[0, 2], g[1, 1] = -0.5 / ((1 + eps) * 2), -0.5 / (eps * 2)
        assert np.allclose(ref["grads"][key], g, rtol=1e-14, atol=0) and ref["counts"]["semantic"] == 2
    ki = lr.losses64({"fix_instance": p}, {"instance": lab}, {"fix_instance": 0.5}, 0, C)
    assert np.array_equal(ki["per_ray"]["fix_instance"], ref["per_ray"]["semantic"]) and ki["losses"][5] == ref["losses"][2]


def test_depth_and_counts_on_hand_written_targets():
    d = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], np.float32)
    gt = np.array([1.0, 4.0, 0.0, -0.0, -2.0, np.nan, 6.5], np.float32)
    sem = np.array([0, -1, 3, 2, 255, lr.INT_MIN, lr.INT_MAX], np.int32)
    inst = np.array([-7, 0, 1, 2, 1, 0, 5], np.int32)
    maps = {"depth": d, "semantic": np.zeros((7, 3), np.float32), "instance": np.zeros((7, 2), np.float32)}
    ref = lr.losses64(maps, {"depth": gt, "semantic": sem, "instance": inst}, {"depth": 0.5, "semantic": 1, "instance": 1}, 3, 2)
    assert ref["counts"] == {"depth": 3, "semantic": 2, "instance": 4}
    assert np.array_equal(ref["grads"]["depth"], [0, -0.5 / 3, 0, 0, 0, 0, 0.5 / 3])       # depth == depth_gt: gradient 0
    assert ref["losses"][1] == (0 + 2 + 0.5) / 3
    l2 = lr.losses64(maps, {"depth": gt}, {"depth": 0.5}, 0, 0, depth_l2=True)
    assert l2["losses"][1] == (0 + 4 + 0.25) / 3 and np.allclose(l2["grads"]["depth"], [0, -2 / 3, 0, 0, 0, 0, 0.5 / 3])
    assert np.array_equal(np.nonzero(ref["per_ray"]["semantic"])[0], [0, 3]) and ref["n"]["instance"] == 4
    bits = ref["exact"]["depth"][1]
    assert bits.dtype == np.float32 and bits[1] == -(np.float32(0.5) / np.float32(3)) and bits[6] == np.float32(0.5) / np.float32(3)


def test_all_ignored_gives_zero_terms_zero_gradients_zero_counts():
    for cid in ("nolabel", "nodepth"):
        maps, tg, ref = _ref(BY_ID[cid])
        keys = ("semantic", "fix_semantic", "instance", "fix_instance") if cid == "nolabel" else ("depth",)
        for k in keys:
            assert ref["losses"][lr.KEYS.index(k)] == 0 and not ref["grads"][k].any() and not ref["per_ray"][k].any(), (cid, k)
        assert ref["counts"]["depth" if cid == "nodepth" else "semantic"] == 0
        assert cid == "nodepth" or ref["counts"]["instance"] == 0
    x, lab = lr.ce3d_inputs(next(c for c in CE3D_CASES if c["id"] == "nolabel"))
    c3 = lr.ce3d64(x.T, 0, x.shape[1], lab)
    assert c3["mean"] == 0 and c3["count"] == 0 and lr.ce3d32(x, lab)[:2] == (0.0, 0)


# ------------------------------------------------------------------------------------------- independent restatements
def test_losses64_equals_the_torch_oracle_in_float64():
    for case in CASES:
        if case["group"] in ("sweep", "shiftmix") and case["C"] % 5 and case["C"] not in (1, 16, 17, 33, 64, 130):
            continue                                     # every fifth class count and the lane boundaries: the formulas do not depend on C
        maps, tg, ref = _ref(case)
        got = _torch(case, maps, tg, torch.float64)
        assert np.allclose(got["losses"], ref["losses"], rtol=1e-12, atol=1e-12), case["id"]
        for k, g in got["grads"].items():
            assert np.allclose(g, ref["grads"][k], rtol=1e-12, atol=1e-14), (case["id"], k)


def test_ce3d64_equals_the_torch_oracle_in_float64():
    for case in CE3D_CASES:
        x, lab = lr.ce3d_inputs(case)
        ref = lr.ce3d64(x.T, 0, case["n"], lab)
        ce, cnt = to.ce3d(torch.tensor(x).double(), torch.tensor(lab))
        assert cnt == ref["count"] and abs(float(ce) - ref["mean"]) <= 1e-12 * max(1.0, abs(ref["mean"])), case["id"]
    # channel offset and padded stride: only [first_channel, +n) x [0, S) is read
    x, lab = lr.ce3d_inputs(CE3D_CASES[5])
    n = x.shape[1]
    buf = np.full((4 + n + 3, len(lab) + 24), np.nan, np.float32)
    buf[4:4 + n, :len(lab)] = x.T
    assert lr.ce3d64(buf, 4, n, lab)["mean"] == lr.ce3d64(x.T, 0, n, lab)["mean"]


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("prob", [False, True])
def test_losses64_gradients_pass_central_differences(l2, prob):
    case = dict(id=f"fd-{l2}-{prob}", R=6, C=4, K=3, l2=l2, prob=prob, offset=None, edge=None)
    maps, tg = lr.loss_inputs(case)
    tg["semantic"][:3], tg["instance"][:3] = [0, -1, 4], [2, 7, -3]
    maps = {k: v.astype(np.float64) for k, v in maps.items()}
    f = lambda m: lr.losses64(m, tg, lr.WEIGHTS, 4, 3, l2, lr.FIX_EPS, prob)     # noqa: E731
    ref = f(maps)
    h = 1e-6
    for k, v in maps.items():
        fd = np.zeros_like(v)
        for i in np.ndindex(v.shape):
            up, dn = {**maps, k: v.copy()}, {**maps, k: v.copy()}
            up[k][i] += h
            dn[k][i] -= h
            fd[i] = (f(up)["losses"][6] - f(dn)["losses"][6]) / (2 * h)
        assert np.allclose(fd, ref["grads"][k], rtol=1e-6, atol=1e-8), k


# ------------------------------------------------------------------------------------------------- corrupted variants
def _clean(ref):
    return {"losses": ref["losses"].copy(), "grads": {k: v.copy() for k, v in ref["grads"].items()},
            "per_ray": {k: v.copy() for k, v in ref["per_ray"].items()}}


def _recount(got, ref, key_pair, n_new):
    """what a kernel that counted n_new rays where the contract counts n returns: every mean and gradient of the field scales"""
    for k in key_pair:
        s = ref["n"][k] / n_new
        got["losses"][lr.KEYS.index(k)] *= s
        got["grads"][k] *= s
    got["losses"][6] = sum(W32[k] * got["losses"][i] for i, k in enumerate(lr.KEYS))
    return got


def _corrupt(name):
    case = BY_ID["edge-l20-p0"]
    maps, tg, ref = _ref(case)
    got = _clean(ref)
    R, C = case["R"], case["C"]
    if name == "mean_over_R":
        return _recount(got, ref, ("semantic", "fix_semantic"), R), ref
    if name == "gradient_without_1_over_n":
        got["grads"]["semantic"] *= ref["n"]["semantic"]
        return got, ref
    if name == "label_C_counted":
        return _recount(got, ref, ("semantic", "fix_semantic"), ref["n"]["semantic"] + int((tg["semantic"] == C).sum())), ref
    if name == "depth_gt_le_0_counted":
        return _recount(got, ref, ("depth",), ref["n"]["depth"] + int((tg["depth"] <= 0).sum())), ref
    if name == "classes_from_16_dropped":
        short = lr.losses64({"semantic": maps["semantic"][:, :16]}, {"semantic": np.where(tg["semantic"] < 16, tg["semantic"], -1)},
                            lr.WEIGHTS, 16, 0)
        low = (tg["semantic"] >= 0) & (tg["semantic"] < 16)           # rays whose label a 16-lane group without its stride loop still sees
        s = short["n"]["semantic"] / ref["n"]["semantic"]
        got["grads"]["semantic"][low, :16] = short["grads"]["semantic"][low] * s
        got["grads"]["semantic"][low, 16:] = 0
        got["per_ray"]["semantic"][low] = short["per_ray"]["semantic"][low]
        return got, ref
    if name == "ce_rounded_at_mx":
        case = BY_ID["shift1000-C45-R157"]
        maps, tg, ref = _ref(case)
        got = lr.losses32(maps, tg, lr.WEIGHTS, case["C"], case["K"], reassoc=False)
        return got, ref
    raise KeyError(name)


CORRUPT = {"mean_over_R": "mean:semantic", "gradient_without_1_over_n": "ce_grad:semantic", "label_C_counted": "mean:semantic",
           "depth_gt_le_0_counted": "mean:depth", "classes_from_16_dropped": "ce_grad:semantic", "ce_rounded_at_mx": "ce_ray:semantic"}


@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_corrupted_variants_leave_the_bounds(name):
    got, ref = _corrupt(name)
    bad = lr.violations(got, ref, exact=True)
    assert any(b.startswith(CORRUPT[name]) for b in bad), (name, bad)
    assert lr.violations(_clean(ref), ref, exact=False) == []


def test_ce_rounded_at_mx_is_caught_per_ray_and_by_ce3d_and_reassociated_is_not():
    """(mx + log den) - x_label on rows offset by 1000 errs by up to |mx| 2^-25 = 3e-5 (1e-3 at 30000); the shift-invariant
    bound is a few 1e-6.  Per ray it is caught in every shifted case; through the means, all a kernel returns, at R = 1, 2."""
    by_mean = {1e3: [], -1e3: [], 3e4: []}
    for case in (c for c in CASES if c["group"] == "shift" and c["offset"] in by_mean and c["C"] > 1):
        maps, tg, ref = _ref(case)
        bad = lr.violations(lr.losses32(maps, tg, lr.WEIGHTS, case["C"], case["K"], reassoc=False), ref, exact=True)
        assert case["R"] <= 2 or any(b.startswith("ce_ray:semantic") for b in bad), (case["id"], bad)
        if case["R"] <= 2 and ref["counts"]["semantic"]:
            by_mean[case["offset"]].append(any(b.startswith("mean:semantic") for b in bad))
    assert all(by_mean[3e4]) and len(by_mean[3e4]) >= 5, by_mean
    assert sum(by_mean[1e3]) + sum(by_mean[-1e3]) >= (len(by_mean[1e3]) + len(by_mean[-1e3])) // 2, by_mean
    for c in (c for c in CE3D_CASES if c["group"] == "shift" and c["offset"] in by_mean and c["n"] > 1):
        x, lab = lr.ce3d_inputs(c)
        r = lr.ce3d64(x.T, 0, c["n"], lab)
        mean, cnt, ps = lr.ce3d32(x, lab, reassoc=False)
        assert c["labels"] == "one" or (np.abs(ps - r["per_sample"]) > lr.K["ce3d_ray"] * r["unit"]).any(), c["id"]
        assert c["offset"] != 3e4 or c["labels"] != "one" or lr.ce3d_violations(mean, cnt, r) != [], c["id"]


# ------------------------------------------------------------------------------------------- the float32 restatements
@pytest.fixture(scope="module")
def f32_pass():
    """one pass over every case: rho per quantity (the worst error / (u * cond) of the float32 restatements and of the float32
    torch graph against float64) and every violation of a quarter of a bound"""
    rho, bad = {}, []
    for case in CASES:
        maps, tg, ref = _ref(case)
        for got, exact in ((lr.losses32(maps, tg, lr.WEIGHTS, case["C"], case["K"], case["l2"], lr.FIX_EPS, case["prob"]), True),
                           (_torch(case, maps, tg, torch.float32), False)):
            lr.worst(got, ref, rho, exact=exact)
            bad += [f"{case['id']}: {b}" for b in lr.violations(got, ref, exact=exact, scale=0.25)]
    rho["ce3d_ray"] = rho["ce3d_mean"] = 0.0
    for case in CE3D_CASES:
        x, lab = lr.ce3d_inputs(case)
        ref = lr.ce3d64(x.T, 0, case["n"], lab)
        mean, cnt, ps = lr.ce3d32(x, lab)
        ce, n = to.ce3d(torch.tensor(x), torch.tensor(lab))
        err = np.abs(ps - ref["per_sample"])
        with np.errstate(all="ignore"):
            rho["ce3d_ray"] = max(rho["ce3d_ray"], float(np.where(err == 0, 0.0, err / ref["unit"]).max()))
        for m, c in ((mean, cnt), (float(ce), n)):
            if ref["count"]:
                rho["ce3d_mean"] = max(rho["ce3d_mean"], abs(float(m) - ref["mean"]) / ref["bound"])
            bad += [f"ce3d {case['id']}: {b}" for b in lr.ce3d_violations(m, c, ref, scale=0.25)]
        if not (err <= 0.25 * lr.K["ce3d_ray"] * ref["unit"]).all():
            bad.append(f"ce3d {case['id']}: per-sample value outside a quarter of its bound")
    return rho, bad


def test_float32_restatements_sit_at_a_quarter_of_the_bounds(f32_pass):
    assert f32_pass[1] == []


def test_k_is_four_times_the_float32_ratio(f32_pass):
    rho = f32_pass[0]
    print({q: round(v, 3) for q, v in sorted(rho.items())})
    for q, k in lr.K.items():
        assert k == max(4, math.ceil(4 * rho[q])), (q, k, rho[q])
    assert rho["mean"] <= 0.25 and rho["total"] <= 0.25 and rho["ce3d_mean"] <= 0.25 and rho.get("absent", 0) == 0 and rho.get("exact", 0) == 0
