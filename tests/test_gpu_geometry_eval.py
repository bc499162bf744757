"""The cloud metrics and Evaluator.evaluate_geometry on an MI355X: k_cloud_metrics (csrc/pnr_nn.hip) against tests/_nn_ref.py
(include/pnr.h "nearest neighbours", CLOUD METRICS).  Counts are integers and must be EQUAL.  The sums are at most 10^4
non-negative float64 terms added in another order than math.fsum: every partial sum is at most the total S and each of the
m - 1 additions rounds by at most 2^-53 of it, so |sum - fsum| <= m 2^-53 S -- for m <= 10^4 a relative 1.2e-12, asserted as
1e-12 (the issue's bound; the tests print the share of it used).  The terms themselves are equal on both sides: the square root of
a float32 in double is correctly rounded in numpy and in the kernel.  On inputs whose roots are exact the sums also equal
_reduce_ref's restatement of the kernel's order of additions bit for bit."""
import math

import numpy as np
import pytest
import torch

import _nn_ref as nr
import _reduce_ref as rr
from panopticnerf_amd import ops, pointcloud
from panopticnerf_amd.evaluate import Evaluator

pytestmark = pytest.mark.gpu

REL = 1e-12
D = 0.25
TAUS = (0.05, 0.1, 0.25)


def N_(t):
    return t.detach().cpu().numpy()


def G(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def close(got, want, what=""):
    if want == 0 or not math.isfinite(want):
        assert got == want or (math.isnan(got) and math.isnan(want)), (what, got, want)
        return
    rel = abs(got - want) / abs(want)
    print("%s: %.3g of the bound" % (what, rel / REL))
    assert rel <= REL, (what, got, want)


def clouds(seed=0, n=1800, m=1500):
    rng, m = np.random.default_rng(seed), min(m, n)
    a = rng.uniform(-4, 4, size=(n, 3)).astype(np.float32)
    b = (a[:m] + rng.normal(size=(m, 3)).astype(np.float32) * np.float32(0.15)).astype(np.float32)
    b[7], a[11] = np.nan, np.inf
    return a, b


def test_cloud_metrics_counts_and_sums(dev):
    ref, q = clouds()
    index, dist2, stats = nr.brute(q, ref, D)
    assert 100 < stats[1] < 1000 and stats[2] == 1
    want_s, want_c = nr.cloud_metrics(index, dist2, D, TAUS, query=q)
    assert want_c[0] == len(q) - 1 and 0 < want_c[2] < want_c[3] < want_c[4] == stats[0]
    i_d, d_d, q_d = G(index, dev), G(dist2, dev), G(q, dev)
    sums, counts = ops.cloud_metrics(i_d, d_d, D, TAUS, query=q_d)
    assert counts.tolist() == want_c + [0] * (10 - len(want_c))
    close(float(sums[0]), want_s[0], "sum d")
    close(float(sums[1]), want_s[1], "sum d^2")
    sums2, counts2 = ops.cloud_metrics(i_d, d_d, D, TAUS, query=q_d)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)) and torch.equal(counts, counts2)       # to the bit
    # without the queries every row counts: the invalid one as a point without a neighbour
    want_s, want_c = nr.cloud_metrics(index, dist2, D, TAUS)
    assert want_c[0] == len(q)
    sums3, counts3 = ops.cloud_metrics(i_d, d_d, D, TAUS)
    assert counts3.tolist()[:5] == want_c
    close(float(sums3[0]), want_s[0], "sum d, all rows")
    # a NaN dist2 never counts; accumulation into caller-owned arrays
    d_nan = d_d.clone()
    d_nan[:3] = float("nan")
    want_s, want_c = nr.cloud_metrics(index, N_(d_nan), D, TAUS, query=q)
    ops.cloud_metrics(i_d, d_nan, D, TAUS, query=q_d, sums=sums, counts=counts)
    assert counts.tolist()[:5] == [a + b for a, b in zip(want_c, nr.cloud_metrics(index, dist2, D, TAUS, query=q)[1])]
    first_s = nr.cloud_metrics(index, dist2, D, TAUS, query=q)[0]
    close(float(sums[0]), math.fsum([want_s[0], first_s[0]]), "sum d, accumulated")
    close(float(sums[1]), math.fsum([want_s[1], first_s[1]]), "sum d^2, accumulated")


# 1 .. 1000: one lane, a wave less one, a wave, two waves, a block less one, a block, two blocks, four; then a second trip
ORDER_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, "second trip")


@pytest.mark.parametrize("m", ORDER_SIZES)
def test_cloud_metrics_sums_in_the_stated_order_to_the_bit(dev, m):
    """both sums equal _reduce_ref's restatement of the order (a thread's stride order, the butterfly, the four waves, the rows
    in block order) bit for bit, for the grid the entry point derives from the device; "second trip": just past 256 x the full
    grid + 1, so threads add a second item.  dist2 holds squares of k 2^e, k < 2^12: exact in float32 with an exact root, so any
    faithful sqrt returns k 2^e and the test pins the order, not the libm; e spans 44 binades, so the additions round and
    another order gives other bits (asserted on the reference side).  Rows without a neighbour add max_dist, rows with a NaN
    dist2 or a non-finite query add nothing.  Accumulating into given sums is old + new to the bit."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if m == "second trip":
        m = 256 * min(1024, 4 * cus) + 77
    grid = rr.blocks_for(m, 1024, cus, 4)
    rng = np.random.default_rng(m)
    root = np.ldexp(rng.integers(1, 4096, m).astype(np.float32), rng.integers(-50, -6, m)).astype(np.float32)
    dist2 = root * root
    assert np.array_equal(dist2.astype(np.float64), root.astype(np.float64) ** 2) and np.array_equal(np.sqrt(dist2.astype(np.float64)), root.astype(np.float64))
    index = rng.integers(0, 1000, m).astype(np.int32)
    q = rng.uniform(-4, 4, size=(m, 3)).astype(np.float32)
    if m > 1:
        lost, nan, bad = (rng.choice(m, max(m // 7, 1), replace=False) for _ in range(3))
        index[lost], dist2[lost] = -1, np.inf
        dist2[nan] = np.nan
        q[bad, rng.integers(0, 3, bad.size)] = np.resize(np.float32([np.nan, np.inf, -np.inf]), bad.size)
    max_dist = 1.7
    active = ~np.isnan(dist2) & nr.finite_rows(q)
    d = np.where(index >= 0, root.astype(np.float64), np.float64(np.float32(max_dist)))
    terms = np.where(active[:, None], np.stack([d, d * d], -1), 0.0)
    want = rr.total(terms, active, grid)
    if m > 1000:
        assert (want != rr.total(terms[::-1], active[::-1], grid)).all(), "the data do not tell two orders apart"
    i_d, d_d, q_d = G(index, dev), G(dist2, dev), G(q, dev)
    sums, counts = ops.cloud_metrics(i_d, d_d, max_dist, query=q_d)
    assert counts.tolist()[:2] == [int(active.sum()), int((active & (index < 0)).sum())] and active.any()
    assert np.array_equal(N_(sums).view(np.uint64), want.view(np.uint64)), (m, grid, N_(sums), want)
    old = torch.tensor([1e6 / 3.0, 0.1], dtype=torch.float64, device=dev)
    acc, acc_c = ops.cloud_metrics(i_d, d_d, max_dist, query=q_d, sums=old.clone(), counts=counts.clone())
    assert np.array_equal(N_(acc).view(np.uint64), (N_(old) + want).view(np.uint64)) and torch.equal(acc_c, 2 * counts)


def test_sqrt_of_a_float32_in_double_is_the_same_on_both_sides(dev):
    """one row per launch: sums[0] is then the kernel's own sqrt((double) dist2), which must be numpy's correctly rounded one"""
    rng = np.random.default_rng(3)
    d2 = np.concatenate([rng.uniform(0, 1, 40).astype(np.float32) ** 3, np.float32([0.0, 1e-40, 1.0, 2.0, 3.0, 1e-30])])
    idx = torch.zeros(1, device=dev, dtype=torch.int32)
    for v in d2:
        sums, _ = ops.cloud_metrics(idx, G(np.float32([v]), dev), 2.0)
        assert float(sums[0]) == float(np.sqrt(np.float64(v))), v


def summary_ref(pred, gt, max_dist, taus):
    sides = []
    for q, ref in ((pred, gt), (gt, pred)):
        index, dist2, _ = nr.brute(q, ref, max_dist)
        sides.append(nr.cloud_metrics(index, dist2, max_dist, taus, query=q))
    return sides


def check_summary(got, sides, n_tau):
    want = nr.summarize(sides[0], sides[1], n_tau)
    assert set(k for k in got if k.startswith("geom_")) == set(want)
    for k, w in want.items():
        if isinstance(w, int):
            assert got[k] == w, k
        elif isinstance(w, list):
            assert len(got[k]) == len(w)
            for a, b in zip(got[k], w):
                close(a, b, k)
        else:
            close(got[k], w, k)


def test_identical_clouds(dev):
    a, _ = clouds(1, n=1500)
    ev = Evaluator()
    res = ev.evaluate_geometry(G(a, dev), G(a, dev), D, TAUS)
    assert set(res) == {"pred_to_gt", "gt_to_pred"}
    out = ev.summarize()
    assert out["geom_accuracy"] == 0 and out["geom_completeness"] == 0 and out["geom_chamfer"] == 0 and out["geom_accuracy_rms"] == 0
    assert out["geom_fscore"] == [1.0, 1.0, 1.0] and out["geom_n_pred"] == 1499 and out["geom_missing_pred"] == 0
    check_summary(out, summary_ref(a, a, D, TAUS), 3)


def test_disjoint_clouds(dev):
    a, _ = clouds(2, n=900)
    b = (a[100:800] + np.float32(10.0)).astype(np.float32)
    ev = Evaluator()
    ev.evaluate_geometry(G(a, dev), G(b, dev), D, TAUS)
    out = ev.summarize()
    d32 = float(np.float32(D))
    close(out["geom_accuracy"], d32, "accuracy")
    close(out["geom_completeness"], d32, "completeness")
    assert all(math.isnan(v) for v in out["geom_fscore"]) and out["geom_precision"] == [0.0] * 3
    assert out["geom_missing_pred"] == out["geom_n_pred"] == 899 and out["geom_missing_gt"] == out["geom_n_gt"] == 700
    check_summary(out, summary_ref(a, b, D, TAUS), 3)


def test_far_cluster_lowers_precision_only(dev):
    gt, _ = clouds(3, n=1200)
    gt = gt[np.isfinite(gt).all(axis=1)]
    pred = np.concatenate([gt, (gt[:300] + np.float32(20.0)).astype(np.float32)])
    ev = Evaluator()
    ev.evaluate_geometry(G(pred, dev), G(gt, dev), D, TAUS)
    out = ev.summarize()
    assert out["geom_recall"] == [1.0] * 3 and all(v == len(gt) / len(pred) for v in out["geom_precision"])
    assert out["geom_completeness"] == 0 and out["geom_accuracy"] > 0 and out["geom_missing_pred"] == 300
    check_summary(out, summary_ref(pred, gt, D, TAUS), 3)


def test_noisy_clouds_accumulation_and_reset(dev):
    gt, pred = clouds(4, n=1000, m=800)
    sides = summary_ref(pred, gt, D, TAUS)
    ev = Evaluator()
    ev.evaluate_geometry(G(pred, dev), G(gt, dev), D, TAUS)
    one = ev.summarize()
    check_summary(one, sides, 3)
    assert 0 < one["geom_precision"][0] < one["geom_precision"][2] < 1 and one["geom_missing_pred"] > 0
    assert ev.geom is None and "geom_accuracy" not in ev.summarize()               # the reset
    # two calls against one call on the concatenation: the counts exactly, the sums to the bound.  The halves are 50 apart,
    # so no point of one half has a neighbour in the other.
    far = np.float32(50.0)
    ev.evaluate_geometry(G(pred, dev), G(gt, dev), D, TAUS)
    ev.evaluate_geometry(G(pred + far, dev), G(gt + far, dev), D, TAUS)
    two = ev.summarize()
    ev.evaluate_geometry(G(np.concatenate([pred, pred + far]), dev), G(np.concatenate([gt, gt + far]), dev), D, TAUS)
    cat = ev.summarize()
    for k, w in cat.items():
        if isinstance(w, int):
            assert two[k] == w, k
        elif isinstance(w, list):
            for a, b in zip(two[k], w):
                close(a, b, k)
        else:
            close(two[k], w, k)
    check_summary(cat, summary_ref(np.concatenate([pred, pred + far]), np.concatenate([gt, gt + far]), D, TAUS), 3)


def test_a_later_call_with_other_settings_is_refused(dev):
    a, b = clouds(5, n=300, m=200)
    ev = Evaluator()
    ev.evaluate_geometry(G(b, dev), G(a, dev), D, TAUS)
    with pytest.raises(ValueError, match="Evaluator.evaluate_geometry: max_dist and thresholds .* differ"):
        ev.evaluate_geometry(G(b, dev), G(a, dev), 0.5, TAUS)
    with pytest.raises(ValueError, match="Evaluator.evaluate_geometry: max_dist and thresholds .* differ"):
        ev.evaluate_geometry(G(b, dev), G(a, dev), D, TAUS[:2])
    ev.evaluate_geometry(G(b, dev), G(a, dev), D, TAUS)                 # the same settings: accumulated
    assert ev.summarize()["geom_n_pred"] == 2 * 199
    ev.evaluate_geometry(G(b, dev), G(a, dev), 0.5, TAUS[:2])           # after summarize(): a fresh start
    assert len(ev.summarize()["geom_fscore"]) == 2


def test_nearest_transfers_labels_and_colours(dev):
    ref, q = clouds(6, n=1000, m=800)
    index, _, _ = nr.brute(q, ref, D)
    labels = np.arange(1000, dtype=np.int32) % 19
    colors = np.random.default_rng(0).uniform(size=(1000, 3)).astype(np.float32)
    out = pointcloud.nearest(G(q, dev), G(ref, dev), D, labels=G(labels, dev), colors=G(colors, dev))
    assert np.array_equal(N_(out["index"]), index) and (index < 0).any() and (index >= 0).any()
    assert np.array_equal(N_(out["label"]), np.where(index >= 0, labels[np.maximum(index, 0)], -1))
    assert np.array_equal(N_(out["rgb"]), np.where((index >= 0)[:, None], colors[np.maximum(index, 0)], 0))
    want = pointcloud.gather(G(labels, dev), out["index"], -1)
    assert torch.equal(out["label"], want)
