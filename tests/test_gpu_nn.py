"""The nearest-neighbour search on an MI355X: k_nn_count / k_nn_fill / k_nn_query and the shared scan (csrc/pnr_nn.hip,
csrc/pnr_scan_dev.h) against tests/_nn_ref.py's brute force over all n (include/pnr.h "nearest neighbours").  index and dist2 are
an integer and a float32 word that must be EQUAL to the restatement's; so must the table's start and every bucket's multiset of
records.  Outputs are interior views of a guarded arena.  tests/test_nn_host.py pins the restatement on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _nn_ref as nr
from _arena import Arena
from panopticnerf_amd import ops, pointcloud

pytestmark = pytest.mark.gpu

NS_ = (1, 2, 63, 64, 65, 255, 257, 1000, 4133)
MS_ = (1, 64, 65, 1000)
BITS = (4, None)


def N_(t):
    return t.detach().cpu().numpy()


def G(a, dev):
    """a device copy of a (read-only) numpy array"""
    return torch.from_numpy(np.array(a)).to(dev)


@functools.lru_cache(maxsize=None)
def case(n, m, offset, D):
    """(ref, q, brute-force index, dist2, stats): computed once, shared by the tests, never written"""
    ref, q = nr.adversarial(n, m, offset, D)
    out = (ref, q) + nr.brute(q, ref, D)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def pad4(k):
    return (k + 3) // 4 * 4


def run_in_arena(dev, ref, q, D, bits):
    """build + query with start, records, index, dist2 as interior views of one guarded arena; returns numpy copies + stats"""
    n, m = ref.shape[0], q.shape[0]
    _, T = ops.nn_params("test", D, n, bits)
    arena = Arena(dev, [("start", pad4(T + 1), 64), ("records", pad4(4 * n), 64), ("index", pad4(m), 64), ("dist2", pad4(m), 64)])
    start = arena.view("start")[: T + 1].view(torch.int32)
    records = arena.view("records")[: 4 * n].view(n, 4)
    index = arena.view("index")[:m].view(torch.int32)
    dist2 = arena.view("dist2")[:m]
    assert records.data_ptr() % 16 == 0
    stats = torch.zeros(3, device=dev, dtype=torch.int64)
    ref_d, q_d = G(ref, dev), G(q, dev)
    s2, r2 = ops.nn_build(ref_d, D, bits, start=start, records=records)
    assert s2 is start and r2 is records
    i2, d2 = ops.nn_query(ref_d, start, records, q_d, D, index=index, dist2=dist2, stats=stats)
    assert i2 is index and d2 is dist2
    torch.cuda.synchronize()
    assert arena.guards_intact()
    return N_(start), N_(records), N_(index), N_(dist2), N_(stats).tolist(), T


def check_table(ref, D, T, start, records):
    """start is the restatement's, and every bucket holds the restatement's multiset of records"""
    b_ref, start_ref = nr.table(ref, D, T)
    assert np.array_equal(start, start_ref)
    k = int(start[-1])
    assert k == int((b_ref >= 0).sum())
    j = records[:k, 3].copy().view(np.int32).astype(np.int64)
    assert np.array_equal(np.sort(j), np.nonzero(b_ref >= 0)[0])                 # every finite point once, no other
    at = np.searchsorted(start, np.arange(k), side="right") - 1                  # the bucket each record lies in
    assert np.array_equal(b_ref[j], at)
    assert np.array_equal(records[:k, :3].view(np.uint32), ref[j].view(np.uint32))


@pytest.mark.parametrize("offset,D", nr.OFFSETS_D)
@pytest.mark.parametrize("n", NS_)
def test_query_is_brute_force(dev, n, offset, D):
    for m in MS_:
        ref, q, bi, bd, bstats = case(n, m, offset, D)
        for bits in BITS:
            start, records, index, dist2, stats, T = run_in_arena(dev, ref, q, D, bits)
            tag = "n %d m %d offset %g D %g T %d" % (n, m, offset, D, T)
            assert np.array_equal(index, bi), tag
            assert np.array_equal(dist2.view(np.uint32), bd.view(np.uint32)), tag
            assert stats == bstats, tag
            check_table(ref, D, T, start, records)
            if n >= 255 and m >= 64:            # neither branch is vacuous
                share = stats[0] / (stats[0] + stats[1])
                assert 0.10 <= share <= 0.90, (tag, share)
                if offset == 0:
                    assert (dist2 == np.float32(D) * np.float32(D)).any() and ((index >= 0) & (index < 50)).any(), tag


def test_one_long_bucket(dev):
    """every point in one cell: one bucket holds the whole cloud"""
    rng = np.random.default_rng(5)
    ref = (10.0 + rng.uniform(0, 0.01, size=(700, 3))).astype(np.float32)
    ref[0] = 10.0                                       # the origin is the cluster's corner, and the cell is 0.024 wide
    q = (10.0 + rng.uniform(-0.02, 0.03, size=(300, 3))).astype(np.float32)
    D = 0.012
    bi, bd, bstats = nr.brute(q, ref, D)
    assert 30 < bstats[0] < 270
    for bits in BITS:
        start, records, index, dist2, stats, T = run_in_arena(dev, ref, q, D, bits)
        assert np.diff(start).max() == 700
        assert np.array_equal(index, bi) and np.array_equal(dist2.view(np.uint32), bd.view(np.uint32)) and stats == bstats
        check_table(ref, D, T, start, records)


def test_empty_reference_and_empty_query(dev):
    q = G(case(64, 65, 0.0, 0.25)[1], dev)
    idx = pointcloud.NearestIndex(torch.zeros((0, 3), device=dev), 0.25)
    assert len(idx) == 0 and int(idx.start.abs().sum()) == 0 and idx.start.numel() == 1025
    stats = torch.zeros(3, device=dev, dtype=torch.int64)
    out = idx.query(q, stats=stats)
    assert (out["index"] == -1).all() and torch.isinf(out["dist2"]).all() and not out["valid"].any()
    assert stats.tolist() == [0, 64, 1]
    idx = pointcloud.NearestIndex(G(case(64, 65, 0.0, 0.25)[0], dev), 0.25)
    out = idx.query(torch.zeros((0, 3), device=dev))
    assert out["index"].shape == (0,) and out["dist2"].shape == (0,)


def test_second_build_and_query_is_identical(dev):
    ref, q, bi, bd, _ = case(4133, 1000, 7.0, 3.0)
    a = run_in_arena(dev, ref, q, 3.0, None)
    b = run_in_arena(dev, ref, q, 3.0, None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))
    assert a[4] == b[4]


def test_index_wrapper_and_dist(dev):
    ref, q, bi, bd, bstats = case(1000, 1000, 0.0, 0.25)
    idx = pointcloud.NearestIndex(G(ref, dev), 0.25, table_bits=6)
    assert idx.table_size == 64 and idx.records.shape == (1000, 4)
    out = idx.query(G(q, dev))
    assert np.array_equal(N_(out["index"]), bi) and np.array_equal(N_(out["valid"]), bi >= 0)
    np.testing.assert_allclose(N_(idx.dist(G(q, dev))), np.sqrt(bd), rtol=2.4e-7, atol=0)     # torch's sqrt: 2 ulp
    with pytest.raises(ValueError, match="nn_query: query: tensor must be contiguous"):
        idx.query(torch.zeros((3, 8), device=dev).t())


def test_capture_build_and_query_then_replay_on_new_data(dev):
    """nn_build + nn_query captured as one chain on one stream; ref overwritten in place; the replay follows the data (the cell
    origin is read from ref[0] on the device)"""
    D = 0.5
    ref_a, q, _, _, _ = case(1000, 1000, -1e5, D)
    ref_b = np.ascontiguousarray(case(1000, 65, 3000.0, D)[0] - np.float32(3000.0) - np.float32(1e5)).astype(np.float32)
    ref_d, q_d = G(ref_a, dev), G(q, dev)
    T = ops.nn_params("test", D, 1000)[1]
    start = torch.empty(T + 1, device=dev, dtype=torch.int32)
    records = torch.empty((1000, 4), device=dev, dtype=torch.float32)
    index = torch.empty(1000, device=dev, dtype=torch.int32)
    dist2 = torch.empty(1000, device=dev, dtype=torch.float32)
    stats = torch.zeros(3, device=dev, dtype=torch.int64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # one warm-up outside the capture
        ops.nn_build(ref_d, D, start=start, records=records)
        ops.nn_query(ref_d, start, records, q_d, D, index=index, dist2=dist2, stats=stats)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.nn_build(ref_d, D, start=start, records=records)
        ops.nn_query(ref_d, start, records, q_d, D, index=index, dist2=dist2, stats=stats)
    g.replay()
    torch.cuda.synchronize()
    bi, bd, _ = nr.brute(q, ref_a, D)
    assert np.array_equal(N_(index), bi) and np.array_equal(N_(dist2).view(np.uint32), bd.view(np.uint32))
    ref_d.copy_(G(ref_b, dev))
    index.fill_(-5)
    stats.zero_()
    g.replay()
    torch.cuda.synchronize()
    got_i, got_d, got_s = N_(index), N_(dist2), stats.tolist()
    eager = pointcloud.NearestIndex(ref_d, D).query(q_d)
    bi, bd, bstats = nr.brute(q, ref_b, D)
    assert np.array_equal(got_i, N_(eager["index"])) and np.array_equal(got_d.view(np.uint32), N_(eager["dist2"]).view(np.uint32))
    assert np.array_equal(got_i, bi) and np.array_equal(got_d.view(np.uint32), bd.view(np.uint32)) and got_s == bstats
