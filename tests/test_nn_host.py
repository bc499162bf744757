"""CPU tests of the nearest-neighbour feature (include/pnr.h "nearest neighbours"): the numpy restatement's hashed search equals
its brute force on the adversarial generator (this protects the rule itself), the sampler restatement's properties, and the
refusals of the entry points, the ops and the wrappers -- all before any launch, so none of it needs a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _nn_ref as nr
from panopticnerf_amd import _lib, mesh, ops, pointcloud
from panopticnerf_amd.evaluate import Evaluator


@pytest.mark.parametrize("offset,D", nr.OFFSETS_D)
@pytest.mark.parametrize("T", [16, 1024])
def test_hashed_search_equals_brute_force(offset, D, T):
    ref, q = nr.adversarial(1000, 400, offset, D)
    bi, bd, stats = nr.brute(q, ref, D)
    hi, hd, span = nr.hashed(q, ref, D, T)
    assert np.array_equal(bi, hi) and np.array_equal(bd.view(np.uint32), hd.view(np.uint32))
    assert span <= 1                                    # h = 2 Dp: the corners one cell apart (rounding can add to it, not on these inputs)
    share = stats[0] / (stats[0] + stats[1])
    print("offset %g D %g T %d: found %.3f, span %d" % (offset, D, T, share, span))
    assert 0.10 <= share <= 0.90 and stats[2] == 1
    if offset == 0:
        r2 = np.float32(D) * np.float32(D)
        assert (bd == r2).any() and ((bi >= 0) & (bi < 50)).any()
    # a non-finite reference point is never an answer
    bad = ~np.isfinite(ref).all(axis=1)
    assert bad.sum() == 2 and not np.isin(bi[bi >= 0], np.nonzero(bad)[0]).any()


def test_a_tie_goes_to_the_lowest_index():
    ref, q = nr.adversarial(400, 64, 0.0, 0.25)
    index, dist2, _ = nr.brute(ref[-50:], ref, 0.25)             # the repeated points, asked for themselves
    assert (dist2 == 0).all() and (index < 350).all() and np.array_equal(ref[index], ref[-50:])


def _triangles(F, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, size=(3 * F, 3)).astype(np.float32)
    return v, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def test_sampler_restatement_points_lie_in_their_triangles():
    v, f = _triangles(65, 3)
    pts, face = nr.sample(v, f, 40.0, seed=7)
    assert len(pts) > 65 and (np.diff(face) >= 0).all()
    p0, p1, p2 = (v[f[face, k]].astype(np.float64) for k in range(3))
    e1, e2, w = p1 - p0, p2 - p0, pts.astype(np.float64) - p0
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (w * e1).sum(1), (w * e2).sum(1)
    det = d11 * d22 - d12 * d12
    u, vv = (b1 * d22 - b2 * d12) / det, (b2 * d11 - b1 * d12) / det
    assert min(u.min(), vv.min(), (1 - u - vv).min()) >= -1e-6
    n = np.cross(e1, e2)
    assert (np.abs((w * n).sum(1)) / np.linalg.norm(n, axis=1)).max() < 1e-5      # and in its plane
    pts2, face2 = nr.sample(v, f, 40.0, seed=7)
    assert np.array_equal(pts, pts2) and np.array_equal(face, face2)
    assert not np.array_equal(nr.sample(v, f, 40.0, seed=8)[0][:50], pts[:50])


def test_sampler_restatement_count_is_unbiased():
    """2000 equal triangles of area 1/2 at rho = 1: rho * area = 0.5, so each holds a point with probability 1/2: the total is
    binomial(2000, 1/2), mean 1000 and sigma = sqrt(500); the bound is 5 sigma"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    v = np.concatenate([tri + np.float32(i) for i in range(2000)])
    f = np.arange(6000, dtype=np.int32).reshape(2000, 3)
    k = nr.sample_counts(v, f, 1.0, seed=11)[0]
    assert set(np.unique(k)) <= {0, 1}
    assert abs(int(k.sum()) - 1000) <= 5 * math.sqrt(500)


def test_sampler_restatement_degenerate_and_clamp():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0], [0, 300, 0], [300, 0, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 4, 5], [0, 1, 9]], dtype=np.int32)
    k = nr.sample_counts(v, f, 100.0, seed=0)[0]
    assert k.tolist() == [0, 0, 65535, 0]               # zero area; NaN corner; 45000 * 100 clamped; index out of range
    k0 = nr.sample_counts(v, f, 0.0, seed=0)[0]
    assert k0.sum() == 0


def _err():
    return _lib.load().pnr_last_error()


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    null, one, one16 = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(64)
    inf = float("inf")
    # pnr_nn_build / pnr_nn_query
    assert lib.pnr_nn_build(null, 4, 0.5, 1024, one, one16, one, null) == -1 and b"null" in _err()
    for d in (0.0, -1.0, inf, float("nan")):
        assert lib.pnr_nn_build(one, 4, d, 1024, one, one16, one, null) == -1 and b"max_dist" in _err()
        assert lib.pnr_nn_query(one, 4, d, 1024, one, one16, one, 4, one, one, null, null) == -1 and b"max_dist" in _err()
    for T in (0, 1, 1000, 1025, 1 << 29):
        assert lib.pnr_nn_build(one, 4, 0.5, T, one, one16, one, null) == -1 and b"table_size" in _err()
        assert lib.pnr_nn_query(one, 4, 0.5, T, one, one16, one, 4, one, one, null, null) == -1 and b"table_size" in _err()
        assert lib.pnr_nn_workspace_bytes(4, T) == -1
    assert lib.pnr_nn_build(one, -1, 0.5, 1024, one, one16, one, null) == -1 and b"n must" in _err()
    assert lib.pnr_nn_build(one, 2 ** 31, 0.5, 1024, one, one16, one, null) == -1 and b"n must" in _err()
    assert lib.pnr_nn_build(one, 4, 0.5, 1024, one, ctypes.c_void_p(72), one, null) == -1 and b"records" in _err()
    assert lib.pnr_nn_build(one, 4, 3e38, 1024, one, one16, one, null) == -1 and b"overflows" in _err()
    for d in (1e-40, 1.4e-39, 1.401298464324817e-45):         # denormals whose 1 / (2 Dp) is +inf: a box of 2^21 cells per axis otherwise
        assert lib.pnr_nn_build(one, 4, d, 1024, one, one16, one, null) == -1 and b"too small" in _err()
        assert lib.pnr_nn_query(one, 4, d, 1024, one, one16, one, 4, one, one, null, null) == -1 and b"too small" in _err()
    assert lib.pnr_nn_build(null, 0, 1.5e-39, 1024, null, null, null, null) == 0            # the smallest scale that is accepted
    assert lib.pnr_nn_query(one, 4, 0.5, 1024, one, one16, null, 4, one, one, null, null) == -1 and b"null" in _err()
    assert lib.pnr_nn_query(one, 4, 0.5, 1024, one, one16, one, 2 ** 31, one, one, null, null) == -1 and b"m must" in _err()
    assert lib.pnr_nn_query(one, 4, 0.5, 1024, one, one16, one, 4, one, one, ctypes.c_void_p(68), null) == -1 and b"stats" in _err()
    assert lib.pnr_nn_build(null, 0, 0.5, 1024, null, null, null, null) == 0              # an empty cloud, nothing to fill: a no-op
    assert lib.pnr_nn_query(null, 0, 0.5, 1024, null, null, null, 0, null, null, null, null) == 0
    assert lib.pnr_nn_query(one, 4, 0.5, 1024, one, one16, null, 0, null, null, null, null) == 0
    assert lib.pnr_nn_workspace_bytes(1000, 2048) >= 2048 * 4 + 8 + 4 * 2
    # pnr_cloud_metrics
    tau = (ctypes.c_float * 9)(*([0.1] * 9))
    assert lib.pnr_cloud_metrics(one, one, null, 4, 0.0, tau, 1, one, one, one, null) == -1 and b"max_dist" in _err()
    assert lib.pnr_cloud_metrics(one, one, null, 4, inf, tau, 1, one, one, one, null) == -1 and b"max_dist" in _err()
    assert lib.pnr_cloud_metrics(one, one, null, 4, 0.5, tau, 9, one, one, one, null) == -1 and b"n_tau" in _err()
    assert lib.pnr_cloud_metrics(one, one, null, 4, 0.5, None, 1, one, one, one, null) == -1 and b"tau_host" in _err()
    assert lib.pnr_cloud_metrics(one, one, null, 4, 0.05, tau, 2, one, one, one, null) == -1 and b"tau[0]" in _err()       # tau > D
    tau[1] = 0.0
    assert lib.pnr_cloud_metrics(one, one, null, 4, 0.5, tau, 2, one, one, one, null) == -1 and b"tau[1]" in _err()
    assert lib.pnr_cloud_metrics(null, one, null, 4, 0.5, tau, 1, one, one, one, null) == -1 and b"null" in _err()
    assert lib.pnr_cloud_metrics(one, one, null, 4, 0.5, tau, 1, ctypes.c_void_p(68), one, one, null) == -1 and b"8-byte" in _err()
    assert lib.pnr_cloud_metrics(null, null, null, 0, 0.5, tau, 1, null, null, null, null) == 0
    assert lib.pnr_cloud_metrics_workspace_bytes(-1) == -1 and lib.pnr_cloud_metrics_workspace_bytes(1) == 16
    assert lib.pnr_cloud_metrics_workspace_bytes(10 ** 7) == 1024 * 16
    # pnr_mesh_sample_count / pnr_mesh_sample_emit
    for rho in (-1.0, inf, float("nan")):
        assert lib.pnr_mesh_sample_count(one, 3, one, 1, rho, 0, one, one, one, null) == -1 and b"rho" in _err()
    assert lib.pnr_mesh_sample_count(one, 3, null, 1, 1.0, 0, one, one, one, null) == -1 and b"faces" in _err()
    assert lib.pnr_mesh_sample_count(one, 3, one, 1, 1.0, 0, null, one, one, null) == -1 and b"null" in _err()
    assert lib.pnr_mesh_sample_count(one, 3, one, 1, 1.0, 0, one, one, null, null) == -1 and b"workspace" in _err()
    assert lib.pnr_mesh_sample_count(one, 3, one, -1, 1.0, 0, one, one, one, null) == -1 and b"n_faces" in _err()
    assert lib.pnr_mesh_sample_count(null, 0, null, 0, 1.0, 0, null, null, null, null) == 0
    assert lib.pnr_mesh_sample_emit(one, 3, one, 1, 0, null, 5, one, one, null) == -1 and b"null" in _err()
    assert lib.pnr_mesh_sample_emit(one, 3, one, 0, 0, one, 5, one, one, null) == -1 and b"without faces" in _err()
    assert lib.pnr_mesh_sample_emit(one, 3, one, 1, 0, one, -1, one, one, null) == -1 and b"n_points" in _err()
    assert lib.pnr_mesh_sample_emit(one, 3, one, 1, 0, one, 0, null, null, null) == 0
    assert lib.pnr_mesh_sample_workspace_bytes(-1) == -1 and lib.pnr_mesh_sample_workspace_bytes(1025) == 8


def test_nn_params():
    assert ops.nn_params("x", 0.25, 0) == (0.25, 1024)
    assert ops.nn_params("x", 0.25, 512)[1] == 1024 and ops.nn_params("x", 0.25, 513)[1] == 2048 and ops.nn_params("x", 0.25, 4133)[1] == 16384
    assert ops.nn_params("x", 0.25, 2 ** 31 - 1)[1] == 2 ** 28
    assert ops.nn_params("x", 0.1, 7, 4) == (float(np.float32(0.1)), 16)
    assert ops.nn_params("x", 1.5e-39, 4)[0] > 0
    for bad in (0, -1.0, float("inf"), float("nan"), 3e38, 1e-40, 1.4e-39, "a", None):
        with pytest.raises(ValueError, match="who: max_dist"):
            ops.nn_params("who", bad, 4)
    for bits in (0, 29, 4.0, True):
        with pytest.raises(ValueError, match="who: table_bits"):
            ops.nn_params("who", 1.0, 4, bits)
    with pytest.raises(ValueError, match="who: the cloud holds"):
        ops.nn_params("who", 1.0, 2 ** 31)


def test_ops_refuse_by_name():
    ref, q = torch.zeros(8, 3), torch.zeros(5, 3)
    start, rec = torch.zeros(1025, dtype=torch.int32), torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="nn_build: ref.*no CPU fallback"):
        ops.nn_build(ref, 0.5)
    with pytest.raises(RuntimeError, match="nn_query: query.*no CPU fallback"):
        ops.nn_query(ref, start, rec, q, 0.5)
    with pytest.raises(ValueError, match="nn_build: ref must be a GPU tensor, got ndarray"):
        ops.nn_build(np.zeros((8, 3), np.float32), 0.5)
    with pytest.raises(TypeError, match="nn_build: ref must be torch.float32"):
        ops.nn_build(ref.double(), 0.5)
    with pytest.raises(ValueError, match=r"nn_build: ref must be \(n, 3\)"):
        ops.nn_build(torch.zeros(8, 4), 0.5)
    with pytest.raises(ValueError, match="nn_build: max_dist"):
        ops.nn_build(ref, 0.0)
    with pytest.raises(ValueError, match="nn_build: start must be"):
        ops.nn_build(ref, 0.5, start=torch.zeros(1024, dtype=torch.int32))
    with pytest.raises(TypeError, match="nn_query: start must be torch.int32"):
        ops.nn_query(ref, start.long(), rec, q, 0.5)
    with pytest.raises(ValueError, match="nn_query: start must be"):
        ops.nn_query(ref, start[:1001], rec, q, 0.5)
    with pytest.raises(ValueError, match="nn_query: records must be"):
        ops.nn_query(ref, start, rec[:7], q, 0.5)
    with pytest.raises(TypeError, match="nn_query: query must be torch.float32"):
        ops.nn_query(ref, start, rec, q.half(), 0.5)
    with pytest.raises(ValueError, match=r"nn_query: query must be \(n, 3\)"):
        ops.nn_query(ref, start, rec, q.reshape(-1), 0.5)
    with pytest.raises(ValueError, match="nn_query: stats must be"):
        ops.nn_query(ref, start, rec, q, 0.5, stats=torch.zeros(4, dtype=torch.int64))
    index, dist2 = torch.zeros(5, dtype=torch.int32), torch.zeros(5)
    with pytest.raises(RuntimeError, match="cloud_metrics: index.*no CPU fallback"):
        ops.cloud_metrics(index, dist2, 0.5, (0.1,))
    with pytest.raises(TypeError, match="cloud_metrics: index must be torch.int32"):
        ops.cloud_metrics(index.long(), dist2, 0.5)
    with pytest.raises(ValueError, match="cloud_metrics: dist2 must be"):
        ops.cloud_metrics(index, dist2[:4], 0.5)
    with pytest.raises(ValueError, match="cloud_metrics: at most 8 thresholds"):
        ops.cloud_metrics(index, dist2, 0.5, [0.1] * 9)
    with pytest.raises(ValueError, match="cloud_metrics: every threshold"):
        ops.cloud_metrics(index, dist2, 0.5, (0.6,))
    with pytest.raises(ValueError, match="cloud_metrics: counts must be"):
        ops.cloud_metrics(index, dist2, 0.5, counts=torch.zeros(5, dtype=torch.int64))
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="mesh_sample_count: vertices.*no CPU fallback"):
        ops.mesh_sample_count(v, f, 1.0)
    with pytest.raises(TypeError, match="mesh_sample_count: faces must be torch.int32"):
        ops.mesh_sample_count(v, f.long(), 1.0)
    for rho in (-1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError, match="mesh_sample_count: density"):
            ops.mesh_sample_count(v, f, rho)
    with pytest.raises(ValueError, match="mesh_sample_count: seed"):
        ops.mesh_sample_count(v, f, 1.0, seed=2 ** 64)
    with pytest.raises(ValueError, match="mesh_sample_emit: face must be"):
        ops.mesh_sample_emit(v, f, 0, torch.zeros(2, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(3, dtype=torch.int32))
    # non-contiguous input and a second device: the checks behind the device check, on tensors that say they are on a GPU
    from _fake_gpu import _fake, z
    with pytest.raises(ValueError, match="nn_build: ref: tensor must be contiguous"):
        ops.nn_build.__wrapped__(_fake(torch.zeros(8, 6))[:, ::2], 0.5)
    with pytest.raises(ValueError, match="nn_query: query: tensor must be contiguous"):
        ops.nn_query.__wrapped__(z(8, 3), z(1025, dtype=torch.int32), z(8, 4), _fake(torch.zeros(3, 5)).t(), 0.5)
    with pytest.raises(ValueError, match="nn_query: records is on"):
        ops.nn_query.__wrapped__(z(8, 3, device="cuda:0"), z(1025, dtype=torch.int32, device="cuda:0"), z(8, 4, device="cuda:1"),
                                 z(5, 3, device="cuda:0"), 0.5)
    with pytest.raises(ValueError, match="mesh_sample_count: faces: tensor must be contiguous"):
        ops.mesh_sample_count.__wrapped__(z(3, 3), _fake(torch.zeros(3, 2, dtype=torch.int32)).t(), 1.0)
    with pytest.raises(RuntimeError, match="cloud_metrics: query.*no CPU fallback"):
        ops.cloud_metrics.__wrapped__(z(5, dtype=torch.int32), z(5), 0.5, query=torch.zeros(5, 3))


def test_wrappers_refuse_by_name():
    m = mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), (2, 2, 2), None, None, 0.0)
    for kw in ({}, {"density": 1.0, "n": 5}):
        with pytest.raises(ValueError, match="Mesh.sample: give exactly one of density and n"):
            m.sample(**kw)
    with pytest.raises(RuntimeError, match="Mesh.sample.*no CPU fallback"):
        m.sample(density=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointcloud.NearestIndex(torch.zeros(4, 3), 0.5)
    with pytest.raises(ValueError, match="pointcloud.nearest: labels must be a tensor with one row per reference point"):
        pointcloud.nearest(torch.zeros(2, 3), torch.zeros(4, 3), 0.5, labels=torch.zeros(3))
    ev = Evaluator()
    with pytest.raises(RuntimeError, match="Evaluator.evaluate_geometry.*no CPU fallback"):
        ev.evaluate_geometry(torch.zeros(4, 3), torch.zeros(4, 3), 0.5, (0.1,))
    with pytest.raises(ValueError, match="Evaluator.evaluate_geometry: max_dist"):
        ev.evaluate_geometry(torch.zeros(4, 3), torch.zeros(4, 3), 1e-40)
    assert ev.geom is None
    with pytest.raises(ValueError, match=r"Evaluator.evaluate_geometry: pred_points must be \(n, 3\)"):
        ev.evaluate_geometry(torch.zeros(4, 2), torch.zeros(4, 3), 0.5)
    with pytest.raises(ValueError, match="Evaluator.evaluate_geometry: every threshold"):
        ev.evaluate_geometry(torch.zeros(4, 3), torch.zeros(4, 3), 0.5, (0.7,))
    assert "geom_accuracy" not in ev.summarize()        # the keys appear only after evaluate_geometry
