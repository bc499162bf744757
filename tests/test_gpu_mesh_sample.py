"""Mesh sampling on an MI355X: k_mesh_sample_count / k_mesh_sample_emit and the shared scan (csrc/pnr_nn.hip) against
tests/_nn_ref.py's restatement (include/pnr.h "nearest neighbours", MESH SAMPLING).  points and face are float32 and int32 words
that must be EQUAL to the restatement's.  tests/test_nn_host.py pins the restatement's own properties on the CPU."""
import numpy as np
import pytest
import torch

import _nn_ref as nr
from _arena import Arena
from panopticnerf_amd import mesh, ops, synthetic

pytestmark = pytest.mark.gpu

UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def N_(t):
    return t.detach().cpu().numpy()


def make(dev, v, f):
    v, f = np.asarray(v, dtype=np.float32).reshape(-1, 3), np.asarray(f, dtype=np.int32).reshape(-1, 3)
    return mesh.Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.zeros(len(v), dtype=torch.int64, device=dev), (2, 2, 2), None, None, 0.0)


def triangles(F, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, size=(3 * F, 3)).astype(np.float32), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def check(dev, v, f, rho, seed=0):
    m = make(dev, v, f)
    pts, face = m.sample(density=rho, seed=seed)
    rp, rf = nr.sample(v, f, rho, seed)
    assert pts.dtype == torch.float32 and face.dtype == torch.int32 and tuple(pts.shape) == (len(rf), 3)
    assert np.array_equal(N_(face), rf)
    assert np.array_equal(N_(pts).view(np.uint32), rp.view(np.uint32))
    return N_(pts), N_(face)


SINGLE = ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def test_single_degenerate_and_nan_triangles(dev):
    pts, face = check(dev, *SINGLE, 200.0, seed=3)
    assert 99 <= len(pts) <= 101 and (face == 0).all()
    assert pts[:, 2].max() == 0 and pts.min() >= 0 and (pts[:, 0] + pts[:, 1]).max() <= 1.0 + 1e-6
    v = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0], [0, 2, 0], [2, 0, 0]]
    f = [[0, 1, 2], [0, 1, 3], [0, 4, 5], [0, 1, 9], [5, 4, 0]]         # zero area, NaN corner, area 2, index out of range, area 2
    pts, face = check(dev, v, f, 50.0, seed=1)
    assert set(np.unique(face)) == {2, 4} and 180 <= len(face) <= 220


@pytest.mark.parametrize("F", [63, 64, 65, 1025])
def test_random_triangles(dev, F):
    v, f = triangles(F, F)
    _, face = check(dev, v, f, 30.0, seed=F)            # mean counts of about 20
    assert len(face) > 5 * F
    _, face = check(dev, v, f, 0.5, seed=F + 1)         # mean counts below 1: many triangles get none
    k = np.bincount(face, minlength=F)
    assert (k == 0).sum() > F // 4 and (k > 0).sum() > F // 8


@pytest.mark.parametrize("res", [8, 16])
def test_sphere_mesh_through_extract(dev, res):
    field = synthetic.sdf_grid("sphere", *UNIT, res, radius=0.7, device=dev)
    m = mesh.extract(field, *UNIT, 0.0)
    v, f = N_(m.vertices), N_(m.faces)
    pts, face = m.sample(density=100.0, seed=9)
    rp, rf = nr.sample(v, f, 100.0, 9)
    assert np.array_equal(N_(face), rf) and np.array_equal(N_(pts).view(np.uint32), rp.view(np.uint32))
    assert abs(len(rf) - 100.0 * m.area()) < 5 * np.sqrt(len(f))        # each count is within 1 of its mean, variance <= 1/4
    r = np.linalg.norm(N_(pts).astype(np.float64), axis=1)
    assert abs(r.mean() - 0.7) < 2.0 / res                              # on the surface of the sphere, to the lattice's step
    pts_n, _ = m.sample(n=2000, seed=2)                                 # n: density = n / area, so about n points
    assert abs(pts_n.shape[0] - 2000) < 5 * np.sqrt(len(f))


def test_density_zero_and_the_clamp(dev):
    m = make(dev, *SINGLE)
    pts, face = m.sample(density=0.0)
    assert tuple(pts.shape) == (0, 3) and tuple(face.shape) == (0,)
    pts, face = m.sample(n=0)
    assert tuple(pts.shape) == (0, 3)
    big = ([[0, 0, 0], [300, 0, 0], [0, 300, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], [[3, 4, 5], [0, 1, 2], [5, 4, 3]])
    pts, face = check(dev, *big, 2.0, seed=4)           # 45000 * 2 = 90000 on the large triangle: clamped to 65535
    assert (face == 1).sum() == 65535 and (face == 0).sum() in (1, 2) and (np.diff(face) >= 0).all()
    empty = make(dev, np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.sample(density=5.0)[0].shape == (0, 3)


def test_same_seed_same_output_other_seed_another(dev):
    v, f = triangles(65, 2)
    m = make(dev, v, f)
    a, b, c = m.sample(density=30.0, seed=5), m.sample(density=30.0, seed=5), m.sample(density=30.0, seed=2 ** 63 + 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape != c[0].shape or not torch.equal(a[0], c[0])
    rp, rf = nr.sample(v, f, 30.0, 2 ** 63 + 5)         # the high seed word is part of the key
    assert np.array_equal(N_(c[1]), rf) and np.array_equal(N_(c[0]).view(np.uint32), rp.view(np.uint32))


def test_ops_write_inside_their_buffers(dev):
    """start, points and face as interior views of a guarded arena; the totals agree with the restatement"""
    v, f = triangles(1025, 8)
    k = nr.sample_counts(v, f, 30.0, 6)[0]
    N = int(k.sum())
    arena = Arena(dev, [("start", 1028, 64), ("points", 3 * N + (-3 * N) % 4, 64), ("face", N + (-N) % 4, 64)])
    start = arena.view("start")[:1026].view(torch.int32)
    points = arena.view("points")[: 3 * N].view(N, 3)
    face = arena.view("face")[:N].view(torch.int32)
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    total, s2 = ops.mesh_sample_count(vd, fd, 30.0, 6, start=start)
    assert s2 is start and int(total.item()) == N
    assert np.array_equal(N_(start), np.concatenate([[0], np.cumsum(k)]).astype(np.int32))
    ops.mesh_sample_emit(vd, fd, 6, start, points, face)
    torch.cuda.synchronize()
    assert arena.guards_intact()
    rp, rf = nr.sample(v, f, 30.0, 6)
    assert np.array_equal(N_(face), rf) and np.array_equal(N_(points).view(np.uint32), rp.view(np.uint32))
