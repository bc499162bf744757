"""panopticnerf_amd/primitives.py on the CPU: what ConvexSet refuses, from_boxes / from_mesh / extrude_polygon against
independent float64 membership tests, and pnr_convex_hits' argument checks (no device is touched)."""
import ctypes

import numpy as np
import pytest
import torch

from panopticnerf_amd import ConvexSet, _lib, extrude_polygon, primitives, synthetic

I32 = np.int32
EYE = np.eye(3)


def _cube_planes():
    return np.array([[1, 0, 0, 1], [-1, 0, 0, 1], [0, 1, 0, 1], [0, -1, 0, 1], [0, 0, 1, 1], [0, 0, -1, 1]], np.float64)


# ------------------------------------------------------------------------------------------------ ConvexSet
def test_convex_set_basics_and_concat():
    a = ConvexSet(_cube_planes(), np.array([0, 6]), np.array([[3, 1]]))
    b = ConvexSet(_cube_planes()[:4].astype(np.float32), np.array([0, 1, 4], I32), np.array([[5, 0], [6, 2]], I32))
    assert len(a) == 1 and len(b) == 2 and a.n_planes == 6
    assert a.planes.dtype == np.float32 and a.offsets.dtype == I32 and a.ids.dtype == I32
    c = ConvexSet.concat(a, b, a)
    assert len(c) == 4 and c.offsets.tolist() == [0, 6, 7, 10, 16] and c.ids.tolist() == [[3, 1], [5, 0], [6, 2], [3, 1]]
    assert len(ConvexSet.concat()) == 0 and ConvexSet.concat().contains(np.zeros((2, 3))).shape == (2, 0)
    t = c.batch()
    assert sorted(t) == ["prim_ids", "prim_offsets", "prim_planes"]
    assert t["prim_planes"].dtype == torch.float32 and tuple(t["prim_planes"].shape) == (16, 4)
    assert t["prim_offsets"].dtype == torch.int32 and t["prim_ids"].dtype == torch.int32 and tuple(t["prim_ids"].shape) == (4, 2)
    assert c.batch()["prim_planes"] is t["prim_planes"]            # the same tensors every time
    inside = c.contains(np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 3.0], [2.0, 0, 0]]))
    assert inside.tolist() == [[True, True, True, True], [False, True, True, False], [False, False, True, False]]
    # tensors are accepted too
    ConvexSet(torch.tensor(_cube_planes()), torch.tensor([0, 6]), torch.tensor([[1, 1]]))


@pytest.mark.parametrize("planes, offsets, ids, exc", [
    (np.zeros((6, 3)), [0, 6], [[0, 0]], ValueError),                                 # planes not (P,4)
    (_cube_planes().astype(np.int64), [0, 6], [[0, 0]], TypeError),                   # integer planes
    (_cube_planes(), [0.0, 6.0], [[0, 0]], TypeError),                                # float offsets
    (_cube_planes(), [0, 6], [[0.0, 0.0]], TypeError),                                # float ids
    (_cube_planes(), [[0, 6]], [[0, 0]], ValueError),                                 # offsets not 1-D
    (_cube_planes(), [0, 6], [[0, 0], [1, 1]], ValueError),                           # ids not (M,2)
    (_cube_planes(), [0, 6], [0, 0], ValueError),
    (_cube_planes(), [0, 4, 2, 6], [[0, 0]] * 3, ValueError),                         # non-monotone
    (_cube_planes(), [1, 6], [[0, 0]], ValueError),                                   # does not start at 0
    (_cube_planes(), [0, 5], [[0, 0]], ValueError),                                   # does not end at P
    (_cube_planes(), [0, 3, 3, 6], [[0, 0]] * 3, ValueError),                         # a primitive without planes
])
def test_convex_set_refuses(planes, offsets, ids, exc):
    with pytest.raises(exc):
        ConvexSet(np.asarray(planes), np.asarray(offsets), np.asarray(ids))


def test_convex_set_refuses_bad_normals():
    for bad, word in ((np.nan, "finite"), (np.inf, "finite")):
        p = _cube_planes()
        p[2, 1] = bad
        with pytest.raises(ValueError, match=word):
            ConvexSet(p, np.array([0, 6]), np.array([[0, 0]]))
    p = _cube_planes()
    p[4, :3] = 0
    with pytest.raises(ValueError, match="plane 4 has a zero normal"):
        ConvexSet(p, np.array([0, 6]), np.array([[0, 0]]))
    p = _cube_planes()
    p[1, 3] = np.nan
    with pytest.raises(ValueError, match="plane 1"):
        ConvexSet(p, np.array([0, 6]), np.array([[0, 0]]))


# ------------------------------------------------------------------------------------------------ from_boxes
def test_from_boxes_membership_equals_the_local_frame_test():
    box, ids = synthetic.random_boxes(24, seed=5)
    cs = ConvexSet.from_boxes(box, ids)
    assert len(cs) == 24 and cs.n_planes == 144 and np.array_equal(cs.ids, ids.numpy())
    assert np.abs(np.linalg.norm(cs.planes64[:, :3], axis=1) - 1).max() < 1e-12          # unit normals
    b = box.numpy().astype(np.float64)
    rng = np.random.default_rng(0)
    # points around every box: its centre plus up to 1.5 half-diagonals
    pts = (b[:, None, 0:3] + rng.uniform(-1.5, 1.5, (24, 400, 3)) * np.linalg.norm(b[:, None, 12:15], axis=-1, keepdims=True)).reshape(-1, 3)
    local = np.einsum("mai,nmi->nma", b[:, 3:12].reshape(24, 3, 3), pts[:, None, :] - b[None, :, 0:3])      # (n,M,3)
    margin = np.abs(np.abs(local) - b[None, :, 12:15]).min(-1)
    want = (np.abs(local) <= b[None, :, 12:15]).all(-1)
    got = cs.contains(pts)
    far = margin > 1e-5         # the rows of the float32 rotations are unit to 1e-7: the two tests differ only that close to a face
    assert far.mean() > 0.99 and want[far].sum() > 500
    assert np.array_equal(got[far], want[far])
    with pytest.raises(ValueError, match="15"):
        ConvexSet.from_boxes(np.zeros((3, 14)), np.zeros((3, 2), I32))
    with pytest.raises(ValueError):
        ConvexSet.from_boxes(box, ids[:5])


# ------------------------------------------------------------------------------------------------ from_mesh
CUBE_V = np.array([[x, y, z] for x in (0, 2) for y in (0, 3) for z in (0, 1)], np.float64)      # index = 4 ix + 2 iy + iz
CUBE_QUADS = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]


def _tri_faces(flip_some=True):
    f = []
    for k, (a, b, c, d) in enumerate(CUBE_QUADS):
        t = [(a, b, c), (a, c, d)]
        if flip_some and k % 2:            # mixed winding: the planes are oriented by the centroid, not by the winding
            t = [(x, z, y) for x, y, z in t]
        f += t
    return np.array(f)


def test_from_mesh_cube_with_triangulated_faces_gives_six_planes():
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
    v = CUBE_V @ rot.T + np.array([5.0, -2.0, 11.0])
    cs = ConvexSet.from_mesh(v, _tri_faces(), (7, 2))
    assert len(cs) == 1 and cs.n_planes == 6 and cs.ids.tolist() == [[7, 2]]
    assert np.abs(np.linalg.norm(cs.planes64[:, :3], axis=1) - 1).max() < 1e-12
    rng = np.random.default_rng(1)
    loc = rng.uniform(-1, 4, (4000, 3))
    want = ((loc >= 0) & (loc <= np.array([2, 3, 1]))).all(1)
    far = np.abs(np.stack([loc, loc - np.array([2, 3, 1])])).min((0, 2)) > 1e-9
    got = cs.contains(loc @ rot.T + np.array([5.0, -2.0, 11.0]))[:, 0]
    assert want.sum() > 100 and np.array_equal(got[far], want[far])
    assert ConvexSet.from_mesh(CUBE_V, np.array(CUBE_QUADS), (1, 1)).n_planes == 6      # polygon faces


def test_from_mesh_refuses_a_dented_cube_and_names_the_vertex():
    v = np.concatenate([CUBE_V, [[1.0, 1.5, 0.5]]])         # the top face z = 1 pushed in at its centre: vertex 8
    top = CUBE_QUADS[5]
    faces = [t for t in _tri_faces(False).tolist() if not set(t) <= set(top)]
    faces += [(top[i], top[(i + 1) % 4], 8) for i in range(4)]
    with pytest.raises(ValueError, match="not convex: vertex"):
        ConvexSet.from_mesh(v, np.array(faces), (0, 0))
    with pytest.raises(ValueError):
        ConvexSet.from_mesh(CUBE_V, np.array(CUBE_QUADS) + 3, (0, 0))           # a face names a vertex that is not there
    with pytest.raises(ValueError):
        ConvexSet.from_mesh(CUBE_V[:, :2], np.array(CUBE_QUADS), (0, 0))


# ------------------------------------------------------------------------------------------------ extrude_polygon
def _shoelace(p):
    p = np.asarray(p, np.float64)
    return 0.5 * abs(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]))


def _even_odd(p, q):
    """float64 crossing-number test of points q (n,2) against polygon p (V,2), and each point's distance to the outline"""
    p = np.asarray(p, np.float64)
    a, b = p[None], np.roll(p, -1, 0)[None]
    x, y = q[:, None, 0], q[:, None, 1]
    with np.errstate(all="ignore"):
        cross = ((a[..., 1] > y) != (b[..., 1] > y)) & (x < (b[..., 0] - a[..., 0]) * (y - a[..., 1]) / (b[..., 1] - a[..., 1]) + a[..., 0])
    ab, aq = b - a, q[:, None, :] - a
    t = np.clip((aq * ab).sum(-1) / (ab * ab).sum(-1), 0, 1)
    dist = np.linalg.norm(aq - t[..., None] * ab, axis=-1).min(1)
    return cross.sum(1) % 2 == 1, dist


OUTLINES = {"L": (synthetic.L_OUTLINE, 4), "U": (synthetic.U_OUTLINE, 6),
            "square with a collinear vertex": (((0.0, 0.0), (1.5, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0)), 2)}


@pytest.mark.parametrize("winding", [1, -1])
@pytest.mark.parametrize("name", list(OUTLINES))
def test_extrude_polygon_pieces_area_and_membership(name, winding):
    outline, pieces = OUTLINES[name]
    outline = np.array(outline)[::winding]
    rot = np.array([[0.0, -1.0, 0.0], [0.6, 0.0, -0.8], [0.8, 0.0, 0.6]])
    assert np.abs(rot @ rot.T - EYE).max() < 1e-15
    trans = np.array([3.0, -1.0, 20.0])
    cs = extrude_polygon(outline, -0.5, 2.0, rot, trans, (9, 4))
    assert len(cs) == pieces and (np.diff(cs.offsets) == 5).all() and (cs.ids == [9, 4]).all()
    assert np.abs(np.linalg.norm(cs.planes64[:, :3], axis=1) - 1).max() < 1e-12
    tri = primitives.ear_clip(outline)
    area = 0.5 * primitives._cross2(tri[:, 0], tri[:, 1], tri[:, 2])
    assert (area > 0).all() and abs(area.sum() - _shoelace(outline)) <= 1e-12 * _shoelace(outline)
    rng = np.random.default_rng(2)
    lo, hi = outline.min(0) - 2, outline.max(0) + 2
    loc = np.concatenate([rng.uniform(lo, hi, (10000, 2)), rng.uniform(-1.5, 3.0, (10000, 1))], 1)
    inside2d, dist = _even_odd(outline, loc[:, :2])
    want = inside2d & (loc[:, 2] >= -0.5) & (loc[:, 2] <= 2.0)
    far = (dist > 1e-6) & (np.abs(loc[:, 2] + 0.5) > 1e-6) & (np.abs(loc[:, 2] - 2.0) > 1e-6)
    got = cs.contains(loc @ rot.T + trans)
    assert far.mean() > 0.99 and want.sum() > 500
    assert np.array_equal(got.any(1)[far], want[far])
    # a point strictly inside belongs to one piece, or to two on a shared diagonal
    assert got.sum(1).max() <= 2


def test_extrude_polygon_refuses():
    sq = [(0, 0), (2, 0), (2, 2), (0, 2)]
    with pytest.raises(ValueError, match="intersects itself"):
        extrude_polygon([(0, 0), (2, 2), (2, 0), (0, 2)], 0, 1, EYE, np.zeros(3), (0, 0))           # a bow-tie
    with pytest.raises(ValueError, match="intersects itself"):
        extrude_polygon([(0, 0), (2, 0), (1, 0), (1, 1)], 0, 1, EYE, np.zeros(3), (0, 0))           # folds back over an edge
    with pytest.raises(ValueError, match="z_lo < z_hi"):
        extrude_polygon(sq, 1, 1, EYE, np.zeros(3), (0, 0))
    with pytest.raises(ValueError, match="orthogonal"):
        extrude_polygon(sq, 0, 1, 2 * EYE, np.zeros(3), (0, 0))
    with pytest.raises(ValueError):
        extrude_polygon(sq[:2], 0, 1, EYE, np.zeros(3), (0, 0))
    with pytest.raises(ValueError, match="repeats a vertex"):
        extrude_polygon(sq + [(0, 2)], 0, 1, EYE, np.zeros(3), (0, 0))
    with pytest.raises(TypeError):
        extrude_polygon(sq, 0, 1, EYE, np.zeros(3), (0.5, 0.0))


def test_primitive_scene_is_seeded():
    a, b, c = synthetic.primitive_scene(seed=3), synthetic.primitive_scene(seed=3), synthetic.primitive_scene(seed=4)
    assert len(a) == 4 + 4 + 6 and np.array_equal(a.planes, b.planes) and not np.array_equal(a.planes, c.planes)
    assert (np.diff(a.offsets)[:4] == 6).all() and (np.diff(a.offsets)[4:] == 5).all()


# ------------------------------------------------------------------------------------------------ the entry point's checks
def test_convex_hits_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)          # non-null, never dereferenced: validation fails first
    f = lib.pnr_convex_hits
    assert f(null, 4, one, one, 3, 8, one, one, one, null) == -1 and b"null" in lib.pnr_last_error()
    assert f(one, 4, one, one, 3, 8, null, one, one, null) == -1
    assert f(one, 4, one, one, 3, 8, one, null, one, null) == -1
    assert f(one, 4, one, one, 3, 8, one, one, null, null) == -1
    assert f(one, 4, null, one, 3, 8, one, one, one, null) == -1 and b"null" in lib.pnr_last_error()
    assert f(one, 4, one, null, 3, 8, one, one, one, null) == -1
    assert f(one, 4, one, one, -1, 8, one, one, one, null) == -1 and b"n_prim" in lib.pnr_last_error()
    assert f(one, 4, one, one, 3, 0, one, one, one, null) == -1 and b"max_hits" in lib.pnr_last_error()
    assert f(one, 0, one, one, 3, -2, one, one, one, null) == -1
    assert f(null, 0, null, null, 0, 8, null, null, null, null) == 0            # no rays: a no-op
    assert f(null, 0, one, one, 3, 8, null, null, null, null) == 0
    assert "pnr_convex_hits" in _lib.SIGNATURES
