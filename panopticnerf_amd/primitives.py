"""Convex bounding primitives for the 3D prior ("oriented 3D bounding primitives"; include/pnr.h "a8b").

KITTI-360 annotates a scene with bounding primitives: cuboids for cars and poles, extruded polygons -- often non-convex -- for
road, sidewalk, ground, buildings and walls, each a small closed mesh with a pose.  The renderer takes them as ONE table of
convex polytopes in half-space form,

    planes  (P, 4) float32   one (n0, n1, n2, dd) per plane, |n| = 1, inside: n.x <= dd
    offsets (M + 1) int32    CSR: primitive m owns planes offsets[m] .. offsets[m + 1] - 1
    ids     (M, 2) int32     (semantic id, instance id); the pieces of one decomposed object repeat its ids

which ops.convex_hits intersects with rays (pnr_convex_hits).  This module is the host-side toolkit that makes the table:
ConvexSet.from_boxes (the cuboid table of ops.bbox_hits, so a scene can mix cuboids with the rest), ConvexSet.from_mesh (a
closed convex mesh) and extrude_polygon (a simple polygon of either winding, ear-clipped into triangular prisms).  Everything
is numpy in float64, rounded to float32 once at the end.  Not here: ellipsoids, non-convex meshes without a decomposition,
merging triangles into larger convex pieces, reading KITTI-360's XML."""
import numpy as np

__all__ = ["ConvexSet", "extrude_polygon", "ear_clip"]


def _np(a):
    if hasattr(a, "detach"):        # a torch tensor
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _ids(ids, n, what):
    ids = _np(ids)
    if ids.dtype.kind not in "iu":
        raise TypeError("%s: ids must be integers, not %s" % (what, ids.dtype))
    ids = ids.reshape(-1, 2) if ids.size == 2 else ids
    if ids.shape == (1, 2):
        ids = np.repeat(ids, n, 0)
    if ids.shape != (n, 2):
        raise ValueError("%s: ids must be (semantic id, instance id) or (%d, 2), not %s" % (what, n, ids.shape))
    return ids.astype(np.int32)


class ConvexSet:
    """M convex polytopes as half-spaces.  planes (P,4) float (float64 is kept for contains() and rounded to float32 once for the
    device), offsets (M+1) integers, ids (M,2) integers.  Refused: wrong shapes or dtypes, offsets that do not start at 0, end
    at P and increase strictly (a primitive without planes), non-finite values, zero normals."""

    def __init__(self, planes, offsets, ids):
        planes, offsets, ids = _np(planes), _np(offsets), _np(ids)
        if planes.dtype.kind != "f":
            raise TypeError("ConvexSet: planes must be floating point, not %s" % planes.dtype)
        if offsets.dtype.kind not in "iu" or ids.dtype.kind not in "iu":
            raise TypeError("ConvexSet: offsets and ids must be integers, not %s / %s" % (offsets.dtype, ids.dtype))
        if planes.ndim != 2 or planes.shape[1] != 4:
            raise ValueError("ConvexSet: planes must be (P, 4), not %s" % (planes.shape,))
        if offsets.ndim != 1 or offsets.size < 1:
            raise ValueError("ConvexSet: offsets must be (M + 1,), not %s" % (offsets.shape,))
        M, P = offsets.size - 1, planes.shape[0]
        if ids.shape != (M, 2):
            raise ValueError("ConvexSet: ids must be (%d, 2), not %s" % (M, ids.shape))
        offsets = offsets.astype(np.int64)
        if P >= 2 ** 31:
            raise ValueError("ConvexSet: plane indices are int32")
        if offsets[0] != 0 or offsets[-1] != P or (M and np.any(np.diff(offsets) < 0)):
            raise ValueError("ConvexSet: offsets must be non-decreasing from 0 to P = %d" % P)
        if M and np.any(np.diff(offsets) == 0):
            raise ValueError("ConvexSet: primitive %d has no planes" % int(np.argmin(np.diff(offsets))))
        p64 = planes.astype(np.float64)
        if not np.all(np.isfinite(p64)):
            raise ValueError("ConvexSet: plane %d is not finite" % int(np.argmax(~np.isfinite(p64).all(1))))
        norm = np.linalg.norm(p64[:, :3], axis=1)
        if np.any(norm == 0):
            raise ValueError("ConvexSet: plane %d has a zero normal" % int(np.argmax(norm == 0)))
        self.planes64 = p64
        self.planes = p64.astype(np.float32)
        self.offsets = offsets.astype(np.int32)
        self.ids = ids.astype(np.int32)
        self.device = None
        self._t = None

    def __len__(self):
        return self.offsets.size - 1

    @property
    def n_planes(self):
        return self.planes.shape[0]

    def to(self, device):
        """Put the three tensors on `device` (kept: batch() hands out the same tensors every time).  Returns self."""
        import torch
        self.device = torch.device(device)
        self._t = None
        self.batch()
        return self

    def batch(self):
        """{"prim_planes" (P,4) float32, "prim_offsets" (M+1) int32, "prim_ids" (M,2) int32}: the batch keys Renderer.render
        takes, on the device of the last to() (host tensors before)."""
        import torch
        if self._t is None:
            dev = self.device if self.device is not None else torch.device("cpu")
            self._t = {"prim_planes": torch.from_numpy(self.planes.copy()).to(dev), "prim_offsets": torch.from_numpy(self.offsets.copy()).to(dev),
                       "prim_ids": torch.from_numpy(self.ids.copy()).to(dev)}
        return dict(self._t)

    def contains(self, points):
        """points (n,3) -> (n, M) bool: n.x <= dd for every plane of the primitive, in float64 on the float64 planes."""
        pts = _np(points).astype(np.float64).reshape(-1, 3)
        if len(self) == 0:
            return np.zeros((pts.shape[0], 0), bool)
        inside = pts @ self.planes64[:, :3].T <= self.planes64[:, 3]
        return np.logical_and.reduceat(inside, self.offsets[:-1].astype(np.int64), axis=1)

    @staticmethod
    def concat(*sets):
        if not sets:
            return ConvexSet(np.zeros((0, 4)), np.zeros(1, np.int32), np.zeros((0, 2), np.int32))
        planes = np.concatenate([s.planes64 for s in sets], 0)
        base = np.cumsum([0] + [s.n_planes for s in sets])
        offsets = np.concatenate([[0]] + [s.offsets[1:].astype(np.int64) + b for s, b in zip(sets, base)])
        return ConvexSet(planes, offsets, np.concatenate([s.ids for s in sets], 0))

    # ---------------------------------------------------------------------------------------------- makers
    @staticmethod
    def from_boxes(bbox, bbox_ids):
        """The cuboid table of ops.bbox_hits, bbox (M,15) = centre(3) rotation rows(9) half extents(3), as six planes per box:
        for axis a, (r_a, e_a + r_a.c) and (-r_a, e_a - r_a.c), the rows scaled to unit length."""
        box = _np(bbox)
        if box.ndim != 2 or box.shape[1] != 15:
            raise ValueError("ConvexSet.from_boxes: bbox must be (M, 15), not %s" % (box.shape,))
        box = box.astype(np.float64)
        M = box.shape[0]
        c, rot, ext = box[:, 0:3], box[:, 3:12].reshape(M, 3, 3), box[:, 12:15]
        ln = np.linalg.norm(rot, axis=2)
        if np.any(ln == 0) or not np.all(np.isfinite(box)):
            raise ValueError("ConvexSet.from_boxes: a box has a zero rotation row or a non-finite value")
        rc = np.einsum("mai,mi->ma", rot, c)
        planes = np.empty((M, 3, 2, 4))
        planes[:, :, 0, :3] = rot / ln[..., None]
        planes[:, :, 0, 3] = (ext + rc) / ln
        planes[:, :, 1, :3] = -rot / ln[..., None]
        planes[:, :, 1, 3] = (ext - rc) / ln
        return ConvexSet(planes.reshape(M * 6, 4), np.arange(M + 1) * 6, _ids(bbox_ids, M, "ConvexSet.from_boxes"))

    @staticmethod
    def from_mesh(vertices, faces, ids, tol=1e-6):
        """One primitive from a closed convex mesh: vertices (V,3), faces (F,k) vertex indices (k >= 3; triangles or polygons).
        A plane per face through its first corner, normal by Newell's sum, oriented away from the vertex centroid; faces whose
        planes coincide (normals within tol, offsets within tol * extent) are merged; zero-area faces are skipped.  ValueError
        naming the worst vertex when a vertex lies outside a plane by more than tol * extent (the mesh is not convex)."""
        v, f = _np(vertices).astype(np.float64), _np(faces)
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 4 or not np.all(np.isfinite(v)):
            raise ValueError("ConvexSet.from_mesh: vertices must be (V >= 4, 3) finite numbers, not %s" % (v.shape,))
        if f.dtype.kind not in "iu" or f.ndim != 2 or f.shape[1] < 3 or f.shape[0] < 4:
            raise ValueError("ConvexSet.from_mesh: faces must be (F >= 4, k >= 3) integers")
        if f.min() < 0 or f.max() >= v.shape[0]:
            raise ValueError("ConvexSet.from_mesh: a face names a vertex outside [0, %d)" % v.shape[0])
        ctr = v.mean(0)
        extent = float(np.linalg.norm(v.max(0) - v.min(0)))
        if extent == 0:
            raise ValueError("ConvexSet.from_mesh: the mesh has no extent")
        corners = v[f]                                               # (F,k,3)
        nrm = np.cross(corners, np.roll(corners, -1, 1)).sum(1)      # Newell: twice the area vector
        ln = np.linalg.norm(nrm, axis=1)
        keep = ln > 1e-12 * extent * extent
        nrm, p0 = nrm[keep] / ln[keep, None], corners[keep, 0]
        flip = np.einsum("fi,fi->f", nrm, ctr - p0) > 0
        nrm[flip] *= -1
        dd = np.einsum("fi,fi->f", nrm, p0)
        planes = []
        for n, d in zip(nrm, dd):
            if not any(np.linalg.norm(n - q[:3]) <= tol and abs(d - q[3]) <= tol * extent for q in planes):
                planes.append(np.append(n, d))
        planes = np.asarray(planes).reshape(-1, 4)
        if planes.shape[0] < 4:
            raise ValueError("ConvexSet.from_mesh: fewer than four distinct face planes: not a closed mesh")
        out = v @ planes[:, :3].T - planes[:, 3]                     # (V,F') signed distances
        worst = np.unravel_index(np.argmax(out), out.shape)
        if out[worst] > tol * extent:
            raise ValueError("ConvexSet.from_mesh: not convex: vertex %d lies %.3g outside the plane of a face (tolerance %.3g)"
                             % (worst[0], out[worst], tol * extent))
        return ConvexSet(planes, np.array([0, planes.shape[0]]), _ids(ids, 1, "ConvexSet.from_mesh"))


# ------------------------------------------------------------------------------------------------- extruded polygons
def _cross2(a, b, c):
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def _outline(xy, what):
    """the outline counter-clockwise without collinear vertices; refuses what is not a simple polygon"""
    p = _np(xy).astype(np.float64)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 3 or not np.all(np.isfinite(p)):
        raise ValueError("%s: xy must be (V >= 3, 2) finite numbers, not %s" % (what, p.shape))
    scale = float(np.linalg.norm(p.max(0) - p.min(0)))
    eps = 1e-12 * scale * scale
    if np.any(np.linalg.norm(p - np.roll(p, -1, 0), axis=1) <= 1e-12 * scale):
        raise ValueError("%s: the outline repeats a vertex" % what)
    V = p.shape[0]
    a, b = p, np.roll(p, -1, 0)
    # every pair of edges: neighbours may share their vertex only (no fold-back), the others may not touch at all
    for i in range(V):
        j = np.arange(i + 1, V)
        c, d = a[j], b[j]
        o1, o2 = _cross2(a[i], b[i], c), _cross2(a[i], b[i], d)
        o3, o4 = _cross2(c, d, a[i]), _cross2(c, d, b[i])
        proper = (o1 * o2 < 0) & (o3 * o4 < 0)

        def on(q, s, t, o):      # q collinear with and inside the closed segment s-t
            return (np.abs(o) <= eps) & (np.minimum(s, t) - 1e-12 * scale <= q).all(-1) & (q <= np.maximum(s, t) + 1e-12 * scale).all(-1)
        touch = on(c, a[i], b[i], o1) | on(d, a[i], b[i], o2) | on(a[i], c, d, o3) | on(b[i], c, d, o4)
        adj = (j == i + 1) | ((i == 0) & (j == V - 1))
        bad = (proper | touch) & ~adj
        # neighbours (consecutive edges, each in outline order): collinear and running back over each other
        far_end = np.where((j == i + 1)[:, None], d, c)              # the neighbour's vertex that is not shared
        fold = adj & (np.abs(_cross2(a[i], b[i], far_end)) <= eps) & ((d - c) @ (b[i] - a[i]) < 0)
        if np.any(bad | fold):
            k = int(j[np.argmax(bad | fold)])
            raise ValueError("%s: the outline intersects itself (edges %d and %d)" % (what, i, k))
    area2 = float(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]))
    if abs(area2) <= eps:
        raise ValueError("%s: the outline has no area" % what)
    if area2 < 0:
        p = p[::-1]
    keep = np.abs(_cross2(np.roll(p, 1, 0), p, np.roll(p, -1, 0))) > eps
    return p[keep], eps


def ear_clip(xy):
    """A simple polygon (V,2), either winding, collinear vertices tolerated (and dropped) -> (T,3,2) float64 counter-clockwise
    triangles, T = V' - 2 for the V' vertices that are corners.  An ear is a convex corner whose closed triangle holds no other
    vertex; a simple polygon always has one.  ValueError for a self-intersecting outline."""
    p, eps = _outline(xy, "ear_clip")
    idx = list(range(p.shape[0]))
    tris = []
    while len(idx) > 3:
        n = len(idx)
        for k in range(n):
            ia, ib, ic = idx[k - 1], idx[k], idx[(k + 1) % n]
            a, b, c = p[ia], p[ib], p[ic]
            if _cross2(a, b, c) <= eps:
                continue                                    # reflex or straight: not an ear
            rest = p[[i for i in idx if i not in (ia, ib, ic)]]
            if rest.size and np.any((_cross2(a, b, rest) >= -eps) & (_cross2(b, c, rest) >= -eps) & (_cross2(c, a, rest) >= -eps)):
                continue                                    # a vertex inside or on the triangle
            tris.append((ia, ib, ic))
            del idx[k]
            break
        else:
            raise ValueError("ear_clip: no ear found: the outline is not a simple polygon")
    tris.append(tuple(idx))
    return p[np.asarray(tris)]


def extrude_polygon(xy, z_lo, z_hi, rot, trans, ids):
    """An extruded polygon as a ConvexSet of triangular prisms.  xy (V,2): a simple polygon in the object's local x-y plane,
    either winding, non-convex allowed; the solid spans local z in [z_lo, z_hi]; pose x_world = rot . x_local + trans with rot
    (3,3) orthogonal; ids = (semantic id, instance id), repeated on every piece.  Each ear-clipped triangle gives 5 planes:
    its three sides (outward normals in the local x-y plane), bottom, top."""
    z_lo, z_hi = float(z_lo), float(z_hi)
    if not (np.isfinite(z_lo) and np.isfinite(z_hi) and z_lo < z_hi):
        raise ValueError("extrude_polygon: need finite z_lo < z_hi")
    rot, trans = _np(rot).astype(np.float64), _np(trans).astype(np.float64).reshape(-1)
    if rot.shape != (3, 3) or trans.shape != (3,) or not np.all(np.isfinite(rot)) or not np.all(np.isfinite(trans)):
        raise ValueError("extrude_polygon: rot must be (3, 3) and trans (3,), finite")
    if np.abs(rot @ rot.T - np.eye(3)).max() > 1e-6:
        raise ValueError("extrude_polygon: rot must be orthogonal (rot . rot^T = I to 1e-6)")
    try:
        tri = ear_clip(xy)                                  # (T,3,2) counter-clockwise
    except ValueError as e:
        raise ValueError(str(e).replace("ear_clip", "extrude_polygon")) from None
    T = tri.shape[0]
    e = np.roll(tri, -1, 1) - tri                            # (T,3,2) edge vectors
    nl = np.zeros((T, 5, 3))
    dl = np.empty((T, 5))
    nl[:, :3, 0], nl[:, :3, 1] = e[..., 1], -e[..., 0]       # outward of a counter-clockwise edge: (dy, -dx)
    nl[:, :3] /= np.linalg.norm(nl[:, :3], axis=2, keepdims=True)
    dl[:, :3] = np.einsum("tki,tki->tk", nl[:, :3, :2], tri)
    nl[:, 3, 2], dl[:, 3] = -1.0, -z_lo
    nl[:, 4, 2], dl[:, 4] = 1.0, z_hi
    nw = nl @ rot.T
    nw /= np.linalg.norm(nw, axis=2, keepdims=True)
    dw = dl + nw @ trans
    planes = np.concatenate([nw, dw[..., None]], -1).reshape(T * 5, 4)
    return ConvexSet(planes, np.arange(T + 1) * 5, _ids(ids, T, "extrude_polygon"))
