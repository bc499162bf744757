"""Mesh extraction: the lattice `Network.query_grid` samples -> a labelled triangle mesh of the surface field = level, on the
GPU (ops.mesh_count / mesh_emit; the rule is written out in include/pnr.h "mesh extraction").

`extract(field, lo, hi, level)` runs marching tetrahedra on the Kuhn split of the lattice: six tetrahedra a cube, no ambiguous
cases, neighbouring cubes agree on every face diagonal, so the surface is watertight wherever it does not leave the lattice.
Every vertex lies on a lattice edge and knows the lattice point on the inside end of that edge (`src`): `Mesh.labels(grid)`
reads any per-point array there.  `from_network` does query_grid + extract + labels.  The numbering of vertices and triangles
is part of the rule, so the result is the CPU restatement's bit for bit, and the same on every call.  `Mesh.sample` puts points
on the surface at a given density (ops.mesh_sample_count / mesh_sample_emit; include/pnr.h "nearest neighbours", MESH SAMPLING):
what `Evaluator.evaluate_geometry` compares with a ground-truth scan.  `Mesh.components` numbers the connected pieces of a
mesh (ops.cc_mesh; include/pnr.h "connected components"), and `Mesh.remove_small`, `Mesh.largest` and `from_network(min_faces=)`
drop the floaters a density field leaves.  `raycast` and `cast_rays` look at a mesh: the first hit of
every pixel's ray of any camera, or of a list of rays, with depth, face, nearest vertex, flat normal and the per-vertex
attributes carried into the image (ops.mesh_raycast / mesh_cast_rays through a `RayIndex`; include/pnr.h "mesh ray casting").

Conventions (this build's, unpinned: the reference ships no extractor): inside is field > level (NaN outside); positions are
query_grid's cell centres lo + (i + 0.5) step; triangles wind so that the normal points from inside to outside; vertices of
different edges are never merged, and zero-area triangles (a lattice value equal to level) are kept.  Out of scope: marching
cubes, welding of coincident vertices, removal of zero-area triangles, normals, decimation or smoothing, colours from the rgb
head (it needs a view direction), z-slab tiling of lattices beyond (2^31 - 1) / 12 points, OBJ or glTF output."""
import numpy as np
import torch

from . import ops
from .camera import is_camera


def _vec3(v, what):
    try:
        vals = [float(x) for x in (v.reshape(-1).tolist() if isinstance(v, (torch.Tensor, np.ndarray)) else v)]
    except (TypeError, ValueError):
        raise ValueError("%s must be three numbers (x, y, z)" % what) from None
    if len(vals) != 3:
        raise ValueError("%s must be three numbers (x, y, z), got %d" % (what, len(vals)))
    a = np.asarray(vals, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite (got %r)" % (what, vals))
    return a


def lattice(lo, hi, res):
    """(lo32, step32) of the lattice query_grid defines over the box [lo, hi] with res = (res_x, res_y, res_z) cells: float32
    lo, and step = (hi32 - lo32) / res32 -- one float32 subtraction and one division, on the host"""
    lo32, hi32 = _vec3(lo, "mesh: lo"), _vec3(hi, "mesh: hi")
    with np.errstate(all="ignore"):
        step = ((hi32 - lo32) / np.asarray(res, dtype=np.float32)).astype(np.float32)
    if not np.isfinite(step).all():
        raise ValueError("mesh: hi - lo overflows float32 (lo %r, hi %r)" % (lo32.tolist(), hi32.tolist()))
    return lo32, step


class Mesh:
    """vertices (V, 3) float32, faces (T, 3) int32, src (V,) int64 -- all on the GPU.  src[v] is the flat index
    (iz * res_y + iy) * res_x + ix of the lattice point on the inside end of vertex v's edge.  res = (res_x, res_y, res_z).
    attributes: per-vertex arrays attached by from_network; grid: the query_grid outputs from_network extracted from, else None.
    A mesh that did not come from a lattice (`from_arrays`) has src, res, lo, step and level None."""

    def __init__(self, vertices, faces, src, res, lo, step, level):
        self.vertices, self.faces, self.src = vertices, faces, src
        self.res, self.lo, self.step, self.level = None if res is None else tuple(res), lo, step, level
        self.attributes = {}
        self.grid = None

    @classmethod
    def from_arrays(cls, vertices, faces, attributes=None, device=None):
        """A mesh from plain arrays: vertices (V, 3) float32 and faces (F, 3) int32, torch tensors or numpy arrays, kept where they
        are or moved to `device`; attributes: a dict of per-vertex arrays (V, ...), moved with them.  No lattice stands behind
        such a mesh: src, res, lo, step and level are None, and labels() refuses it."""
        def tensor(name, a, dtype=None, cols=None):
            t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
            if not isinstance(t, torch.Tensor):
                raise ValueError("Mesh.from_arrays: %s must be a tensor or a numpy array, got %s" % (name, type(a).__name__))
            if dtype is not None and t.dtype != dtype:
                raise TypeError("Mesh.from_arrays: %s must be %s, got %s" % (name, dtype, t.dtype))
            if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
                raise ValueError("Mesh.from_arrays: %s must be (n, %d), got %s" % (name, cols, tuple(t.shape)))
            return (t if device is None else t.to(device)).contiguous()
        v, f = tensor("vertices", vertices, torch.float32, 3), tensor("faces", faces, torch.int32, 3)
        if v.device != f.device:
            raise ValueError("Mesh.from_arrays: faces is on %s, vertices on %s" % (f.device, v.device))
        m = cls(v, f, None, None, None, None, None)
        for name, a in (attributes or {}).items():
            t = tensor("attributes[%r]" % (name,), a)
            if t.dim() < 1 or t.shape[0] != v.shape[0] or t.device != v.device:
                raise ValueError("Mesh.from_arrays: attributes[%r] must hold one row per vertex (%d) on %s, got %s on %s"
                                 % (name, v.shape[0], v.device, tuple(t.shape), t.device))
            m.attributes[name] = t
        return m

    def __repr__(self):
        head = "Mesh(%d vertices, %d faces" % (self.vertices.shape[0], self.faces.shape[0])
        return head + (")" if self.res is None else ", lattice %d x %d x %d)" % self.res)

    def labels(self, grid):
        """grid[src]: any (res_z, res_y, res_x) tensor (labels, sigma, ...) read at the lattice point behind each vertex"""
        if self.res is None or self.src is None:
            raise ValueError("Mesh.labels: this mesh did not come from a lattice (Mesh.from_arrays): it has no src to read a grid at")
        rx, ry, rz = self.res
        if not isinstance(grid, torch.Tensor) or tuple(grid.shape) != (rz, ry, rx):
            raise ValueError("Mesh.labels: grid must be a (%d, %d, %d) tensor (res_z, res_y, res_x), got %s"
                             % (rz, ry, rx, tuple(grid.shape) if isinstance(grid, torch.Tensor) else type(grid).__name__))
        if grid.device != self.src.device:
            raise ValueError("Mesh.labels: grid is on %s, the mesh on %s" % (grid.device, self.src.device))
        return grid.reshape(-1)[self.src]

    def components(self):
        """The connected pieces of the mesh by its indices (components.MeshComponents: vertex_label, face_label, face_size, count
        on the device).  Never synchronises."""
        from . import components
        return components.label_mesh(self)

    def select(self, face_mask):
        """A new Mesh of the faces where face_mask (F,) bool is set: vertices no kept face uses are dropped, what remains keeps
        its order (a kept face with an index out of range is dropped); src and every attribute are carried over, the lattice fields
        kept.  Torch indexing on the mesh's device
        (fusion.filter_mesh's way); the sizes of the result are read back."""
        F, V = self.faces.shape[0], self.vertices.shape[0]
        if not isinstance(face_mask, torch.Tensor) or face_mask.dtype != torch.bool or tuple(face_mask.shape) != (F,):
            raise ValueError("Mesh.select: face_mask must be a (%d,) bool tensor, got %s" % (
                F, "%s %s" % (face_mask.dtype, tuple(face_mask.shape)) if isinstance(face_mask, torch.Tensor) else type(face_mask).__name__))
        if face_mask.device != self.faces.device:
            raise ValueError("Mesh.select: face_mask is on %s, the mesh on %s" % (face_mask.device, self.faces.device))
        f = self.faces.long()[face_mask]
        f = f[((f >= 0) & (f < V)).all(dim=1)]               # a face with an index out of range is dropped
        used = torch.zeros(V, dtype=torch.bool, device=self.vertices.device)
        used[f.reshape(-1)] = True
        new = torch.cumsum(used, 0) - 1
        index = torch.nonzero(used).reshape(-1)
        faces = new[f].to(torch.int32)
        m = Mesh(self.vertices[index], faces.contiguous(), None if self.src is None else self.src[index], self.res, self.lo, self.step, self.level)
        for name, a in self.attributes.items():
            m.attributes[name] = a[index]
        m.grid = self.grid
        return m

    def remove_small(self, min_faces):
        """select() of the pieces with at least min_faces faces; min_faces <= 1 keeps every valid face's piece"""
        return self.select(self.components().keep(min_faces))

    def largest(self, k=1):
        """select() of the k pieces with the most faces (a tie goes to the piece with the lower first vertex)"""
        return self.select(self.components().largest(k))

    def _corners(self):
        v = self.vertices.to(torch.float64)
        f = self.faces.long()
        return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]

    def area(self):
        """the surface area, summed in float64 torch (a Python float)"""
        p0, p1, p2 = self._corners()
        return float(torch.linalg.cross(p1 - p0, p2 - p0).norm(dim=1).sum() / 2.0)

    def volume(self):
        """the signed volume sum p0 . (p1 x p2) / 6 in float64 torch: positive for a closed surface, whose normals point outwards"""
        p0, p1, p2 = self._corners()
        return float((p0 * torch.linalg.cross(p1, p2)).sum() / 6.0)

    def sample(self, density=None, n=None, seed=0):
        """Points on the surface: (points (N, 3) float32, face (N,) int32), face[i] the triangle point i lies on; in triangle
        order, and the same for the same seed.  Exactly one of density (points per unit area) and n is given; n means
        density = n / self.area(), so ABOUT n points come back, not exactly n: a triangle of area a gets floor(a density + u)
        points, u uniform in [0, 1), at most 65535.  Degenerate triangles and triangles with a non-finite corner get none.
        Per-vertex attributes come through the triangle's first corner: mesh.attributes[name][mesh.faces[face, 0].long()].
        One host synchronisation, as in extract: the total is read back between the count and the emit launch; with n= there is
        a second one before it, because self.area() returns a Python float."""
        if (density is None) == (n is None):
            raise ValueError("Mesh.sample: give exactly one of density and n")
        if not self.vertices.is_cuda:
            raise RuntimeError("Mesh.sample: the mesh must be on the GPU (the HIP path has no CPU fallback)")
        if n is not None:
            n, area = int(n), self.area()
            if n < 0:
                raise ValueError("Mesh.sample: n must be >= 0 (got %d)" % n)
            if n and not (0.0 < area < float("inf")):
                raise ValueError("Mesh.sample: n needs a mesh of positive finite area (it is %r); give density instead" % area)
            density = n / area if n else 0.0
        total, start = ops.mesh_sample_count(self.vertices, self.faces, density, seed)
        N = int(total.item())                                   # the one host synchronisation
        if N > ops.NN_MAX_POINTS:
            raise ValueError("Mesh.sample: density %r asks for %d points, more than 2^31 - 1" % (density, N))
        dev = self.vertices.device
        points = torch.empty((N, 3), device=dev, dtype=torch.float32)
        face = torch.empty((N,), device=dev, dtype=torch.int32)
        if N:
            ops.mesh_sample_emit(self.vertices, self.faces, seed, start, points, face)
        return points, face

    def save_ply(self, path, colors=None, labels=None):
        """Write a binary little-endian PLY (host code: the arrays are copied off the device).  colors: (V, 3) uint8 as red green
        blue; labels: (V,) integers as an int32 `label` property."""
        V, T = self.vertices.shape[0], self.faces.shape[0]
        cols = [self.vertices.detach().cpu().numpy().astype("<f4")]
        dtype = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
        header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % V, "property float x", "property float y", "property float z"]
        if colors is not None:
            c = colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
            if c.shape != (V, 3) or c.dtype != np.uint8:
                raise ValueError("Mesh.save_ply: colors must be (%d, 3) uint8, got %s %s" % (V, c.shape, c.dtype))
            header += ["property uchar red", "property uchar green", "property uchar blue"]
            dtype += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        if labels is not None:
            lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
            if lab.shape != (V,) or lab.dtype.kind not in "iu":
                raise ValueError("Mesh.save_ply: labels must be (%d,) integers, got %s %s" % (V, lab.shape, lab.dtype))
            header += ["property int label"]
            dtype += [("label", "<i4")]
        header += ["element face %d" % T, "property list uchar int vertex_indices", "end_header"]
        rec = np.zeros((V,), dtype=np.dtype(dtype))
        rec["x"], rec["y"], rec["z"] = cols[0][:, 0], cols[0][:, 1], cols[0][:, 2]
        if colors is not None:
            rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
        if labels is not None:
            rec["label"] = lab
        face = np.zeros((T,), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        face["n"] = 3
        face["v"] = self.faces.detach().cpu().numpy()
        with open(path, "wb") as fh:
            fh.write(("\n".join(header) + "\n").encode("ascii"))
            fh.write(rec.tobytes())
            fh.write(face.tobytes())


def extract(field, lo, hi, level):
    """The mesh of field = level.  field: (res_z, res_y, res_x) float32 on the GPU, the layout query_grid returns, sampled at
    the cell centres of the box [lo, hi]; a point is inside where field > level.  Two launches' worth of work with ONE host
    synchronisation between them: ops.mesh_count classifies and scans, then the two totals are read back (`totals.tolist()`,
    which waits for the stream), the outputs are allocated at exactly that size, and ops.mesh_emit fills them.  A lattice
    with a res below 2 gives an empty mesh."""
    rx, ry, rz, level = ops._mesh_field("mesh.extract", field, level)
    lo32, step = lattice(lo, hi, (rx, ry, rz))
    if not field.is_cuda:
        raise RuntimeError("mesh.extract: field must be a GPU tensor (the HIP path has no CPU fallback)")
    totals, ws = ops.mesh_count(field, level)
    n_v, n_t = (int(v) for v in totals.tolist())            # the one host synchronisation
    dev = field.device
    vertices = torch.empty((n_v, 3), device=dev, dtype=torch.float32)
    faces = torch.empty((n_t, 3), device=dev, dtype=torch.int32)
    src = torch.empty((n_v,), device=dev, dtype=torch.int64)
    ops.mesh_emit(field, level, lo32, step, ws, vertices, faces, src)
    return Mesh(vertices, faces, src, (rx, ry, rz), lo32, step, level)


def _min_faces(what, min_faces):
    if isinstance(min_faces, bool) or not isinstance(min_faces, int) or min_faces < 0:
        raise ValueError("%s: min_faces must be an integer >= 0 (got %r)" % (what, min_faces))
    return min_faces


def from_network(net, lo, hi, res, level, want=("labels",), min_faces=0, **query_kw):
    """query_grid + extract on the raw density + per-vertex labels: the mesh of sigma = level of `net` over the box [lo, hi] at
    res cells per axis.  want: what query_grid computes beside sigma; "labels" also asks for "panoptic", so a network with
    both heads gives sem_label, inst_label and panoptic (query_grid leaves out the keys of a head the network lacks, "panoptic"
    with the semantic head: that is no refusal).  Every (res_z, res_y, res_x) output of the query is attached per
    vertex, through src, as mesh.attributes[name].  query_kw: query_grid's other keywords (is_thing, chunk, device, fast);
    nerf_level= is query()'s level (0 = coarse, 1 = fine), since `level` is the iso-value here.  mesh.grid holds the query's
    own outputs.  min_faces > 0: the pieces of fewer faces -- the floaters of a density field -- are removed last
    (Mesh.remove_small); 0 returns every piece."""
    min_faces = _min_faces("mesh.from_network", min_faces)
    want = (want,) if isinstance(want, str) else tuple(want)
    level = float(level)
    if not (abs(level) < float("inf")):
        raise ValueError("mesh.from_network: level must be finite (got %r)" % level)
    lattice(lo, hi, (1, 1, 1))                               # refuse a bad box before the network runs
    asked = ("sigma",) + tuple(w for w in want if w != "sigma") + (("panoptic",) if "labels" in want and "panoptic" not in want else ())
    if "nerf_level" in query_kw:
        query_kw["level"] = query_kw.pop("nerf_level")
    grid = net.query_grid(lo, hi, res, want=asked, **query_kw)
    mesh = extract(grid["sigma"].contiguous(), lo, hi, level)
    for name, g in grid.items():
        if g.dim() == 3:
            mesh.attributes[name] = mesh.labels(g)
    mesh.grid = grid
    return mesh.remove_small(min_faces) if min_faces else mesh


HIT, NO_RAY, MISSED = ops.RAYCAST_HIT, ops.RAYCAST_NO_RAY, ops.RAYCAST_MISSED
_TWO_FACES_A_CELL = 2.0


class RayIndex:
    """The uniform grid `raycast` and `cast_rays` prune with (include/pnr.h "mesh ray casting", THE INDEX): per cell the 48-byte
    records -- three corners and the face index -- of the faces whose padded box touches it.  It never changes an answer: a cast
    equals brute force over all faces bit for bit, whatever `res` is.

    The build SYNCHRONISES twice, as mesh.extract and Mesh.sample read their totals: the bounds of the usable faces (every index
    in range, every corner finite) are read back to choose the resolution, and the entry total to size the records.  The box is
    the bounds widened per side by max(extent / 1024, largest |coordinate| / 2^20, 1e-30), so a flat mesh still has cells of
    positive size.  res=None: about two faces a cell -- (volume / (usable faces / 2))^(1/3) over the axes that are not flat gives the
    number of cells per axis, at most 1024, one cell on a flat axis; res=(res_x, res_y, res_z) overrides it.  The cells are cubes: one
    size, the smallest with which res cells cover the box on every axis (grid_box).
    Memory: 48 bytes per entry (a face is entered in every cell it touches: two to three times on a mesh whose triangles are
    about the size of a cell, and (cells it spans) times when they are much larger) plus 4 bytes per cell; an entry total above
    2^31 - 1 is refused.  The index is for the mesh as it was: after vertices move, build a new one."""

    def __init__(self, mesh, res=None):
        if not isinstance(mesh, Mesh):
            raise TypeError("mesh.RayIndex: mesh must be a mesh.Mesh")
        if res is not None:
            res = ops.meshcast_res("mesh.RayIndex", res)
        V, F = ops.meshcast_mesh("mesh.RayIndex", mesh.vertices, mesh.faces)
        if not mesh.vertices.is_cuda:
            raise RuntimeError("mesh.RayIndex: the mesh must be on the GPU (the HIP path has no CPU fallback)")
        self.n_vertices, self.n_faces = V, F
        b = ops.mesh_grid_bounds(mesh.vertices, mesh.faces).cpu()   # the first host synchronisation: all eight words at once
        usable = int(b.view(torch.int32)[6])
        self.lo, self.cell, auto = grid_box(b[:6].numpy(), usable, res)
        self.res = auto if res is None else res
        total, self.start, ws = ops.mesh_grid_count(mesh.vertices, mesh.faces, self.res, self.lo, self.cell)
        n = int(total.item())                                     # the second
        if n > ops.MESHCAST_MAX_ENTRIES:
            raise ValueError("mesh.RayIndex: a grid of %d x %d x %d holds %d entries, more than 2^31 - 1; pass a coarser res" % (self.res + (n,)))
        self.records = torch.empty((n, 12), device=mesh.vertices.device, dtype=torch.float32)
        ops.mesh_grid_fill(mesh.vertices, mesh.faces, self.res, self.lo, self.cell, self.start, self.records, ws)

    def __repr__(self):
        return "RayIndex(%d x %d x %d cells, %d entries of %d faces)" % (self.res + (self.records.shape[0], self.n_faces))


def grid_box(bounds, usable, res=None):
    """(lo, cell, res) of a RayIndex from the six bounds (float32 numpy) of `usable` faces: float32 numpy lo and cell size per
    axis and the resolution (the default, or `res` as given).  The cells are CUBES -- one size on all three axes, the smallest
    with which `res` cells cover the widened box on every axis, the box centred in the grid: a cast walks the grid only while
    its reach is within 4096 of the SMALLEST cell (include/pnr.h), so unequal cells would send rays to the plain loop.  Host
    arithmetic; the rule is RayIndex's docstring."""
    f = np.float32
    if not usable or not np.isfinite(bounds).all():
        return np.zeros(3, f), np.ones(3, f), (1, 1, 1)
    lo, hi = bounds[:3].astype(f), bounds[3:6].astype(f)
    with np.errstate(all="ignore"):
        ext = (hi - lo).astype(np.float64)
    if not np.isfinite(ext).all():
        raise ValueError("mesh.RayIndex: the mesh's bounds %r leave no finite float32 grid" % (bounds[:6].tolist(),))
    if res is None:
        live = ext > 0
        k = int(live.sum())
        r = [1, 1, 1]
        if k:
            side = (float(np.prod(ext[live])) / max(usable / _TWO_FACES_A_CELL, 1.0)) ** (1.0 / k)
            r = [min(max(int(np.ceil(e / side)), 1), ops.MESHCAST_MAX_RES) if l and side > 0 else 1 for e, l in zip(ext, live)]
        res = tuple(r)
    with np.errstate(all="ignore"):
        m = f(max(float(ext.max()) / 1024.0, float(np.abs(bounds[:6]).max()) / 2.0 ** 20, 1e-30))
        lo, hi = (lo - m).astype(f), (hi + m).astype(f)
        r32 = np.asarray(res, f)
        side = ((hi - lo) / r32).astype(f).max()
        lo = (lo - (r32 * side - (hi - lo)) * f(0.5)).astype(f)
        cell = np.full(3, side, f)
    if not (np.isfinite(lo).all() and np.isfinite(side) and side > 0 and (lo + r32 * side >= hi - m).all() and (lo <= bounds[:3]).all()):
        raise ValueError("mesh.RayIndex: the mesh's bounds %r leave no finite float32 grid" % (bounds[:6].tolist(),))
    return lo, cell, res


def _index_for(what, mesh, index):
    if not isinstance(mesh, Mesh):
        raise TypeError("%s: mesh must be a mesh.Mesh" % what)
    if index is None:
        return RayIndex(mesh)
    if not isinstance(index, RayIndex):
        raise TypeError("%s: index must be a mesh.RayIndex" % what)
    if (index.n_vertices, index.n_faces) != (mesh.vertices.shape[0], mesh.faces.shape[0]):
        raise ValueError("%s: index was built for a mesh of %d vertices and %d faces, this one has %d and %d"
                         % (what, index.n_vertices, index.n_faces, mesh.vertices.shape[0], mesh.faces.shape[0]))
    return index


def _attribute_names(what, mesh, attributes):
    taken = [n for n, _, _ in ops.MESHCAST_OUTPUTS] + ["valid"]
    for name in mesh.attributes if attributes else ():
        if name in taken:
            raise ValueError("%s: the attribute %r has the name of one of the maps (%s); rename it or pass attributes=False"
                             % (what, name, ", ".join(taken)))


def _cast_maps(mesh, lead, normals):
    dev = mesh.vertices.device
    return {n: torch.empty(lead + tail, dtype=dt, device=dev) for n, dt, tail in ops.MESHCAST_OUTPUTS if normals or n != "normal"}


def _finish(mesh, maps, attributes):
    maps["valid"] = maps["code"] == HIT
    if attributes:
        at = maps["vertex"].clamp(min=0).long()
        for name, a in mesh.attributes.items():
            if not mesh.vertices.shape[0]:
                continue
            v = maps["valid"].reshape(maps["valid"].shape + (1,) * (a.dim() - 1))
            off = torch.zeros((), dtype=a.dtype, device=a.device) if a.dtype == torch.uint8 or a.dtype.is_floating_point or a.dtype == torch.bool \
                else torch.full((), -1, dtype=a.dtype, device=a.device)
            maps[name] = torch.where(v, a[at], off)
    return maps


def raycast(mesh, camera, c2w, near, far, index=None, normals=True, attributes=True):
    """Render `mesh` into (camera, c2w): the first hit of every pixel's ray, in ONE launch (ops.mesh_raycast; the rule is in
    include/pnr.h "mesh ray casting"): a watertight ray-triangle test, two-sided, the nearest face winning and a tie going to the
    lowest face index -- a ray through a shared edge or vertex of a closed mesh hits (a hit must lie within its face's box:
    a ray in the plane of a face does not hit that face somewhere else).  camera: camera.Pinhole / Fisheye /
    Equirect; c2w: 3x4 camera-to-world; index: a RayIndex of this mesh (None: one is built here, which synchronises twice -- keep
    one to cast again).  Returns a maps dict of (height, width, ...) images on the mesh's device, which (camera, c2w, maps)
    makes a view for consistency.reproject, pointcloud.lift, Evaluator.evaluate_depth and fusion.track:
        depth   float32   the ray parameter of the hit, render_view's convention (z-depth in a pinhole, range in a fisheye /
                          equirect frame); 0 off the surface
        code    uint8     HIT, NO_RAY or MISSED;  valid  bool = code == HIT
        face    int32     the face hit;  vertex  int32  its corner nearest the hit;  both -1 off the surface
        bary    float32 (., 3)  the weights of the face's three corners at the hit, 0 off the surface
        normal  float32 (., 3)  with normals: the face's unit normal turned towards the camera, 0 off the surface
        side    int8      +1 where the ray met the side the winding normal points to, -1 the other, 0 off the surface
        with attributes: every per-vertex array of mesh.attributes gathered at vertex with torch indexing -- integer arrays -1
        off the surface, uint8 colours and floats 0.  An attribute named like one of the maps above is refused by name.
    The cast never synchronises and can be captured in a graph."""
    what = "mesh.raycast"
    index = _index_for(what, mesh, index)
    _attribute_names(what, mesh, attributes)
    if not is_camera(camera):
        raise TypeError("%s: camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect, not %r" % (what, camera))
    near, far = ops.meshcast_range(what, near, far)
    if not mesh.vertices.is_cuda:
        raise RuntimeError("%s: the mesh must be on the GPU (the HIP path has no CPU fallback)" % what)
    h, w = int(camera.height), int(camera.width)
    maps = _cast_maps(mesh, (h, w), normals)
    ops.mesh_raycast(camera.model, camera.params, c2w, w, h, near, far, mesh.vertices, mesh.faces, index.res, index.lo, index.cell,
                     index.start, index.records, maps)
    return _finish(mesh, maps, attributes)


def cast_rays(mesh, rays, index=None, normals=True, attributes=True):
    """`raycast` along rays (n, 8) float32 = (o, d, near, far) on the mesh's device (ops.mesh_cast_rays): the same maps as (n, ...)
    arrays; depth is in units of each ray's own d.  A ray with a non-finite o or d, d = 0 or !(0 <= near <= far) is NO_RAY.
    Consecutive rays share a wave: callers who want coherence sort them.  The rays are read when the kernel runs, so a captured
    cast follows a ray tensor edited in place."""
    what = "mesh.cast_rays"
    index = _index_for(what, mesh, index)
    _attribute_names(what, mesh, attributes)
    if not isinstance(rays, torch.Tensor) or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError("%s: rays must be an (n, 8) float32 tensor, got %s"
                         % (what, "%s %s" % (rays.dtype, tuple(rays.shape)) if isinstance(rays, torch.Tensor) else type(rays).__name__))
    if not mesh.vertices.is_cuda:
        raise RuntimeError("%s: the mesh must be on the GPU (the HIP path has no CPU fallback)" % what)
    maps = _cast_maps(mesh, (rays.shape[0],), normals)
    ops.mesh_cast_rays(rays, mesh.vertices, mesh.faces, index.res, index.lo, index.cell, index.start, index.records, maps)
    return _finish(mesh, maps, attributes)
