"""Mesh extraction: the lattice `Network.query_grid` samples -> a labelled triangle mesh of the surface field = level, on the
GPU (ops.mesh_count / mesh_emit; the rule is written out in include/pnr.h "mesh extraction").

`extract(field, lo, hi, level)` runs marching tetrahedra on the Kuhn split of the lattice: six tetrahedra a cube, no ambiguous
cases, neighbouring cubes agree on every face diagonal, so the surface is watertight wherever it does not leave the lattice.
Every vertex lies on a lattice edge and knows the lattice point on the inside end of that edge (`src`): `Mesh.labels(grid)`
reads any per-point array there.  `from_network` does query_grid + extract + labels.  The numbering of vertices and triangles
is part of the rule, so the result is the CPU restatement's bit for bit, and the same on every call.  `Mesh.sample` puts points
on the surface at a given density (ops.mesh_sample_count / mesh_sample_emit; include/pnr.h "nearest neighbours", MESH SAMPLING):
what `Evaluator.evaluate_geometry` compares with a ground-truth scan.

Conventions (this build's, unpinned: the reference ships no extractor): inside is field > level (NaN outside); positions are
query_grid's cell centres lo + (i + 0.5) step; triangles wind so that the normal points from inside to outside; vertices of
different edges are never merged, and zero-area triangles (a lattice value equal to level) are kept.  Out of scope: marching
cubes, welding of coincident vertices, removal of zero-area triangles, normals, decimation or smoothing, colours from the rgb
head (it needs a view direction), z-slab tiling of lattices beyond (2^31 - 1) / 12 points, OBJ or glTF output."""
import numpy as np
import torch

from . import ops


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
    attributes: per-vertex arrays attached by from_network; grid: the query_grid outputs from_network extracted from, else None."""

    def __init__(self, vertices, faces, src, res, lo, step, level):
        self.vertices, self.faces, self.src = vertices, faces, src
        self.res, self.lo, self.step, self.level = tuple(res), lo, step, level
        self.attributes = {}
        self.grid = None

    def __repr__(self):
        return "Mesh(%d vertices, %d faces, lattice %d x %d x %d)" % ((self.vertices.shape[0], self.faces.shape[0]) + self.res)

    def labels(self, grid):
        """grid[src]: any (res_z, res_y, res_x) tensor (labels, sigma, ...) read at the lattice point behind each vertex"""
        rx, ry, rz = self.res
        if not isinstance(grid, torch.Tensor) or tuple(grid.shape) != (rz, ry, rx):
            raise ValueError("Mesh.labels: grid must be a (%d, %d, %d) tensor (res_z, res_y, res_x), got %s"
                             % (rz, ry, rx, tuple(grid.shape) if isinstance(grid, torch.Tensor) else type(grid).__name__))
        if grid.device != self.src.device:
            raise ValueError("Mesh.labels: grid is on %s, the mesh on %s" % (grid.device, self.src.device))
        return grid.reshape(-1)[self.src]

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


def from_network(net, lo, hi, res, level, want=("labels",), **query_kw):
    """query_grid + extract on the raw density + per-vertex labels: the mesh of sigma = level of `net` over the box [lo, hi] at
    res cells per axis.  want: what query_grid computes beside sigma; "labels" also asks for "panoptic", so a network with
    both heads gives sem_label, inst_label and panoptic (query_grid leaves out the keys of a head the network lacks, "panoptic"
    with the semantic head: that is no refusal).  Every (res_z, res_y, res_x) output of the query is attached per
    vertex, through src, as mesh.attributes[name].  query_kw: query_grid's other keywords (is_thing, chunk, device, fast);
    nerf_level= is query()'s level (0 = coarse, 1 = fine), since `level` is the iso-value here.  mesh.grid holds the query's
    own outputs."""
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
    return mesh
