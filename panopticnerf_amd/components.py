"""Connected components of images, lattices and meshes on the GPU (ops.cc_label / cc_mesh / cc_stats; the rule is written out in
include/pnr.h "connected components").

    c = components.label(mask)                      # a 2-D or 3-D bool / integer / float32 GPU tensor
    mask = c.keep(100)                              # the components of at least 100 elements: no read-back
    segments = components.label(grid["panoptic"], connectivity=26)       # one car, then another
    print(segments.n, segments.sizes(), segments.boxes(lo, step))
    parts = components.label_mesh(mesh)             # or mesh.components(); mesh.largest(), mesh.remove_small(500)

Integer data are KEYS: an element is foreground where its key is >= 0 (False of a bool mask becomes -1) and two neighbours are
linked where their keys are equal, so a panoptic lattice splits into its instances.  float32 data are VALUES and need `tol`:
foreground where finite and > 0 (the "0 = no depth" convention), linked where |a - b| <= tol; a component is the transitive
closure.  The components are numbered by their lowest flat index (raster order of the first element, scipy.ndimage.label's
order), so the result is the CPU restatement's bit for bit, whatever the GPU's schedule.  `label` and `label_mesh` never
synchronise and can be captured in a graph; `.n`, `.sizes()`, `.boxes()` and `.largest()` read the count back once.

Out of scope: periodic lattices, anisotropic or user-given neighbourhoods, labels beyond int32, merging of coincident mesh
vertices (mesh.extract already shares the vertex of a lattice edge between the faces round it)."""
import torch

from . import ops

_CONNECTIVITY = {2: (4, 8), 3: (6, 26)}


def _full(what, dim, connectivity):
    few, many = _CONNECTIVITY[dim]
    if connectivity is None:
        return False
    if isinstance(connectivity, bool) or connectivity not in (few, many):
        raise ValueError("%s: connectivity must be %d or %d for a %d-D tensor (got %r)" % (what, few, many, dim, connectivity))
    return connectivity == many


def _keys(what, x):
    """x as the int32 keys or float32 values cc_label takes"""
    if x.dtype in (torch.int32, torch.float32):
        return x
    if x.dtype == torch.bool:
        return x.to(torch.int32) - 1
    if x.dtype in (torch.uint8, torch.int16):
        return x.to(torch.int32)
    if x.dtype == torch.int64:
        raise TypeError("%s: int64 keys are not taken (a key beyond int32 could not be told without reading back): cast to int32" % what)
    raise TypeError("%s: x must be bool, uint8, int16 or int32 (keys) or float32 (values), got %s" % (what, x.dtype))


class _Counted:
    """what Components and MeshComponents share: the count read back once, and the statistics through ops.cc_stats"""

    @property
    def n(self):
        """the number of components, a Python int: ONE host synchronisation, then cached"""
        if self._n is None:
            self._n = int(self.count.item())
        return self._n

    def _stats(self):
        if self._sizes is None:
            lab, size = self._stat_arrays()
            self._sizes, self._boxes = ops.cc_stats(lab, size, self.n, boxes=self._want_boxes)
        return self._sizes, self._boxes

    def sizes(self):
        """(n,) int32 on the device: the number of elements (faces, for a mesh) of every component"""
        return self._stats()[0]

    def _largest(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError("largest: k must be an integer >= 0 (got %r)" % (k,))
        sizes = self.sizes()
        keep = torch.zeros((self.n + 1,), dtype=torch.bool, device=sizes.device)       # the last row: label -1
        if k and self.n:
            order = torch.sort(sizes, descending=True, stable=True).indices            # a tie goes to the lower number
            keep[order[:k]] = True
        return keep


class Components(_Counted):
    """labels (int32, x's shape; -1 on background), count (1,) int64 on the device, size (int32, x's shape; None when label was
    called with size=False).  connectivity is the one used."""

    _want_boxes = True

    def __init__(self, labels, count, size, connectivity):
        self.labels, self.count, self.size, self.connectivity = labels, count, size, connectivity
        self._n = self._sizes = self._boxes = None

    def __repr__(self):
        return "Components(%s, connectivity %d%s)" % (" x ".join(str(s) for s in self.labels.shape), self.connectivity,
                                                      "" if self._n is None else ", %d components" % self._n)

    def _need_size(self, what):
        if self.size is None:
            raise ValueError("Components.%s: label was called with size=False" % what)

    def keep(self, min_size):
        """bool mask of the elements whose component holds at least min_size elements; never synchronises"""
        self._need_size("keep")
        return self.size >= max(int(min_size), 1)

    def _stat_arrays(self):
        self._need_size("sizes")
        return self.labels, self.size

    def boxes(self, lo=None, step=None):
        """(n, 6) int32 (ix_min, iy_min, iz_min, ix_max, iy_max, iz_max) in lattice indices; with lo and step (three numbers each,
        x y z) the world-space corners (n, 2, 3) float32: lo + i_min * step and lo + (i_max + 1) * step"""
        boxes = self._stats()[1]
        if lo is None and step is None:
            return boxes
        if lo is None or step is None:
            raise ValueError("Components.boxes: give both lo and step, or neither")
        lo_h, step_h = ops._lattice_floats("Components.boxes", lo, step, nonzero_step=False)
        lo_t = torch.tensor(list(lo_h), dtype=torch.float32, device=boxes.device)
        step_t = torch.tensor(list(step_h), dtype=torch.float32, device=boxes.device)
        b = boxes.to(torch.float32)
        return torch.stack((lo_t + b[:, :3] * step_t, lo_t + (b[:, 3:] + 1.0) * step_t), dim=1)

    def largest(self, k=1):
        """bool mask of the k largest components; a size tie goes to the lower number"""
        return self._largest(k)[self.labels.long()]


class MeshComponents(_Counted):
    """vertex_label (V,) and face_label (F,) int32 (-1: a vertex no valid face uses, a face with an index out of range),
    face_size (F,) int32 the valid faces of each face's component, count (1,) int64 on the device"""

    _want_boxes = False

    def __init__(self, vertex_label, face_label, face_size, count):
        self.vertex_label, self.face_label, self.face_size, self.count = vertex_label, face_label, face_size, count
        self._n = self._sizes = self._boxes = None

    def __repr__(self):
        return "MeshComponents(%d vertices, %d faces%s)" % (self.vertex_label.shape[0], self.face_label.shape[0],
                                                            "" if self._n is None else ", %d components" % self._n)

    def _stat_arrays(self):
        return self.face_label, self.face_size

    def keep(self, min_faces):
        """bool mask of the faces whose component holds at least min_faces valid faces; never synchronises"""
        return self.face_size >= max(int(min_faces), 1)

    def largest(self, k=1):
        """bool mask of the faces of the k components with the most faces; a tie goes to the lower number"""
        return self._largest(k)[self.face_label.long()]


def label(x, connectivity=None, tol=None, size=True):
    """The connected components of a 2-D or 3-D GPU tensor, as a `Components` record.  bool, uint8, int16 and int32 are keys
    (False becomes -1; int64 is refused: cast it); float32 are values and need tol.  connectivity: 4 (default) or 8 for 2-D, 6
    (default) or 26 for 3-D.  Never synchronises."""
    what = "components.label"
    ops._tensor(what, "x", x)
    if x.dim() not in _CONNECTIVITY:
        raise ValueError("%s: x must be 2-D (an image) or 3-D (res_z, res_y, res_x), got %s" % (what, tuple(x.shape)))
    full = _full(what, x.dim(), connectivity)
    data = _keys(what, x)
    if data.dtype == torch.float32:
        if tol is None:
            raise ValueError("%s: float32 x are values and need tol" % what)
        tol = ops.cc_tol(what, tol)
    elif tol is not None:
        raise ValueError("%s: tol goes with float32 values; integer keys are linked where they are equal" % what)
    if not x.is_cuda:
        raise RuntimeError("%s: x must be a GPU tensor (the HIP path has no CPU fallback)" % what)
    labels, sz, count = ops.cc_label(data.contiguous(), full, tol, size=bool(size))
    return Components(labels, count, sz, _CONNECTIVITY[x.dim()][int(full)])


def label_mesh(mesh):
    """The connected components of a mesh.Mesh by its indices, as a `MeshComponents` record.  Never synchronises."""
    from .mesh import Mesh
    if not isinstance(mesh, Mesh):
        raise TypeError("components.label_mesh: mesh must be a mesh.Mesh")
    if not mesh.faces.is_cuda:
        raise RuntimeError("components.label_mesh: the mesh must be on the GPU (the HIP path has no CPU fallback)")
    return MeshComponents(*ops.cc_mesh(mesh.faces, int(mesh.vertices.shape[0])))
