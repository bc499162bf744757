"""Point clouds and views: the forward direction of consistency.py (ops.splat_points / pnr_splat_points; the rule is written
out in include/pnr.h "point splatting"), and cloud against cloud: an exact fixed-radius nearest-neighbour search (ops.nn_build /
nn_query; include/pnr.h "nearest neighbours").

`splat(camera, c2w, points)` scatters world points -- a LiDAR scan, labelled 3D points, a cloud from `Network.query_grid` --
into a view of any camera model through a z-buffer: per pixel the nearest point wins, a depth tie goes to the lowest index.
`lift(view)` turns a rendered view back into a cloud, `forward_warp(view_a, camera_b, c2w_b)` does both.  `consistency.warp`
is a backward gather and needs B's depth; `forward_warp` is a forward scatter, needs only A, and leaves holes.
`NearestIndex(ref, max_dist)` is a spatial-hash index over a reference cloud; `nearest(query, ref, max_dist, labels=)` finds for
every query point the nearest reference point within max_dist and carries the reference's labels or colours over: from an
annotated 3D scan onto mesh vertices or `Network.query` points.  `Evaluator.evaluate_geometry` builds its metrics on the same search.

Conventions (this build's, unpinned): nearest pixel, a square footprint of half width `radius` clipped at the border (no
longitude wrap), depth as render_view writes it (z-depth in a pinhole view, range in a fisheye / equirect view), 0 where no
point landed.  The nearest neighbour is the float32 squared distance's, a tie goes to the lowest index, a reference point counts
when its distance is at most max_dist (inclusive), non-finite reference points are never found, and a non-finite query finds
nothing; the answer is brute force's bit for bit, whatever the size of the hash table.  Out of scope: see-through removal for
sparse clouds, weighted or sub-pixel splats, per-point radii or normals, reading scan files, gradients through the splat; more
than one neighbour per query, point-to-triangle distance, a closest-point (non-projective) ICP on top of the index, sorting the
queries by cell."""
import torch

from . import consistency, ops
from .camera import invert_pose


def _table(t, n, name):
    if not isinstance(t, torch.Tensor) or t.dim() < 1:
        raise ValueError("pointcloud.splat: %s must be a tensor with one row per point" % name)
    if t.shape[0] < n:
        raise ValueError("pointcloud.splat: %s holds %d rows, the cloud reaches index %d" % (name, t.shape[0], n))
    return t


def gather(table, index, fill):
    """table[index] where index >= 0, `fill` elsewhere (torch indexing, as consistency.warp gathers)"""
    if table.device != index.device:
        raise ValueError("pointcloud: the attribute table is on %s, the index image on %s" % (table.device, index.device))
    got = table[index.clamp(min=0).long()]
    seen = (index >= 0).reshape(*index.shape, *([1] * (got.dim() - index.dim())))
    return torch.where(seen, got, torch.full_like(got, fill))


def splat(camera, c2w, points, labels=None, colors=None, near=0.0, far=float("inf"), radius=0, into=None, index_base=0):
    """Scatter world points (P, 3) on the GPU into the view (camera, c2w).  Returns a dict:
      depth (height, width) float32: depth of the nearest point per pixel, 0 where none landed;
      index (height, width) int32: that point's index_base + i, -1 where none;   valid = index >= 0;
      zbuf  (height, width) int64: the packed buffer, to pass as `into=` of a later call (multi-scan fusion: each call its
            own index_base range; the result does not depend on the order of the calls);
      label / rgb: labels (N, ...) / colors (N, 3) gathered through index, -1 / 0 where no point landed.  With `into=` the
            tables are the CONCATENATED tables of every call so far (row = global index)."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("pointcloud.splat: points must be a (P, 3) tensor")
    top = int(index_base) + points.shape[0]
    if labels is not None:
        _table(labels, top, "labels")
    if colors is not None:
        _table(colors, top, "colors")
    zbuf = ops.splat_points(camera, invert_pose(c2w), points, zbuf=into, index_base=index_base, near=near, far=far, radius=radius)
    depth, index = ops.splat_resolve(zbuf)
    out = {"depth": depth, "index": index, "valid": index >= 0, "zbuf": zbuf}
    if labels is not None:
        out["label"] = gather(labels, index, -1)
    if colors is not None:
        out["rgb"] = gather(colors, index, 0)
    return out


class NearestIndex:
    """A spatial-hash index over the reference cloud ref (n, 3) float32 on the GPU for searches within max_dist (ops.nn_build).
    It owns `start`, `records` and `ref` itself -- not a copy: the cell origin is read from ref[0] on the device, so ref must stay
    as it was built.  table_bits: 2^table_bits buckets instead of the default max(1024, the power of two at or above 2 n)."""

    def __init__(self, ref, max_dist, table_bits=None):
        self.max_dist = float(max_dist)
        self.start, self.records = ops.nn_build(ref, max_dist, table_bits)
        self.ref = ref
        self.table_size = self.start.numel() - 1

    def __len__(self):
        return self.ref.shape[0]

    def query(self, points, stats=None):
        """For every row of points (m, 3) float32 the nearest reference point within max_dist.  Returns a dict: index (m,) int32,
        -1 where there is none; dist2 (m,) float32, the squared distance, +inf where there is none; valid = index >= 0.
        stats: (3,) int64 on the device, accumulated: found / none in the radius / invalid queries.  No host synchronisation."""
        index, dist2 = ops.nn_query(self.ref, self.start, self.records, points, self.max_dist, stats=stats)
        return {"index": index, "dist2": dist2, "valid": index >= 0}

    def dist(self, points):
        """the distance to the nearest reference point, +inf where none is within max_dist"""
        return self.query(points)["dist2"].sqrt()


def nearest(query, ref, max_dist, labels=None, colors=None):
    """Build an index over ref (n, 3), query it with query (m, 3), and carry attributes of ref onto the queries.  Returns
    NearestIndex.query's dict plus label / rgb: labels (n, ...) / colors (n, 3) of the reference cloud gathered through index,
    -1 / 0 where no reference point is within max_dist."""
    for name, t in (("labels", labels), ("colors", colors)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() < 1 or not isinstance(ref, torch.Tensor) or t.shape[0] != ref.shape[0]):
            raise ValueError("pointcloud.nearest: %s must be a tensor with one row per reference point" % name)
    out = NearestIndex(ref, max_dist).query(query)
    if labels is not None:
        out["label"] = gather(labels, out["index"], -1)
    if colors is not None:
        out["rgb"] = gather(colors, out["index"], 0)
    return out


def lift(view, depth=None):
    """World points of a view (camera, c2w, maps), as consistency takes views: points (m, 3) float32 and pix (m) int32, the
    linear indices of the pixels whose depth is positive and finite and that lie inside the lens.  X = rays_o + depth * rays_d
    on camera.rays, one multiply and one add per component: the arithmetic of reprojection step 3.  depth: the maps key."""
    cam, c2w, d = consistency.view_depth(view, "view", depth)
    if not d.is_cuda:
        raise RuntimeError("pointcloud.lift: the depth image is not on the GPU (the HIP path has no CPU fallback)")
    pix = cam.valid_pix(d.device)
    t = d.reshape(-1)[pix.long()]
    keep = (t > 0) & torch.isfinite(t)
    pix, t = pix[keep].contiguous(), t[keep]
    rays = cam.rays(c2w, 0.0, 0.0, pix=pix)
    prod = t[:, None] * rays[:, 3:6]
    return (rays[:, 0:3] + prod).contiguous(), pix


def forward_warp(view_a, camera_b, c2w_b, radius=0, images=None, near=0.0, far=float("inf")):
    """Lift view A and splat it into (camera_b, c2w_b).  Returns a dict: depth / index / valid / zbuf as `splat` (index counts
    A's lifted points), source (height_b, width_b) int32 = the pixel of A seen at each pixel of B (-1 in the holes), and
    images: {name: the image of A carried into B's grid} for every (height_a, width_a, ...) tensor in `images` (integer
    images are filled with -1 in the holes, others with 0)."""
    cam_a = consistency._view(view_a, "view_a")[0]
    images = dict(images or {})
    for name, img in images.items():
        if not isinstance(img, torch.Tensor) or tuple(img.shape[:2]) != (cam_a.height, cam_a.width):
            raise ValueError("pointcloud.forward_warp: image %r must be a (%d, %d, ...) tensor of view A" % (name, cam_a.height, cam_a.width))
    points, pix = lift(view_a)
    out = splat(camera_b, c2w_b, points, near=near, far=far, radius=radius)
    out["source"] = gather(pix, out["index"], -1)
    out["images"] = {}
    for name, img in images.items():
        flat = img.reshape(cam_a.height * cam_a.width, *img.shape[2:])
        out["images"][name] = gather(flat, out["source"], 0 if img.dtype.is_floating_point or img.dtype == torch.bool else -1)
    return out
