"""Cross-view consistency: join two rendered views through depth (ops.reproject / pnr_reproject; the rule is written out in
include/pnr.h "cross-view reprojection").

A view is `(camera, c2w, maps)`: a camera.Pinhole / Fisheye / Equirect, its 3x4 camera-to-world pose (host values) and what
`Renderer.render_view` returned for it -- or any dict that holds a (height, width) depth image on the GPU under `depth_key`.
`reproject(view_a, view_b)` says for every pixel of A which pixel of B shows the same surface point (or why none does),
`warp(image_b, match)` carries any image of B into A's pixel grid along that match.  `Evaluator.evaluate_pair` builds the
multi-view consistency metric on the same kernel.

Conventions (this build's, unpinned like the evaluator's other conventions): nearest target pixel, no sub-pixel lookup; a
pixel is visible when the depth B renders at the matched pixel agrees with the depth the lifted point has in B,
|e - depth_b[q]| <= tol[0] + tol[1] * e with the default tol = (0, 0.02); depth is z-depth in a pinhole frame and range in a
fisheye frame, as render_view writes it.  The forward direction (splatting with a z-buffer) and depth-error metrics live in
pointcloud.py and Evaluator.evaluate_depth.  Out of scope: bilinear lookup, reading poses from files, more than two views per call."""
import torch

from . import ops
from .camera import invert_pose

NOTHING, LEFT_VIEW, UNKNOWN, OCCLUDED = -1, -2, -3, -4        # match codes (include/pnr.h "cross-view reprojection")
DEFAULT_TOL = (0.0, 0.02)


def depth_key(maps, key=None):
    """The depth image of a maps dict: `key`, else the finest depth_<level> present, else "depth"."""
    if key is not None:
        if key not in maps:
            raise ValueError("consistency: the view's maps hold no %r" % (key,))
        return key
    for k in ("depth_1", "depth_0", "depth"):
        if k in maps:
            return k
    raise ValueError("consistency: the view's maps hold no depth image (depth_1, depth_0 or depth)")


def _view(view, what):
    try:
        cam, c2w, maps = view
    except (TypeError, ValueError):
        raise ValueError("consistency: %s must be (camera, c2w, maps)" % what) from None
    if not hasattr(maps, "keys"):
        raise ValueError("consistency: the maps of %s must be a dict (what Renderer.render_view returns)" % what)
    return cam, c2w, maps


def view_depth(view, what, key=None):
    """(camera, c2w, contiguous float32 (height, width) depth image) of a view"""
    cam, c2w, maps = _view(view, what)
    d = maps[depth_key(maps, key)]
    if not isinstance(d, torch.Tensor):
        raise ValueError("consistency: the depth image of %s must be a GPU tensor" % what)
    if tuple(d.shape) != (cam.height, cam.width):
        raise ValueError("consistency: the depth image of %s is %s, its camera (%d, %d)" % (what, tuple(d.shape), cam.height, cam.width))
    return cam, c2w, d.float().contiguous()


def reproject(view_a, view_b, tol=DEFAULT_TOL, occlusion=True, pix=None, depth=None):
    """match (height_a, width_a) int32: for every pixel of view A the linear index row * width_b + column of the pixel of
    view B that shows the same surface point, or a negative code: NOTHING (-1: no depth there, or outside the lens),
    LEFT_VIEW (-2), UNKNOWN (-3: B has no depth at the matched pixel), OCCLUDED (-4: B sees something else there).
    occlusion=False skips B's depth test (codes -3 and -4 never occur).  pix: int32 GPU indices of A's pixels -> match (R).
    depth: the maps key of the depth image (default: the finest level present)."""
    cam_a, c2w_a, d_a = view_depth(view_a, "view_a", depth)
    cam_b, c2w_b, d_b = view_depth(view_b, "view_b", depth)
    m = ops.reproject(cam_a, c2w_a, d_a, cam_b, invert_pose(c2w_b), d_b if occlusion else None, pix=pix, tol=tol)["match"]
    return m if pix is not None else m.reshape(cam_a.height, cam_a.width)


def warp(image_b, match, fill=0):
    """Gather an image of view B, (height_b, width_b, ...), into view A's pixel grid: out[a] = image_b[match[a]] where
    match[a] >= 0, `fill` elsewhere.  Plumbing (torch indexing), no kernel of its own."""
    if not isinstance(image_b, torch.Tensor) or image_b.dim() < 2:
        raise ValueError("warp: image_b must be a (height, width, ...) tensor")
    if not isinstance(match, torch.Tensor) or match.dtype not in (torch.int32, torch.int64):
        raise ValueError("warp: match must be the int32 tensor consistency.reproject returned")
    if match.device != image_b.device:
        raise ValueError("warp: image_b is on %s, match on %s" % (image_b.device, match.device))
    flat = image_b.reshape(image_b.shape[0] * image_b.shape[1], *image_b.shape[2:])
    seen = match >= 0
    got = flat[match.clamp(min=0).long()]
    return torch.where(seen.reshape(*match.shape, *([1] * (got.dim() - match.dim()))), got, torch.full_like(got, fill))
