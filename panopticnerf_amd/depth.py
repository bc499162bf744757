"""The depth front end: any depth image -> a view (ops.depth_filter / ops.depth_normals; the rule is written out in include/pnr.h
"depth front end").  The step between the depth producers (stereo.depth_from_pair, pointcloud.splat, Renderer.render_view, a
sensor) and everything that takes a view with normals:

    d = depth.filter(raw, radius=3, min_support=4)               # edge-preserving smoothing; isolated speckles become holes
    view = depth.view(camera, c2w, raw, filter=dict(radius=3))   # (camera, c2w, {"depth", "normal", "code", "valid"})
    c2w_live, info = fusion.track(view, camera, live_depth, guess)

A view is `(camera, c2w, maps)` as fusion.raycast and Renderer.render_view make them, so consistency.reproject, pointcloud.lift and
Evaluator.evaluate_depth take it as it stands, and fusion.track takes it as its MODEL view: a frame can be aligned to another
frame before any volume exists (fusion.odometry).

Conventions (this build's, unpinned): a depth is valid iff it is positive and finite; depth as render_view writes it (z-depth in a
pinhole frame, range in a fisheye / equirect frame); the filter never fills a hole; normals are world-space unit vectors that face
the camera (fusion.raycast's convention), from central differences of the camera-relative points where both neighbours pass the
jump gate and one-sided ones otherwise.  `despeckle` removes whole blobs of wrong depth, which the filter's min_support cannot: the
segments of similar depth (ops.cc_label, the values mode of include/pnr.h "connected components") below a size.  Out of scope: image pyramids, hole filling, a median, normals from a larger stencil or a
plane fit, per-pixel confidence."""
import torch

from . import ops
from .camera import is_camera

OK, NO_DEPTH, NO_NEIGHBOUR, DEGENERATE, GRAZING = (ops.NORMAL_OK, ops.NORMAL_NO_DEPTH, ops.NORMAL_NO_NEIGHBOUR, ops.NORMAL_DEGENERATE,
                                                   ops.NORMAL_GRAZING)
MAX_RADIUS = ops.DEPTH_MAX_RADIUS
_FILTER_ARGS = ("radius", "sigma_space", "sigma_range", "min_support")


def _image(what, depth, camera=None):
    """a depth image the kernels can index flat: a contiguous float32 (height, width) GPU tensor (of the camera's size)"""
    if not isinstance(depth, torch.Tensor):
        raise TypeError("%s: depth must be a GPU tensor, got %s" % (what, type(depth).__name__))
    shape = (int(camera.height), int(camera.width)) if camera is not None else None
    if depth.dtype != torch.float32 or depth.dim() != 2 or (shape is not None and tuple(depth.shape) != shape):
        raise ValueError("%s: depth must be a float32 tensor of shape %s, got %s %s"
                         % (what, shape if shape is not None else "(height, width)", depth.dtype, tuple(depth.shape)))
    if not depth.is_cuda:
        raise RuntimeError("%s: depth is not on the GPU (the HIP path has no CPU fallback)" % what)
    if not depth.is_contiguous():
        raise ValueError("%s: depth must be contiguous (a transposed or strided view is not taken; call .contiguous())" % what)
    return depth


def filter(depth, radius=3, sigma_space=1.5, sigma_range=(0.0, 0.03), min_support=1, support=False):
    """Edge-preserving smoothing of a (height, width) float32 GPU depth image, in ONE launch (ops.depth_filter).  A pixel becomes the
    weighted mean of the valid pixels of its (2 radius + 1)^2 window whose depth lies within sigma = a + b * depth of its own
    (sigma_range = (a, b)): the weight is a spatial Gaussian of sigma_space pixels times the biweight (1 - x^2)^2 of x = difference
    / sigma, so a depth step larger than sigma is not blurred.  A pixel averaged over fewer than min_support pixels (itself
    included) becomes 0: with min_support > 1 isolated speckles turn into holes.  Invalid pixels stay 0.  radius 0 .. MAX_RADIUS.
    Returns the filtered image, with support=True (filtered, support int16: the number of pixels each result was averaged over).
    Nothing is synchronised; the launch can be captured in a graph."""
    what = "depth.filter"
    radius, _, sigma_a, sigma_b, min_support = ops.depth_filter_params(what, radius, sigma_space, sigma_range, min_support)
    _image(what, depth)
    out = torch.empty_like(depth)
    sup = torch.empty(depth.shape, dtype=torch.int16, device=depth.device) if support else None
    ops.depth_filter(depth, out, radius, sigma_space, (sigma_a, sigma_b), min_support, support=sup)
    return (out, sup) if support else out


def despeckle(depth, max_diff, min_size, connectivity=4):
    """The depth image with every segment of fewer than min_size pixels set to 0 (the speckle stage of stereo matchers).  A
    segment is a connected set of valid pixels, 4- or 8-linked, neighbours linked where |difference of depth| <= max_diff; its
    closure, so a slope stays one segment.  Every other pixel is unchanged bit for bit (an invalid one stays what it was).  One
    ops.cc_label and one torch.where; nothing is synchronised, the call can be captured in a graph."""
    what = "depth.despeckle"
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be 4 or 8 (got %r)" % (what, connectivity))
    tol = ops.cc_tol(what, max_diff)
    if isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 0:
        raise ValueError("%s: min_size must be an integer >= 0 (got %r)" % (what, min_size))
    _image(what, depth)
    _, size, _ = ops.cc_label(depth, connectivity == 8, tol)
    return torch.where((size > 0) & (size < min_size), torch.zeros((), dtype=depth.dtype, device=depth.device), depth)


def _pose(what, c2w):
    if isinstance(c2w, torch.Tensor) and c2w.is_cuda:
        raise TypeError("%s: c2w must be host values (the pose is baked into the launch), not a device tensor" % what)
    c2w = torch.as_tensor(c2w, dtype=torch.float32)
    if c2w.numel() not in (12, 16):
        raise ValueError("%s: c2w must be a 3x4 (or 4x4) matrix" % what)
    return c2w.reshape(-1)[:12].reshape(3, 4)


def _normals(what, camera, c2w, depth, jump, min_cos, vertex):
    if not is_camera(camera):
        raise TypeError("%s: camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect, not %r" % (what, camera))
    c2w = _pose(what, c2w)
    jump_a, jump_b, _ = ops.depth_normals_params(what, jump, min_cos)
    _image(what, depth, camera)
    dev, h, w = depth.device, int(camera.height), int(camera.width)
    maps = {"depth": depth, "normal": torch.empty((h, w, 3), dtype=torch.float32, device=dev),
            "code": torch.empty((h, w), dtype=torch.uint8, device=dev)}
    if vertex:
        maps["vertex"] = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    ops.depth_normals(camera.model, camera.params, c2w, w, h, depth, maps["normal"], (jump_a, jump_b), float(min_cos),
                      vertex=maps.get("vertex"), code=maps["code"])
    maps["valid"] = maps["code"] == OK
    return maps


def normals(camera, c2w, depth, jump=(0.0, 0.05), min_cos=0.1, vertex=False):
    """World-space normals (and vertices) of a depth image seen by (camera, c2w), in ONE launch (ops.depth_normals).  camera:
    camera.Pinhole / Fisheye / Equirect; c2w: 3x4 camera-to-world, host values; depth: (height, width) float32 GPU image in
    render_view's convention.  Returns a maps dict of (height, width, ...) images:
        depth   the image given
        normal  float32 (., 3)  the unit normal towards the camera, 0 where there is none
        code    uint8           OK, NO_DEPTH (no valid depth, or outside a fisheye lens), NO_NEIGHBOUR (no neighbour within the jump
                                gate along an image axis), DEGENERATE (the two differences are parallel) or GRAZING (the surface
                                is seen at a cosine below min_cos);  valid  bool = code == OK
        vertex  float32 (., 3)  with vertex=True: the world point, 0 where code is NO_DEPTH
    jump = (a, b): a neighbour is differenced against while |its depth - this depth| <= a + b * depth.  Nothing is synchronised; the
    launch can be captured in a graph, and a replay sees the depth image's current contents."""
    return _normals("depth.normals", camera, c2w, depth, jump, min_cos, vertex)


def _filter_args(what, filter):
    """depth.filter's arguments of a `filter=` dict with the defaults filled in and checked in the caller's name; None stays None"""
    if filter is None:
        return None
    if not hasattr(filter, "keys"):
        raise TypeError("%s: filter must be None or a dict of depth.filter's arguments (%s)" % (what, ", ".join(_FILTER_ARGS)))
    ops._names(what, filter, _FILTER_ARGS, "unknown filter argument %(key)s (known: %(known)s)")
    fa = dict(radius=3, sigma_space=1.5, sigma_range=(0.0, 0.03), min_support=1)
    fa.update(filter)
    ops.depth_filter_params(what, **fa)
    return fa


def view(camera, c2w, depth, filter=None, **normals_args):
    """(camera, c2w, maps): the view of a depth image, accepted as it stands by fusion.track as the MODEL view and by
    consistency.reproject, pointcloud.lift and Evaluator.evaluate_depth.  filter: None, or a dict of depth.filter's arguments
    (radius, sigma_space, sigma_range, min_support) -- maps["depth"] is then the filtered image, which the normals are made of.
    normals_args: jump, min_cos, vertex of depth.normals.  Two launches at most."""
    what = "depth.view"
    ops._names(what, normals_args, ("jump", "min_cos", "vertex"), "unknown argument %(key)s (the arguments of depth.normals: %(known)s)")
    fa = _filter_args(what, filter)
    if not is_camera(camera):
        raise TypeError("%s: camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect, not %r" % (what, camera))
    c2w = _pose(what, c2w)
    ops.depth_normals_params(what, normals_args.get("jump", (0.0, 0.05)), normals_args.get("min_cos", 0.1))
    _image(what, depth, camera)
    if fa is not None:
        out = torch.empty_like(depth)
        ops.depth_filter(depth, out, **fa)
        depth = out
    return camera, c2w, _normals(what, camera, c2w, depth, normals_args.get("jump", (0.0, 0.05)), normals_args.get("min_cos", 0.1),
                                 normals_args.get("vertex", False))
