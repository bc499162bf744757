"""torch-tensor front ends of the C-ABI kernels (include/pnr.h).

PyTorch is used only for device memory and the current HIP stream: every op takes CUDA
(ROCm) float32 / int32 tensors, checks them, and passes raw pointers + sizes through ctypes.
All ops fail loudly off-GPU; nothing here computes on the CPU.
"""
import ctypes
import functools
import math
import os

import torch

from . import _lib
from . import camera as _camera          # camera imports this module at its top: the module, not a name from it
from ._lib import MlpDesc, MlpParamsHost


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _on_device(fn):
    """Run `fn` with the device of its first GPU-tensor argument current, so that `_stream()` is THAT device's current
    stream (a tensor on cuda:1 while cuda:0 is current would otherwise be launched on the wrong device's stream)."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        cand = []
        for a in list(args) + list(kwargs.values()):
            cand.extend(a.values() if isinstance(a, dict) else (a,))
        for a in cand:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index == torch.cuda.current_device():
                    break
                with torch.cuda.device(a.device):
                    return fn(*args, **kwargs)
        return fn(*args, **kwargs)

    return wrapper


def _host_floats(v, n, what):
    vals = [float(x) for x in torch.as_tensor(v, dtype=torch.float32).reshape(-1).tolist()]
    if len(vals) != n:
        raise ValueError(f"{what}: expected {n} values, got {len(vals)}")
    return (ctypes.c_float * n)(*vals)


# The argument checks of the geometry ops.  Each takes the caller's name `what` first and refuses in that name, so an op and the
# wrapper above it (fusion.*, mesh.extract, stereo.sgm) state a rule once; the ops call them in the order their refusals come.
_INF = float("inf")
MAX_PIXELS = 2 ** 31 - 1                        # of any image the ops take
_MODEL_WORDS = {"pinhole": (_lib.CAMERA_PINHOLE, 4), "fisheye": (_lib.CAMERA_FISHEYE, 7), "equirect": (_lib.CAMERA_EQUIRECT, 4)}


def _is_tensor(t, dtype=None, shape=None):
    return isinstance(t, torch.Tensor) and (dtype is None or t.dtype == dtype) and (shape is None or tuple(t.shape) == tuple(shape))


def _gpu(t, name):
    if not _is_tensor(t):
        raise ValueError("%s: expected a GPU tensor, got %s" % (name, type(t).__name__))


def _tensor(what, name, t, must_be="a GPU tensor"):
    """the other spelling of _gpu's test, with room for what the tensor holds"""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be %s, got %s" % (what, name, must_be, type(t).__name__))


def _tensor_table(what, needed, optional=()):
    """rows of (name, tensor, dtype, shape): type, then dtype, then shape of each, on any device; a None among `optional` is absent"""
    for rows, may_be_none in ((needed, False), (optional, True)):
        for name, t, dtype, shape in rows:
            if t is None and may_be_none:
                continue
            _tensor(what, name, t)
            if t.dtype != dtype:
                raise TypeError("%s: %s must be %s, got %s" % (what, name, dtype, t.dtype))
            if tuple(t.shape) != shape:
                raise ValueError("%s: %s must be %s, got %s" % (what, name, shape, tuple(t.shape)))


def _same_device(what, **tensors):
    """device and contiguity of every tensor given (None: absent); all on the first one's device"""
    ref = None
    for name, t in tensors.items():
        if t is None:
            continue
        _chk(t, "%s: %s" % (what, name), t.dtype)
        if ref is None:
            ref = t
        elif t.device != ref.device:
            raise ValueError("%s: %s is on %s, not on %s" % (what, name, t.device, ref.device))


def _on(what, dev, ref_name, **tensors):
    """every tensor given (None: absent) is on `dev`, the device of the argument `ref_name`; for the ops that _chk each tensor"""
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise ValueError("%s: %s is on %s, %s on %s" % (what, name, t.device, ref_name, dev))


def _lattice_shape(what, name, t, min_res, max_points=2 ** 31 - 1, limit="2^31 - 1"):
    """(res_x, res_y, res_z) of the (res_z, res_y, res_x) tensor `t`, the volume of the TSDF ops or the field of the mesh ops"""
    _tensor(what, name, t)
    if t.dim() != 3 or min(t.shape) < min_res:
        raise ValueError("%s: %s must be (res_z, res_y, res_x) with every res >= %d, got %s" % (what, name, min_res, tuple(t.shape)))
    if t.numel() > max_points:
        raise ValueError("%s: %s holds %d points, more than the limit of %s" % (what, name, t.numel(), limit))
    rz, ry, rx = t.shape
    return rx, ry, rz


def _lattice_floats(what, lo, step, nonzero_step=True):
    """the lattice's origin and step per axis as host floats"""
    lo_h, step_h = _host_floats(lo, 3, what + ": lo"), _host_floats(step, 3, what + ": step")
    for name, h in (("lo", lo_h), ("step", step_h)):
        if not all(abs(v) < _INF for v in h):
            raise ValueError("%s: %s must be finite (got %r)" % (what, name, list(h)))
    if nonzero_step and not all(v != 0.0 for v in step_h):
        raise ValueError("%s: step must be non-zero (got %r)" % (what, list(step_h)))
    return lo_h, step_h


def _model_word(what, name, model):
    """(model word, number of camera floats) of the model name given as argument `name`"""
    if model not in _MODEL_WORDS:
        raise ValueError("%s: %s must be 'pinhole', 'fisheye' or 'equirect', not %r" % (what, name, model))
    return _MODEL_WORDS[model]


def _camera_model(what, name, model, cam, cam_name="cam"):
    """(model word, host floats) of a camera given as a model name (argument `name`) and its floats (argument `cam_name`)"""
    word, n = _model_word(what, name, model)
    return word, _host_floats(cam, n, "%s: model %r %s" % (what, model, cam_name))


def _image_size(what, width, height, of="image"):
    width, height = int(width), int(height)
    if width < 1 or height < 1 or width * height > MAX_PIXELS:
        raise ValueError("%s: bad %s %d x %d (width, height >= 1, at most 2^31 - 1 pixels)" % (what, of, width, height))
    return width, height


def _d_range(what, d_range, may_be_inf):
    try:
        d_min, d_max = (float(v) for v in d_range)
    except (TypeError, ValueError):
        raise ValueError("%s: d_range must be (d_min, d_max)" % what) from None
    if not (0.0 < d_min <= d_max) or (d_max == _INF and not may_be_inf):
        raise ValueError("%s: d_range must satisfy 0 < d_min <= d_max%s" % (what, " (d_max may be inf)" if may_be_inf else ", both finite"))
    return d_min, d_max


def _names(what, keys, known, refusal):
    """every key is one of `known`, or the refusal: a template of %(key)s and %(known)s"""
    for k in keys:
        if k not in known:
            raise ValueError("%s: %s" % (what, refusal % {"key": repr(k), "known": ", ".join(known)}))


def _gen_rays(name, cam_h, c2w_h, width, height, near, far, pix, device, want_valid=None, ask_first=False):
    """The body of the three gen_rays*: entry point pnr_<name>.  want_valid: None where the entry point takes no `valid` buffer.
    Returns rays (R,8) and valid (R) uint8 or None."""
    pix = _chk(pix, "pix", torch.int32)
    dev = pix.device if pix is not None else torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError(f"{name}: expected a GPU device (the HIP path has no CPU fallback)")
    R = pix.numel() if pix is not None else int(width) * int(height)
    fn, head = getattr(_lib.load(), "pnr_" + name), (cam_h, c2w_h, int(width), int(height), float(near), float(far))
    if ask_first:       # every refusal of the entry point comes before its first use of the device: asked first, with no memory allocated
        _lib.check(fn(*head, None, 0, None, *(() if want_valid is None else (None,)), None), "pnr_" + name)
    rays = torch.empty((R, 8), device=dev, dtype=torch.float32)
    valid = torch.empty((R,), device=dev, dtype=torch.uint8) if want_valid else None
    with torch.cuda.device(dev):
        _lib.check(fn(*head, _p(pix), R, _p(rays), *(() if want_valid is None else (_p(valid),)), _stream()), "pnr_" + name)
    return rays, valid


def gen_rays(intr, c2w, width, height, near, far, pix=None, device=None):
    """Pinhole ray generation on the GPU (pnr_gen_rays).  intr: fx, fy, cx, cy; c2w: 3x4 camera-to-world
    (host values); pix: int32 GPU tensor of linear pixel indices or None (whole frame).  Returns rays (R,8).  d is NOT normalised
    (z_cam = 1), so depth_* of a render on these rays is z-depth; gen_rays_fisheye's rays are unit length and its depth is range."""
    intr_h = (ctypes.c_float * 4)(*[float(v) for v in torch.as_tensor(intr, dtype=torch.float32).reshape(4).tolist()])
    c2w_h = (ctypes.c_float * 12)(*[float(v) for v in torch.as_tensor(c2w, dtype=torch.float32).reshape(12).tolist()])
    return _gen_rays("gen_rays", intr_h, c2w_h, width, height, near, far, pix, device)[0]


def gen_rays_fisheye(cam, c2w, width, height, near, far, pix=None, device=None, want_valid=True):
    """Fisheye ray generation on the GPU (pnr_gen_rays_fisheye; the model is in include/pnr.h "cameras").  cam: xi, k1, k2,
    gamma1, gamma2, u0, v0; c2w, pix, device as gen_rays.  Returns rays (R,8) and valid (R) uint8 (None with
    want_valid=False).  Unlike gen_rays' directions (z_cam = 1: depth along them is z-depth) these are UNIT LENGTH, so
    depth_* of a render on them is range along the ray.  A pixel outside the lens gets o, d = 0, near = far = 0, valid = 0."""
    cam_h, c2w_h = _host_floats(cam, 7, "gen_rays_fisheye: cam"), _host_floats(c2w, 12, "gen_rays_fisheye: c2w")
    return _gen_rays("gen_rays_fisheye", cam_h, c2w_h, width, height, near, far, pix, device, want_valid=bool(want_valid))


def gen_rays_equirect(cam, c2w, width, height, near, far, pix=None, device=None):
    """Panoramic ray generation on the GPU (pnr_gen_rays_equirect; the model is in include/pnr.h "cameras").  cam: lon0, dlon,
    lat0, dlat in half-turns (camera.Equirect makes them from degrees); c2w, pix, device as gen_rays.  Returns rays (R,8):
    UNIT-LENGTH directions like gen_rays_fisheye's (depth_* of a render on them is range), every pixel valid."""
    cam_h, c2w_h = _host_floats(cam, 4, "gen_rays_equirect: cam"), _host_floats(c2w, 12, "gen_rays_equirect: c2w")
    return _gen_rays("gen_rays_equirect", cam_h, c2w_h, width, height, near, far, pix, device, ask_first=True)[0]


@_on_device
def project_points(model, cam, w2c, width, height, points):
    """World points (P,3) -> uv (P,2) pixel coordinates, range (P) = distance from the camera centre, valid (P) uint8 = inside
    the projection's domain and inside the image (pnr_project_points).  model: "pinhole" (cam: fx, fy, cx, cy), "fisheye"
    (cam: xi, k1, k2, gamma1, gamma2, u0, v0) or "equirect" (cam: lon0, dlon, lat0, dlat in half-turns; u wraps round a full
    circle); w2c: 3x4 world-to-camera (host values)."""
    word, cam_h = _camera_model("project_points", "model", model, cam)
    w2c_h = _host_floats(w2c, 12, "project_points: w2c")
    points = _chk(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("project_points: points must be (P, 3)")
    P, dev = points.shape[0], points.device
    uv = torch.empty((P, 2), device=dev, dtype=torch.float32)
    rng = torch.empty((P,), device=dev, dtype=torch.float32)
    valid = torch.empty((P,), device=dev, dtype=torch.uint8)
    _lib.check(_lib.load().pnr_project_points(word, cam_h, w2c_h, int(width), int(height), _p(points), P, _p(uv), _p(rng), _p(valid),
                                              _stream()), "pnr_project_points")
    return uv, rng, valid


def _camera_words(cam, what):
    """(model word, host floats, width, height) of a camera.Pinhole / camera.Fisheye / camera.Equirect"""
    if not _camera.is_camera(cam):
        raise ValueError("%s: expected a camera.Pinhole or camera.Fisheye (or camera.Equirect), not %r" % (what, cam))
    return cam.word, _host_floats(cam.params, len(cam.params), what), int(cam.width), int(cam.height)


def _image(t, width, height, name):
    """a (height, width) or (height * width) map of a camera, flattened; None stays None"""
    if t is None:
        return None
    if not _is_tensor(t) or tuple(t.shape) not in ((height, width), (height * width,)):
        raise ValueError("%s: expected a (%d, %d) image (or its %d flattened pixels), got %s"
                         % (name, height, width, height * width, tuple(t.shape) if _is_tensor(t) else type(t).__name__))
    return t.reshape(-1) if t.is_contiguous() else t


REPROJECT_OUTPUTS = ("match", "uv", "agree", "stats")


@_on_device
def reproject(src, c2w_src, depth_src, tgt, w2c_tgt, depth_tgt=None, pix=None, tol=(0.0, 0.02), label_src=None, label_tgt=None,
              n_classes=0, agree=None, stats=None, want=("match",), out=None):
    """Cross-view reprojection (pnr_reproject; the rule is in include/pnr.h "cross-view reprojection"): every pixel of the
    source view -- or the int32 GPU pixel indices `pix` -- is lifted with depth_src (a (height, width) image of the source
    camera), projected into the target view and matched to the nearest target pixel; with depth_tgt the match is tested
    against the target's depth, |e - depth_tgt[q]| <= tol[0] + tol[1] * e.  src, tgt: camera.Pinhole / Fisheye / Equirect;
    c2w_src, w2c_tgt: 3x4 host values (camera.invert_pose makes the second from a c2w).  The default tolerance (0, 0.02) is
    this build's choice, not a pinned convention.

    Returns a dict of what `want` names plus every accumulator that was passed:
      match (R) int32: the target pixel q = row * width + column, or -1 nothing to reproject, -2 leaves the view, -3 target
          depth unknown, -4 occluded;   uv (R, 2) float32: where the point lands (0 outside the projection's domain);
      agree (n_classes, n_classes) int64: agree[label_src[p], label_tgt[q]] += 1 over visible pixels with both labels in
          [0, n_classes) (label images on both sides required);   stats (5) int64: pixels matched / -1 / -2 / -3 / -4.
    agree / stats: accumulated into when given, fresh zeroed tensors when only named in `want`.  out: {"match": ..., "uv": ...}
    caller-owned tensors to write into."""
    ms, cam_s, ws, hs = _camera_words(src, "reproject: src")
    mt, cam_t, wt, ht = _camera_words(tgt, "reproject: tgt")
    c2w_h, w2c_h = _host_floats(c2w_src, 12, "reproject: c2w_src"), _host_floats(w2c_tgt, 12, "reproject: w2c_tgt")
    want = tuple(want)
    _names("reproject", want, REPROJECT_OUTPUTS, "unknown output %(key)s (one of %(known)s)")
    if depth_src is None:
        raise ValueError("reproject: depth_src is required")
    if (label_src is None) != (label_tgt is None):
        raise ValueError("reproject: label_src and label_tgt come together")
    tol_abs, tol_rel = (float(v) for v in tol)
    if not (0.0 <= tol_abs < _INF and 0.0 <= tol_rel < _INF):
        raise ValueError("reproject: tol = (absolute, relative) must be finite and >= 0")
    n_classes = int(n_classes)
    if (agree is not None or "agree" in want) and label_src is None:
        raise ValueError("reproject: agree needs label_src and label_tgt")
    if label_src is not None and not 1 <= n_classes <= 8192:
        raise ValueError("reproject: n_classes must be in 1 .. 8192 with label images (got %d)" % n_classes)
    if pix is not None and pix.dim() != 1:
        raise ValueError("reproject: pix must be a 1-D tensor of linear pixel indices")
    # shapes first, then dtype / device / contiguity of each
    depth_src, depth_tgt = _image(depth_src, ws, hs, "reproject: depth_src"), _image(depth_tgt, wt, ht, "reproject: depth_tgt")
    label_src, label_tgt = _image(label_src, ws, hs, "reproject: label_src"), _image(label_tgt, wt, ht, "reproject: label_tgt")
    depth_src, depth_tgt = _chk(depth_src, "reproject: depth_src"), _chk(depth_tgt, "reproject: depth_tgt")
    label_src, label_tgt = _chk(label_src, "reproject: label_src", torch.int32), _chk(label_tgt, "reproject: label_tgt", torch.int32)
    dev = depth_src.device
    pix = _chk(pix, "reproject: pix", torch.int32)
    R = pix.numel() if pix is not None else ws * hs
    if agree is None and "agree" in want:
        agree = torch.zeros((n_classes, n_classes), device=dev, dtype=torch.int64)
    if stats is None and "stats" in want:
        stats = torch.zeros((5,), device=dev, dtype=torch.int64)
    if _chk(agree, "reproject: agree", torch.int64) is not None and tuple(agree.shape) != (n_classes, n_classes):
        raise ValueError("reproject: agree must be (n_classes, n_classes) = (%d, %d)" % (n_classes, n_classes))
    if _chk(stats, "reproject: stats", torch.int64) is not None and tuple(stats.shape) != (5,):
        raise ValueError("reproject: stats must be (5,)")
    out = out or {}
    _names("reproject", out, ("match", "uv"), "out holds %(key)s (only 'match' and 'uv' can be caller-owned)")
    match = _own(out.get("match"), (R,), torch.int32, dev, "reproject: match") if "match" in want or "match" in out else None
    uv = _own(out.get("uv"), (R, 2), torch.float32, dev, "reproject: uv") if "uv" in want or "uv" in out else None
    _on("reproject", dev, "depth_src", depth_tgt=depth_tgt, label_src=label_src, label_tgt=label_tgt, pix=pix, agree=agree, stats=stats)
    _lib.check(_lib.load().pnr_reproject(ms, cam_s, c2w_h, ws, hs, _p(pix), R, _p(depth_src), mt, cam_t, w2c_h, wt, ht, _p(depth_tgt),
                                         tol_abs, tol_rel, _p(label_src), _p(label_tgt), n_classes if label_src is not None else 0,
                                         _p(match), _p(uv), _p(agree), _p(stats), _stream()), "pnr_reproject")
    ret = {"match": match, "uv": uv, "agree": agree, "stats": stats}
    return {k: v for k, v in ret.items() if v is not None}


@_on_device
def splat_points(camera, w2c, points, zbuf=None, index_base=0, near=0.0, far=float("inf"), radius=0, stats=None):
    """Scatter world points (P, 3) into a view through a z-buffer (pnr_splat_points; the rule is in include/pnr.h "point
    splatting").  camera: camera.Pinhole / Fisheye / Equirect; w2c: 3x4 world-to-camera host values (camera.invert_pose).
    Returns zbuf (height, width) int64: per pixel the packed key (depth bits << 32 | point index) of the nearest point that
    covers it, -1 where none does -- a fresh buffer filled with -1 when `zbuf` is None, else `zbuf` itself, accumulated into
    (several scans or chunks: give each a distinct index_base range; the result does not depend on their order).  Depth is
    z-depth in a pinhole view and range in a fisheye / equirect view; points outside [near, far] are clipped; radius 0, 1 or 2
    is the half width of the square footprint (clipped at the border, never wrapped).  stats: (3) int64, accumulated:
    points landed / left the view / clipped.  splat_resolve unpacks the buffer."""
    model, cam_h, width, height = _camera_words(camera, "splat_points: camera")
    w2c_h = _host_floats(w2c, 12, "splat_points: w2c")
    _gpu(points, "splat_points: points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("splat_points: points must be (P, 3)")
    radius, index_base = int(radius), int(index_base)
    if radius not in (0, 1, 2):
        raise ValueError("splat_points: radius must be 0, 1 or 2 (got %d)" % radius)
    near, far = float(near), float(far)
    if not (0.0 <= near <= far):
        raise ValueError("splat_points: near and far must satisfy 0 <= near <= far (far may be inf)")
    P = points.shape[0]
    if index_base < 0 or index_base + P > 2 ** 31 - 1:
        raise ValueError("splat_points: index_base + the number of points must stay within 0 .. 2^31 - 1")
    if zbuf is not None and not _is_tensor(zbuf, shape=(height, width)):
        raise ValueError("splat_points: zbuf must be a (%d, %d) int64 tensor" % (height, width))
    if stats is not None and not _is_tensor(stats, shape=(3,)):
        raise ValueError("splat_points: stats must be (3,)")
    points = _chk(points, "splat_points: points")
    dev = points.device
    zbuf, stats = _chk(zbuf, "splat_points: zbuf", torch.int64), _chk(stats, "splat_points: stats", torch.int64)
    _on("splat_points", dev, "points", zbuf=zbuf, stats=stats)
    zbuf = torch.full((height, width), -1, device=dev, dtype=torch.int64) if zbuf is None else zbuf
    _lib.check(_lib.load().pnr_splat_points(model, cam_h, w2c_h, width, height, _p(points), P, index_base, near, far, radius,
                                            _p(zbuf), _p(stats), _stream()), "pnr_splat_points")
    return zbuf


@_on_device
def splat_resolve(zbuf, want=("depth", "index"), out=None):
    """(depth, index) images of a z-buffer splat_points made (pnr_splat_resolve): depth float32 in the view's convention,
    0 where no point landed (the "unknown" depth ops.reproject reads); index int32 = the winning point's index_base + i, -1
    where none.  want: which of the two to make (the other is None); out: {"depth": ..., "index": ...} caller-owned tensors."""
    _gpu(zbuf, "splat_resolve: zbuf")
    want, out = tuple(want), out or {}
    _names("splat_resolve", want, ("depth", "index"), "unknown output %(key)s (%(known)s)")
    _names("splat_resolve", out, ("depth", "index"), "out holds %(key)s (only 'depth' and 'index')")
    zbuf = _chk(zbuf, "splat_resolve: zbuf", torch.int64)
    dev, shape = zbuf.device, tuple(zbuf.shape)
    depth = _own(out.get("depth"), shape, torch.float32, dev, "splat_resolve: depth") if "depth" in want or "depth" in out else None
    index = _own(out.get("index"), shape, torch.int32, dev, "splat_resolve: index") if "index" in want or "index" in out else None
    _lib.check(_lib.load().pnr_splat_resolve(_p(zbuf), zbuf.numel(), _p(depth), _p(index), _stream()), "pnr_splat_resolve")
    return depth, index


DEPTH_RANGE = (1e-3, 80.0)          # default ground-truth range of depth_metrics: this build's, unpinned


@_on_device
def depth_metrics(pred, gt, mask=None, d_range=DEPTH_RANGE, sums=None, counts=None):
    """Depth-error terms of a predicted depth image against a ground truth of the same shape (pnr_depth_metrics; the rule is
    in include/pnr.h "point splatting").  A pixel counts where mask (bool / uint8, optional) is set and gt is finite and inside
    d_range = (d_min, d_max).  Returns (sums (5) float64, counts (5) int64), accumulated into when given:
      counts: compared pixels, ratio < 1.25, < 1.25^2, < 1.25^3 (ratio = max(pred/gt, gt/pred), strict), missing predictions
      sums:   |d|, d^2, |d|/gt, d^2/gt, (log pred - log gt)^2 with d = pred - gt, over the compared pixels.
    Deterministic: no floating atomics."""
    _gpu(pred, "depth_metrics: pred")
    _gpu(gt, "depth_metrics: gt")
    if pred.shape != gt.shape:
        raise ValueError("depth_metrics: pred is %s, gt %s" % (tuple(pred.shape), tuple(gt.shape)))
    if mask is not None and not _is_tensor(mask, shape=gt.shape):
        raise ValueError("depth_metrics: mask must have gt's shape %s" % (tuple(gt.shape),))
    d_min, d_max = _d_range("depth_metrics", d_range, may_be_inf=False)
    for name, t in (("sums", sums), ("counts", counts)):
        if t is not None and not _is_tensor(t, shape=(5,)):
            raise ValueError("depth_metrics: %s must be (5,)" % name)
    pred, gt = _chk(pred, "depth_metrics: pred"), _chk(gt, "depth_metrics: gt")
    dev = gt.device
    if mask is not None and mask.dtype == torch.bool and mask.is_cuda and mask.is_contiguous():
        mask = mask.view(torch.uint8)
    mask = _chk(mask, "depth_metrics: mask (bool or uint8)", torch.uint8)
    sums, counts = _chk(sums, "depth_metrics: sums", torch.float64), _chk(counts, "depth_metrics: counts", torch.int64)
    _on("depth_metrics", dev, "gt", pred=pred, mask=mask, sums=sums, counts=counts)
    sums = torch.zeros((5,), device=dev, dtype=torch.float64) if sums is None else sums
    counts = torch.zeros((5,), device=dev, dtype=torch.int64) if counts is None else counts
    n = gt.numel()
    ws = torch.empty((_size_or_raise(_lib.load().pnr_depth_metrics_workspace_bytes(n), "pnr_depth_metrics_workspace_bytes") // 8,),
                     device=dev, dtype=torch.float64)
    _lib.check(_lib.load().pnr_depth_metrics(_p(pred), _p(gt), _p(mask), n, d_min, d_max, _p(sums), _p(counts), _p(ws), _stream()),
               "pnr_depth_metrics")
    return sums, counts


def _stereo_arg(t, name, dtype, shape=None, ndim=None, optional=False):
    """A tensor argument of the stereo ops (None: an absent `optional` one): type, dtype and shape, refused by name on any device.
    Not _tensor_table's rows: the messages say "expected", and there are ndim and empty."""
    if t is None and optional:
        return None
    _gpu(t, name)
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s: expected %d dimensions, got shape %s" % (name, ndim, tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if t.numel() == 0:
        raise ValueError("%s: empty tensor" % name)
    return t


def _stereo_disp(what, max_disp):
    max_disp = int(max_disp)
    if max_disp < 16 or max_disp > 256 or max_disp % 16:
        raise ValueError("%s: max_disp must be a multiple of 16 in 16 .. 256 (got %d)" % (what, max_disp))
    return max_disp


def sgm_aggregate_params(what, max_disp, p1, p2, paths):
    """the parameters of pnr_sgm_aggregate as integers, or the refusal by name (`what`: the caller's name)"""
    max_disp = _stereo_disp(what, max_disp)
    p1, p2, paths = int(p1), int(p2), int(paths)
    if not (0 < p1 <= p2 <= 192):
        raise ValueError("%s: p1 and p2 must satisfy 0 < p1 <= p2 <= 192 (got %d, %d)" % (what, p1, p2))
    if paths not in (4, 8):
        raise ValueError("%s: paths must be 4 or 8 (got %d)" % (what, paths))
    return max_disp, p1, p2, paths


def sgm_select_params(what, uniqueness, lr_tol):
    """the parameters of pnr_sgm_select as integers, or the refusal by name"""
    uniqueness, lr_tol = int(uniqueness), int(lr_tol)
    if not (0 <= uniqueness <= 99):
        raise ValueError("%s: uniqueness must lie in 0 .. 99 (got %d)" % (what, uniqueness))
    if lr_tol < -1:
        raise ValueError("%s: lr_tol must be >= 0, or -1 for no left-right check (got %d)" % (what, lr_tol))
    return uniqueness, lr_tol


@_on_device
def census(img, out=None):
    """Census words of an (H, W) uint8 image (pnr_census; include/pnr.h "stereo matching" step 1): (H, W) int64, the 62
    comparisons of the 9 x 7 window with a replicated border."""
    img = _stereo_arg(img, "census: img", torch.uint8, ndim=2)
    out = _stereo_arg(out, "census: out", torch.int64, shape=img.shape, optional=True)
    _same_device("census", img=img, out=out)
    out = torch.empty(tuple(img.shape), device=img.device, dtype=torch.int64) if out is None else out
    H, W = img.shape
    _lib.check(_lib.load().pnr_census(_p(img), W, H, _p(out), _stream()), "pnr_census")
    return out


@_on_device
def sgm_aggregate(census_l, census_r, max_disp=128, p1=10, p2=120, paths=8, out=None):
    """The summed path-cost volume S (H, W, max_disp) of two census images (pnr_sgm_aggregate; the rule's steps 2 and 3): the
    header's uint16 volume held as an int16 tensor (a sum is at most 2040).  out: a caller-owned volume (it need not be
    zeroed)."""
    census_l = _stereo_arg(census_l, "sgm_aggregate: census_l", torch.int64, ndim=2)
    census_r = _stereo_arg(census_r, "sgm_aggregate: census_r", torch.int64, shape=census_l.shape)
    max_disp, p1, p2, paths = sgm_aggregate_params("sgm_aggregate", max_disp, p1, p2, paths)
    H, W = census_l.shape
    out = _stereo_arg(out, "sgm_aggregate: out", torch.int16, shape=(H, W, max_disp), optional=True)
    _same_device("sgm_aggregate", census_l=census_l, census_r=census_r, out=out)
    lib = _lib.load()
    out = torch.empty((H, W, max_disp), device=census_l.device, dtype=torch.int16) if out is None else out
    nbytes = _size_or_raise(lib.pnr_sgm_workspace_bytes(W, H, max_disp, paths), "pnr_sgm_workspace_bytes")
    ws = torch.empty((nbytes,), device=census_l.device, dtype=torch.uint8) if nbytes else None
    _lib.check(lib.pnr_sgm_aggregate(_p(census_l), _p(census_r), W, H, max_disp, p1, p2, paths, _p(out), _p(ws), _stream()),
               "pnr_sgm_aggregate")
    return out


@_on_device
def sgm_select(S, uniqueness=5, lr_tol=1, out=None, disp_right=None):
    """(d16, disp_right) of a volume sgm_aggregate made (pnr_sgm_select; the rule's steps 4 and 5).  d16 (H, W) int16:
    the disparity in sixteenths of a pixel, or -1 (no right pixel), -2 (not unique), -3 (left-right check).  disp_right
    (H, W) int16: the right image's disparity; None with lr_tol = -1 (no left-right check) unless a tensor is given."""
    S = _stereo_arg(S, "sgm_select: S", torch.int16, ndim=3)
    H, W, D = S.shape
    _stereo_disp("sgm_select (the last dimension of S)", D)
    uniqueness, lr_tol = sgm_select_params("sgm_select", uniqueness, lr_tol)
    out = _stereo_arg(out, "sgm_select: out", torch.int16, shape=(H, W), optional=True)
    disp_right = _stereo_arg(disp_right, "sgm_select: disp_right", torch.int16, shape=(H, W), optional=True)
    _same_device("sgm_select", S=S, out=out, disp_right=disp_right)
    out = torch.empty((H, W), device=S.device, dtype=torch.int16) if out is None else out
    if disp_right is None and lr_tol >= 0:
        disp_right = torch.empty((H, W), device=S.device, dtype=torch.int16)
    _lib.check(_lib.load().pnr_sgm_select(_p(S), W, H, D, uniqueness, lr_tol, _p(out), _p(disp_right), _stream()), "pnr_sgm_select")
    return out, disp_right


@_on_device
def disparity_depth(d16, fb, d_range=(1e-3, float("inf")), out=None):
    """depth = fb / (d16 / 16) in float32 (pnr_disparity_depth; the rule's step 6): 0 where d16 <= 0 or the quotient is
    outside d_range = (d_min, d_max).  fb = fx * baseline, a float32 value."""
    d16 = _stereo_arg(d16, "disparity_depth: d16", torch.int16)
    fb = float(fb)
    if not (0.0 < fb < _INF):
        raise ValueError("disparity_depth: fb = fx * baseline must be positive and finite (got %r)" % fb)
    d_min, d_max = _d_range("disparity_depth", d_range, may_be_inf=True)
    out = _stereo_arg(out, "disparity_depth: out", torch.float32, shape=d16.shape, optional=True)
    _same_device("disparity_depth", d16=d16, out=out)
    out = torch.empty(tuple(d16.shape), device=d16.device, dtype=torch.float32) if out is None else out
    _lib.check(_lib.load().pnr_disparity_depth(_p(d16), d16.numel(), fb, d_min, d_max, _p(out), _stream()), "pnr_disparity_depth")
    return out


MESH_MAX_POINTS = (2 ** 31 - 1) // 12          # include/pnr.h "mesh extraction", LIMITS


def _mesh_field(what, field, level):
    """the lattice argument of the mesh ops: (res_x, res_y, res_z, level) or the refusal by name, on any device"""
    _tensor(what, "field", field)
    if field.dtype != torch.float32:            # a ValueError that says "float32": not _tensor_table's TypeError
        raise ValueError("%s: field must be float32, got %s" % (what, field.dtype))
    rx, ry, rz = _lattice_shape(what, "field", field, 1, MESH_MAX_POINTS, "%d ((2^31 - 1) / 12)" % MESH_MAX_POINTS)
    level = float(level)
    if not (abs(level) < _INF):
        raise ValueError("%s: level must be finite (got %r)" % (what, level))
    return rx, ry, rz, level


def mesh_workspace_bytes(res_x, res_y, res_z):
    """pnr_mesh_workspace_bytes: host arithmetic only; a lattice the entry points refuse raises"""
    return _size_or_raise(_lib.load().pnr_mesh_workspace_bytes(int(res_x), int(res_y), int(res_z)), "pnr_mesh_workspace_bytes")


@_on_device
def mesh_count(field, level, workspace=None, totals=None):
    """Classify the lattice `field` (res_z, res_y, res_x) float32 against `level` and scan the counts (pnr_mesh_count; the rule
    is in include/pnr.h "mesh extraction").  Returns (totals, workspace): totals (2) int64 ON THE DEVICE = (vertices, triangles)
    -- reading it is the caller's synchronisation --, workspace the uint8 buffer mesh_emit needs.  Both may be caller-owned."""
    rx, ry, rz, level = _mesh_field("mesh_count", field, level)
    nbytes = mesh_workspace_bytes(rx, ry, rz)
    if workspace is not None and (not _is_tensor(workspace, torch.uint8) or workspace.numel() < nbytes):
        raise ValueError("mesh_count: workspace must be a uint8 tensor of at least %d bytes" % nbytes)
    if totals is not None and not _is_tensor(totals, torch.int64, (2,)):
        raise ValueError("mesh_count: totals must be a (2,) int64 tensor")
    _same_device("mesh_count", field=field, workspace=workspace, totals=totals)
    workspace = torch.empty((nbytes,), device=field.device, dtype=torch.uint8) if workspace is None else workspace
    totals = torch.empty((2,), device=field.device, dtype=torch.int64) if totals is None else totals
    _lib.check(_lib.load().pnr_mesh_count(_p(field), rx, ry, rz, level, _p(workspace), _p(totals), _stream()), "pnr_mesh_count")
    return totals, workspace


@_on_device
def mesh_emit(field, level, lo, step, workspace, vertices, faces, src=None):
    """Write the mesh mesh_count counted (pnr_mesh_emit): vertices (V, 3) float32, faces (T, 3) int32, src (V,) int64 or None,
    caller-owned and sized by mesh_count's totals.  lo, step: the lattice's float32 origin and step per axis (x, y, z), host
    values.  field, level and workspace are mesh_count's."""
    rx, ry, rz, level = _mesh_field("mesh_emit", field, level)
    lo_h, step_h = _lattice_floats("mesh_emit", lo, step, nonzero_step=False)
    nbytes = mesh_workspace_bytes(rx, ry, rz)
    if not _is_tensor(workspace, torch.uint8) or workspace.numel() < nbytes:
        raise ValueError("mesh_emit: workspace must be the uint8 tensor of at least %d bytes that mesh_count filled" % nbytes)
    # one message for type, dtype and shape, and n is free: not _tensor_table's rows
    for name, t, dtype, cols in (("vertices", vertices, torch.float32, 3), ("faces", faces, torch.int32, 3), ("src", src, torch.int64, 0)):
        if t is None and name == "src":
            continue
        if not _is_tensor(t, dtype) or t.dim() != (2 if cols else 1) or (cols and t.shape[1] != cols):
            raise ValueError("mesh_emit: %s must be a %s %s tensor" % (name, "(n, 3)" if cols else "(n,)", dtype))
    if src is not None and src.shape[0] != vertices.shape[0]:
        raise ValueError("mesh_emit: src holds %d rows, vertices %d" % (src.shape[0], vertices.shape[0]))
    _same_device("mesh_emit", field=field, workspace=workspace, vertices=vertices, faces=faces, src=src)
    _lib.check(_lib.load().pnr_mesh_emit(_p(field), rx, ry, rz, level, lo_h, step_h, _p(workspace),
                                         _p(vertices if vertices.numel() else None), _p(faces if faces.numel() else None),
                                         _p(src if src is not None and src.numel() else None), _stream()), "pnr_mesh_emit")
    return vertices, faces, src


NN_MAX_POINTS = 2 ** 31 - 1                     # include/pnr.h "nearest neighbours": n, m and the number of sampled points
NN_MAX_TABLE_BITS = 28                          # PNR_NN_MAX_TABLE = 2^28 buckets
CLOUD_MAX_TAU = _lib.CLOUD_MAX_TAU
CLOUD_COUNTS = 2 + CLOUD_MAX_TAU                # counted, missing, then one per threshold
_NN_PAD = 1.0009765625                          # PNR_NN_PAD


def _f32(v):
    """the float32 nearest to the Python number v, as a Python float (what ctypes.c_float passes)"""
    return ctypes.c_float(v).value


def nn_params(what, max_dist, n, table_bits=None):
    """(max_dist, table_size) of an index over n reference points, or the refusal by name: max_dist positive and finite as a
    float32, with a cell size 2 max_dist that does not overflow and whose inverse does not either (max_dist above about 1.5e-39); table_bits None for the default table of max(1024, the power of
    two at or above 2 n) buckets, or 1 .. 28 for 2^table_bits buckets"""
    try:
        d = _f32(float(max_dist))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: max_dist must be a positive finite number (got %r)" % (what, max_dist)) from None
    h = _f32(_f32(d * _NN_PAD) * 2.0) if 0.0 < d < _INF else 0.0
    if not (0.0 < h < _INF) or not (_f32(1.0 / h) < _INF):
        raise ValueError("%s: max_dist must be positive and finite, with 2 max_dist and 1 / (2 max_dist) finite in float32 (got %r)" % (what, max_dist))
    n = int(n)
    if n < 0 or n > NN_MAX_POINTS:
        raise ValueError("%s: the cloud holds %d points, outside 0 .. 2^31 - 1" % (what, n))
    if table_bits is None:
        table_bits = min(max(10, (2 * n - 1).bit_length() if n else 0), NN_MAX_TABLE_BITS)
    elif isinstance(table_bits, bool) or not isinstance(table_bits, int) or not (1 <= table_bits <= NN_MAX_TABLE_BITS):
        raise ValueError("%s: table_bits must be an integer in 1 .. %d (got %r)" % (what, NN_MAX_TABLE_BITS, table_bits))
    return d, 1 << table_bits


def nn_cloud(what, name, t):
    """rows of the point cloud `t`, a float32 (n, 3) tensor on any device, or the refusal by name: the public check the wrappers reuse"""
    return _cloud(what, name, t)


def _cloud(what, name, t, dtype=torch.float32, cols=3):
    """the (rows, cols) tensor `t` of `dtype` on any device, cols = 0 for (rows,): type, dtype, shape; returns rows"""
    _tensor(what, name, t)
    if t.dtype != dtype:
        raise TypeError("%s: %s must be %s, got %s" % (what, name, dtype, t.dtype))
    if t.dim() != (2 if cols else 1) or (cols and t.shape[1] != cols):
        raise ValueError("%s: %s must be %s, got %s" % (what, name, "(n, %d)" % cols if cols else "(n,)", tuple(t.shape)))
    if t.shape[0] > NN_MAX_POINTS:
        raise ValueError("%s: %s holds %d rows, more than 2^31 - 1" % (what, name, t.shape[0]))
    return t.shape[0]


def _nn_table(what, start, records, n):
    """table_size of the (start, records) pair of an index over n points: type, dtype, shape"""
    _tensor(what, "start", start)
    if start.dtype != torch.int32:
        raise TypeError("%s: start must be torch.int32, got %s" % (what, start.dtype))
    T = start.numel() - 1
    if start.dim() != 1 or T < 2 or T & (T - 1) or T > 1 << NN_MAX_TABLE_BITS:
        raise ValueError("%s: start must be (table_size + 1,) with table_size a power of two in 2 .. 2^28, got %s" % (what, tuple(start.shape)))
    _tensor_table(what, [("records", records, torch.float32, (n, 4))])
    return T


@_on_device
def nn_build(ref, max_dist, table_bits=None, start=None, records=None):
    """Build the spatial-hash index of the reference cloud ref (n, 3) float32 for radius max_dist (pnr_nn_build; the rule is in
    include/pnr.h "nearest neighbours").  Returns (start (table_size + 1,) int32, records (n, 4) float32): per bucket the range
    of its records, and the records (x, y, z, bits = index) in bucket order.  Both may be caller-owned.  Never synchronises."""
    n = _cloud("nn_build", "ref", ref)
    d, T = nn_params("nn_build", max_dist, n, table_bits)
    _tensor_table("nn_build", (), [("start", start, torch.int32, (T + 1,)), ("records", records, torch.float32, (n, 4))])
    _same_device("nn_build", ref=ref, start=start, records=records)
    dev = ref.device
    start = torch.empty((T + 1,), device=dev, dtype=torch.int32) if start is None else start
    records = torch.empty((n, 4), device=dev, dtype=torch.float32) if records is None else records
    ws = torch.empty((_size_or_raise(_lib.load().pnr_nn_workspace_bytes(n, T), "pnr_nn_workspace_bytes") // 8,), device=dev, dtype=torch.int64)
    _lib.check(_lib.load().pnr_nn_build(_p(ref if n else None), n, d, T, _p(start), _p(records if n else None), _p(ws), _stream()), "pnr_nn_build")
    return start, records


@_on_device
def nn_query(ref, start, records, query, max_dist, index=None, dist2=None, stats=None):
    """Nearest reference point within max_dist of every row of query (m, 3) float32 (pnr_nn_query).  ref, start, records and
    max_dist are nn_build's.  Returns (index (m,) int32, dist2 (m,) float32): -1 and +inf where no reference point is within
    max_dist or the query is not finite; a tie in distance goes to the lowest index.  stats: (3,) int64, accumulated: queries
    that found a neighbour / had none in the radius / were invalid.  Never synchronises: the call can be captured."""
    n = _cloud("nn_query", "ref", ref)
    T = _nn_table("nn_query", start, records, n)
    m = _cloud("nn_query", "query", query)
    d, T = nn_params("nn_query", max_dist, n, T.bit_length() - 1)
    _tensor_table("nn_query", (), [("index", index, torch.int32, (m,)), ("dist2", dist2, torch.float32, (m,)), ("stats", stats, torch.int64, (3,))])
    _same_device("nn_query", query=query, ref=ref, start=start, records=records, index=index, dist2=dist2, stats=stats)
    dev = query.device
    index = torch.empty((m,), device=dev, dtype=torch.int32) if index is None else index
    dist2 = torch.empty((m,), device=dev, dtype=torch.float32) if dist2 is None else dist2
    _lib.check(_lib.load().pnr_nn_query(_p(ref if n else None), n, d, T, _p(start), _p(records if n else None), _p(query if m else None), m,
                                        _p(index if m else None), _p(dist2 if m else None), _p(stats), _stream()), "pnr_nn_query")
    return index, dist2


def cloud_thresholds(what, thresholds, max_dist):
    """the thresholds of cloud_metrics as host floats: at most 8, each in (0, max_dist] as float32"""
    try:
        taus = [_f32(float(t)) for t in thresholds]
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: thresholds must be a sequence of numbers (got %r)" % (what, thresholds)) from None
    if len(taus) > CLOUD_MAX_TAU:
        raise ValueError("%s: at most %d thresholds (got %d)" % (what, CLOUD_MAX_TAU, len(taus)))
    for t in taus:
        if not (0.0 < t <= max_dist):
            raise ValueError("%s: every threshold must satisfy 0 < tau <= max_dist = %r (got %r)" % (what, max_dist, t))
    return taus


@_on_device
def cloud_metrics(index, dist2, max_dist, thresholds=(), query=None, sums=None, counts=None):
    """Distance terms of one direction of a cloud comparison from nn_query's answers (pnr_cloud_metrics; the rule is in
    include/pnr.h "nearest neighbours").  A row counts where dist2 is not NaN and, when `query` (m, 3) -- the coordinates that
    were asked -- is given, the query was finite.  d = sqrt(dist2) in double where a neighbour was found, else max_dist.
    Returns (sums (2,) float64, counts (10,) int64), accumulated into when given:
      sums:   d, d^2;     counts: rows counted, rows without a neighbour, then per threshold tau_k the rows with dist2 <= tau_k^2.
    Deterministic: no floating atomics."""
    m = _cloud("cloud_metrics", "index", index, torch.int32, 0)
    _tensor_table("cloud_metrics", [("dist2", dist2, torch.float32, (m,))],
                  [("query", query, torch.float32, (m, 3)), ("sums", sums, torch.float64, (2,)), ("counts", counts, torch.int64, (CLOUD_COUNTS,))])
    d, _ = nn_params("cloud_metrics", max_dist, m)
    taus = cloud_thresholds("cloud_metrics", thresholds, d)
    _same_device("cloud_metrics", index=index, dist2=dist2, query=query, sums=sums, counts=counts)
    dev = index.device
    sums = torch.zeros((2,), device=dev, dtype=torch.float64) if sums is None else sums
    counts = torch.zeros((CLOUD_COUNTS,), device=dev, dtype=torch.int64) if counts is None else counts
    ws = torch.empty((_size_or_raise(_lib.load().pnr_cloud_metrics_workspace_bytes(m), "pnr_cloud_metrics_workspace_bytes") // 8,),
                     device=dev, dtype=torch.float64)
    tau_h = (ctypes.c_float * max(len(taus), 1))(*taus)
    _lib.check(_lib.load().pnr_cloud_metrics(_p(index if m else None), _p(dist2 if m else None), _p(query if m else None), m, d, tau_h, len(taus),
                                             _p(sums), _p(counts), _p(ws), _stream()), "pnr_cloud_metrics")
    return sums, counts


def _sample_mesh(what, vertices, faces, seed):
    """(V, F, seed as a signed 64-bit word) of the mesh arguments of the sampling ops: type, dtype, shape"""
    V = _cloud(what, "vertices", vertices)
    F = _cloud(what, "faces", faces, torch.int32)
    if F > NN_MAX_POINTS - 1:
        raise ValueError("%s: faces holds %d rows, more than 2^31 - 2" % (what, F))
    if isinstance(seed, bool) or not isinstance(seed, int) or not (-2 ** 63 <= seed < 2 ** 64):
        raise ValueError("%s: seed must be an integer of at most 64 bits (got %r)" % (what, seed))
    return V, F, seed - 2 ** 64 if seed >= 2 ** 63 else seed


@_on_device
def mesh_sample_count(vertices, faces, density, seed=0, start=None, total=None):
    """Count the surface points mesh sampling puts on every triangle at `density` points per unit area and scan the counts
    (pnr_mesh_sample_count; the rule is in include/pnr.h "nearest neighbours", MESH SAMPLING).  vertices (V, 3) float32, faces
    (F, 3) int32.  Returns (total, start): total (1,) int64 ON THE DEVICE -- reading it is the caller's synchronisation --,
    start (F + 1,) int32 the exclusive scan mesh_sample_emit needs.  Both may be caller-owned."""
    V, F, seed = _sample_mesh("mesh_sample_count", vertices, faces, seed)
    try:
        rho = _f32(float(density))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("mesh_sample_count: density must be a finite number >= 0 (got %r)" % (density,)) from None
    if not (0.0 <= rho < _INF):
        raise ValueError("mesh_sample_count: density must be finite and >= 0 (got %r)" % (density,))
    _tensor_table("mesh_sample_count", (), [("start", start, torch.int32, (F + 1,)), ("total", total, torch.int64, (1,))])
    _same_device("mesh_sample_count", vertices=vertices, faces=faces, start=start, total=total)
    dev = vertices.device
    start = torch.empty((F + 1,), device=dev, dtype=torch.int32) if start is None else start
    total = torch.empty((1,), device=dev, dtype=torch.int64) if total is None else total
    ws = torch.empty((_size_or_raise(_lib.load().pnr_mesh_sample_workspace_bytes(F), "pnr_mesh_sample_workspace_bytes") // 8,), device=dev, dtype=torch.int64)
    _lib.check(_lib.load().pnr_mesh_sample_count(_p(vertices if V else None), V, _p(faces if F else None), F, rho, seed, _p(start), _p(total), _p(ws),
                                                 _stream()), "pnr_mesh_sample_count")
    return total, start


@_on_device
def mesh_sample_emit(vertices, faces, seed, start, points, face):
    """Write the points mesh_sample_count counted (pnr_mesh_sample_emit): points (N, 3) float32 and face (N,) int32, the triangle
    of each point, caller-owned and sized by mesh_sample_count's total; in triangle order, then draw order.  vertices, faces,
    seed and start are mesh_sample_count's."""
    V, F, seed = _sample_mesh("mesh_sample_emit", vertices, faces, seed)
    N = _cloud("mesh_sample_emit", "points", points)
    _tensor_table("mesh_sample_emit", [("start", start, torch.int32, (F + 1,)), ("face", face, torch.int32, (N,))])
    if N and not F:
        raise ValueError("mesh_sample_emit: %d points asked of a mesh without faces" % N)
    _same_device("mesh_sample_emit", vertices=vertices, faces=faces, start=start, points=points, face=face)
    _lib.check(_lib.load().pnr_mesh_sample_emit(_p(vertices if V else None), V, _p(faces if F else None), F, seed, _p(start), N,
                                                _p(points if N else None), _p(face if N else None), _stream()), "pnr_mesh_sample_emit")
    return points, face


CC_MAX_ELEMENTS = 2 ** 31 - 2                   # include/pnr.h "connected components": n + 1 int32 entries are scanned
CC_KEYS, CC_VALUES = _lib.CC_KEYS, _lib.CC_VALUES
CC_TILE_2D, CC_TILE_3D = _lib.CC_TILE_2D, _lib.CC_TILE_3D      # (tx, ty) of an image, (tx, ty, tz) of a volume
_CC_MODES = {torch.int32: CC_KEYS, torch.float32: CC_VALUES}


def cc_tol(what, tol):
    """tol of the values mode as a float32: >= 0, +inf allowed, NaN refused"""
    try:
        t = _f32(float(tol))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: tol must be a number >= 0 (got %r)" % (what, tol)) from None
    if not (t >= 0.0):
        raise ValueError("%s: tol must be >= 0 and not NaN (got %r)" % (what, tol))
    return t


def _cc_lattice(what, name, t):
    """(res_x, res_y, res_z) of a components lattice: (res_z, res_y, res_x), or an image (height, width) as res_z = 1"""
    if t.dim() not in (2, 3):
        raise ValueError("%s: %s must be an image (height, width) or a lattice (res_z, res_y, res_x), got %s" % (what, name, tuple(t.shape)))
    return _lattice_shape(what, name, t.unsqueeze(0) if t.dim() == 2 else t, 1, CC_MAX_ELEMENTS, "2^31 - 2")


def _cc_workspace(what, n, workspace, dev):
    """the int64 workspace of a components call over n elements: the caller's, checked, or a new one"""
    words = cc_workspace_bytes(n) // 8
    if workspace is None:
        return torch.empty((words,), device=dev, dtype=torch.int64)
    if not _is_tensor(workspace, torch.int64) or workspace.dim() != 1 or workspace.numel() < words:
        raise ValueError("%s: workspace must be an int64 tensor of at least %d words" % (what, words))
    return workspace


def cc_workspace_bytes(n_elements):
    """pnr_cc_workspace_bytes: host arithmetic only; more than 2^31 - 2 elements raises"""
    return _size_or_raise(_lib.load().pnr_cc_workspace_bytes(int(n_elements)), "pnr_cc_workspace_bytes")


@_on_device
def cc_label(data, full=False, tol=None, labels=None, size=True, count=None, workspace=None):
    """Connected components of the lattice `data` (res_z, res_y, res_x), or of an image (height, width) (pnr_cc_label; the rule
    is in include/pnr.h "connected components").  int32 data are keys: foreground iff key >= 0, neighbours linked iff their
    keys are equal.  float32 data are values and need tol: foreground iff finite and > 0, linked iff |a - b| <= tol.  full:
    False links the 4 / 6 axis neighbours, True the 8 / 26.  Returns (labels, size, count): labels int32 of the data's shape,
    -1 on background, else the component's number in 0 .. count - 1, by lowest flat index; size int32 of that shape, the
    number of elements of each element's component (size=False: None; a tensor: caller-owned); count (1,) int64 ON THE
    DEVICE.  Never synchronises: the call can be captured."""
    what = "cc_label"
    _tensor(what, "data", data)
    if data.dtype not in _CC_MODES:
        raise TypeError("%s: data must be torch.int32 (keys) or torch.float32 (values), got %s" % (what, data.dtype))
    rx, ry, rz = _cc_lattice(what, "data", data)
    mode = _CC_MODES[data.dtype]
    if mode == CC_VALUES:
        if tol is None:
            raise ValueError("%s: float32 data are values and need tol" % what)
        tol = cc_tol(what, tol)
    elif tol is not None:
        raise ValueError("%s: tol goes with float32 data; int32 keys are linked where they are equal" % what)
    if full not in (False, True, 0, 1):
        raise ValueError("%s: full must be False or True (got %r)" % (what, full))
    shape = tuple(data.shape)
    own_size = size if isinstance(size, torch.Tensor) else None
    if own_size is None and size not in (False, True, None):
        raise ValueError("%s: size must be True, False or an int32 tensor of the data's shape (got %s)" % (what, type(size).__name__))
    _tensor_table(what, (), [("labels", labels, torch.int32, shape), ("size", own_size, torch.int32, shape), ("count", count, torch.int64, (1,))])
    _same_device(what, data=data, labels=labels, size=own_size, count=count, workspace=workspace)
    for name, t in (("labels", labels), ("size", own_size)):
        if t is not None and t.data_ptr() == data.data_ptr():
            raise ValueError("%s: %s may not alias data" % (what, name))
    dev = data.device
    workspace = _cc_workspace(what, data.numel(), workspace, dev)
    labels = torch.empty(shape, device=dev, dtype=torch.int32) if labels is None else labels
    if own_size is None and size:
        own_size = torch.empty(shape, device=dev, dtype=torch.int32)
    count = torch.empty((1,), device=dev, dtype=torch.int64) if count is None else count
    _lib.check(_lib.load().pnr_cc_label(_p(data), mode, tol if mode == CC_VALUES else 0.0, rx, ry, rz, int(bool(full)), _p(labels), _p(own_size),
                                        _p(count), _p(workspace), _stream()), "pnr_cc_label")
    return labels, own_size, count


@_on_device
def cc_mesh(faces, n_vertices, vertex_label=None, face_label=None, face_size=True, count=None, workspace=None):
    """Connected components of a mesh by its indices (pnr_cc_mesh): faces (F, 3) int32 over the vertices 0 .. n_vertices - 1; a
    face links its three vertices, a face with an index out of range links nothing.  Returns (vertex_label (V,), face_label
    (F,), face_size (F,), count (1,) int64 ON THE DEVICE): labels by lowest vertex index, -1 for a vertex no valid face uses and
    for a face that is not valid; face_size the number of valid faces of the face's component (False: None).  Every output may
    be caller-owned.  Never synchronises."""
    what = "cc_mesh"
    F = _cloud(what, "faces", faces, torch.int32)
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, int) or not (0 <= n_vertices <= CC_MAX_ELEMENTS):
        raise ValueError("%s: n_vertices must be an integer in 0 .. 2^31 - 2 (got %r)" % (what, n_vertices))
    V = n_vertices
    own_size = face_size if isinstance(face_size, torch.Tensor) else None
    if own_size is None and face_size not in (False, True, None):
        raise ValueError("%s: face_size must be True, False or an (F,) int32 tensor (got %s)" % (what, type(face_size).__name__))
    _tensor_table(what, (), [("vertex_label", vertex_label, torch.int32, (V,)), ("face_label", face_label, torch.int32, (F,)),
                             ("face_size", own_size, torch.int32, (F,)), ("count", count, torch.int64, (1,))])
    _same_device(what, faces=faces, vertex_label=vertex_label, face_label=face_label, face_size=own_size, count=count, workspace=workspace)
    dev = faces.device
    workspace = _cc_workspace(what, V, workspace, dev)
    vertex_label = torch.empty((V,), device=dev, dtype=torch.int32) if vertex_label is None else vertex_label
    face_label = torch.empty((F,), device=dev, dtype=torch.int32) if face_label is None else face_label
    if own_size is None and face_size:
        own_size = torch.empty((F,), device=dev, dtype=torch.int32)
    count = torch.empty((1,), device=dev, dtype=torch.int64) if count is None else count
    _lib.check(_lib.load().pnr_cc_mesh(_p(faces if F else None), F, V, _p(vertex_label if V else None), _p(face_label if F else None),
                                       _p(own_size if own_size is not None and F else None), _p(count), _p(workspace), _stream()), "pnr_cc_mesh")
    return vertex_label, face_label, own_size, count


@_on_device
def cc_stats(labels, size, n_components, sizes=None, boxes=True):
    """Per-component statistics of a labelling (pnr_cc_stats): labels and size as cc_label wrote them (or cc_mesh's face_label
    and face_size, (F,) viewed as a 1 x 1 x F lattice), n_components the count the caller read.  Returns (sizes (n,) int32,
    boxes (n, 6) int32 = (ix_min, iy_min, iz_min, ix_max, iy_max, iz_max); boxes=False: None).  Both may be caller-owned.
    Never synchronises."""
    what = "cc_stats"
    _tensor(what, "labels", labels)
    if labels.dtype != torch.int32:
        raise TypeError("%s: labels must be %s, got %s" % (what, torch.int32, labels.dtype))
    if isinstance(n_components, bool) or not isinstance(n_components, int) or not (0 <= n_components <= CC_MAX_ELEMENTS):
        raise ValueError("%s: n_components must be an integer in 0 .. 2^31 - 2 (got %r)" % (what, n_components))
    n = n_components
    own_boxes = boxes if isinstance(boxes, torch.Tensor) else None
    if own_boxes is None and boxes not in (False, True, None):
        raise ValueError("%s: boxes must be True, False or an (n, 6) int32 tensor (got %s)" % (what, type(boxes).__name__))
    dev = labels.device
    if labels.dim() == 1 and not labels.numel():            # no elements (a mesh without faces): nothing to launch
        rx = ry = rz = 0
    else:                                                   # (F,): a mesh's faces as a 1 x 1 x F lattice
        rx, ry, rz = _cc_lattice(what, "labels", labels.reshape(1, 1, -1) if labels.dim() == 1 else labels)
    _tensor_table(what, [("labels", labels, torch.int32, tuple(labels.shape)), ("size", size, torch.int32, tuple(labels.shape))],
                  [("sizes", sizes, torch.int32, (n,)), ("boxes", own_boxes, torch.int32, (n, 6))])
    _same_device(what, labels=labels, size=size, sizes=sizes, boxes=own_boxes)
    sizes = torch.zeros((n,), device=dev, dtype=torch.int32) if sizes is None else sizes
    if own_boxes is None and boxes:
        own_boxes = torch.zeros((n, 6), device=dev, dtype=torch.int32)
    if rx and n:
        _lib.check(_lib.load().pnr_cc_stats(_p(labels), _p(size), rx, ry, rz, n, _p(sizes), _p(own_boxes), _stream()), "pnr_cc_stats")
    return sizes, own_boxes


TSDF_MAX_POINTS = 2 ** 31 - 1                   # include/pnr.h "depth fusion"
TSDF_BLOCK, TSDF_BLOCKS_PER_CU = 256, 8         # PNR_TSDF_BLOCK, PNR_TSDF_BLOCKS_PER_CU


def integrate_params(what, trunc, max_depth, w_max):
    """the scalars of pnr_tsdf_integrate as floats, or the refusal by name (`what`: the caller's name)"""
    trunc, max_depth, w_max = float(trunc), float(max_depth), float(w_max)
    if not (0.0 < trunc < _INF):
        raise ValueError("%s: trunc must be positive and finite (got %r)" % (what, trunc))
    if not (max_depth > 0.0):
        raise ValueError("%s: max_depth must be positive (it may be inf; got %r)" % (what, max_depth))
    if not (w_max >= 1.0):
        raise ValueError("%s: w_max must be >= 1 (it may be inf; got %r)" % (what, w_max))
    return trunc, max_depth, w_max


@_on_device
def tsdf_integrate(frames, w2c, first, last, lo, step, trunc, tsdf, weight, rgb=None, rgb_weight=None, label=None, conf=None,
                   max_depth=float("inf"), w_max=float("inf")):
    """Fuse the depth frames first .. last - 1 of a device-resident frame table into a TSDF volume (pnr_tsdf_integrate; the rule
    is in include/pnr.h "depth fusion").  frames: uint8 GPU tensor of pnr_frame records (FrameSet.table); w2c: (F, 12) float32,
    row f = camera.invert_pose of frame f's c2w; both are read when the kernel runs.  lo, step: the lattice's float32 origin
    and step per axis (x, y, z), host values (mesh.lattice).  tsdf, weight: (res_z, res_y, res_x) float32, accumulated in
    place; rgb (res_z, res_y, res_x, 3) with rgb_weight, label with conf (int32): optional pairs.  Returns None."""
    what = "tsdf_integrate"
    rx, ry, rz = _lattice_shape(what, "tsdf", tsdf, 1)
    if (rgb is None) != (rgb_weight is None):
        raise ValueError("%s: rgb and rgb_weight go together (both or neither)" % what)
    if (label is None) != (conf is None):
        raise ValueError("%s: label and conf go together (both or neither)" % what)
    res = (rz, ry, rx)
    _tensor_table(what, (("tsdf", tsdf, torch.float32, res), ("weight", weight, torch.float32, res)),
                  (("rgb", rgb, torch.float32, res + (3,)), ("rgb_weight", rgb_weight, torch.float32, res),
                   ("label", label, torch.int32, res), ("conf", conf, torch.int32, res)))
    if not _is_tensor(frames, torch.uint8) or frames.dim() != 1 or frames.numel() % ctypes.sizeof(_lib.Frame):
        raise ValueError("%s: frames must be a uint8 tensor of whole pnr_frame records (%d bytes each)" % (what, ctypes.sizeof(_lib.Frame)))
    if not _is_tensor(w2c, torch.float32) or w2c.dim() != 2 or w2c.shape[1] != 12:
        raise ValueError("%s: w2c must be an (F, 12) float32 tensor" % what)
    first, last = int(first), int(last)
    n_rec = min(frames.numel() // ctypes.sizeof(_lib.Frame), w2c.shape[0])
    if not 0 <= first <= last <= n_rec:
        raise ValueError("%s: need 0 <= first <= last <= %d (the records and w2c rows given), got [%d, %d)" % (what, n_rec, first, last))
    lo_h, step_h = _lattice_floats(what, lo, step)
    trunc, max_depth, w_max = integrate_params(what, trunc, max_depth, w_max)
    _same_device(what, tsdf=tsdf, weight=weight, rgb=rgb, rgb_weight=rgb_weight, label=label, conf=conf, frames=frames, w2c=w2c)
    if first == last:
        return
    _lib.check(_lib.load().pnr_tsdf_integrate(_p(frames), _p(w2c), first, last, rx, ry, rz, lo_h, step_h, trunc, max_depth, w_max,
                                              _p(tsdf), _p(weight), _p(rgb), _p(rgb_weight), _p(label), _p(conf), _stream()),
               "pnr_tsdf_integrate")


RAYCAST_HIT, RAYCAST_NO_RAY, RAYCAST_MISSED, RAYCAST_NO_SURFACE = 0, 1, 2, 3      # PNR_RAYCAST_* (include/pnr.h "volume ray casting")


def raycast_params(what, near, far, min_weight, dt, max_steps, res, step, dt_name="dt"):
    """the scalars of pnr_tsdf_raycast with the defaults of dt and max_steps filled in, or the refusal by name (dt_name: the caller's)"""
    near, far, min_weight = float(near), float(far), float(min_weight)
    if not (near >= 0.0 and far > near):
        raise ValueError("%s: need 0 <= near < far (got %r, %r)" % (what, near, far))
    if not (min_weight > 0.0):
        raise ValueError("%s: min_weight must be positive (got %r)" % (what, min_weight))
    dt = raycast_default_dt(step) if dt is None else float(dt)
    if not (0.0 < dt < _INF):
        raise ValueError("%s: %s must be positive and finite (got %r)" % (what, dt_name, dt))
    max_steps = raycast_default_max_steps(res, step, dt) if max_steps is None else int(max_steps)
    if max_steps < 0:
        raise ValueError("%s: max_steps must be >= 0 (got %d)" % (what, max_steps))
    return near, far, min_weight, dt, max_steps


@_on_device
def tsdf_raycast(camera_model, cam, c2w, width, height, near, far, lo, step, tsdf, weight, depth, code, normal=None, src=None,
                 min_weight=1.0, dt=None, max_steps=None):
    """Render a TSDF volume into a camera (pnr_tsdf_raycast; the rule is in include/pnr.h "volume ray casting").  camera_model:
    "pinhole", "fisheye" or "equirect" with cam as project_points takes it; c2w: 3x4 camera-to-world (host values).  lo, step: the
    lattice's float32 origin and step per axis (x, y, z), host values (mesh.lattice); tsdf, weight: (res_z, res_y, res_x) float32,
    every res >= 2, read when the kernel runs.  Outputs, caller-owned (height, width) images: depth float32, code uint8, and
    optionally normal (height, width, 3) float32 and src int32.  dt: the march step in units of the ray parameter (None: half the
    smallest |step|); max_steps: the most samples a ray takes (None: enough for the lattice's diagonal at that dt).  Returns None."""
    what = "tsdf_raycast"
    word, cam_h = _camera_model(what, "camera_model", camera_model, cam)
    c2w_h = _host_floats(c2w, 12, what + ": c2w")
    width, height = _image_size(what, width, height)
    rx, ry, rz = _lattice_shape(what, "tsdf", tsdf, 2)
    _tensor_table(what, (("tsdf", tsdf, torch.float32, (rz, ry, rx)), ("weight", weight, torch.float32, (rz, ry, rx)),
                         ("depth", depth, torch.float32, (height, width)), ("code", code, torch.uint8, (height, width))),
                  (("normal", normal, torch.float32, (height, width, 3)), ("src", src, torch.int32, (height, width))))
    lo_h, step_h = _lattice_floats(what, lo, step)
    near, far, min_weight, dt, max_steps = raycast_params(what, near, far, min_weight, dt, max_steps, (rx, ry, rz), step_h)
    _same_device(what, tsdf=tsdf, weight=weight, depth=depth, code=code, normal=normal, src=src)
    _lib.check(_lib.load().pnr_tsdf_raycast(word, cam_h, c2w_h, width, height, near, far, rx, ry, rz, lo_h, step_h, _p(tsdf), _p(weight),
                                            min_weight, dt, max_steps, _p(depth), _p(normal), _p(src), _p(code), _stream()),
               "pnr_tsdf_raycast")


def raycast_default_dt(step):
    """half the smallest |step| of the lattice, as a float32: roughly every second sample stays in its cell"""
    return float(torch.tensor([abs(float(s)) for s in step], dtype=torch.float32).min() * 0.5)


def raycast_default_max_steps(res, step, dt):
    """samples enough for the lattice's diagonal at march step dt: a ray's parameter never runs faster than arc length (|d| >= 1
    in every model), so no ray inside the lattice takes more"""
    diag = sum(((int(r) - 1) * float(s)) ** 2 for r, s in zip(res, step)) ** 0.5
    return min(int(diag / float(dt)) + 2, 2 ** 31 - 1)


MESHCAST_MAX_RES = _lib.MESHCAST_MAX_RES        # PNR_MESHCAST_MAX_RES (include/pnr.h "mesh ray casting")
MESHCAST_MAX_ENTRIES = 2 ** 31 - 1
MESHCAST_OUTPUTS = (("depth", torch.float32, ()), ("face", torch.int32, ()), ("code", torch.uint8, ()), ("bary", torch.float32, (3,)),
                    ("vertex", torch.int32, ()), ("normal", torch.float32, (3,)), ("side", torch.int8, ()))


def meshcast_mesh(what, vertices, faces):
    """(V, F) of the mesh arguments of the ray-casting ops: vertices (V, 3) float32, faces (F, 3) int32 on any device"""
    return _cloud(what, "vertices", vertices), _cloud(what, "faces", faces, torch.int32)


def meshcast_res(what, res):
    """res = (res_x, res_y, res_z) of a ray-casting grid as ints, each within 1 .. 1024, or the refusal by name"""
    try:
        r = tuple(int(v) for v in res)
    except (TypeError, ValueError):
        raise ValueError("%s: res must be three integers (res_x, res_y, res_z), got %r" % (what, res)) from None
    if len(r) != 3 or any(isinstance(v, bool) for v in res) or not all(1 <= v <= MESHCAST_MAX_RES for v in r):
        raise ValueError("%s: res must be three integers within 1 .. %d, got %r" % (what, MESHCAST_MAX_RES, res))
    return r


def meshcast_grid(what, res, lo, cell):
    """(res, lo, cell) of a ray-casting grid with lo and cell as host floats: lo finite, cell positive and finite with a finite
    float32 inverse"""
    res = meshcast_res(what, res)
    lo_h, cell_h = _host_floats(lo, 3, what + ": lo"), _host_floats(cell, 3, what + ": cell")
    if not all(abs(v) < _INF for v in lo_h):
        raise ValueError("%s: lo must be finite (got %r)" % (what, list(lo_h)))
    if not all(0.0 < v < _INF and _f32(1.0 / v) < _INF for v in cell_h):
        raise ValueError("%s: cell must be positive and finite, with a finite inverse (got %r)" % (what, list(cell_h)))
    return res, lo_h, cell_h


def meshcast_range(what, near, far):
    near, far = float(near), float(far)
    if not (near >= 0.0 and far > near):
        raise ValueError("%s: need 0 <= near < far (got %r, %r)" % (what, near, far))
    return near, far


def _meshcast_table(what, res, start, records):
    """n_entries of the (start, records) pair of a grid of `res`: type, dtype, shape"""
    cells = res[0] * res[1] * res[2]
    _tensor_table(what, [("start", start, torch.int32, (cells + 1,))])
    _tensor(what, "records", records)
    if records.dtype != torch.float32:
        raise TypeError("%s: records must be torch.float32, got %s" % (what, records.dtype))
    if records.dim() != 2 or records.shape[1] != 12 or records.shape[0] > MESHCAST_MAX_ENTRIES:
        raise ValueError("%s: records must be (n_entries, 12) with at most 2^31 - 1 entries, got %s" % (what, tuple(records.shape)))
    return records.shape[0]


def mesh_grid_workspace(res, device):
    """the block that mesh_grid_bounds, mesh_grid_count and mesh_grid_fill share for a grid of `res`"""
    res = meshcast_res("mesh_grid_workspace", res)
    return torch.empty((_size_or_raise(_lib.load().pnr_mesh_grid_workspace_bytes(*res), "pnr_mesh_grid_workspace_bytes") // 8,), device=device, dtype=torch.int64)


@_on_device
def mesh_grid_bounds(vertices, faces, bounds=None):
    """The box of a mesh's usable faces (pnr_mesh_grid_bounds; include/pnr.h "mesh ray casting", THE INDEX).  Returns bounds (8,)
    float32 ON THE DEVICE -- reading it is the caller's synchronisation: lo (3), hi (3), the bits of the number of usable faces
    (bounds.view(torch.int32)[6]), 0.  +inf / -inf without a usable face."""
    what = "mesh_grid_bounds"
    V, F = meshcast_mesh(what, vertices, faces)
    _tensor_table(what, (), [("bounds", bounds, torch.float32, (8,))])
    _same_device(what, vertices=vertices, faces=faces, bounds=bounds)
    dev = vertices.device
    bounds = torch.empty((8,), device=dev, dtype=torch.float32) if bounds is None else bounds
    ws = mesh_grid_workspace((1, 1, 1), dev)
    _lib.check(_lib.load().pnr_mesh_grid_bounds(_p(vertices if V else None), V, _p(faces if F else None), F, _p(bounds), _p(ws), _stream()),
               "pnr_mesh_grid_bounds")
    return bounds


@_on_device
def mesh_grid_count(vertices, faces, res, lo, cell, start=None, total=None, workspace=None):
    """Count the entries of every cell of a ray-casting grid and scan them (pnr_mesh_grid_count).  res = (res_x, res_y, res_z); lo,
    cell: the grid's float32 origin and cell size per axis, host values.  Returns (total, start, workspace): total (1,) int64 ON
    THE DEVICE -- reading it is the caller's synchronisation --, start (cells + 1,) int32, and the workspace mesh_grid_fill needs."""
    what = "mesh_grid_count"
    V, F = meshcast_mesh(what, vertices, faces)
    res, lo_h, cell_h = meshcast_grid(what, res, lo, cell)
    cells = res[0] * res[1] * res[2]
    _tensor_table(what, (), [("start", start, torch.int32, (cells + 1,)), ("total", total, torch.int64, (1,))])
    _same_device(what, vertices=vertices, faces=faces, start=start, total=total, workspace=workspace)
    dev = vertices.device
    start = torch.empty((cells + 1,), device=dev, dtype=torch.int32) if start is None else start
    total = torch.empty((1,), device=dev, dtype=torch.int64) if total is None else total
    workspace = mesh_grid_workspace(res, dev) if workspace is None else workspace
    _lib.check(_lib.load().pnr_mesh_grid_count(_p(vertices if V else None), V, _p(faces if F else None), F, res[0], res[1], res[2], lo_h, cell_h,
                                               _p(start), _p(total), _p(workspace), _stream()), "pnr_mesh_grid_count")
    return total, start, workspace


@_on_device
def mesh_grid_fill(vertices, faces, res, lo, cell, start, records, workspace):
    """Write the 48-byte records mesh_grid_count counted (pnr_mesh_grid_fill): records (n_entries, 12) float32, caller-owned and
    sized by mesh_grid_count's total; mesh, grid, start and workspace are mesh_grid_count's."""
    what = "mesh_grid_fill"
    V, F = meshcast_mesh(what, vertices, faces)
    res, lo_h, cell_h = meshcast_grid(what, res, lo, cell)
    n = _meshcast_table(what, res, start, records)
    _tensor(what, "workspace", workspace)
    _same_device(what, vertices=vertices, faces=faces, start=start, records=records, workspace=workspace)
    _lib.check(_lib.load().pnr_mesh_grid_fill(_p(vertices if V else None), V, _p(faces if F else None), F, res[0], res[1], res[2], lo_h, cell_h,
                                              _p(start), n, _p(records if n else None), _p(workspace), _stream()), "pnr_mesh_grid_fill")
    return records


def _meshcast_outputs(what, lead, out):
    """the output arrays of a cast as pnr_mesh_* takes them: `out` maps names of MESHCAST_OUTPUTS to caller-owned tensors of shape
    lead + the output's own; depth, face and code are needed"""
    if not isinstance(out, dict):
        raise ValueError("%s: out must be a dict of output tensors, got %s" % (what, type(out).__name__))
    _names(what, out, [n for n, _, _ in MESHCAST_OUTPUTS], "unknown output %(key)s (known: %(known)s)")
    _tensor_table(what, [(n, out.get(n), dt, lead + tail) for n, dt, tail in MESHCAST_OUTPUTS[:3]],
                  [(n, out.get(n), dt, lead + tail) for n, dt, tail in MESHCAST_OUTPUTS[3:]])
    return [out.get(n) for n, _, _ in MESHCAST_OUTPUTS]


@_on_device
def mesh_raycast(camera_model, cam, c2w, width, height, near, far, vertices, faces, res, lo, cell, start, records, out):
    """First hit of every pixel's ray with a triangle mesh (pnr_mesh_raycast; the rule is in include/pnr.h "mesh ray casting").
    camera_model, cam, c2w, width, height: as tsdf_raycast takes them.  vertices, faces: the mesh; res, lo, cell, start, records:
    the grid mesh_grid_count / mesh_grid_fill built for it.  out: dict of caller-owned (height, width, ...) images -- depth float32,
    face int32, code uint8, and optionally bary (., 3) float32, vertex int32, normal (., 3) float32, side int8.  Never
    synchronises; returns None."""
    what = "mesh_raycast"
    word, cam_h = _camera_model(what, "camera_model", camera_model, cam)
    c2w_h = _host_floats(c2w, 12, what + ": c2w")
    width, height = _image_size(what, width, height)
    near, far = meshcast_range(what, near, far)
    V, F = meshcast_mesh(what, vertices, faces)
    res, lo_h, cell_h = meshcast_grid(what, res, lo, cell)
    n = _meshcast_table(what, res, start, records)
    outs = _meshcast_outputs(what, (height, width), out)
    _same_device(what, vertices=vertices, faces=faces, start=start, records=records, **out)
    _lib.check(_lib.load().pnr_mesh_raycast(word, cam_h, c2w_h, width, height, near, far, _p(vertices if V else None), V, _p(faces if F else None), F,
                                            res[0], res[1], res[2], lo_h, cell_h, _p(start), _p(records if n else None), n, *[_p(t) for t in outs],
                                            _stream()), "pnr_mesh_raycast")


@_on_device
def mesh_cast_rays(rays, vertices, faces, res, lo, cell, start, records, out):
    """First hit of every ray of rays (n, 8) float32 = (o, d, near, far) with a triangle mesh (pnr_mesh_cast_rays): mesh_raycast
    with the rays given; out: (n, ...) arrays.  The rays are read when the kernel runs.  Never synchronises; returns None."""
    what = "mesh_cast_rays"
    _tensor(what, "rays", rays)
    if rays.dtype != torch.float32:
        raise TypeError("%s: rays must be torch.float32, got %s" % (what, rays.dtype))
    R = _rays(what, rays)
    if R > NN_MAX_POINTS:
        raise ValueError("%s: rays holds %d rows, more than 2^31 - 1" % (what, R))
    V, F = meshcast_mesh(what, vertices, faces)
    res, lo_h, cell_h = meshcast_grid(what, res, lo, cell)
    n = _meshcast_table(what, res, start, records)
    outs = _meshcast_outputs(what, (R,), out)
    _same_device(what, rays=rays, vertices=vertices, faces=faces, start=start, records=records, **out)
    if R == 0:
        return
    _lib.check(_lib.load().pnr_mesh_cast_rays(_p(rays), R, _p(vertices if V else None), V, _p(faces if F else None), F, res[0], res[1], res[2],
                                              lo_h, cell_h, _p(start), _p(records if n else None), n, *[_p(t) for t in outs], _stream()),
               "pnr_mesh_cast_rays")


# PNR_ICP_* (include/pnr.h "pose tracking"): the per-pixel codes and the solve's status
ICP_MATCH, ICP_NO_DEPTH, ICP_OUTSIDE, ICP_NO_MODEL, ICP_TOO_FAR, ICP_BACK_FACING = 0, 1, 2, 3, 4, 5
ICP_OK, ICP_TOO_FEW, ICP_DEGENERATE, ICP_STEP_TOO_LARGE = 0, 1, 2, 3
ICP_MAX_ROT = 0.5


def icp_accumulate_params(what, dist_max):
    """the scalar of pnr_icp_accumulate as a float, or the refusal by name (`what`: the caller's name)"""
    dist_max = float(dist_max)
    if not (0.0 < dist_max < 1.8e19):
        raise ValueError("%s: dist_max must be positive with a finite float32 square (got %r)" % (what, dist_max))
    return dist_max


def icp_solve_params(what, min_matches, max_rot, max_trans):
    """the scalars of pnr_icp_solve, or the refusal by name"""
    min_matches, max_rot, max_trans = int(min_matches), float(max_rot), float(max_trans)
    if min_matches < 1:
        raise ValueError("%s: min_matches must be >= 1 (got %d)" % (what, min_matches))
    if not (0.0 < max_rot <= ICP_MAX_ROT):
        raise ValueError("%s: max_rot must lie in (0, %g] radians (got %r)" % (what, ICP_MAX_ROT, max_rot))
    if not (max_trans > 0.0):
        raise ValueError("%s: max_trans must be positive (it may be inf; got %r)" % (what, max_trans))
    return min_matches, max_rot, max_trans


def icp_workspace(n_pix, device):
    """the workspace of icp_accumulate / icp_solve for a live frame of n_pix pixels: a float64 tensor on `device`"""
    n = _size_or_raise(_lib.load().pnr_icp_workspace_bytes(int(n_pix)), "pnr_icp_workspace_bytes")
    return torch.empty((n // 8,), dtype=torch.float64, device=device)


def _icp_pose(pose12, what):
    _tensor(what, "pose12", pose12, "a GPU tensor of 12 float32 (the 3x4 camera-to-world, updated in place)")
    _chk(pose12, what + ": pose12")
    if pose12.numel() != 12:
        raise ValueError("%s: pose12 must hold 12 values (3x4 row-major), got %s" % (what, tuple(pose12.shape)))


def _icp_workspace(workspace, n_pix, what):
    _tensor(what, "workspace", workspace, "a GPU tensor (ops.icp_workspace)")
    _chk(workspace, what + ": workspace", torch.float64)
    need = _size_or_raise(_lib.load().pnr_icp_workspace_bytes(n_pix), "pnr_icp_workspace_bytes") // 8
    if workspace.dim() != 1 or workspace.numel() < need:
        raise ValueError("%s: workspace must be a flat float64 tensor of at least %d elements (ops.icp_workspace), got %s"
                         % (what, need, tuple(workspace.shape)))


@_on_device
def icp_accumulate(camera_model, cam, width, height, depth, pose12, model_camera_model, model_cam, model_c2w, model_width, model_height,
                   model_depth, model_normal, dist_max, workspace, code=None, residual=None):
    """One linearisation of point-to-plane ICP (pnr_icp_accumulate; the rule is in include/pnr.h "pose tracking").  The live side:
    camera_model / cam / width / height as project_points takes a camera, depth a (height, width) float32 image, pose12 the
    DEVICE pose (12 float32, 3x4 camera-to-world), read when the kernel runs.  The model side: its camera, model_c2w (3x4 host
    values; the w2c is camera.invert_pose of it), model_depth (model_height, model_width) and model_normal (., ., 3) float32 as
    fusion.raycast writes them.  workspace: ops.icp_workspace(width * height, device); it receives one row of partial sums per
    workgroup, which icp_solve adds.  Optional outputs: code (height, width) uint8, residual (height, width) float32.  Returns None."""
    what = "icp_accumulate"
    _model_word(what, "camera_model", camera_model), _model_word(what, "model_camera_model", model_camera_model)     # both names first
    word_l, cam_l = _camera_model(what, "camera_model", camera_model, cam)
    word_m, cam_m = _camera_model(what, "model_camera_model", model_camera_model, model_cam, "model_cam")
    c2w_m = _host_floats(model_c2w, 12, what + ": model_c2w")
    w2c_m = _host_floats(_camera.invert_pose(torch.tensor(list(c2w_m), dtype=torch.float32)), 12, what + ": model w2c")
    width, height = _image_size(what, width, height, "size of the live image,")
    wm, hm = _image_size(what, model_width, model_height, "size of the model image,")
    _tensor_table(what, (("depth", depth, torch.float32, (height, width)), ("model_depth", model_depth, torch.float32, (hm, wm)),
                         ("model_normal", model_normal, torch.float32, (hm, wm, 3))),
                  (("code", code, torch.uint8, (height, width)), ("residual", residual, torch.float32, (height, width))))
    dist_max = icp_accumulate_params(what, dist_max)
    _icp_pose(pose12, what)
    _icp_workspace(workspace, width * height, what)
    _same_device(what, depth=depth, pose12=pose12, model_depth=model_depth, model_normal=model_normal, workspace=workspace, code=code,
                 residual=residual)
    _lib.check(_lib.load().pnr_icp_accumulate(word_l, cam_l, width, height, _p(depth), _p(pose12), word_m, cam_m, c2w_m, w2c_m, wm, hm,
                                              _p(model_depth), _p(model_normal), dist_max, _p(workspace), _p(code), _p(residual),
                                              _stream()), "pnr_icp_accumulate")


@_on_device
def icp_solve(workspace, n_pix, pose12, history_row, min_matches=6, max_rot=ICP_MAX_ROT, max_trans=float("inf"), update=True):
    """Add the rows icp_accumulate left in `workspace`, solve the 6 x 6 normal equations and update the device pose in place
    (pnr_icp_solve; one workgroup).  n_pix: the live frame's width * height; pose12: 12 float32 on the GPU; history_row: (5,)
    float64 on the GPU, which receives count, E, |omega|^2, |v|^2, status (ICP_OK, ICP_TOO_FEW, ICP_DEGENERATE,
    ICP_STEP_TOO_LARGE).  The pose changes only with status ICP_OK.  update=False: count and E only, nothing is solved."""
    what = "icp_solve"
    n_pix = int(n_pix)
    if n_pix < 1 or n_pix > MAX_PIXELS:
        raise ValueError("%s: n_pix must lie in 1 .. 2^31 - 1 (got %d)" % (what, n_pix))
    min_matches, max_rot, max_trans = icp_solve_params(what, min_matches, max_rot, max_trans)
    _icp_pose(pose12, what)
    _icp_workspace(workspace, n_pix, what)
    _tensor(what, "history_row", history_row, "a GPU tensor of 5 float64")
    _chk(history_row, what + ": history_row", torch.float64)
    if tuple(history_row.shape) != (5,):
        raise ValueError("%s: history_row must be (5,), got %s" % (what, tuple(history_row.shape)))
    _same_device(what, workspace=workspace, pose12=pose12, history_row=history_row)
    _lib.check(_lib.load().pnr_icp_solve(_p(workspace), n_pix, min_matches, max_rot, max_trans, 1 if update else 0, _p(pose12),
                                         _p(history_row), _stream()), "pnr_icp_solve")


# PNR_NORMAL_* and PNR_DEPTH_MAX_RADIUS (include/pnr.h "depth front end")
NORMAL_OK, NORMAL_NO_DEPTH, NORMAL_NO_NEIGHBOUR, NORMAL_DEGENERATE, NORMAL_GRAZING = (
    _lib.NORMAL_OK, _lib.NORMAL_NO_DEPTH, _lib.NORMAL_NO_NEIGHBOUR, _lib.NORMAL_DEGENERATE, _lib.NORMAL_GRAZING)
DEPTH_MAX_RADIUS = _lib.DEPTH_MAX_RADIUS


def _pair(what, name, v, meaning):
    try:
        a, b = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be (a, b): %s" % (what, name, meaning)) from None
    return a, b


def depth_filter_params(what, radius, sigma_space, sigma_range, min_support):
    """the scalars of pnr_depth_filter, or the refusal by name (`what`: the caller's name): (radius, g, sigma_a, sigma_b, min_support)
    with g the radius + 1 spatial weights exp(-k^2 / (2 sigma_space^2)), made in float64 and rounded to float32 once"""
    radius, sigma_space, min_support = int(radius), float(sigma_space), int(min_support)
    if not 0 <= radius <= DEPTH_MAX_RADIUS:
        raise ValueError("%s: radius must lie in 0 .. %d (got %d)" % (what, DEPTH_MAX_RADIUS, radius))
    if not (0.0 < sigma_space < _INF):
        raise ValueError("%s: sigma_space must be positive and finite (got %r)" % (what, sigma_space))
    g = [float(torch.tensor(math.exp(-(k * k) / (2.0 * sigma_space * sigma_space)), dtype=torch.float64).to(torch.float32)) for k in range(radius + 1)]
    if not all(v > 0.0 for v in g):
        raise ValueError("%s: sigma_space %r is too small for radius %d (the weight at the window's edge rounds to 0)" % (what, sigma_space, radius))
    sigma_a, sigma_b = _pair(what, "sigma_range", sigma_range, "sigma = a + b * depth")
    if not (0.0 <= sigma_a < _INF and 0.0 <= sigma_b < _INF and (sigma_a > 0.0 or sigma_b > 0.0)):
        raise ValueError("%s: sigma_range must be non-negative and finite, not both 0 (got %r)" % (what, (sigma_a, sigma_b)))
    if min_support < 1:
        raise ValueError("%s: min_support must be >= 1 (got %d)" % (what, min_support))
    return radius, g, sigma_a, sigma_b, min_support


def depth_normals_params(what, jump, min_cos):
    """the scalars of pnr_depth_normals, or the refusal by name: (jump_a, jump_b, mc2) with mc2 = min_cos^2 in float64 (the entry
    point's float argument rounds it once)"""
    jump_a, jump_b = _pair(what, "jump", jump, "a neighbour is used while |difference| <= a + b * depth")
    if not (jump_a >= 0.0 and jump_b >= 0.0):
        raise ValueError("%s: jump must be non-negative (it may be inf; got %r)" % (what, (jump_a, jump_b)))
    min_cos = float(min_cos)
    if not (0.0 <= min_cos <= 1.0):
        raise ValueError("%s: min_cos must lie in [0, 1] (got %r)" % (what, min_cos))
    return jump_a, jump_b, min_cos * min_cos


def _depth_image(what, name, depth):
    """(width, height) of a 2-D depth image of any dtype and device: the shape the other images are held to"""
    _tensor(what, name, depth)
    if depth.dim() != 2:
        raise ValueError("%s: %s must be a (height, width) image, got %s" % (what, name, tuple(depth.shape)))
    return _image_size(what, depth.shape[1], depth.shape[0])


@_on_device
def depth_filter(depth, out, radius=3, sigma_space=1.5, sigma_range=(0.0, 0.03), min_support=1, support=None):
    """Edge-preserving smoothing of a depth image with a speckle rule (pnr_depth_filter; the rule is in include/pnr.h "depth front
    end").  depth: (height, width) float32; out: the same shape, another tensor; support: optional int16 image of the number of
    pixels each result was averaged over.  radius: the window's half width, at most DEPTH_MAX_RADIUS; sigma_space: the spatial
    Gaussian's sigma in pixels; sigma_range = (a, b): a neighbour counts while |difference| < a + b * depth of the centre, weighted by
    a biweight; min_support: a pixel with fewer counted neighbours (itself included) becomes 0.  Invalid pixels (0, negative, NaN,
    Inf) stay 0: holes are not filled.  Returns None."""
    what = "depth_filter"
    width, height = _depth_image(what, "depth", depth)
    _tensor_table(what, (("depth", depth, torch.float32, (height, width)), ("out", out, torch.float32, (height, width))),
                  (("support", support, torch.int16, (height, width)),))
    radius, g, sigma_a, sigma_b, min_support = depth_filter_params(what, radius, sigma_space, sigma_range, min_support)
    _same_device(what, depth=depth, out=out, support=support)
    if depth.data_ptr() == out.data_ptr():
        raise ValueError("%s: out must not be depth itself (a pixel reads its neighbours)" % what)
    g_h = (ctypes.c_float * len(g))(*g)
    _lib.check(_lib.load().pnr_depth_filter(width, height, _p(depth), radius, g_h, sigma_a, sigma_b, min_support, _p(out), _p(support),
                                            _stream()), "pnr_depth_filter")


@_on_device
def depth_normals(camera_model, cam, c2w, width, height, depth, normal, jump=(0.0, 0.05), min_cos=0.1, vertex=None, code=None):
    """World-space vertices and normals of a depth image (pnr_depth_normals; the rule is in include/pnr.h "depth front end").
    camera_model / cam / c2w / width / height as tsdf_raycast takes its camera (c2w: host values); depth: (height, width) float32 in
    render_view's convention.  Outputs, caller-owned: normal (height, width, 3) float32, the unit normal towards the camera, 0 where
    there is none; optional vertex (height, width, 3) float32 and code (height, width) uint8 (NORMAL_OK, NORMAL_NO_DEPTH,
    NORMAL_NO_NEIGHBOUR, NORMAL_DEGENERATE, NORMAL_GRAZING).  jump = (a, b): a neighbour is differenced against while its depth lies
    within a + b * depth; min_cos: normals at a steeper angle to the ray are dropped as GRAZING.  Returns None."""
    what = "depth_normals"
    word, cam_h = _camera_model(what, "camera_model", camera_model, cam)
    c2w_h = _host_floats(c2w, 12, what + ": c2w")
    width, height = _image_size(what, width, height)
    _tensor_table(what, (("depth", depth, torch.float32, (height, width)), ("normal", normal, torch.float32, (height, width, 3))),
                  (("vertex", vertex, torch.float32, (height, width, 3)), ("code", code, torch.uint8, (height, width))))
    jump_a, jump_b, mc2 = depth_normals_params(what, jump, min_cos)
    _same_device(what, depth=depth, normal=normal, vertex=vertex, code=code)
    _lib.check(_lib.load().pnr_depth_normals(word, cam_h, c2w_h, width, height, _p(depth), jump_a, jump_b, mc2, _p(normal), _p(vertex),
                                             _p(code), _stream()), "pnr_depth_normals")


class Draw:
    """One in-kernel random stream of a launch (include/pnr.h "in-kernel RNG", pnr_rng): `call` is the (2,) int64 GPU tensor
    {seed, offset} that rng_begin wrote, `tag` the stream (1 = t_rand, 2 = u, 3 + level = sigma noise), `ray_base` the global
    index of the launch's ray 0, `scale` the standard deviation of normal draws.  The ops that take explicit uniforms / noise
    (stratified, ray_setup, sample_pdf, sample_pdf_labels, composite, composite_backward) accept a Draw in their place and then
    call the _rng twin of their entry point: the draws are made inside the kernel, and equal what rng_fill materialises."""
    __slots__ = ("call", "tag", "ray_base", "scale")

    def __init__(self, call, tag, ray_base=0, scale=1.0):
        self.call, self.tag, self.ray_base, self.scale = call, int(tag), int(ray_base), float(scale)

    def at(self, ray_base):
        """the same stream for a launch whose ray 0 is global ray `ray_base`"""
        return Draw(self.call, self.tag, ray_base, self.scale)

    def desc(self):
        _chk(self.call, "call", torch.int64)
        if self.call.numel() != 2:
            raise ValueError("Draw.call must hold 2 int64 values (seed, offset)")
        return _lib.RngDesc(self.call.data_ptr(), self.ray_base, self.tag, self.scale)


def _draw(x):
    return isinstance(x, Draw)


def _twin(name, tensor, draw, rng_name=None, what=None):
    """The call site of an op that takes a Draw in place of a tensor: the _rng twin of an entry point takes the pnr_rng* in the
    positional slot of the float pointer it replaces.  -> (entry point, that slot's argument, its name for _lib.check)."""
    if draw is not None:
        rng_name = rng_name or name + "_rng"
        return getattr(_lib.load(), rng_name), ctypes.byref(draw.desc()), rng_name
    return getattr(_lib.load(), name), _p(tensor), what or name


@_on_device
def rng_begin(state, call=None):
    """pnr_rng_begin: call = state (seed, offset), then state[1] += 1, on the current stream.  state: (2,) int64 GPU tensor owned
    by the caller (Renderer.rng_state).  Returns call (a fresh (2,) int64 tensor unless one is given)."""
    _chk(state, "state", torch.int64)
    if call is None:
        call = torch.empty(2, device=state.device, dtype=torch.int64)
    _chk(call, "call", torch.int64)
    if state.numel() != 2 or call.numel() != 2:
        raise ValueError("rng_begin: state and call hold 2 int64 values each")
    _lib.check(_lib.load().pnr_rng_begin(_p(state), _p(call), _stream()), "pnr_rng_begin")
    return call


@_on_device
def rng_fill(call, tag, ray_base, n_rays, n, normal=False, std=1.0):
    """The stream `tag` of `call` for global rays ray_base .. ray_base + n_rays - 1 as an (n_rays, n) fp32 tensor: uniforms in
    [0, 1), or std * standard normals (pnr_rng_fill) -- exactly the values the _rng kernels draw in line."""
    d = Draw(call, tag, ray_base, std)
    out = torch.empty((int(n_rays), int(n)), device=call.device, dtype=torch.float32)
    _lib.check(_lib.load().pnr_rng_fill(ctypes.byref(d.desc()), int(n_rays), int(n), int(bool(normal)), _p(out), _stream()),
               "pnr_rng_fill")
    return out


BATCH_OUTPUTS = (("rays", (8,), torch.float32), ("rgb", (3,), torch.float32), ("depth", (), torch.float32), ("sem", (), torch.int32),
                 ("inst", (), torch.int32), ("frame", (), torch.int32), ("pix", (), torch.int32))


@_on_device
def sample_batch(frames, cum, n_frames, draw, n_rays, mode="pooled", want=None, out=None):
    """One ray batch from a device-resident frame table (pnr_sample_batch; include/pnr.h "training frames").  frames: uint8 GPU
    tensor of pnr_frame records (_lib.Frame), cum: (capacity + 1) int64 prefix sums of n_valid, n_frames: (1) int32 -- all read
    when the kernel runs.  draw: the Draw of the PIXEL stream (tag _lib.TAG_PIXEL; the frame stream is _lib.TAG_FRAME).  mode:
    "pooled" (every drawable pixel of the set alike) or "frame" (one frame per call).  Returns {rays (R,8), rgb (R,3), depth (R),
    sem, inst, frame, pix (R) int32}, or the subset `want` names (the others are not computed: NULL outputs); `out`: a dict of
    caller-owned tensors to write into (a captured graph's static batch)."""
    frames, cum, n_frames = _chk(frames, "frames", torch.uint8), _chk(cum, "cum", torch.int64), _chk(n_frames, "n_frames", torch.int32)
    if not _draw(draw):
        raise TypeError("sample_batch: draw must be an ops.Draw")
    if mode not in ("pooled", "frame"):
        raise ValueError("sample_batch: mode must be 'pooled' or 'frame', not %r" % (mode,))
    R, dev = int(n_rays), frames.device
    names = [n for n, _, _ in BATCH_OUTPUTS]
    want = names if want is None else list(want)
    _names("sample_batch", want, names, "unknown output %(key)s (one of %(known)s)")
    res = {n: _own(None if out is None else out.get(n), (R,) + tail, dt, dev, "sample_batch: " + n)
           for n, tail, dt in BATCH_OUTPUTS if n in want}
    _lib.check(_lib.load().pnr_sample_batch(_p(frames), _p(cum), _p(n_frames), _lib.SAMPLE_POOLED if mode == "pooled" else _lib.SAMPLE_FRAME,
                                            ctypes.byref(draw.desc()), R, *[_p(res.get(n)) for n in names], _stream()),
               "pnr_sample_batch")
    return res


def _own(out, shape, dtype, dev, what):
    """`out` (a caller-owned tensor: checked) or a fresh tensor."""
    if out is None:
        return torch.empty(shape, device=dev, dtype=dtype)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous %s tensor of shape %s on %s" % (what, dtype, tuple(shape), dev))
    return out


# The argument checks of the NeRF core ops, in the vocabulary of the geometry ops above (the caller's name `what` first, plain calls in
# the order the refusals come).  Below these ops the kernels index flat, so before an op asks for the stream every tensor it hands over
# has been compared with the sizes passed beside it.  The rule is on ELEMENT COUNT (`_count`: a label as (S,) or (R, N) is the same
# memory); a shape is tested only where a size is read from it (`_level`: z is (R, N); `_rays`: rays is (R, 8); `_hit_lists`).  A
# buffer whose size the library computes may be longer than needed, an arena slice (`_at_least`).  One device per call (`_on`).
def _count(what, name, t, n, why):
    """`t` (None: absent) holds exactly the n elements the kernel will index; `why`: n in the call's own sizes"""
    if t is not None and t.numel() != n:
        raise ValueError("%s: %s holds %d elements, expected %d (%s)" % (what, name, t.numel(), n, why))


def _at_least(what, name, t, n, why):
    if t.numel() < n:
        raise ValueError("%s: %s holds %d elements, needs at least %d (%s)" % (what, name, t.numel(), n, why))


def _rays(what, rays, R=None):
    """R of the GPU tensor rays (R, 8); with the R that another argument gave (see _level), rays hold R * 8 floats"""
    _chk(rays, "rays")
    if R is not None:
        _count(what, "rays", rays, R * 8, "8 floats per ray")
    elif rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError("%s: rays must be (R, 8), got %s" % (what, tuple(rays.shape)))
    return rays.shape[0] if R is None else R


_IMAGE_BYTES = {}       # (bytes(desc), backward) -> pnr_mlp_[bwd_]packed_bytes: the library builds a plan per query, so an image's size is asked once


def _packed(what, desc, packed, name="packed", backward=False):
    """`packed`: GPU bytes, at least the image the library packs for `desc`.  A descriptor the library has no image for is left
    to the entry point, which refuses it in its own words before it reads anything."""
    _chk(packed, name, torch.uint8)
    key = (bytes(desc), backward)
    n = _IMAGE_BYTES.get(key)
    if n is None:
        lib = _lib.load()
        n = int((lib.pnr_mlp_bwd_packed_bytes if backward else lib.pnr_mlp_packed_bytes)(ctypes.byref(desc)))
        if n < 0:
            return
        _IMAGE_BYTES[key] = n
    _at_least(what, name, packed, n, "the image of this descriptor")


def _level(what, rays, z, desc=None, packed=None):
    """(R, N) of a level's samples z (R, N), whose rays hold R * 8 floats and whose `packed` the image of `desc`, all on z's device"""
    _chk(rays, "rays"), _chk(z, "z")
    if z.dim() != 2:
        raise ValueError("%s: z must be (R, N), got %s" % (what, tuple(z.shape)))
    R, N = z.shape
    _count(what, "rays", rays, R * 8, "8 floats per ray")
    if packed is not None:
        _packed(what, desc, packed)
    _on(what, z.device, "z", rays=rays, packed=packed)
    return R, N


def _coarse(what, z, weights, u, draw, n_importance):
    """(R, Nc, device) of sample_pdf's coarse z (R, Nc): weights hold one per sample, u (None: absent) n_importance per ray"""
    _chk(z, "z"), _chk(weights, "weights")
    if z.dim() != 2:
        raise ValueError("%s: z must be (R, Nc), got %s" % (what, tuple(z.shape)))
    R, Nc = z.shape
    _count(what, "weights", weights, R * Nc, "one per coarse sample")
    _count(what, "u", u, R * int(n_importance), "n_importance per ray")
    _on(what, z.device, "z", weights=weights, u=u, call=draw.call if draw else None)
    return R, Nc, z.device


def _draw_or(x, name):
    """(tensor or None, Draw or None) of an argument that is explicit values, a Draw in their place, or None"""
    return (None, x) if _draw(x) else (_chk(x, name), None)


def _labels(what, label_sem, label_inst, n, dev, ref_name="z"):
    """the per-sample labels of a level (None: absent): int32, n = R * N of each, on `dev`"""
    label_sem, label_inst = _chk(label_sem, "label_sem", torch.int32), _chk(label_inst, "label_inst", torch.int32)
    _count(what, "label_sem", label_sem, n, "one per sample")
    _count(what, "label_inst", label_inst, n, "one per sample")
    _on(what, dev, ref_name, label_sem=label_sem, label_inst=label_inst)
    return label_sem, label_inst


def _hit_lists(what, R, hit_t, hit_box, hit_count, dev, ref_name):
    """max_hits of the lists bbox_hits / convex_hits / ray_setup made for R rays: hit_t (R, mh, 2), hit_box (R, mh) (None where the op
    takes none), hit_count (R,), on `dev`"""
    _chk(hit_t, "hit_t"), _chk(hit_box, "hit_box", torch.int32), _chk(hit_count, "hit_count", torch.int32)
    if hit_t.dim() != 3 or hit_t.shape[0] != R or hit_t.shape[2] != 2:
        raise ValueError("%s: hit_t must be (%d, max_hits, 2), got %s" % (what, R, tuple(hit_t.shape)))
    mh = hit_t.shape[1]
    for name, t, shape in (("hit_count", hit_count, (R,)), ("hit_box", hit_box, (R, mh))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError("%s: %s must be %s, got %s" % (what, name, shape, tuple(t.shape)))
    _on(what, dev, ref_name, hit_t=hit_t, hit_box=hit_box, hit_count=hit_count)
    return mh


def _new_hit_lists(what, R, max_hits, dev, out=None):
    """(hit_t, hit_box, hit_count) for R rays: fresh, or the caller-owned `out`"""
    o = out if out is not None else (None, None, None)
    return (_own(o[0], (R, max_hits, 2), torch.float32, dev, what), _own(o[1], (R, max_hits), torch.int32, dev, what),
            _own(o[2], (R,), torch.int32, dev, what))


def _boxes(what, box, dev, box_ids=None):
    """M of box (M, 15); box_ids (None: absent) holds its M (semantic id, instance id) pairs"""
    _chk(box, "box"), _chk(box_ids, "box_ids", torch.int32)
    if box.dim() != 2 or box.shape[1] != 15:
        raise ValueError("%s: box must be (M, 15), got %s" % (what, tuple(box.shape)))
    _count(what, "box_ids", box_ids, 2 * box.shape[0], "a semantic and an instance id per box")
    _on(what, dev, "rays", box=box, box_ids=box_ids)
    return box.shape[0]


@_on_device
def stratified(rays, n_samples, lindisp=False, t_rand=None, out=None):
    """rays (R,8) -> z (R,N).  SURVEY 8a row a3.  t_rand: (R,N) uniforms, a Draw (pnr_stratified_rng) or None."""
    R = _rays("stratified", rays)
    z = _own(out, (R, n_samples), torch.float32, rays.device, "stratified")
    t_rand, draw = _draw_or(t_rand, "t_rand")
    _count("stratified", "t_rand", t_rand, R * n_samples, "one per sample")
    _on("stratified", rays.device, "rays", t_rand=t_rand, call=draw.call if draw else None)
    fn, rand, what = _twin("pnr_stratified", t_rand, draw)
    _lib.check(fn(_p(rays), R, n_samples, int(bool(lindisp)), rand, _p(z), _stream()), what)
    return z


@_on_device
def points(rays, z):
    """rays (R,8), z (R,N) -> the sample positions o + z d, (R,N,3)."""
    R, N = _level("points", rays, z)
    pts = torch.empty((R, N, 3), device=z.device, dtype=torch.float32)
    _lib.check(_lib.load().pnr_points(_p(rays), _p(z), R, N, _p(pts), _stream()), "pnr_points")
    return pts


@_on_device
def embed(x, L):
    """x (n,3) -> (n, 3+6L).  SURVEY 8a row a4."""
    x = _chk(x, "x")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("embed: x must be (n, 3), got %s" % (tuple(x.shape),))
    n = x.shape[0]
    out = torch.empty((n, 3 + 6 * L), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().pnr_embed(_p(x), n, L, _p(out), _stream()), "pnr_embed")
    return out


def default_schedule():
    """pnr_mlp_desc.schedule of new descriptors: 0 (ping-pong inference / lock-step training forward) unless the A/B tools'
    environment variable PNR_MLP_VARIANT asks otherwise (its historical values: 0 = lock-step everywhere -> schedule 1,
    1 = the default -> 0, 2 = ping-pong everywhere -> 2).  Read here, on the Python side: libpnr.so keeps no process-global."""
    return {"0": 1, "1": 0, "2": 2}.get(os.environ.get("PNR_MLP_VARIANT", "1"), 0)


def make_desc(D=8, W=256, skip=4, xyz_L=10, dir_L=4, n_sem=0, n_inst=0, head_W=None, precision="bf16", head_tap="trunk",
              head_depth=2, schedule=None):
    """head_tap: what the semantic / instance heads read -- 'trunk' (the trunk output h) or 'feature' (the feature_linear
    output); head_depth: 2 (W -> head_W -> n) or 1 (one Linear W -> n).  SURVEY.md 9 item 4 as switches.
    schedule: pnr_mlp_desc.schedule (tests / A/B tools: 1 = lock-step kernels everywhere, 2 = ping-pong everywhere)."""
    d = MlpDesc()
    d.D, d.W, d.skip, d.xyz_L, d.dir_L = D, W, skip, xyz_L, dir_L
    d.n_sem, d.n_inst = n_sem, n_inst
    d.head_W = W // 2 if head_W is None else head_W
    d.precision = {"bf16": _lib.PREC_BF16, "fp32": _lib.PREC_FP32}[precision]
    d.head_tap = {"trunk": 0, "feature": 1}[head_tap]
    d.head_depth = {1: 1, 2: 2}[int(head_depth)]
    d.schedule = default_schedule() if schedule is None else int(schedule)
    return d


def _desc_with(desc, **fields):
    """A copy of desc with the given fields replaced."""
    d = MlpDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc), ctypes.sizeof(d))
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _size_or_raise(n, what):
    """A size the library computed (bytes / floats), or its error: a negative value means pnr_last_error has the reason."""
    if n < 0:
        raise RuntimeError(what + ": " + _lib.load().pnr_last_error().decode(errors="replace"))
    return int(n)


def fused_plan(desc, limit=None):
    """desc.plan to use for an image that only mlp_forward_composite will consume (pnr_mlp_fused_plan): 2 where the geometry has
    the two-tile assembly kernel, 1 where it has the fused-inference chunk order of the 8-wave kernel, else 0.  limit (or the
    environment's PNR_FUSED_PLAN, for A/B runs) caps it."""
    best = int(_lib.load().pnr_mlp_fused_plan(ctypes.byref(desc)))
    cap = limit if limit is not None else os.environ.get("PNR_FUSED_PLAN")
    if cap is None or int(cap) >= best:
        return best
    # below the best plan: plan 1 where the library takes it (a semantic head of depth 2: the merged logit chunk), else the classic order
    if int(cap) >= 1:
        if int(_lib.load().pnr_mlp_packed_bytes(ctypes.byref(_desc_with(desc, plan=1)))) > 0:
            return 1
    return 0


def param_in_place(t, device):
    """Can a kernel read parameter `t` where it lies -- float32, contiguous, on `device`?  Otherwise _param_struct hands it a
    temporary float32 copy, and nothing that outlives the call (the descriptors of pack_mlp_device) may point at it."""
    return t.device == torch.device(device) and t.dtype == torch.float32 and t.is_contiguous()


def param_shapes(desc):
    """name -> shape of every parameter of the descriptor's network, under the canonical NeRF names (network.py): what the
    entry points that take a pnr_mlp_params_host read, or write, behind each of its pointers."""
    W, H, ex, ed = desc.W, desc.W // 2, 3 + 6 * desc.xyz_L, 3 + 6 * desc.dir_L
    lin = {"pts_linears.%d" % i: (W, ex if i == 0 else W + ex if i - 1 == desc.skip else W) for i in range(desc.D)}
    lin.update({"alpha_linear": (1, W), "feature_linear": (W, W), "views_linears.0": (H, W + ed), "rgb_linear": (3, H)})
    for head, n in (("semantic_linears", desc.n_sem), ("instance_linears", desc.n_inst)):
        if n:
            lin.update({head + ".0": (H, W), head + ".1": (n, H)} if desc.head_depth == 2 else {head + ".0": (n, W)})
    shapes = {}
    for k, (o, i) in lin.items():
        shapes[k + ".weight"], shapes[k + ".bias"] = (o, i), (o,)
    return shapes


def _param_struct(desc, params, device, what="_param_struct"):
    """pnr_mlp_params_host filled with pointers to `params` (dict name -> tensor) moved/kept on `device`.  Every parameter of
    param_shapes(desc) that is present has that shape; an absent one is a null pointer, other names are ignored.
    Returns (struct, keep-alive list): a parameter that is not param_in_place is pointed to through a temporary copy, and that
    pointer is valid only while the keep-alive list is."""
    for name, shape in param_shapes(desc).items():
        if name in params and tuple(params[name].shape) != shape:
            raise ValueError("%s: parameter %s is %s, the descriptor's network has %s" % (what, name, tuple(params[name].shape), shape))
    keep = []

    def fp(name):
        if name not in params:
            return None
        t = params[name].detach()
        if not param_in_place(t, device):
            t = t.to(device, torch.float32).contiguous()
        keep.append(t)
        return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))

    P = MlpParamsHost()
    D = desc.D
    pw = (ctypes.POINTER(ctypes.c_float) * D)(*[fp(f"pts_linears.{i}.weight") for i in range(D)])
    pb = (ctypes.POINTER(ctypes.c_float) * D)(*[fp(f"pts_linears.{i}.bias") for i in range(D)])
    keep += [pw, pb]
    P.pts_w, P.pts_b = pw, pb
    P.alpha_w, P.alpha_b = fp("alpha_linear.weight"), fp("alpha_linear.bias")
    P.feature_w, P.feature_b = fp("feature_linear.weight"), fp("feature_linear.bias")
    P.views_w, P.views_b = fp("views_linears.0.weight"), fp("views_linears.0.bias")
    P.rgb_w, P.rgb_b = fp("rgb_linear.weight"), fp("rgb_linear.bias")
    last = 0 if desc.head_depth == 1 else 1            # head_depth 1: the head is its single Linear (the struct's *1 slot)
    if desc.n_sem:
        if last:
            P.sem0_w, P.sem0_b = fp("semantic_linears.0.weight"), fp("semantic_linears.0.bias")
        P.sem1_w, P.sem1_b = fp(f"semantic_linears.{last}.weight"), fp(f"semantic_linears.{last}.bias")
    if desc.n_inst:
        if last:
            P.inst0_w, P.inst0_b = fp("instance_linears.0.weight"), fp("instance_linears.0.bias")
        P.inst1_w, P.inst1_b = fp(f"instance_linears.{last}.weight"), fp(f"instance_linears.{last}.bias")
    return P, keep


@_on_device
def pack_mlp_device(desc, params, backward=False, out=None, workspace=None, repack=False):
    """Pack on the GPU straight from the (CUDA, fp32) parameter tensors: pnr_mlp_pack_device.
    Returns (image uint8 CUDA tensor, workspace) -- pass both back in to reuse the buffers.
    repack=True: `out` / `workspace` come from an earlier call with the SAME parameter tensors (same data pointers) whose
    values changed in place: only the packing kernel runs (pnr_mlp_repack_device; no host copies, graph-capture safe).
    The descriptors a full pack leaves in `workspace` hold the addresses the kernel reads.  A parameter that is not float32
    and contiguous (a .double() / .bfloat16() network, a transposed view) is packed from a temporary float32 copy that
    dies with the call, so such parameters take a full pack every time: repack=True with one of them is a ValueError,
    raised before anything is launched.  The full pack synchronises, so a network like that cannot run under stream
    capture."""
    lib = _lib.load()
    dev = next(iter(params.values())).device
    if dev.type != "cuda":
        raise RuntimeError("pack_mlp_device: parameters must be on the GPU")
    if repack:
        for name, t in params.items():
            if not param_in_place(t, dev):
                raise ValueError("pack_mlp_device(repack=True): parameter %r (%s%s) is packed from a temporary copy; a repack needs "
                                 "the float32, contiguous tensors the descriptors point at -- make a full pack (repack=False)"
                                 % (name, t.dtype, "" if t.is_contiguous() else ", not contiguous"))
    nbytes = (lib.pnr_mlp_bwd_packed_bytes if backward else lib.pnr_mlp_packed_bytes)(ctypes.byref(desc))
    if nbytes < 0:
        _lib.check(int(nbytes), "pnr_mlp_packed_bytes")
    wbytes = lib.pnr_mlp_pack_workspace_bytes(ctypes.byref(desc), int(backward))
    if out is None or out.numel() != nbytes:
        out = torch.zeros(int(nbytes), dtype=torch.uint8, device=dev)     # zeros: the table->data alignment gap
    if workspace is None or workspace.numel() < wbytes:
        workspace = torch.empty(int(wbytes), dtype=torch.uint8, device=dev)
    _chk(out, "out", torch.uint8), _chk(workspace, "workspace", torch.uint8)
    _on("pack_mlp_device", dev, "the parameters", out=out, workspace=workspace)
    P, keep = _param_struct(desc, params, dev, "pack_mlp_device")
    fn = lib.pnr_mlp_repack_device if repack else lib.pnr_mlp_pack_device
    _lib.check(fn(ctypes.byref(desc), ctypes.byref(P), int(backward), _p(workspace), _p(out), _stream()), "pnr_mlp_pack_device")
    return out, workspace


def _pack_host(what, desc, params, size, pack):
    """The body of pack_mlp / pack_mlp_bwd: the entry points `size` and `pack`, by name."""
    lib = _lib.load()
    nbytes = getattr(lib, size)(ctypes.byref(desc))
    if nbytes < 0:
        _lib.check(int(nbytes), size)
    P, keep = _param_struct(desc, params, "cpu", what)
    img = torch.empty(int(nbytes), dtype=torch.uint8)
    _lib.check(getattr(lib, pack)(ctypes.byref(desc), ctypes.byref(P), ctypes.c_void_p(img.data_ptr())), pack)
    return img


def pack_mlp(desc, params):
    """params: dict name -> float32 tensor (canonical NeRF names, see network.py).
    Returns the packed image as a CPU uint8 tensor (pure host work, no GPU needed)."""
    return _pack_host("pack_mlp", desc, params, "pnr_mlp_packed_bytes", "pnr_mlp_pack")


def pack_mlp_bwd(desc, params):
    """Transposed-weight image for pnr_mlp_backward (CPU uint8 tensor).  bf16, n_sem/n_inst <= 64."""
    return _pack_host("pack_mlp_bwd", desc, params, "pnr_mlp_bwd_packed_bytes", "pnr_mlp_pack_bwd")


def train_layout(desc, n_samples):
    """(acts_off, dys_off): element offsets (bf16 units) of the saved-activation / dY regions; last = total."""
    a = (ctypes.c_int64 * (desc.D + 7))()
    d = (ctypes.c_int64 * (desc.D + 8))()
    _lib.check(_lib.load().pnr_mlp_train_layout(ctypes.byref(desc), int(n_samples), a, d), "pnr_mlp_train_layout")
    return list(a), list(d)


@_on_device
def mlp_forward_train(desc, packed, rays, z):
    """Forward that also saves activations for the backward.  Returns (raw (ch,S) channel-major, acts bf16)."""
    R, N = _level("mlp_forward_train", rays, z, desc, packed)
    S = R * N
    acts_off, _ = train_layout(desc, S)
    raw = torch.empty((n_channels(desc), S), device=z.device, dtype=torch.float32)
    acts = torch.empty((acts_off[-1],), device=z.device, dtype=torch.bfloat16)
    _lib.check(_lib.load().pnr_mlp_forward_train(ctypes.byref(desc), _p(packed), _p(rays), _p(z), R, N, _p(raw), 1, S,
                                                 _p(acts), _stream()), "pnr_mlp_forward_train")
    return raw, acts


@_on_device
def mlp_backward(desc, packed_bwd, d_raw, acts, n_rays, n_samples):
    """Data-gradient pass: d_raw (ch,S) + saved activations -> dys (bf16, every layer's pre-activation gradient)."""
    d_raw, acts = _chk(d_raw, "d_raw"), _chk(acts, "acts", torch.bfloat16)
    S = int(n_rays) * int(n_samples)
    acts_off, dys_off = train_layout(desc, S)
    _count("mlp_backward", "d_raw", d_raw, n_channels(desc) * S, "(ch, n_rays * n_samples)")
    _packed("mlp_backward", desc, packed_bwd, "packed_bwd", backward=True)
    _at_least("mlp_backward", "acts", acts, acts_off[-1], "train_layout")
    _on("mlp_backward", d_raw.device, "d_raw", packed_bwd=packed_bwd, acts=acts)
    dys = torch.empty((dys_off[-1],), device=d_raw.device, dtype=torch.bfloat16)
    _lib.check(_lib.load().pnr_mlp_backward(ctypes.byref(desc), _p(packed_bwd), _p(d_raw), _p(acts), _p(dys), n_rays,
                                            n_samples, _stream()), "pnr_mlp_backward")
    return dys


@_on_device
def mlp_wgrad(desc, acts, dys, n_samples, shapes):
    """Weight gradients of every Linear from the training forward's `acts` and the data-gradient pass's `dys`
    (pnr_mlp_wgrad: hand-written MFMA kernel + deterministic slab reduction).  shapes: dict name -> shape of the
    parameters (state_dict names): its keys say which gradients to return, its shapes must be param_shapes(desc)'s.
    Returns dict name -> fp32 gradient tensor.  SURVEY 8a row a9."""
    acts, dys = _chk(acts, "acts", torch.bfloat16), _chk(dys, "dys", torch.bfloat16)
    lib = _lib.load()
    dev = acts.device
    acts_off, dys_off = train_layout(desc, n_samples)
    _at_least("mlp_wgrad", "acts", acts, acts_off[-1], "train_layout")
    _at_least("mlp_wgrad", "dys", dys, dys_off[-1], "train_layout")
    _on("mlp_wgrad", dev, "acts", dys=dys)
    table = param_shapes(desc)
    for k, shp in shapes.items():
        if k in table and tuple(shp) != table[k]:
            raise ValueError("mlp_wgrad: shapes[%r] is %s, the descriptor's network has %s" % (k, tuple(shp), table[k]))
    nbytes = _size_or_raise(lib.pnr_mlp_wgrad_workspace_bytes(ctypes.byref(desc), int(n_samples)), "pnr_mlp_wgrad_workspace_bytes")
    # per call, from torch's caching allocator: stream-ordered and graph-pool aware, so a captured step keeps its own
    # block alive and concurrent streams never share scratch (a process-global buffer did neither)
    ws = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
    grads = {k: torch.empty(tuple(shp), device=dev, dtype=torch.float32) for k, shp in shapes.items()}
    G, keep = _param_struct(desc, grads, dev, "mlp_wgrad")
    _lib.check(lib.pnr_mlp_wgrad(ctypes.byref(desc), _p(acts), _p(dys), int(n_samples), ctypes.byref(G), _p(ws), _stream()),
               "pnr_mlp_wgrad")
    return grads


@_on_device
def mlp_forward_train_fp32(desc, params, rays, z):
    """fp32 parity mode of the training forward (pnr_mlp_forward_train_fp32): params = dict name -> fp32 GPU parameter
    tensor (read in place, nothing is packed).  Returns (raw (ch,S) channel-major, acts fp32)."""
    R, N = _level("mlp_forward_train_fp32", rays, z)
    S = R * N
    lib = _lib.load()
    n = _size_or_raise(lib.pnr_mlp_fp32_acts_floats(ctypes.byref(desc), S), "pnr_mlp_fp32_acts_floats")
    raw = torch.empty((n_channels(desc), S), device=z.device, dtype=torch.float32)
    acts = torch.empty((int(n),), device=z.device, dtype=torch.float32)
    P, keep = _param_struct(desc, params, z.device, "mlp_forward_train_fp32")
    _lib.check(lib.pnr_mlp_forward_train_fp32(ctypes.byref(desc), ctypes.byref(P), _p(rays), _p(z), R, N, _p(raw), 1, S, _p(acts),
                                              _stream()), "pnr_mlp_forward_train_fp32")
    return raw, acts


@_on_device
def mlp_backward_fp32(desc, params, d_raw, acts, n_rays, n_samples):
    """fp32 parity mode of the data-gradient + weight-gradient passes (pnr_mlp_backward_fp32).  d_raw (ch,S) channel-major
    fp32.  Returns dict name -> fp32 gradient tensor for every parameter in `params`."""
    d_raw, acts = _chk(d_raw, "d_raw"), _chk(acts, "acts")
    S = int(n_rays) * int(n_samples)
    if tuple(d_raw.shape) != (n_channels(desc), S):
        raise ValueError(f"d_raw: expected {(n_channels(desc), S)}, got {tuple(d_raw.shape)}")
    lib = _lib.load()
    dev = acts.device
    n = _size_or_raise(lib.pnr_mlp_fp32_acts_floats(ctypes.byref(desc), S), "pnr_mlp_fp32_acts_floats")
    _at_least("mlp_backward_fp32", "acts", acts, n, "pnr_mlp_fp32_acts_floats")
    _on("mlp_backward_fp32", dev, "acts", d_raw=d_raw)
    nbytes = _size_or_raise(lib.pnr_mlp_backward_fp32_workspace_bytes(ctypes.byref(desc), S), "pnr_mlp_backward_fp32_workspace_bytes")
    ws = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
    grads = {k: torch.empty_like(v, dtype=torch.float32, memory_format=torch.contiguous_format) for k, v in params.items()}
    P, keep = _param_struct(desc, params, dev, "mlp_backward_fp32")
    G, keep2 = _param_struct(desc, grads, dev, "mlp_backward_fp32")
    _lib.check(lib.pnr_mlp_backward_fp32(ctypes.byref(desc), ctypes.byref(P), _p(d_raw), d_raw.stride(0), _p(acts), int(n_rays),
                                         int(n_samples), ctypes.byref(G), _p(ws), _stream()), "pnr_mlp_backward_fp32")
    return grads


def n_channels(desc):
    return 4 + desc.n_sem + desc.n_inst


RAW_PAD = 64      # floats between the channel rows of a channel-major raw image (see alloc_raw)


def alloc_raw(ch, S, device, pad=RAW_PAD):
    """Channel-major raw image (ch, S) whose channel rows are S + pad floats apart.  With the dense stride the 81
    rows of a ray sit exactly S*4 B apart (48 MiB at the fine level) and the 8 row loads of a compositing batch hit
    the same HBM channel; a 256 B skew per row is worth +3 % compositing bandwidth (tools/stride_probe.py)."""
    buf = torch.empty(ch * (S + pad), device=device, dtype=torch.float32)
    return buf.as_strided((ch, S), (S + pad, 1))


def _chk_raw(raw, ch, S):
    """channel-major raw: (ch, S) fp32 on the GPU, unit sample stride, any channel stride >= S"""
    if not raw.is_cuda or raw.dtype != torch.float32:
        raise TypeError("raw: expected a float32 GPU tensor")
    if tuple(raw.shape) != (ch, S) or raw.stride(1) != 1 or raw.stride(0) < S:
        raise ValueError(f"raw: expected shape {(ch, S)} with unit sample stride, got {tuple(raw.shape)} strides {raw.stride()}")
    return raw.stride(0)


@_on_device
def mlp_forward(desc, packed, rays, z, channel_major=True, out=None):
    """Fused gamma() + NeRF MLP + heads on every sample.  SURVEY 8a rows a4+a5.
    Returns raw as (ch, R*N) when channel_major (fast layout; channel stride padded, see alloc_raw) else (R, N, ch)."""
    R, N = _level("mlp_forward", rays, z, desc, packed)
    ch = n_channels(desc)
    S = R * N
    if channel_major:
        raw = out if out is not None else alloc_raw(ch, S, z.device)
        ss, sc = 1, _chk_raw(raw, ch, S)
    else:
        raw = out if out is not None else torch.empty((R, N, ch), device=z.device, dtype=torch.float32)
        ss, sc = ch, 1
        _count("mlp_forward", "out", _chk(raw, "raw"), S * ch, "(R, N, ch)")
    _on("mlp_forward", z.device, "z", out=raw)
    _lib.check(_lib.load().pnr_mlp_forward(ctypes.byref(desc), _p(packed), _p(rays), _p(z), R, N, _p(raw), ss, sc,
                                           _stream()), "pnr_mlp_forward")
    return raw


@_on_device
def composite(raw, z, rays, n_sem=0, n_inst=0, channel_major=True, noise=None, label_sem=None, label_inst=None,
              sem_mode=0, white_bkgd=False, want_weights=True, out=None):
    """raw2outputs.  SURVEY 8a row a6.  Returns dict of maps (out: optional caller-owned tensors, see _maps).  noise: (R,N) sigma
    noise, a Draw (pnr_composite_rng: noise = draw.scale * the stream's normals, channel-major raw only) or None."""
    noise, draw = _draw_or(noise, "noise")
    R, N = _level("composite", rays, z)
    ch = 4 + n_sem + n_inst
    if channel_major:
        ss, sc = 1, _chk_raw(raw, ch, R * N)
    else:
        _count("composite", "raw", _chk(raw, "raw"), R * N * ch, "(R, N, ch)")
        ss, sc = ch, 1
    dev = z.device
    _count("composite", "noise", noise, R * N, "one per sample")
    label_sem, label_inst = _labels("composite", label_sem, label_inst, R * N, dev)
    _on("composite", dev, "z", raw=raw, noise=noise, call=draw.call if draw else None)
    out = _maps(out, R, N, n_sem, n_inst, label_sem, label_inst, want_weights, dev)
    g = out.get
    fn, nz, what = _twin("pnr_composite", noise, draw)
    _lib.check(fn(_p(raw), ss, sc, _p(z), _p(rays), nz, _p(label_sem), _p(label_inst), R, N, n_sem, n_inst, int(sem_mode),
                  int(bool(white_bkgd)), _p(out["rgb"]), _p(out["depth"]), _p(out["acc"]), _p(g("weights")), _p(g("semantic")),
                  _p(g("instance")), _p(g("fix_semantic")), _p(g("fix_instance")), _stream()), what)
    return out


def _maps(out, R, N, n_sem, n_inst, label_sem, label_inst, want_weights, dev, drop=()):
    """The per-ray output tensors of a compositing call.  `out`: optional dict of caller-owned tensors (e.g. row slices of
    frame-sized maps: Renderer.render hands every chunk its slice, so a frame is never concatenated); anything it lacks is
    allocated.  Caller-owned tensors must be contiguous fp32 of the exact shape on the right device.  drop: keys the call does
    not produce (mlp_forward_weights: rgb, semantic, instance)."""
    f32 = dict(device=dev, dtype=torch.float32)
    shapes = {"rgb": (R, 3), "depth": (R,), "acc": (R,)}
    if want_weights:
        shapes["weights"] = (R, N)
    if n_sem:
        shapes["semantic"] = (R, n_sem)
        if label_sem is not None:
            shapes["fix_semantic"] = (R, n_sem)
    if n_inst:
        shapes["instance"] = (R, n_inst)
        if label_inst is not None:
            shapes["fix_instance"] = (R, n_inst)
    for k in drop:
        shapes.pop(k, None)
    res = {}
    for k, shp in shapes.items():
        t = out.get(k) if out else None
        if t is None:
            t = torch.empty(shp, **f32)
        elif tuple(t.shape) != shp or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError("out[%r] must be a contiguous fp32 tensor of shape %s on %s" % (k, shp, dev))
        res[k] = t
    return res


def fused_supported(desc, n_samples, sem_mode=0, noise=None):
    """Can pnr_mlp_forward_composite take this level?  bf16, no sigma noise, N a multiple of 32; softmax compositing
    (sem_mode 1) where the geometry has a softmax kernel (a head's logit blocks in registers together: plan 2 or 1), on that image:
    net.packed(level, device, fused=fused_image(sem_mode))."""
    ok = (desc.precision == _lib.PREC_BF16 and int(sem_mode) in (0, 1) and noise is None and n_samples % 32 == 0
          and 32 <= n_samples <= 256 and desc.n_sem + desc.n_inst <= 128)
    if ok and int(sem_mode) == 1 and desc.n_sem + desc.n_inst > 0:
        ok = int(_lib.load().pnr_mlp_fused_plan(ctypes.byref(desc_for_mode(desc, 1)))) >= 1     # (flag-aware: a plan with a softmax kernel)
    return ok


def desc_for_mode(desc, sem_mode):
    """desc, or a copy of it, whose PNR_MLP_SOFTMAX flag says sem_mode (what pnr_mlp_forward_composite / _tiles composite)."""
    want = _lib.MLP_SOFTMAX if int(sem_mode) == 1 else 0
    if (desc.flags & _lib.MLP_SOFTMAX) == want:
        return desc
    return _desc_with(desc, flags=(desc.flags & ~_lib.MLP_SOFTMAX) | want)


def fused_image(sem_mode=0):
    """The `fused` argument of PanopticNetwork.packed for a compositing mode: the best plan the geometry has for logits (True), the
    best plan that has a SOFTMAX kernel for softmax ("softmax": plan 2 = k_mlp_tt_sm_* for heads of depth 2, else plan 1)."""
    return "softmax" if int(sem_mode) == 1 else True


@_on_device
def mlp_forward_composite(desc, packed, rays, z, label_sem=None, label_inst=None, white_bkgd=False, want_weights=True, out=None,
                          sem_mode=0, wg_cap=0):
    """Rows a5 + a6 in one pass (inference): the fused MLP reduces every 32-sample tile to one compositing record in its
    epilogue and k_composite_combine finishes the rays -- the raw image (324 B per sample at 45 / 32 heads) is never
    written.  Same dict as composite().  Sums are associated per tile, so results equal mlp_forward + composite to fp32
    rounding (not bit for bit).  sem_mode as in composite(): 1 composites softmax(logits) of each learned field
    (PNR_MLP_SOFTMAX; an image of a plan with a softmax kernel, see fused_supported / fused_image).  wg_cap: plan 2 only, the MLP launch
    on at most that many workgroups (PNR_MLP_WG_CAP) -- a share of the device, for a launch that runs beside another one."""
    image = desc
    desc = desc_for_mode(desc, sem_mode)
    if wg_cap:          # PNR_MLP_WG_CAP: the plan-2 launch on a share of the compute units (Renderer's overlapped levels)
        desc = _desc_with(desc, flags=(desc.flags & 0xFFFF) | ((int(wg_cap) & 0x1FF) << 16))
    return _fused_level("mlp_forward_composite", desc, image, packed, rays, z, label_sem, label_inst, white_bkgd, want_weights, out)


def _fused_level(what, desc, image, packed, rays, z, label_sem, label_inst, white_bkgd, want_weights, out, drop=()):
    """The body of mlp_forward_composite / mlp_forward_weights: pnr_mlp_forward_composite with the maps of `drop` not asked for.
    image: the descriptor `packed` was made for (desc: that one with the call's flags)."""
    R, N = _level(what, rays, z, image, packed)
    dev = z.device
    label_sem, label_inst = _labels(what, label_sem, label_inst, R * N, dev)
    lib = _lib.load()
    nbytes = lib.pnr_mlp_forward_composite_workspace_bytes(ctypes.byref(desc), R, N, int(bool(want_weights)))
    if nbytes < 0:
        raise RuntimeError("pnr_mlp_forward_composite: unsupported geometry (n_samples=%d must be a multiple of 32)" % N)
    ws = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
    out = _maps(out, R, N, desc.n_sem, desc.n_inst, label_sem, label_inst, want_weights, dev, drop=drop)
    g = out.get
    _lib.check(lib.pnr_mlp_forward_composite(ctypes.byref(desc), _p(packed), _p(rays), _p(z), R, N, _p(label_sem), _p(label_inst),
                                             int(bool(white_bkgd)), _p(g("rgb")), _p(out["depth"]), _p(out["acc"]),
                                             _p(g("weights")), _p(g("semantic")), _p(g("instance")), _p(g("fix_semantic")),
                                             _p(g("fix_instance")), _p(ws), _stream()), "pnr_mlp_forward_composite")
    return out


WEIGHTS_ONLY_DROPS = ("rgb", "semantic", "instance")      # the maps a level rendered for its weights alone does not have


def sigma_pass_supported(desc, n_samples, noise=None):
    """Can mlp_forward_weights take this level?  bf16, no sigma noise, N a multiple of 32 in [32, 256], n_sem + n_inst <= 128 (the
    fix_* histograms), and a geometry with a plan-3 image (net.packed(level, device, fused="sigma"))."""
    if not (desc.precision == _lib.PREC_BF16 and noise is None and n_samples % 32 == 0 and 32 <= n_samples <= 256
            and desc.n_sem + desc.n_inst <= 128):
        return False
    return int(_lib.load().pnr_mlp_packed_bytes(ctypes.byref(_desc_with(desc, plan=3)))) > 0


@_on_device
def mlp_forward_weights(desc, packed, rays, z, label_sem=None, label_inst=None, out=None):
    """The compositing weights of a level and nothing else (inference): pnr_mlp_forward_composite on a plan-3 image
    (net.packed(level, device, fused="sigma")), whose kernel runs the trunk and the sigma row alone -- no feature, views, rgb or
    head layers.  Returns {depth, acc, weights[, fix_semantic][, fix_instance]}: bit for bit what mlp_forward_composite returns
    for these keys on any other plan of the same network."""
    if desc.plan != 3:
        raise ValueError("mlp_forward_weights: needs the plan-3 image (net.packed(level, device, fused='sigma')), not plan %d" % desc.plan)
    return _fused_level("mlp_forward_weights", desc, desc, packed, rays, z, label_sem, label_inst, False, True, out, WEIGHTS_ONLY_DROPS)


QUERY_WANTS = ("sigma", "labels", "panoptic", "logits")


def field_query_supported(desc):
    """Does the field-query kernel (pnr_mlp_query, the plan-4 image) exist for this geometry?  bf16, W = 128 or 256."""
    return bool(_lib.load().pnr_mlp_query_supported(ctypes.byref(desc)))


def query_keys(desc, want):
    """The keys mlp_query / Network.query return for `want` on a network of this geometry (ValueError for an unknown name)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [w for w in want if w not in QUERY_WANTS]
    if bad:
        raise ValueError("query: unknown output %r in want (known: %s)" % (bad[0], ", ".join(QUERY_WANTS)))
    keys = []
    if "sigma" in want:
        keys.append("sigma")
    if "labels" in want:
        keys += (["sem_label"] if desc.n_sem else []) + (["inst_label"] if desc.n_inst else [])
    if "panoptic" in want and desc.n_sem:
        keys.append("panoptic")
    if "logits" in want:
        keys += (["sem_logits"] if desc.n_sem else []) + (["inst_logits"] if desc.n_inst else [])
    if not keys:
        raise ValueError("query: want=%r asks for nothing this network has (n_sem=%d, n_inst=%d)" % (want, desc.n_sem, desc.n_inst))
    return keys


@_on_device
def mlp_query(desc, packed, points, want=("sigma", "labels"), is_thing=None, out=None):
    """Density and panoptic labels at 3D points (pnr_mlp_query; inference, no autograd).  desc / packed: the plan-4 image
    (net.packed(level, device, fused="field")).  points (P, 3) fp32.  want: any of "sigma" (raw pre-activation density, (P) fp32),
    "labels" (sem_label / inst_label, (P) int32: argmax of the head, lowest index among equals; inst_label = -1 off the things of
    is_thing, an int32[n_sem] table), "panoptic" ((P) int32: class * 1000 + instance, or the class), "logits" (sem_logits
    (n_sem, P) / inst_logits (n_inst, P) fp32, channel-major, channel stride >= P).  Returns a dict of the keys asked for that the
    network has; only the layers they need are evaluated.  out: dict of caller tensors to write into (any missing key is
    allocated).  sigma and the logits are bit for bit rows 3, 4.. of mlp_forward's raw image at the same positions."""
    if desc.plan != 4:
        raise ValueError("mlp_query: needs the plan-4 image (net.packed(level, device, fused='field')), not plan %d" % desc.plan)
    keys = query_keys(desc, want)
    points = _chk(points, "points")
    is_thing = _chk(is_thing, "is_thing", torch.int32)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("mlp_query: points must be (P, 3), got %s" % (tuple(points.shape),))
    if is_thing is not None and (not desc.n_sem or is_thing.numel() != desc.n_sem):
        raise ValueError("mlp_query: is_thing must hold n_sem=%d entries of a network with a semantic head" % desc.n_sem)
    P, dev = points.shape[0], points.device
    _packed("mlp_query", desc, packed)
    _on("mlp_query", dev, "points", packed=packed, is_thing=is_thing)
    out = dict(out) if out else {}
    res, stride = {}, P
    for k in keys:
        if k.endswith("_logits"):
            n = desc.n_sem if k == "sem_logits" else desc.n_inst
            t = out.get(k)
            if t is None:
                t = alloc_raw(n, P, dev)
            elif (not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (n, P) or (P > 0 and t.stride(1) != 1)
                  or (n > 1 and t.stride(0) < P)):
                raise ValueError("mlp_query: out[%r] must be a float32 GPU tensor of shape %s with unit point stride" % (k, (n, P)))
            res[k] = t
        else:
            res[k] = _own(out.get(k), (P,), torch.float32 if k == "sigma" else torch.int32, dev, "mlp_query: out[%r]" % k)
    lg = [res[k] for k in ("sem_logits", "inst_logits") if k in res]
    _on("mlp_query", dev, "points", **{"out[%r]" % k: res[k] for k in ("sem_logits", "inst_logits") if k in res})
    if lg:
        stride = lg[0].stride(0) if lg[0].shape[0] > 1 else max(P, lg[0].stride(0))
        if any((t.stride(0) if t.shape[0] > 1 else stride) != stride for t in lg):
            raise ValueError("mlp_query: sem_logits and inst_logits must share one channel stride")
    g = res.get
    _lib.check(_lib.load().pnr_mlp_query(ctypes.byref(desc), _p(packed), _p(points), P, _p(g("sigma")), _p(g("sem_label")),
                                         _p(g("inst_label")), _p(g("panoptic")), _p(is_thing), _p(g("sem_logits")),
                                         _p(g("inst_logits")), stride, _stream()), "pnr_mlp_query")
    return res


@_on_device
def composite_backward(raw, z, rays, n_sem, n_inst, grads, noise=None, label_sem=None, label_inst=None,
                       ce_sem=None, ce_inst=None, sem_mode=0):
    """Backward of composite() for channel-major raw.  grads: dict with any of rgb, depth, acc, semantic,
    instance, weights, fix_semantic, fix_instance (upstream gradients, contiguous fp32); the fixed-field
    gradients need the per-sample labels.  ce_sem / ce_inst: 1-element device tensors, the scale of the per-sample
    3D cross-entropy gradient (see ce3d).  sem_mode as in composite().  noise: the forward's tensor, or its Draw (the noise is then
    regenerated in the kernel: pnr_composite_backward_rng).  Returns d_raw (ch, R*N).  SURVEY 8a row a9, 8f-1."""
    raw = _chk(raw, "raw")
    noise, draw = _draw_or(noise, "noise")
    R, N = _level("composite_backward", rays, z)
    dev, ch = z.device, 4 + n_sem + n_inst
    _count("composite_backward", "raw", raw, ch * R * N, "(ch, R * N)")
    _count("composite_backward", "noise", noise, R * N, "one per sample")
    label_sem, label_inst = _labels("composite_backward", label_sem, label_inst, R * N, dev)
    g = {k: _chk(v.contiguous().float(), "g_" + k) for k, v in grads.items() if v is not None}
    per_ray = {"rgb": 3, "depth": 1, "acc": 1, "weights": N, "semantic": n_sem, "fix_semantic": n_sem, "instance": n_inst, "fix_instance": n_inst}
    for k, n in per_ray.items():        # a map of a head the network does not have (n = 0) is not read
        if n:
            _count("composite_backward", "g_" + k, g.get(k), R * n, "a gradient of R rows")
    ce_sem = None if ce_sem is None else _chk(ce_sem.reshape(1).float().contiguous(), "ce_sem")
    ce_inst = None if ce_inst is None else _chk(ce_inst.reshape(1).float().contiguous(), "ce_inst")
    _on("composite_backward", dev, "z", raw=raw, noise=noise, call=draw.call if draw else None, ce_sem=ce_sem, ce_inst=ce_inst,
        **{"g_" + k: v for k, v in g.items() if k in per_ray})
    d_raw = torch.empty_like(raw)
    fn, nz, what = _twin("pnr_composite_backward3", noise, draw, rng_name="pnr_composite_backward_rng", what="pnr_composite_backward")
    _lib.check(fn(_p(raw), R * N, _p(z), _p(rays), nz, R, N, n_sem, n_inst, int(sem_mode), _p(g.get("rgb")), _p(g.get("depth")),
                  _p(g.get("acc")), _p(g.get("semantic")), _p(g.get("instance")), _p(g.get("weights")), _p(label_sem), _p(label_inst),
                  _p(g.get("fix_semantic")), _p(g.get("fix_instance")), _p(ce_sem), _p(ce_inst), _p(d_raw), _stream()), what)
    return d_raw


_LOSS_KEYS = ("rgb", "depth", "semantic", "fix_semantic", "instance", "fix_instance")


@_on_device
def losses(weights, maps, targets, n_sem=0, n_inst=0, depth_l2=False, fix_eps=1e-5, want_grads=True, maps_are_prob=False):
    """The trainer's per-ray loss terms of one level and the gradient of their weighted total w.r.t. every map
    (pnr_losses).  weights: dict over rgb/depth/semantic/fix_semantic/instance/fix_instance;
    maps: dict of (R,·) fp32 GPU tensors (any subset); targets: rgb (R,3), depth (R), semantic (R) int32,
    instance (R) int32.  Returns (losses (8,) device tensor: the six means, total, 0; dict of gradients)."""
    m = {k: _chk(v.detach().contiguous(), k) for k, v in maps.items() if k in _LOSS_KEYS and v is not None and v.numel()}
    if not m:
        raise ValueError("ops.losses: no usable map: `maps` holds none of %s with at least one ray (R = 0?)" % ", ".join(_LOSS_KEYS))
    lib = _lib.load()
    any_map = next(iter(m.values()))
    dev, R = any_map.device, any_map.shape[0]
    t_rgb, t_depth = _chk(targets.get("rgb"), "rgb_gt"), _chk(targets.get("depth"), "depth_gt")
    t_sem = _chk(targets.get("semantic"), "sem_gt", torch.int32)
    t_inst = _chk(targets.get("instance"), "inst_gt", torch.int32)
    cfg = _lib.LossCfg(*(float(weights.get(k, 0.0)) for k in _LOSS_KEYS), int(bool(depth_l2)), float(fix_eps), int(bool(maps_are_prob)))
    use = {"rgb": t_rgb is not None, "depth": t_depth is not None, "semantic": t_sem is not None, "fix_semantic": t_sem is not None,
           "instance": t_inst is not None, "fix_instance": t_inst is not None}
    m = {k: v for k, v in m.items() if use[k]}
    per_ray = {"rgb": 3, "depth": 1, "semantic": int(n_sem), "fix_semantic": int(n_sem), "instance": int(n_inst), "fix_instance": int(n_inst)}
    named = {k: (v, per_ray[k]) for k, v in m.items()}
    named.update(rgb_gt=(t_rgb, 3), depth_gt=(t_depth, 1), sem_gt=(t_sem, 1), inst_gt=(t_inst, 1))
    for name, (t, n) in named.items():
        _count("losses", name, t, R * n, "R rows")
    _on("losses", dev, "the first map", **{name: t for name, (t, n) in named.items()})
    grads = {k: torch.empty_like(v) for k, v in m.items()} if want_grads else {}
    out = torch.empty(8, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.pnr_losses_workspace_bytes(R)), device=dev, dtype=torch.uint8)
    g = grads.get
    _lib.check(lib.pnr_losses(ctypes.byref(cfg), R, int(n_sem), int(n_inst), _p(m.get("rgb")), _p(m.get("depth")),
                              _p(m.get("semantic")), _p(m.get("fix_semantic")), _p(m.get("instance")), _p(m.get("fix_instance")),
                              _p(t_rgb), _p(t_depth), _p(t_sem), _p(t_inst), _p(out), _p(g("rgb")), _p(g("depth")),
                              _p(g("semantic")), _p(g("fix_semantic")), _p(g("instance")), _p(g("fix_instance")), _p(ws),
                              _stream()), "pnr_losses")
    return out, grads


@_on_device
def ce3d(raw, first_channel, n_classes, label):
    """Per-sample 3D cross-entropy of the learned logits raw[first_channel:+n_classes] (channel-major (ch,S)) against
    label (S or (R,N)) int32, -1 = unlabelled.  Returns a 2-element device tensor (mean CE, labelled count)."""
    lib = _lib.load()
    label = _chk(label, "label", torch.int32)
    S = label.numel()
    sc = _chk_raw(raw, raw.shape[0], S)
    if not 0 <= int(first_channel) <= int(first_channel) + int(n_classes) <= raw.shape[0]:
        raise ValueError("ce3d: channels %d .. %d are not all among raw's %d" % (first_channel, first_channel + n_classes - 1, raw.shape[0]))
    _on("ce3d", raw.device, "raw", label=label)
    out = torch.empty(2, device=raw.device, dtype=torch.float32)
    ws = torch.empty(int(lib.pnr_ce3d_workspace_bytes(S)), device=raw.device, dtype=torch.uint8)
    _lib.check(lib.pnr_ce3d(_p(raw), sc, int(first_channel), int(n_classes), _p(label), S, _p(out), _p(ws), _stream()), "pnr_ce3d")
    return out


@_on_device
def sample_pdf(z, weights, n_importance, u=None, want_samples=True, out=None):
    """Coarse z, weights (R,Nc) -> z_fine (R,Nc+Nf) sorted [, z_samples (R,Nf), inds (R,Nf)].
    SURVEY 8a row a7.  u: (R,Nf) uniforms, a Draw (pnr_sample_pdf_rng) or None (deterministic u)."""
    u, draw = _draw_or(u, "u")
    R, Nc, dev = _coarse("sample_pdf", z, weights, u, draw, n_importance)
    z_fine = _own(out, (R, Nc + n_importance), torch.float32, dev, "sample_pdf")
    zs = inds = None
    if want_samples:
        zs = torch.empty((R, n_importance), device=dev, dtype=torch.float32)
        inds = torch.empty((R, n_importance), device=dev, dtype=torch.int32)
    fn, uu, what = _twin("pnr_sample_pdf", u, draw)
    _lib.check(fn(_p(z), _p(weights), uu, R, Nc, n_importance, _p(zs), _p(inds), _p(z_fine), _stream()), what)
    return z_fine, zs, inds


@_on_device
def bbox_hits(rays, box, max_hits=8):
    """rays (R,8), box (M,15) -> hit_t (R,mh,2), hit_box (R,mh) int32, hit_count (R) int32.  Row a8."""
    R, M = _rays("bbox_hits", rays), _boxes("bbox_hits", box, rays.device)
    dev = rays.device
    hit_t, hit_box, hit_count = _new_hit_lists("bbox_hits", R, max_hits, dev)
    _lib.check(_lib.load().pnr_bbox_hits(_p(rays), R, _p(box), M, max_hits, _p(hit_t), _p(hit_box), _p(hit_count),
                                         _stream()), "pnr_bbox_hits")
    return hit_t, hit_box, hit_count


@_on_device
def convex_hits(rays, planes, offsets, max_hits=8, out=None):
    """rays (R,8), planes (P,4) = (n, dd) with inside n.x <= dd, offsets (M+1) int32 CSR -> hit_t (R,mh,2), hit_box (R,mh) int32,
    hit_count (R) int32: bbox_hits' lists for convex polytopes (pnr_convex_hits, row a8b; primitives.ConvexSet makes the table).
    offsets must be non-decreasing with offsets[M] <= P (ConvexSet guarantees it; it lives on the device and is not read here).
    out: (hit_t, hit_box, hit_count) caller-owned."""
    rays, planes, offsets = _chk(rays, "rays"), _chk(planes, "planes"), _chk(offsets, "offsets", torch.int32)
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError("convex_hits: rays must be (R, 8), not %s" % (tuple(rays.shape),))
    if planes.dim() != 2 or planes.shape[1] != 4:
        raise ValueError("convex_hits: planes must be (P, 4), not %s" % (tuple(planes.shape),))
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("convex_hits: offsets must be (M + 1,), not %s" % (tuple(offsets.shape),))
    R, M = rays.shape[0], offsets.numel() - 1
    max_hits = int(max_hits)
    if max_hits < 1:
        raise ValueError("convex_hits: max_hits must be >= 1, not %d" % max_hits)
    dev = rays.device
    if planes.shape[0] == 0 and M > 0:          # primitives without planes (each the whole ray): an empty tensor has no address
        planes = planes.new_zeros((1, 4))
    hit_t, hit_box, hit_count = _new_hit_lists("convex_hits", R, max_hits, dev, out)
    _lib.check(_lib.load().pnr_convex_hits(_p(rays), R, _p(planes), _p(offsets), M, max_hits, _p(hit_t), _p(hit_box), _p(hit_count),
                                           _stream()), "pnr_convex_hits")
    return hit_t, hit_box, hit_count


RAY_SETUP_MAX_HITS = 8      # pnr_ray_setup keeps the hit lists of 256 rays in LDS


@_on_device
def ray_setup(rays, box, box_ids=None, n_samples=64, max_hits=8, lindisp=False, t_rand=None, hull=False, out=None):
    """The coarse level's per-ray preamble in ONE launch (pnr_ray_setup): (hit_t, hit_box, hit_count) as bbox_hits, z (R,N) as
    stratified -- over the hull of the kept intervals with hull=True, as restrict_rays + stratified --, and (label_sem,
    label_inst) as sample_labels when box_ids is given (else None, None).  Bit for bit the separate ops; max_hits <= 8.  t_rand: (R,N)
    uniforms, a Draw (pnr_ray_setup_rng) or None."""
    t_rand, draw = _draw_or(t_rand, "t_rand")
    R, M = _rays("ray_setup", rays), _boxes("ray_setup", box, rays.device, box_ids)
    dev, N = rays.device, int(n_samples)
    _count("ray_setup", "t_rand", t_rand, R * N, "one per sample")
    _on("ray_setup", dev, "rays", t_rand=t_rand, call=draw.call if draw else None)
    hit_t, hit_box, hit_count = _new_hit_lists("ray_setup", R, max_hits, dev)
    z = _own(out, (R, N), torch.float32, dev, "ray_setup")
    ls = li = None
    if box_ids is not None:
        ls = torch.empty((R, N), device=dev, dtype=torch.int32)
        li = torch.empty((R, N), device=dev, dtype=torch.int32)
    fn, rand, what = _twin("pnr_ray_setup", t_rand, draw)
    _lib.check(fn(_p(rays), R, _p(box), M, int(max_hits), _p(box_ids), N, int(bool(lindisp)), rand, int(bool(hull)), _p(hit_t),
                  _p(hit_box), _p(hit_count), _p(z), _p(ls), _p(li), _stream()), what)
    return (hit_t, hit_box, hit_count), z, ls, li


@_on_device
def sample_pdf_labels(z, weights, n_importance, hits, box_ids, u=None, out=None):
    """sample_pdf + sample_labels of its result in ONE launch (pnr_sample_pdf_labels): (z_fine (R,Nc+Nf), label_sem, label_inst).
    hits = (hit_t, hit_box, hit_count) of bbox_hits / ray_setup.  Bit for bit the separate ops.  u: as in sample_pdf."""
    u, draw = _draw_or(u, "u")
    R, Nc, dev = _coarse("sample_pdf_labels", z, weights, u, draw, n_importance)
    hit_t, hit_box, hit_count = hits
    mh = _hit_lists("sample_pdf_labels", R, hit_t, hit_box, hit_count, dev, "z")
    box_ids = _chk(box_ids, "box_ids", torch.int32)
    _on("sample_pdf_labels", dev, "z", box_ids=box_ids)
    Nt = Nc + int(n_importance)
    z_fine = _own(out, (R, Nt), torch.float32, dev, "sample_pdf_labels")
    ls = torch.empty((R, Nt), device=dev, dtype=torch.int32)
    li = torch.empty((R, Nt), device=dev, dtype=torch.int32)
    fn, uu, what = _twin("pnr_sample_pdf_labels", u, draw)
    _lib.check(fn(_p(z), _p(weights), uu, R, Nc, int(n_importance), _p(z_fine), _p(hit_t), _p(hit_box), _p(hit_count), mh,
                  _p(box_ids), _p(ls), _p(li), _stream()), what)
    return z_fine, ls, li


@_on_device
def restrict_rays(rays, hit_t, hit_count):
    """rays with near / far replaced by the hull of each ray's kept bbox intervals (pnr_restrict_rays); no hit: unchanged."""
    R = _rays("restrict_rays", rays)
    mh = _hit_lists("restrict_rays", R, hit_t, None, hit_count, rays.device, "rays")
    out = torch.empty_like(rays)
    _lib.check(_lib.load().pnr_restrict_rays(_p(rays), R, _p(hit_t), _p(hit_count), mh, _p(out), _stream()), "pnr_restrict_rays")
    return out


@_on_device
def sample_labels(z, hit_t, hit_box, hit_count, box_ids):
    """z (R,N) + the hit lists of its rays + box_ids (M,2) -> (label_sem, label_inst), each (R,N) int32: the ids of the first kept
    box whose interval holds the sample, -1 outside every box (pnr_sample_labels).  box_ids is indexed by hit_box's values."""
    z = _chk(z, "z")
    if z.dim() != 2:
        raise ValueError("sample_labels: z must be (R, N), got %s" % (tuple(z.shape),))
    R, N = z.shape
    mh = _hit_lists("sample_labels", R, hit_t, hit_box, hit_count, z.device, "z")
    box_ids = _chk(box_ids, "box_ids", torch.int32)
    _on("sample_labels", z.device, "z", box_ids=box_ids)
    ls = torch.empty((R, N), device=z.device, dtype=torch.int32)
    li = torch.empty((R, N), device=z.device, dtype=torch.int32)
    _lib.check(_lib.load().pnr_sample_labels(_p(z), R, N, _p(hit_t), _p(hit_box), _p(hit_count), mh,
                                             _p(box_ids), _p(ls), _p(li), _stream()), "pnr_sample_labels")
    return ls, li


@_on_device
def panoptic_labels(sem, inst=None, is_thing=None):
    """Composited maps -> (semantic label, instance label, panoptic id), each (R) int32 (pnr_panoptic_labels)."""
    sem, inst = _chk(sem, "sem"), _chk(inst, "inst")
    is_thing = _chk(is_thing, "is_thing", torch.int32)
    if sem.dim() != 2 or (inst is not None and (inst.dim() != 2 or inst.shape[0] != sem.shape[0])):
        raise ValueError("panoptic_labels: sem must be (R, n_sem) and inst (R, n_inst), got %s and %s"
                         % (tuple(sem.shape), None if inst is None else tuple(inst.shape)))
    R, C = sem.shape
    K = inst.shape[1] if inst is not None else 0
    _count("panoptic_labels", "is_thing", is_thing, C, "one per class of sem")
    _on("panoptic_labels", sem.device, "sem", inst=inst, is_thing=is_thing)
    out = [torch.empty(R, device=sem.device, dtype=torch.int32) for _ in range(3)]
    _lib.check(_lib.load().pnr_panoptic_labels(_p(sem), _p(inst), _p(is_thing), R, C, K, _p(out[0]), _p(out[1]), _p(out[2]),
                                               _stream()), "pnr_panoptic_labels")
    return tuple(out)


@_on_device
def confusion(pred, gt, n_classes, conf=None):
    """Accumulate the (n_classes, n_classes) int64 confusion matrix conf[gt, pred] (pnr_confusion).  gt < 0 = ignore."""
    pred, gt = _chk(pred, "pred", torch.int32), _chk(gt, "gt", torch.int32)
    if conf is None:
        conf = torch.zeros((n_classes, n_classes), device=pred.device, dtype=torch.int64)
    _chk(conf, "conf", torch.int64)
    _count("confusion", "gt", gt, pred.numel(), "one per element of pred")
    _count("confusion", "conf", conf, int(n_classes) ** 2, "(n_classes, n_classes)")
    _on("confusion", pred.device, "pred", gt=gt, conf=conf)
    _lib.check(_lib.load().pnr_confusion(_p(pred), _p(gt), pred.numel(), int(n_classes), _p(conf), _stream()), "pnr_confusion")
    return conf
