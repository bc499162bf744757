"""Stereo depth: semi-global matching from a rectified pair to the depth image the loss wrapper's stereo term, `FrameSet.add(...,
depth=)` and `Evaluator.evaluate_depth` consume (ops.census / sgm_aggregate / sgm_select / disparity_depth; the rule is written
out in include/pnr.h "stereo matching").

`sgm(left, right)` matches two rectified 8-bit images on the GPU: census words, the Hamming cost aggregated along 4 or 8
directions, then per pixel the disparity in sixteenths of a pixel with a uniqueness test and a left-right check.  `depth` turns
that into z-depth of a pinhole camera, `depth_from_pair` does both.  All integer up to the one float32 division of the depth,
so the result is the CPU restatement's bit for bit.

Conventions (this build's, unpinned: the reference's matcher is not available): the 9 x 7 census with a replicated border,
constant penalties P1 / P2, the codes -1 (no right pixel) / -2 (not unique) / -3 (left-right check) / -4 (speckle, written by
`despeckle` alone), 0 = no depth.  Out of scope: P2 adapted to image gradients, median filtering, fisheye or panoramic pairs, rectification, gradients through the
matcher, more than 256 disparities."""
import numpy as np
import torch

from . import ops
from .camera import Pinhole

CODES = {-1: "no right pixel", -2: "not unique", -3: "left-right check", -4: "speckle"}
SPECKLE = -4


def to_gray(rgb):
    """(H, W, 3) uint8 -> (H, W) uint8: (77 R + 150 G + 29 B + 128) >> 8 in integer arithmetic (the weights add up to 256)."""
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[-1] != 3:
        raise ValueError("stereo.to_gray: expected an (H, W, 3) uint8 tensor")
    c = rgb.to(torch.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).to(torch.uint8).contiguous()


def _gray(img, name):
    if not isinstance(img, torch.Tensor):
        raise ValueError("stereo.sgm: %s must be a tensor, got %s" % (name, type(img).__name__))
    if img.dtype != torch.uint8:
        raise TypeError("stereo.sgm: %s must be uint8, got %s" % (name, img.dtype))
    if img.dim() == 3 and img.shape[-1] == 3:
        return to_gray(img)
    if img.dim() != 2:
        raise ValueError("stereo.sgm: %s must be (H, W) or (H, W, 3), got %s" % (name, tuple(img.shape)))
    return img.contiguous()


def sgm(left, right, max_disp=128, p1=10, p2=120, paths=8, uniqueness=5, lr_tol=1, keep_volume=False):
    """Match a rectified pair (a point at left column x is at right column x - d, d >= 0).  left, right: (H, W) uint8 GPU
    tensors, or (H, W, 3) uint8 through to_gray.  max_disp: the number of disparities searched, a multiple of 16 in 16 .. 256;
    0 < p1 <= p2 <= 192 the penalties of a disparity step of one / of more; paths 4 or 8; uniqueness 0 .. 99 (per cent by which
    the runner-up outside d* +- 1 must exceed the best); lr_tol the left-right tolerance in pixels, -1 = no check.  Returns a dict:
      d16        (H, W) int16: the disparity in sixteenths of a pixel, or the code -1 / -2 / -3 (CODES);
      disparity  (H, W) float32 pixels, 0 where invalid;     valid (H, W) bool;     code (H, W) int16: 0 where valid, else the code;
      disp_right (H, W) int16: the right image's integer disparity (None with lr_tol = -1);
      S          (H, W, max_disp) int16, the summed path costs, when keep_volume is set."""
    left, right = _gray(left, "left"), _gray(right, "right")
    if left.shape != right.shape:
        raise ValueError("stereo.sgm: left is %s, right %s" % (tuple(left.shape), tuple(right.shape)))
    ops.sgm_aggregate_params("stereo.sgm", max_disp, p1, p2, paths)         # every parameter is refused before anything runs
    ops.sgm_select_params("stereo.sgm", uniqueness, lr_tol)
    cl, cr = ops.census(left), ops.census(right)
    S = ops.sgm_aggregate(cl, cr, max_disp, p1, p2, paths)
    d16, disp_right = ops.sgm_select(S, uniqueness, lr_tol)
    valid = d16 >= 0
    out = {"d16": d16, "disparity": torch.where(valid, d16.to(torch.float32) * 0.0625, torch.zeros((), device=d16.device)),
           "valid": valid, "code": torch.where(valid, torch.zeros_like(d16), d16), "disp_right": disp_right}
    if keep_volume:
        out["S"] = S
    return out


def _speckle_params(what, max_diff, min_size):
    try:
        max_diff = float(max_diff)
    except (TypeError, ValueError):
        raise ValueError("%s: max_diff must be a number >= 0 (got %r)" % (what, max_diff)) from None
    if not (0.0 <= max_diff < float("inf")):
        raise ValueError("%s: max_diff must be finite and >= 0 pixels (got %r)" % (what, max_diff))
    if isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 0:
        raise ValueError("%s: min_size must be an integer >= 0 (got %r)" % (what, min_size))
    return max_diff, min_size


def despeckle(result, max_diff=1.0, min_size=100):
    """The speckle stage: a result of `sgm` with every segment of fewer than min_size pixels invalidated.  A segment is a
    4-connected set of valid pixels, neighbours linked where their disparities differ by at most max_diff pixels (ops.cc_label
    in the values mode on d16 + 1 as float32 with tol = 16 max_diff: exact integers, the + 1 keeps a valid disparity of 0 in
    the foreground and cancels in the difference).  Returns a new dict of the same keys: removed pixels get the code -4 in d16
    and code, disparity 0 and valid False; everything else is the result's.  Never synchronises."""
    what = "stereo.despeckle"
    if not hasattr(result, "keys") or "d16" not in result:
        raise TypeError("%s: result must be the dict stereo.sgm returns" % what)
    max_diff, min_size = _speckle_params(what, max_diff, min_size)
    d16 = result["d16"]
    if not isinstance(d16, torch.Tensor) or d16.dtype != torch.int16 or d16.dim() != 2:
        raise ValueError("%s: result['d16'] must be an (H, W) int16 tensor" % what)
    values = (d16.to(torch.int32) + 1).to(torch.float32)
    _, size, _ = ops.cc_label(values, False, 16.0 * max_diff)
    gone = (size > 0) & (size < min_size)
    out = dict(result)
    out["d16"] = torch.where(gone, torch.full((), SPECKLE, dtype=d16.dtype, device=d16.device), d16)
    valid = out["d16"] >= 0
    out["disparity"] = torch.where(valid, out["d16"].to(torch.float32) * 0.0625, torch.zeros((), device=d16.device))
    out["valid"] = valid
    out["code"] = torch.where(valid, torch.zeros_like(d16), out["d16"])
    return out


def focal_baseline(camera, baseline):
    """fb = fx * baseline as the rule makes it: one float32 multiply on the host"""
    if not isinstance(camera, Pinhole):
        raise TypeError("stereo.depth: camera must be a camera.Pinhole (a rectified pair has pinhole geometry), not %s"
                        % type(camera).__name__)
    baseline = float(baseline)
    if not (0.0 < baseline < float("inf")):
        raise ValueError("stereo.depth: baseline must be positive and finite (got %r)" % baseline)
    fb = float(np.float32(camera.intr[0]) * np.float32(baseline))
    if not (0.0 < fb < float("inf")):
        raise ValueError("stereo.depth: fx * baseline must be positive and finite (fx = %r)" % camera.intr[0])
    return fb


def depth(result_or_d16, camera, baseline, d_range=(1e-3, float("inf"))):
    """z-depth (H, W) float32 of a result of `sgm` (or its d16 image) in the LEFT camera, a Pinhole: fx * baseline / disparity,
    0 where there is no disparity (a code, or disparity 0) or the depth is outside d_range -- FrameSet's "no stereo depth"."""
    fb = focal_baseline(camera, baseline)
    d16 = result_or_d16["d16"] if hasattr(result_or_d16, "keys") else result_or_d16
    if isinstance(d16, torch.Tensor) and d16.dim() == 2 and tuple(d16.shape) != (camera.height, camera.width):
        raise ValueError("stereo.depth: d16 is %s, the camera %s" % (tuple(d16.shape), (camera.height, camera.width)))
    return ops.disparity_depth(d16, fb, d_range)


def depth_from_pair(left, right, camera, baseline, d_range=(1e-3, float("inf")), speckle=None, **sgm_args):
    """`depth(sgm(left, right, **sgm_args), camera, baseline)`: the depth image of the left frame, ready for
    `FrameSet.add(depth=...)` and `Evaluator.evaluate_depth(..., depth_gt)`.  speckle: None, or (max_diff, min_size) of
    `despeckle`, applied to the match before the division."""
    focal_baseline(camera, baseline)            # refuse before matching
    if speckle is not None:
        try:
            max_diff, min_size = speckle
        except (TypeError, ValueError):
            raise ValueError("stereo.depth_from_pair: speckle must be None or (max_diff, min_size)") from None
        _speckle_params("stereo.depth_from_pair", max_diff, min_size)
    result = sgm(left, right, **sgm_args)
    if speckle is not None:
        result = despeckle(result, max_diff, min_size)
    return depth(result, camera, baseline, d_range)
