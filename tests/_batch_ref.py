"""numpy reference of pnr_sample_batch (include/pnr.h "training frames"): the draw rule in Python integers on the Philox words
of tests/_philox.py, rays from the references the camera kernels are pinned against (oracle.torch_oracle.gen_rays for pinhole
frames, _camera_ref.unproject32 for fisheye frames), targets by plain indexing.  tests/test_batch_ref.py pins it (closed-form
draws, frame boundaries, a uniformity test, corrupted variants that fail) before the kernel is measured against it.

A frame is a dict: model ("pinhole" | "fisheye"), width, height, cam (4 or 7 values), c2w (3, 4), near, far, valid_pix (int32
array or None = every pixel), rgb (H, W, 3) uint8, depth (H, W) float32 or None, sem / inst (H, W) int16 or None.
"""
import numpy as np
import torch

import _camera_ref as cr
import _philox as ph
from oracle import torch_oracle as to

TAG_PIXEL, TAG_FRAME = 16, 17
VARIANTS = (None, "mod_low_word", "frame_off_by_one", "pix_is_k")       # the last three are deliberately WRONG


def mulhi64(a, b):
    """floor(a * b / 2^64) on Python integers"""
    return (int(a) * int(b)) >> 64


def words64(seed, offset, tag, ray_base, n_rays):
    """W = w0 * 2^32 + w1 of the block (j = 0, tag, ray_base + r), as a list of Python integers"""
    w = ph.stream_words(seed, offset, tag, ray_base, n_rays, 2)
    return [(int(a) << 32) | int(b) for a, b in w]


def n_valid(fr):
    return fr["width"] * fr["height"] if fr["valid_pix"] is None else len(fr["valid_pix"])


def cum_of(frames):
    return np.concatenate([[0], np.cumsum([n_valid(f) for f in frames])]).astype(np.int64)


def draw_one(W, cum, mode, f_call=None, n_of=None, variant=None):
    """(frame, k) of one ray from its 64-bit word; (-1, 0) where nothing can be drawn."""
    F = len(cum) - 1
    if mode == 0:
        n = int(cum[F]) if F > 0 else 0
        if n == 0:
            return -1, 0
        idx = (W & 0xFFFFFFFF) % n if variant == "mod_low_word" else mulhi64(W, n)
        f = int(np.searchsorted(cum, idx, "right")) - 1
        if variant == "frame_off_by_one":
            f = max(int(np.searchsorted(cum, idx, "left")) - 1, 0)
        return f, idx - int(cum[f])
    n = n_of(f_call) if f_call is not None and f_call >= 0 else 0
    if n == 0:
        return -1, 0
    return f_call, ((W & 0xFFFFFFFF) % n if variant == "mod_low_word" else mulhi64(W, n))


def frame_of_call(seed, offset, F):
    """mode 1: the call's frame, from global ray 0 of the frame stream whatever ray_base is"""
    if F <= 0:
        return -1
    return mulhi64(words64(seed, offset, TAG_FRAME, 0, 1)[0], F)


def draw(frames, seed, offset, n_rays, mode, ray_base=0, variant=None):
    """frame (R) int32, pix (R) int32 of a batch (-1, -1 where nothing can be drawn)"""
    cum = cum_of(frames)
    F = len(frames)
    f_call = frame_of_call(seed, offset, F) if mode == 1 else None
    fo, po = np.full(n_rays, -1, np.int32), np.full(n_rays, -1, np.int32)
    for r, W in enumerate(words64(seed, offset, TAG_PIXEL, ray_base, n_rays)):
        f, k = draw_one(W, cum, mode, f_call, lambda i: n_valid(frames[i]), variant)
        if f < 0:
            continue
        vp = frames[f]["valid_pix"]
        fo[r] = f
        po[r] = k if (vp is None or variant == "pix_is_k") else vp[k]
    return fo, po


def ref_frame(model, cam, width, height, c2w, near, far, rgb, depth=None, sem=None, inst=None, mask=None):
    """A reference frame from host arrays; a fisheye frame's valid_pix is the lens (unproject32's valid) and the user mask."""
    vp = None
    if model == "fisheye":
        ok = cr.unproject32(cam, np.eye(3, 4), width, height, 0.0, 1.0)[1] != 0
        if mask is not None:
            ok &= np.asarray(mask).reshape(-1) != 0
        if not ok.all():
            vp = np.nonzero(ok)[0].astype(np.int32)
    a = lambda t, dt: None if t is None else np.ascontiguousarray(np.asarray(t), dtype=dt)
    return {"model": model, "cam": [float(v) for v in cam], "width": int(width), "height": int(height),
            "c2w": np.asarray(c2w, dtype=np.float32).reshape(3, 4), "near": float(near), "far": float(far), "valid_pix": vp,
            "rgb": a(rgb, np.uint8), "depth": a(depth, np.float32), "sem": a(sem, np.int16), "inst": a(inst, np.int16)}


def rays_of(fr, pix):
    if fr["model"] == "pinhole":
        return to.gen_rays(fr["cam"][:4], fr["c2w"], fr["width"], fr["height"], fr["near"], fr["far"], torch.as_tensor(pix)).numpy()
    return cr.unproject32(fr["cam"], fr["c2w"], fr["width"], fr["height"], fr["near"], fr["far"], pix)[0]


def sample(frames, seed, offset, n_rays, mode, ray_base=0):
    """The whole batch: rays (R,8), rgb (R,3), depth (R) float32, sem, inst, frame, pix (R) int32."""
    fo, po = draw(frames, seed, offset, n_rays, mode, ray_base)
    out = {"rays": np.zeros((n_rays, 8), np.float32), "rgb": np.zeros((n_rays, 3), np.float32), "depth": np.zeros(n_rays, np.float32),
           "sem": np.full(n_rays, -1, np.int32), "inst": np.full(n_rays, -1, np.int32), "frame": fo, "pix": po}
    for f, fr in enumerate(frames):
        rows = np.nonzero(fo == f)[0]
        if not len(rows):
            continue
        p = po[rows].astype(np.int64)
        out["rays"][rows] = rays_of(fr, p)
        out["rgb"][rows] = fr["rgb"].reshape(-1, 3)[p].astype(np.float32) / np.float32(255.0)
        if fr["depth"] is not None:
            out["depth"][rows] = fr["depth"].reshape(-1)[p]
        for key in ("sem", "inst"):
            if fr[key] is not None:
                out[key][rows] = fr[key].reshape(-1)[p].astype(np.int32)
    return out
