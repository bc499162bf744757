"""CPU references of the camera kernels (csrc/pnr_camera.hip; include/pnr.h "cameras").

(a) unproject32 / project32: numpy float32 restatements in EXACTLY the kernels' operation order (one rounding per
    + - * / sqrt; the library is built with -ffp-contract=off and correctly rounded divide / sqrt, numpy's float32 ufuncs
    round the same way), so the GPU output must equal them bit for bit.
(b) unproject64 / project64: the model in float64, Newton run to convergence.  tests/test_camera_ref.py pins (b) with
    closed-form answers and corrupted variants before anything is measured against it.

Camera words: fisheye cam = (xi, k1, k2, gamma1, gamma2, u0, v0); pinhole cam = (fx, fy, cx, cy).  Pixel (i = column,
j = row), linear index j * width + i.  c2w / w2c: 3x4 row-major [R | t].
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINHOLE, FISHEYE = 0, 1


def _header_constant(name):
    src = open(os.path.join(ROOT, "include", "pnr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


NEWTON_STEPS = _header_constant("PNR_FISHEYE_NEWTON_STEPS")       # the kernel's own constant: one definition for both

# KITTI-360-shaped parameter sets (the dataset's two fisheye cameras are public; rounded: shaped, not copied) and the
# two degenerate ones.  1400 x 1400 each.
KITTI_FISHEYE = (2.2134, 0.016798, 1.6548, 1336.3, 1335.8, 716.94, 705.76)
STRONG_FISHEYE = (2.5535, 0.04981, 4.5397, 1485.4, 1484.9, 687.93, 724.32)      # stronger distortion: k2 2.7 x, xi + 15 %
XI1_FISHEYE = (1.0, 0.0, 0.0, 700.0, 700.0, 699.5, 699.5)                       # xi = 1, no distortion: disc = 1 everywhere
XI0_FISHEYE = (0.0, 0.0, 0.0, 900.0, 905.0, 700.0, 690.0)                       # xi = 0: a normalised pinhole
PARAM_SETS = {"kitti": KITTI_FISHEYE, "strong": STRONG_FISHEYE, "xi1": XI1_FISHEYE, "xi0": XI0_FISHEYE}
FRAME = 1400


def pixel_grid(width, height, pix=None):
    if pix is None:
        pix = np.arange(int(width) * int(height), dtype=np.int64)
    pix = np.asarray(pix, dtype=np.int64)
    j = pix // int(width)
    return pix - j * int(width), j


# ------------------------------------------------------------------------------------------------ float32 restatements
def unproject32(cam, c2w, width, height, near, far, pix=None, steps=None):
    """k_gen_rays_fisheye: rays (R, 8) float32, valid (R,) uint8."""
    f = np.float32
    steps = NEWTON_STEPS if steps is None else steps
    xi, k1, k2, g1, g2, u0, v0 = (f(v) for v in cam)
    M = np.asarray(c2w, dtype=np.float32).reshape(3, 4)
    i, j = pixel_grid(width, height, pix)
    one, three, five = f(1.0), f(3.0), f(5.0)
    with np.errstate(all="ignore"):
        x = (i.astype(np.float32) - u0) / g1
        y = (j.astype(np.float32) - v0) / g2
        rd = np.sqrt(x * x + y * y)
        r = rd.copy()
        for _ in range(steps):
            r2 = r * r
            r4 = r2 * r2
            a = k1 * r2
            b = k2 * r4
            fr = r * ((one + a) + b) - rd
            fp = (one + three * a) + five * b
            r = r - fr / fp
        sc = np.where(rd > f(0.0), r / rd, one).astype(np.float32)
        x = x * sc
        y = y * sc
        r2 = x * x + y * y
        disc = one + (one - xi * xi) * r2
        valid = (disc >= f(0.0)) & (r2 <= np.finfo(np.float32).max)
        lam = (xi + np.sqrt(disc)) / (r2 + one)
        dc = (lam * x, lam * y, lam - xi)
        rays = np.zeros((i.shape[0], 8), dtype=np.float32)
        for k in range(3):
            rays[:, k] = M[k, 3]
            rays[:, 3 + k] = (M[k, 0] * dc[0] + M[k, 1] * dc[1]) + M[k, 2] * dc[2]
    rays[:, 6] = f(near)
    rays[:, 7] = f(far)
    rays[~valid, 3:] = 0.0
    return rays, valid.astype(np.uint8)


def project32(model, cam, w2c, width, height, pts):
    """k_project_points: uv (P, 2) float32, range (P,) float32, valid (P,) uint8."""
    f = np.float32
    M = np.asarray(w2c, dtype=np.float32).reshape(3, 4)
    P = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    one, zero, fmax = f(1.0), f(0.0), np.finfo(np.float32).max
    with np.errstate(all="ignore"):
        p = [((M[k, 0] * P[:, 0] + M[k, 1] * P[:, 1]) + M[k, 2] * P[:, 2]) + M[k, 3] for k in range(3)]
        rng = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
        if model == PINHOLE:
            fx, fy, cx, cy = (f(v) for v in cam)
            dom = p[2] > zero
            x = p[0] / p[2]
            y = p[1] / p[2]
            u = fx * x + cx
            v = fy * y + cy
        else:
            xi, k1, k2, g1, g2, u0, v0 = (f(v) for v in cam)
            xs, ys, zs = p[0] / rng, p[1] / rng, p[2] / rng
            den = zs + xi
            dom = (den > zero) & (xi * zs + one > zero) & (rng <= fmax)
            x = xs / den
            y = ys / den
            r2 = x * x + y * y
            s = (one + k1 * r2) + k2 * (r2 * r2)
            u = (g1 * x) * s + u0
            v = (g2 * y) * s + v0
        fin = (np.abs(u) <= fmax) & (np.abs(v) <= fmax)
        dom = dom & fin
        u = np.where(dom, u, zero).astype(np.float32)
        v = np.where(dom, v, zero).astype(np.float32)
        inside = (u >= f(-0.5)) & (u < f(width) - f(0.5)) & (v >= f(-0.5)) & (v < f(height) - f(0.5))
    return np.stack([u, v], -1), rng.astype(np.float32), (dom & inside).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ float64 reference
def undistort64(cam, rd, max_steps=100):
    """r with r (1 + k1 r^2 + k2 r^4) = rd, Newton from r = rd until no element moves (float64)."""
    _, k1, k2 = (float(v) for v in cam[:3])
    r = rd.copy()
    for _ in range(max_steps):
        r2 = r * r
        step = (r * (1.0 + k1 * r2 + k2 * r2 * r2) - rd) / (1.0 + 3.0 * k1 * r2 + 5.0 * k2 * r2 * r2)
        r = r - step
        if not np.any(np.abs(step) > 1e-16 * np.maximum(np.abs(r), 1.0)):
            break
    return r


def unproject64(cam, width, height, pix=None, c2w=None, variant=None):
    """d (R, 3) float64 (camera space, or world space with c2w), valid (R,) bool, disc (R,) float64.
    variant: None, or one of the deliberately WRONG models "sign" / "distort" / "gamma_swap" that test_camera_ref.py uses
    to show that its checks can fail."""
    xi, k1, k2, g1, g2, u0, v0 = (float(v) for v in cam)
    if variant == "gamma_swap":
        g1, g2 = g2, g1
    i, j = pixel_grid(width, height, pix)
    with np.errstate(all="ignore"):
        x = (i.astype(np.float64) - u0) / g1
        y = (j.astype(np.float64) - v0) / g2
        rd = np.sqrt(x * x + y * y)
        if variant == "distort":
            r = rd * (1.0 + k1 * rd ** 2 + k2 * rd ** 4)
        else:
            r = undistort64(cam, rd)
        sc = np.where(rd > 0.0, r / np.where(rd > 0.0, rd, 1.0), 1.0)
        x, y = x * sc, y * sc
        r2 = x * x + y * y
        disc = 1.0 + (1.0 - xi * xi) * r2
        valid = disc >= 0.0
        lam = (xi + np.sqrt(np.where(valid, disc, 0.0))) / (r2 + 1.0)
        z = (lam + xi) if variant == "sign" else (lam - xi)
        d = np.stack([lam * x, lam * y, z], -1)
    d[~valid] = 0.0
    if c2w is not None:
        d = d @ np.asarray(c2w, dtype=np.float64).reshape(3, 4)[:, :3].T
    return d, valid, disc


def project64(model, cam, w2c, width, height, pts):
    """uv (P, 2), range (P,), valid (P,) bool in float64.  w2c None: pts are camera-space points."""
    P = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    if w2c is not None:
        M = np.asarray(w2c, dtype=np.float64).reshape(3, 4)
        P = P @ M[:, :3].T + M[:, 3]
    rng = np.sqrt((P * P).sum(-1))
    with np.errstate(all="ignore"):
        if model == PINHOLE:
            fx, fy, cx, cy = (float(v) for v in cam)
            dom = P[:, 2] > 0.0
            u = fx * P[:, 0] / P[:, 2] + cx
            v = fy * P[:, 1] / P[:, 2] + cy
        else:
            xi, k1, k2, g1, g2, u0, v0 = (float(v) for v in cam)
            n = P / rng[:, None]
            den = n[:, 2] + xi
            dom = (den > 0.0) & (xi * n[:, 2] + 1.0 > 0.0) & (rng <= np.finfo(np.float32).max)
            x, y = n[:, 0] / den, n[:, 1] / den
            r2 = x * x + y * y
            s = 1.0 + k1 * r2 + k2 * r2 * r2
            u = g1 * x * s + u0
            v = g2 * y * s + v0
    dom = dom & np.isfinite(u) & np.isfinite(v)
    u, v = np.where(dom, u, 0.0), np.where(dom, v, 0.0)
    inside = (u >= -0.5) & (u < width - 0.5) & (v >= -0.5) & (v < height - 0.5)
    return np.stack([u, v], -1), rng, dom & inside


def invert_pose(c2w):
    """w2c (3, 4) float64 of a rigid c2w = [R | t]: [R^T | -R^T t]."""
    M = np.asarray(c2w, dtype=np.float64).reshape(3, 4)
    return np.concatenate([M[:, :3].T, -(M[:, :3].T @ M[:, 3:])], 1)


def pose(yaw, pitch=0.0, origin=(0.0, 0.0, 0.0)):
    """c2w (3, 4) float64: yaw about y, then pitch about x."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    return np.concatenate([Ry @ Rx, np.asarray(origin, dtype=np.float64).reshape(3, 1)], 1)


POSES = {"identity": pose(0.0), "sideways": pose(np.pi / 2, 0.0, (1.0, 1.55, -0.5)), "oblique": pose(-2.2, 0.35, (-12.5, 0.8, 40.25))}

# ------------------------------------------------------------------------------------------------ measured figures
# Taken on the CPU with the functions above on WHOLE 1400 x 1400 frames (tests/test_camera_ref.py re-measures them on a
# pixel subset that holds every near-rim pixel and asserts that none is exceeded); tests/test_gpu_camera.py takes its bounds
# from them with a margin of 2 x, which only guards against a different pixel set: the kernels equal the float32
# restatements bit for bit.
# (1) max |d32 - d64| over a direction component, unproject32 (PNR_FISHEYE_NEWTON_STEPS steps) against unproject64, the
#     largest of the three POSES.  The worst pixels sit at the rim, where sqrt(disc) is near 0.
F32_VS_F64 = {"kitti": 9.04e-5, "strong": 1.35e-4, "xi1": 2.83e-7, "xi0": 1.94e-7}
#     pixels with |disc64| < 1e-4 (validity may flip there under another operation order): share of the frame
NEAR_RIM_SHARE = {"kitti": 259 / 1400 ** 2, "strong": 332 / 1400 ** 2, "xi1": 0.0, "xi0": 0.0}        # 0.013 %, 0.017 %
NEAR_RIM_DISC, NEAR_RIM_CAP = 1e-4, 5e-4
# (2) the all-float32 round trip project32(o + t d) - pixel, in pixels (max over u, v, the frame and the four parameter
#     sets), per pose and t.  The oblique pose stands 42 m from the world origin: at t = 0.5 the float32 rounding of
#     o + t d (ulp(40) = 3.8e-6 m over 0.5 m = 7.6e-6 rad) alone is 1e-2 px at gamma = 1336.
ROUND_TRIP32_PX = {("identity", 0.5): 3.67e-4, ("identity", 7.0): 3.67e-4, ("identity", 90.0): 3.67e-4,
                   ("sideways", 0.5): 4.89e-4, ("sideways", 7.0): 3.67e-4, ("sideways", 90.0): 3.67e-4,
                   ("oblique", 0.5): 1.96e-2, ("oblique", 7.0): 1.47e-3, ("oblique", 90.0): 3.67e-4}
