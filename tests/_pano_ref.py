"""CPU references of the panoramic (equirectangular) camera (include/pnr.h "cameras", model word PNR_CAMERA_EQUIRECT;
csrc/pnr_camera_dev.h).

(a) sincospi32 / atan2pi32 / unproject32 / project32: numpy float32 restatements in EXACTLY the device code's operation order
    (one rounding per + - * / sqrt, Horner's scheme with separate multiply and add; the coefficients are read from the header,
    one definition for both), so the GPU output must equal them bit for bit.
(b) unproject64 / project64: the model in float64 on math / numpy's own sine, cosine and arctangent -- the truth.
    tests/test_pano_ref.py pins (b) with closed forms and corrupted variants (`variant`) before (a) is measured against it.
(c) reproject32 / reproject64: steps 2-8 of the cross-view reprojection rule restated, with a panoramic view in either role and
    _camera_ref / _warp_ref's pieces for the other two models; chain_bound / excluded: _warp_ref.E's running error bound
    carried through the panoramic ray and projection.
(d) frames of a FrameSet with a panoramic camera: the draw of _batch_ref (on _philox) and the rays of (a).

cam = (lon0, dlon, lat0, dlat) in half-turns; pixel (i = column, j = row), linear index j * width + i; c2w / w2c 3x4 [R | t].
Views of (c) are (model, cam, pose, width, height) as in _warp_ref, model EQUIRECT = 3.
"""
import math
import os
import re

import numpy as np

import _batch_ref as br
import _camera_ref as cr
import _warp_ref as wr

ROOT = cr.ROOT
PINHOLE, FISHEYE = cr.PINHOLE, cr.FISHEYE
EQUIRECT = cr._header_constant("PNR_CAMERA_EQUIRECT")
NOTHING, LEFT_VIEW, UNKNOWN, OCCLUDED = wr.NOTHING, wr.LEFT_VIEW, wr.UNKNOWN, wr.OCCLUDED
VARIANTS = ("y_up", "no_half", "no_wrap", "radians")      # deliberately WRONG models (test_pano_ref.py: its checks can fail)
U32 = wr.U32
FMAX = np.finfo(np.float32).max


def _coefficients(prefix):
    src = open(os.path.join(ROOT, "include", "pnr.h")).read()
    found = re.findall(r"#define\s+%s(\d+)\s+(-?0x[0-9a-fA-F.]+p[+-]?\d+)f" % prefix, src)
    assert [int(k) for k, _ in found] == list(range(len(found))) and found, prefix
    vals = [float.fromhex(v) for _, v in found]
    assert all(float(np.float32(v)) == v for v in vals), "%s: a coefficient is not a float32 value" % prefix
    return [np.float32(v) for v in vals]


P, Q, A = _coefficients("PNR_SINPI_P"), _coefficients("PNR_COSPI_Q"), _coefficients("PNR_ATANPI_A")
TAN_PI_8 = np.float32(float.fromhex(re.search(r"#define\s+PNR_TAN_PI_8\s+(0x[0-9a-fA-F.]+p[+-]?\d+)f",
                                              open(os.path.join(ROOT, "include", "pnr.h")).read()).group(1)))


def equirect_cam(width, height, lon=(-180.0, 180.0), lat=(90.0, -90.0)):
    """camera.Equirect's four parameters from degrees: float64, rounded to float32 once"""
    c = (lon[0] / 180.0, (lon[1] - lon[0]) / 180.0 / width, -lat[0] / 180.0, (lat[0] - lat[1]) / 180.0 / height)
    return tuple(float(np.float32(v)) for v in c)


# ------------------------------------------------------------------------------------------------ float32 restatements
def _horner32(c, t):
    p = np.full(t.shape, c[-1], np.float32)
    for k in range(len(c) - 2, -1, -1):
        p = p * t + c[k]
    return p


def sincospi32(x):
    """pnr_sincospi: (sin(pi x), cos(pi x)) float32, x finite"""
    f = np.float32
    x = np.asarray(x, np.float32)
    k = np.rint(f(2.0) * x)                 # ties to even
    r = x - f(0.5) * k
    t = r * r
    s = r * _horner32(P, t)
    c = _horner32(Q, t)
    q = k.astype(np.int64) & 3
    return (np.choose(q, [s, c, -s, -c]).astype(np.float32), np.choose(q, [c, -s, -c, s]).astype(np.float32))


def atan2pi32(y, x):
    """pnr_atan2pi: atan2(y, x) / pi float32"""
    f = np.float32
    y, x = np.broadcast_arrays(np.asarray(y, np.float32), np.asarray(x, np.float32))
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        steep = ay > ax
        mx, mn = np.where(steep, ay, ax), np.where(steep, ax, ay)
        a = mn / mx
        upper = a > TAN_PI_8
        b = np.where(upper, (a - f(1.0)) / (a + f(1.0)), a).astype(np.float32)
        r = np.where(upper, f(0.25), f(0.0)) + b * _horner32(A, b * b)
        r = np.where(mx == f(0.0), f(0.0), r)
        r = np.where(steep, f(0.5) - r, r)
        r = np.where(x < f(0.0), f(1.0) - r, r)
        r = np.where(y < f(0.0), -r, r)
    return r.astype(np.float32)


def unproject32(cam, c2w, width, height, near, far, pix=None):
    """k_gen_rays_equirect: rays (R, 8) float32"""
    f = np.float32
    lon0, dlon, lat0, dlat = (f(v) for v in cam)
    M = np.asarray(c2w, dtype=np.float32).reshape(3, 4)
    i, j = cr.pixel_grid(width, height, pix)
    lam = lon0 + (i.astype(np.float32) + f(0.5)) * dlon
    psi = lat0 + (j.astype(np.float32) + f(0.5)) * dlat
    sl, cl = sincospi32(lam)
    sp, cp = sincospi32(psi)
    dc = (cp * sl, sp, cp * cl)
    rays = np.zeros((i.shape[0], 8), dtype=np.float32)
    for k in range(3):
        rays[:, k] = M[k, 3]
        rays[:, 3 + k] = (M[k, 0] * dc[0] + M[k, 1] * dc[1]) + M[k, 2] * dc[2]
    rays[:, 6] = f(near)
    rays[:, 7] = f(far)
    return rays


def project32(cam, w2c, width, height, pts):
    """k_project_points with model word 3: uv (P, 2) float32, range (P,) float32, valid (P,) uint8"""
    f = np.float32
    lon0, dlon, lat0, dlat = (f(v) for v in cam)
    M = np.asarray(w2c, dtype=np.float32).reshape(3, 4)
    X = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    zero, half = f(0.0), f(0.5)
    umax, vmax = f(width) - half, f(height) - half
    with np.errstate(all="ignore"):
        p = [((M[k, 0] * X[:, 0] + M[k, 1] * X[:, 1]) + M[k, 2] * X[:, 2]) + M[k, 3] for k in range(3)]
        rng = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
        lam = atan2pi32(p[0], p[2])
        h = np.sqrt(p[0] * p[0] + p[2] * p[2])
        psi = atan2pi32(p[1], h)
        dom = (rng > zero) & (rng <= FMAX)
        u = (lam - lon0) / dlon - half
        v = (psi - lat0) / dlat - half
        per = f(2.0) / np.abs(dlon)
        u = np.where(u < -half, u + per, np.where(u >= umax, u - per, u)).astype(np.float32)
        dom = dom & (np.abs(u) <= FMAX) & (np.abs(v) <= FMAX)
        u = np.where(dom, u, zero).astype(np.float32)
        v = np.where(dom, v, zero).astype(np.float32)
        inside = (u >= -half) & (u < umax) & (v >= -half) & (v < vmax)
    return np.stack([u, v], -1), rng.astype(np.float32), (dom & inside).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ float64 reference
def angles64(cam, width, height, pix=None, variant=None, rounded=False):
    """(lam, psi) of the pixel centres in half-turns, float64.  rounded: the float32 angles of unproject32 (so that a
    comparison measures the trigonometry and the rotation, not the rounding of the angle itself)."""
    lon0, dlon, lat0, dlat = (float(np.float32(v)) for v in cam)
    i, j = cr.pixel_grid(width, height, pix)
    if rounded:
        f = np.float32
        lam = f(lon0) + (i.astype(np.float32) + f(0.5)) * f(dlon)
        psi = f(lat0) + (j.astype(np.float32) + f(0.5)) * f(dlat)
        return lam.astype(np.float64), psi.astype(np.float64)
    off = 0.0 if variant == "no_half" else 0.5
    return lon0 + (i + off) * dlon, lat0 + (j + off) * dlat


def unproject64(cam, width, height, pix=None, c2w=None, variant=None, rounded=False):
    """d (R, 3) float64, unit length (camera space, or world space with c2w)"""
    lam, psi = angles64(cam, width, height, pix, variant, rounded)
    k = 1.0 if variant == "radians" else math.pi
    sl, cl, sp, cp = np.sin(k * lam), np.cos(k * lam), np.sin(k * psi), np.cos(k * psi)
    d = np.stack([cp * sl, -sp if variant == "y_up" else sp, cp * cl], -1)
    if c2w is not None:
        d = d @ np.asarray(c2w, dtype=np.float64).reshape(3, 4)[:, :3].T
    return d


def project64(cam, w2c, width, height, pts, variant=None):
    """uv (P, 2), range (P,), valid (P,) bool in float64.  w2c None: pts are camera-space points."""
    lon0, dlon, lat0, dlat = (float(np.float32(v)) for v in cam)
    X = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    if w2c is not None:
        M = np.asarray(w2c, dtype=np.float64).reshape(3, 4)
        X = X @ M[:, :3].T + M[:, 3]
    k = 1.0 if variant == "radians" else math.pi
    with np.errstate(all="ignore"):
        rng = np.sqrt((X * X).sum(-1))
        lam = np.arctan2(X[:, 0], X[:, 2]) / k
        y = -X[:, 1] if variant == "y_up" else X[:, 1]
        psi = np.arctan2(y, np.hypot(X[:, 0], X[:, 2])) / k
        off = 0.0 if variant == "no_half" else 0.5
        u = (lam - lon0) / dlon - off
        v = (psi - lat0) / dlat - off
        if variant != "no_wrap":
            per = 2.0 / abs(dlon)
            u = np.where(u < -0.5, u + per, np.where(u >= width - 0.5, u - per, u))
        dom = (rng > 0) & (rng <= FMAX) & np.isfinite(u) & np.isfinite(v)
    u, v = np.where(dom, u, 0.0), np.where(dom, v, 0.0)
    inside = (u >= -0.5) & (u < width - 0.5) & (v >= -0.5) & (v < height - 0.5)
    return np.stack([u, v], -1), rng, dom & inside


# ------------------------------------------------------------------------------------------------ reprojection, steps 2-8
def _rays(f, view, pc):
    """step 1 of either evaluation: o (3), d (R, 3), ok (R) of the source pixels pc"""
    m, cam, c2w, w, h = view
    R = pc.size
    if f is np.float32:
        if m == PINHOLE:
            o, d = wr.pinhole_rays32(cam, c2w, w, h, pc)
            return o, d, np.ones(R, bool)
        if m == FISHEYE:
            rays, valid = cr.unproject32(cam, c2w, w, h, 0.0, 0.0, pix=pc)
        else:
            rays, valid = unproject32(cam, c2w, w, h, 0.0, 0.0, pix=pc), np.ones(R, np.uint8)
        return np.asarray(c2w, np.float32).reshape(3, 4)[:, 3], rays[:, 3:6], valid != 0
    M = np.asarray(c2w, np.float64).reshape(3, 4)
    if m == PINHOLE:
        fx, fy, cx, cy = (float(v) for v in cam)
        i, j = cr.pixel_grid(w, h, pc)
        return M[:, 3], np.stack([(i - cx) / fx, (j - cy) / fy, np.ones(R)], -1) @ M[:, :3].T, np.ones(R, bool)
    if m == FISHEYE:
        d, ok, _ = cr.unproject64(cam, w, h, pix=pc, c2w=c2w)
        return M[:, 3], d, ok
    return M[:, 3], unproject64(cam, w, h, pix=pc, c2w=c2w), np.ones(R, bool)


def _project(f, view, X):
    m, cam, w2c, w, h = view
    if f is np.float32:
        uv, rng, valid = project32(cam, w2c, w, h, X) if m == EQUIRECT else cr.project32(m, cam, w2c, w, h, X)
        Mt = np.asarray(w2c, np.float32).reshape(3, 4)
        z = ((Mt[2, 0] * X[:, 0] + Mt[2, 1] * X[:, 1]) + Mt[2, 2] * X[:, 2]) + Mt[2, 3]
    else:
        uv, rng, valid = project64(cam, w2c, w, h, X) if m == EQUIRECT else cr.project64(m, cam, w2c, w, h, X)
        Mt = np.asarray(w2c, np.float64).reshape(3, 4)
        z = X @ Mt[2, :3] + Mt[2, 3]
    return uv, rng, valid != 0, z


def _reproject(f, src, depth_src, tgt, depth_tgt, tol, pix, label_src, label_tgt, n_classes):
    ws, hs = src[3], src[4]
    mt, wt, ht = tgt[0], tgt[3], tgt[4]
    depth_src = wr._flat(depth_src, f, ws * hs, "depth_src")
    depth_tgt = wr._flat(depth_tgt, f, wt * ht, "depth_tgt")
    p = np.arange(ws * hs, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64).reshape(-1)
    inside_src = (p >= 0) & (p < ws * hs)
    pc = np.where(inside_src, p, 0)
    with np.errstate(all="ignore"):
        o, d, ok = _rays(f, src, pc)                                                    # 1
        t = depth_src[pc]                                                               # 2
        have = inside_src & ok & (t > 0) & (np.abs(t) <= FMAX)
        t = np.where(have, t, f(1.0)).astype(f)
        X = np.stack([o[k] + t * d[:, k] for k in range(3)], -1).astype(f)              # 3
        uv, rng, valid, z = _project(f, tgt, X)                                         # 4
        half = f(0.5)                                                                   # 5
        iu = np.minimum(np.floor(np.where(valid, uv[:, 0], 0) + half).astype(np.int64), wt - 1)
        iv = np.minimum(np.floor(np.where(valid, uv[:, 1], 0) + half).astype(np.int64), ht - 1)
        q = iv * wt + iu
        code = np.where(valid, q, LEFT_VIEW)
        e = (z if mt == PINHOLE else rng).astype(f)                                     # 6
        dt = thr = None
        if depth_tgt is not None:
            dt = depth_tgt[np.where(valid, q, 0)]
            known = (dt > 0) & (np.abs(dt) <= FMAX)
            thr = f(np.float32(tol[0])) + f(np.float32(tol[1])) * e
            code = np.where(valid & ~known, UNKNOWN, code)
            code = np.where(valid & known & ~(np.abs(e - dt) <= thr), OCCLUDED, code)
        code = np.where(have, code, NOTHING).astype(np.int32)                           # 7
        uv = np.where(have[:, None], uv, 0).astype(f)
    out = {"match": code, "uv": uv, "have": have, "e": e, "dt": dt, "thr": thr, "rng": rng, "z": z,
           "stats": np.array([(code >= 0).sum()] + [(code == c).sum() for c in (-1, -2, -3, -4)], np.int64)}
    if label_src is not None:                                                           # 8
        ls = wr._flat(label_src, np.int64, ws * hs, "label_src")[pc]
        lt = wr._flat(label_tgt, np.int64, wt * ht, "label_tgt")[np.maximum(code, 0)]
        use = (code >= 0) & (ls >= 0) & (ls < n_classes) & (lt >= 0) & (lt < n_classes)
        agree = np.zeros((n_classes, n_classes), np.int64)
        np.add.at(agree, (ls[use], lt[use]), 1)
        out["agree"] = agree
    return out


def reproject32(src, depth_src, tgt, depth_tgt=None, tol=(0.0, 0.02), pix=None, label_src=None, label_tgt=None, n_classes=0):
    """The rule in float32 (k_reproject, bit for bit): dict of match, uv, stats, agree with labels (and e, dt, thr, have)."""
    return _reproject(np.float32, src, depth_src, tgt, depth_tgt, tol, pix, label_src, label_tgt, n_classes)


def reproject64(src, depth_src, tgt, depth_tgt=None, tol=(0.0, 0.02), pix=None, label_src=None, label_tgt=None, n_classes=0):
    return _reproject(np.float64, src, depth_src, tgt, depth_tgt, tol, pix, label_src, label_tgt, n_classes)


# ------------------------------------------------------------------------------------------------ the float32 error of the chain
# _warp_ref.E carries |float32 - float64| through + - * / sqrt.  The panoramic model adds two functions whose float32 versions
# are polynomials, not single roundings; they enter with the absolute bounds below, which tests/test_pano_ref.py asserts as
# conditions on sincospi32 / atan2pi32 against float64 (measured: 1.5 u and 1.1 u, u = 2^-24):
#   sincospi(x):     |sin32 - sin(pi x)| <= pi |cos(pi x)| ex + SINCOS_BOUND      (and likewise the cosine)
#   atan2pi(y, x):   |at32 - atan2(y, x)/pi| <= (|x| ey + |y| ex) / (pi (x^2 + y^2)) + ATAN_BOUND   (first order, as E's rules)
SINCOS_BOUND = 2.0 * U32
ATAN_BOUND = 2.0 * U32
E = wr.E


def _sincospi_E(x):
    s, c = np.sin(math.pi * x.v), np.cos(math.pi * x.v)
    return E(s, math.pi * np.abs(c) * x.e + SINCOS_BOUND), E(c, math.pi * np.abs(s) * x.e + SINCOS_BOUND)


def _atan2pi_E(y, x):
    with np.errstate(all="ignore"):
        r2 = x.v * x.v + y.v * y.v
        e = (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / (math.pi * r2) + ATAN_BOUND
        e = np.where(x.e + y.e >= wr.GUARD * np.sqrt(r2), np.inf, e)
    return E(np.arctan2(y.v, x.v) / math.pi, e)


def ray_chain(view, pix):
    """(o, d (3) E, signs) of the source ray; the panoramic ray restated, _warp_ref.ray_chain for the other models"""
    m, cam, c2w, w, h = view
    if m != EQUIRECT:
        o, d, disc = wr.ray_chain(E, m, cam, c2w, w, h, pix)
        return o, d, ([disc] if disc is not None else [])
    lon0, dlon, lat0, dlat = (float(np.float32(v)) for v in cam)
    M = np.asarray(c2w, np.float64).reshape(3, 4).tolist()
    i, j = cr.pixel_grid(w, h, pix)
    lam = lon0 + E(i + 0.5) * dlon              # (i + 0.5 is exact in float32)
    psi = lat0 + E(j + 0.5) * dlat
    (sl, cl), (sp, cp) = _sincospi_E(lam), _sincospi_E(psi)
    dc = [cp * sl, sp, cp * cl]
    return [M[k][3] for k in range(3)], [(M[k][0] * dc[0] + M[k][1] * dc[1]) + M[k][2] * dc[2] for k in range(3)], []


def chain_bound(src, depth_src, tgt, pix=None):
    """Per source pixel: bounds (du, dv, de) on |float32 - float64| of u + 0.5, v + 0.5 and the expected depth e, as
    _warp_ref.chain_bound with N = E: inf where a decision before them may already differ, 0 where the point is clearly
    outside the projection's domain."""
    ws, hs = src[3], src[4]
    mt, cam_t, w2c, wt, ht = tgt
    pix = np.arange(ws * hs, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64).reshape(-1)
    o, d, signs = ray_chain(src, pix)
    t = np.asarray(depth_src, np.float64).reshape(-1)[pix]
    with np.errstate(all="ignore"):
        t = np.where((t > 0) & np.isfinite(t), t, 1.0)
        X = [o[k] + t * d[k] for k in range(3)]
        Mt = np.asarray(w2c, np.float64).reshape(3, 4).tolist()
        pc = [((Mt[k][0] * X[0] + Mt[k][1] * X[1]) + Mt[k][2] * X[2]) + Mt[k][3] for k in range(3)]
        rng = ((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]).sqrt()
        if mt == PINHOLE:
            fx, fy, cx, cy = (float(v) for v in cam_t)
            u, v, e, dom_signs = fx * (pc[0] / pc[2]) + cx, fy * (pc[1] / pc[2]) + cy, pc[2], [pc[2]]
        elif mt == FISHEYE:
            xi, k1, k2, g1, g2, u0, v0 = (float(x) for x in cam_t)
            xs, ys, zs = pc[0] / rng, pc[1] / rng, pc[2] / rng
            den = zs + xi
            x, y = xs / den, ys / den
            r2 = x * x + y * y
            s = (1.0 + k1 * r2) + k2 * (r2 * r2)
            u, v, e, dom_signs = (g1 * x) * s + u0, (g2 * y) * s + v0, rng, [den, xi * zs + 1.0]
        else:
            lon0, dlon, lat0, dlat = (float(np.float32(x)) for x in cam_t)
            lam = _atan2pi_E(pc[0], pc[2])
            hh = (pc[0] * pc[0] + pc[2] * pc[2]).sqrt()
            psi = _atan2pi_E(pc[1], hh)
            u = (lam - lon0) / dlon - 0.5
            v = (psi - lat0) / dlat - 0.5
            # the wrap adds the period once: one more rounding of a value of at most width
            u = E(u.v, u.e + U32 * (np.abs(u.v) + 2.0 / abs(dlon)))
            e, dom_signs = rng, []
        out = [a.bound() for a in (u + 0.5, v + 0.5, e)]
        edge = np.zeros(pix.shape, bool)
        dom = np.ones(pix.shape, bool)
        for sgn in dom_signs + signs:
            edge |= ~(sgn.e < wr.GUARD * np.abs(sgn.v))
        for sgn in dom_signs:
            dom &= sgn.v > 0
        return tuple(np.where(edge, np.inf, np.where(dom, b, 0.0)) for b in out)


def excluded(ref64, src, depth_src, tgt, tol, pix=None):
    """Pixels where float32 may legitimately decide differently from float64 (_warp_ref.near_decision under chain_bound).  With
    a panoramic target the wrap of u is decided at u = -0.5 and u = width - 0.5, which are rounding boundaries of u + 0.5 (0 and
    width) already."""
    du, dv, de = chain_bound(src, depth_src, tgt, pix)
    return wr.near_decision(ref64, tgt, tol, du, dv, de), du


def sphere_depth(cam, c2w, width, height, centre, radius):
    """(height, width) float32 range image of a panoramic camera INSIDE a sphere (as _warp_ref.sphere_depth)"""
    M = np.asarray(c2w, np.float64).reshape(3, 4)
    d = unproject64(cam, width, height, c2w=c2w)
    oc = M[:, 3] - np.asarray(centre, np.float64)
    b, c = d @ oc, oc @ oc - radius * radius
    assert c < 0, "the camera must stand inside the sphere"
    return (-b + np.sqrt(b * b - c)).astype(np.float32).reshape(height, width)


# ------------------------------------------------------------------------------------------------ frames of a FrameSet
def ref_frame(cam, width, height, c2w, near, far, rgb, depth=None, sem=None, inst=None):
    """_batch_ref.ref_frame for a panoramic camera: every pixel drawable"""
    return br.ref_frame("equirect", cam, width, height, c2w, near, far, rgb, depth, sem, inst)


def rays_of(fr, pix):
    if fr["model"] == "equirect":
        return unproject32(fr["cam"][:4], fr["c2w"], fr["width"], fr["height"], fr["near"], fr["far"], pix)
    return br.rays_of(fr, pix)


def sample(frames, seed, offset, n_rays, mode, ray_base=0):
    """_batch_ref.sample over a set that may hold panoramic frames: the same draw, the rays by model"""
    fo, po = br.draw(frames, seed, offset, n_rays, mode, ray_base)
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
