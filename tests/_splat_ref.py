"""CPU references of point splatting and the depth metrics (csrc/pnr_splat.hip; the rule is include/pnr.h "point splatting").

(a) splat32: the rule in numpy float32 on _camera_ref.project32 / _pano_ref.project32 (already pinned bit for bit against
    k_project_points) plus p_cam.z, the nearest pixel, the clip and the key as integers, the minimum with np.minimum.at on
    uint64.  k_splat_points must equal it bit for bit, counters included.  `variant`: deliberately WRONG rules
    (test_splat_ref.py: its checks can fail).
(b) resolve: zbuf -> (depth, index).
(c) splat64: per point (not per winner) the pixel, the clip decision and the depth in float64; project_bound: a running
    first-order bound (_warp_ref.E) on |float32 - float64| of u + 0.5, v + 0.5 and e over the PROJECTION chain alone (the
    points are the same float32 numbers in both); near_decision: the points that may legitimately decide differently.
(d) metrics32_64: the counts by the float32 rule, the sums in float64 with math.fsum, and a derived bound on
    |device sums - these sums|.

Views are (model, cam, w2c, width, height) with the model words of include/pnr.h, as in _pano_ref.py.
"""
import math

import numpy as np

import _camera_ref as cr
import _pano_ref as pr
import _warp_ref as wr

PINHOLE, FISHEYE, EQUIRECT = pr.PINHOLE, pr.FISHEYE, pr.EQUIRECT
VARIANTS = ("farthest", "tie_high", "trunc", "range_pinhole")
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
U32, U64 = 2.0 ** -24, 2.0 ** -53
FMAX = pr.FMAX


def key(e, index):
    """the packed key of a float32 depth and a point index, as a Python integer"""
    return (int(np.float32(e).view(np.uint32)) << 32) | (int(index) & 0xFFFFFFFF)


def empty(width, height):
    return np.full(int(width) * int(height), EMPTY, np.uint64)


def points32(view, pts, near=0.0, far=np.inf, variant=None):
    """steps 1-3 per point in float32: landed (P) bool, left (P) bool, iu, iv (P) int64, e (P) float32"""
    m, _, _, w, h = view
    X = np.asarray(pts, np.float32).reshape(-1, 3)
    f = np.float32
    with np.errstate(all="ignore"):
        uv, rng, valid, z = pr._project(f, view, X)
        off = f(0.0) if variant == "trunc" else f(0.5)
        uu, vv = np.where(valid, uv[:, 0], 0).astype(f) + off, np.where(valid, uv[:, 1], 0).astype(f) + off
        iu = np.minimum((np.trunc(uu) if variant == "trunc" else np.floor(uu)).astype(np.int64), w - 1)
        iv = np.minimum((np.trunc(vv) if variant == "trunc" else np.floor(vv)).astype(np.int64), h - 1)
        e = (z if (m == PINHOLE) != (variant == "range_pinhole") else rng).astype(f)
        inrange = (e >= f(near)) & (e <= f(far))
    return valid & inrange, ~valid, iu, iv, e


def splat32(model, cam, w2c, width, height, pts, index_base=0, near=0.0, far=np.inf, radius=0, zbuf=None, variant=None):
    """The rule in float32: (zbuf (height * width) uint64, stats (3) int64).  zbuf given: accumulated into a copy."""
    assert variant is None or variant in VARIANTS
    assert radius in (0, 1, 2) and 0.0 <= near <= far
    view = (model, cam, w2c, int(width), int(height))
    w, h = view[3], view[4]
    landed, left, iu, iv, e = points32(view, pts, near, far, variant)
    P = landed.size
    assert index_base >= 0 and index_base + P <= 2 ** 31 - 1
    idx = (np.arange(P, dtype=np.int64) + index_base).astype(np.uint64)
    bits = e.view(np.uint32).astype(np.uint64)
    if variant == "farthest":
        bits = np.uint64(0xFFFFFFFF) - bits
    low = np.uint64(0xFFFFFFFF) - idx if variant == "tie_high" else idx
    keys = (bits << np.uint64(32)) | low
    out = empty(w, h) if zbuf is None else np.array(zbuf, np.uint64).reshape(-1).copy()
    assert out.size == w * h
    if variant in ("farthest", "tie_high"):          # (the wrong variants are one-shot: no accumulation through their encoding)
        assert zbuf is None
    k = np.flatnonzero(landed)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = iu[k] + dx, iv[k] + dy
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            np.minimum.at(out, (y * w + x)[ok], keys[k][ok])
    if variant == "farthest":
        filled = out != EMPTY
        out[filled] = ((np.uint64(0xFFFFFFFF) - (out[filled] >> np.uint64(32))) << np.uint64(32)) | (out[filled] & np.uint64(0xFFFFFFFF))
    if variant == "tie_high":
        filled = out != EMPTY
        out[filled] = (out[filled] & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - (out[filled] & np.uint64(0xFFFFFFFF)))
    stats = np.array([landed.sum(), left.sum(), (~landed & ~left).sum()], np.int64)
    return out, stats


def resolve(zbuf):
    """(depth float32, index int32) of a z-buffer, in its shape: 0.0 / -1 where the cell is empty"""
    z = np.asarray(zbuf)
    z = z.view(np.uint64) if z.dtype == np.int64 else z.astype(np.uint64)
    filled = z != EMPTY
    depth = np.where(filled, (z >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0.0)).astype(np.float32)
    index = np.where(filled, (z & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), np.int32(-1)).astype(np.int32)
    return depth, index


def splat64(view, pts, near=0.0, far=np.inf):
    """Per point in float64: dict of inside (P) bool (in the domain and the image), uv (P, 2), iu, iv (P) int64, e (P),
    landed (P) bool."""
    m, _, _, w, h = view
    X = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        uv, rng, valid, z = pr._project(np.float64, view, X)
        iu = np.minimum(np.floor(np.where(valid, uv[:, 0], 0) + 0.5).astype(np.int64), w - 1)
        iv = np.minimum(np.floor(np.where(valid, uv[:, 1], 0) + 0.5).astype(np.int64), h - 1)
        e = z if m == PINHOLE else rng
        # the clip compares against the float32 near / far the kernel receives
        landed = valid & (e >= float(np.float32(near))) & (e <= float(np.float32(far)))
    return {"inside": valid, "uv": uv, "iu": iu, "iv": iv, "e": e, "landed": landed}


def project_bound(view, pts):
    """(du, dv, de): bounds on |float32 - float64| of u + 0.5, v + 0.5 (the addition included) and of the depth e of every
    point, over the projection chain alone (_warp_ref.E; the points enter exactly).  inf where the domain decision itself may
    differ, 0 where the point is clearly outside the domain -- as _pano_ref.chain_bound from its step 4 on."""
    E = wr.E
    m, cam, w2c, w, h = view
    X64 = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    X = [E(X64[:, k]) for k in range(3)]
    with np.errstate(all="ignore"):
        Mt = np.asarray(w2c, np.float32).astype(np.float64).reshape(3, 4).tolist()
        pc = [((Mt[k][0] * X[0] + Mt[k][1] * X[1]) + Mt[k][2] * X[2]) + Mt[k][3] for k in range(3)]
        rng = ((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]).sqrt()
        if m == PINHOLE:
            fx, fy, cx, cy = (float(np.float32(v)) for v in cam)
            u, v, e, dom_signs = fx * (pc[0] / pc[2]) + cx, fy * (pc[1] / pc[2]) + cy, pc[2], [pc[2]]
        elif m == FISHEYE:
            xi, k1, k2, g1, g2, u0, v0 = (float(np.float32(x)) for x in cam)
            xs, ys, zs = pc[0] / rng, pc[1] / rng, pc[2] / rng
            den = zs + xi
            x, y = xs / den, ys / den
            r2 = x * x + y * y
            s = (1.0 + k1 * r2) + k2 * (r2 * r2)
            u, v, e, dom_signs = (g1 * x) * s + u0, (g2 * y) * s + v0, rng, [den, xi * zs + 1.0]
        else:
            lon0, dlon, lat0, dlat = (float(np.float32(x)) for x in cam)
            lam = pr._atan2pi_E(pc[0], pc[2])
            hh = (pc[0] * pc[0] + pc[2] * pc[2]).sqrt()
            psi = pr._atan2pi_E(pc[1], hh)
            u = (lam - lon0) / dlon - 0.5
            v = (psi - lat0) / dlat - 0.5
            u = E(u.v, u.e + U32 * (np.abs(u.v) + 2.0 / abs(dlon)))           # the wrap: one more rounding
            e, dom_signs = rng, [rng]
        out = [a.bound() for a in (u + 0.5, v + 0.5, e)]
        edge = np.zeros(X64.shape[0], bool)
        dom = np.ones(X64.shape[0], bool)
        for sgn in dom_signs:
            edge |= ~(sgn.e < wr.GUARD * np.abs(sgn.v))
            dom &= sgn.v > 0
        return tuple(np.where(edge, np.inf, np.where(dom, b, 0.0)) for b in out)


def near_decision(ref64, view, near, far, du, dv, de, inflate=wr.INFLATE):
    """Points where float32 may legitimately decide differently from float64 under the bounds given: u + 0.5 or v + 0.5 of the
    float64 evaluation lies within its bound of an integer (the nearest pixel and the image border are decided there), or e
    lies within its bound of near or far.  Points far outside the image decide nothing at the other integers."""
    _, _, _, w, h = view
    uv, e = ref64["uv"], ref64["e"]
    with np.errstate(all="ignore"):
        out = np.zeros(len(uv), bool)
        for k, dk in ((0, du), (1, dv)):
            a = uv[:, k] + 0.5
            out |= ~(np.abs(a - np.round(a)) > inflate * dk)
        out &= ((uv[:, 0] > -1.0) & (uv[:, 0] < w) & (uv[:, 1] > -1.0) & (uv[:, 1] < h)) | ~np.isfinite(du) | ~np.isfinite(dv)
        for lim in (float(np.float32(near)), float(np.float32(far))):
            if np.isfinite(lim):
                out |= ref64["inside"] & ~(np.abs(e - lim) > inflate * de)
        out |= ~np.isfinite(de)
    return out


# ------------------------------------------------------------------------------------------------ depth metrics
THRESHOLDS = (1.25, 1.5625, 1.953125)
DEVICE_LOG_ULP, NUMPY_LOG_ULP = 2.0, 1.0        # what the bound allows the two logarithms (DESIGN.md "Point splatting")
VARIANT_METRICS = ("le", "missing_in_sums")


def metrics32_64(pred, gt, mask=None, d_range=(1e-3, 80.0), variant=None):
    """(sums (5) float64, counts (5) int64, bound (5) float64).  counts by the float32 rule; sums: each term in float64 in the
    kernel's operation order, added with math.fsum; bound: on |kernel's sums - sums|, derived per term and summed:
      with r = 2^-53 and exact inputs, d = p - g carries r |d|; |d|: r; d d: 3 r; |d| / g: 2 r; d d / g: 4 r (relative);
      a logarithm good to k ulp carries 2 k r |log x| (an ulp is at most 2 r |log x|), so l = log p - log g carries
      dl = 2 k r (|log p| + |log g|) + r |l|, and l l carries 2 |l| dl + dl^2 + r l^2;
    both evaluations commit these (the kernel with k = DEVICE_LOG_ULP, numpy with NUMPY_LOG_ULP), so the per-term bounds of
    the two are added; the kernel's summation adds n r times the sum of the terms (any order of n additions), fsum r times it."""
    assert variant is None or variant in VARIANT_METRICS
    f = np.float32
    p, g = np.asarray(pred, f).reshape(-1), np.asarray(gt, f).reshape(-1)
    assert p.size == g.size
    d_min, d_max = f(d_range[0]), f(d_range[1])
    with np.errstate(all="ignore"):
        use = (np.abs(g) <= FMAX) & (g >= d_min) & (g <= d_max)
        if mask is not None:
            use &= np.asarray(mask).reshape(-1) != 0
        have = (p > 0) & (np.abs(p) <= FMAX)
        ok = use & have
        p32, g32 = p[ok], g[ok]
        ratio = np.maximum(p32 / g32, g32 / p32)
        cmp = (lambda a, b: a <= b) if variant == "le" else (lambda a, b: a < b)
        counts = np.array([ok.sum()] + [cmp(ratio, f(t)).sum() for t in THRESHOLDS] + [(use & ~have).sum()], np.int64)
        if variant == "missing_in_sums":
            ok = use
            p32, g32 = np.where(have, p, f(0.0))[ok], g[ok]
        pd, gd = p32.astype(np.float64), g32.astype(np.float64)
        d = pd - gd
        ad, d2 = np.abs(d), d * d
        lp, lg = np.log(np.maximum(pd, np.finfo(np.float64).tiny)), np.log(gd)
        l = lp - lg
        terms = [ad, d2, ad / gd, d2 / gd, l * l]
        sums = np.array([math.fsum(t.tolist()) for t in terms], np.float64)
        n = int(ok.sum())
        per = []
        for k_ulp in (DEVICE_LOG_ULP, NUMPY_LOG_ULP):
            dl = k_ulp * 2.0 * U64 * (np.abs(lp) + np.abs(lg)) + U64 * np.abs(l)
            per.append([U64 * ad, 3 * U64 * d2, 2 * U64 * terms[2], 4 * U64 * terms[3], 2 * np.abs(l) * dl + dl * dl + U64 * terms[4]])
        bound = np.array([math.fsum((per[0][k] + per[1][k]).tolist()) + (n + 1) * U64 * sums[k] for k in range(5)], np.float64)
    return sums, counts, bound


def metric_terms(pred, gt, mask=None, d_range=(1e-3, 80.0)):
    """((n, 5) float64, (n) bool): every pixel's five terms in the kernel's operation order (zeros where the pixel adds nothing)
    and the pixels that add.  Terms 0 .. 3 are single IEEE + - * / on doubles made from float32 inputs: the kernel's bits.
    Term 4 goes through the logarithm and is the kernel's only to the bound of metrics32_64."""
    f = np.float32
    p, g = np.asarray(pred, f).reshape(-1), np.asarray(gt, f).reshape(-1)
    with np.errstate(all="ignore"):
        ok = (np.abs(g) <= FMAX) & (g >= f(d_range[0])) & (g <= f(d_range[1])) & (p > 0) & (np.abs(p) <= FMAX)
        if mask is not None:
            ok &= np.asarray(mask).reshape(-1) != 0
        pd, gd = np.where(ok, p, f(1.0)).astype(np.float64), np.where(ok, g, f(1.0)).astype(np.float64)
        d = pd - gd
        ad, d2 = np.abs(d), d * d
        l = np.log(pd) - np.log(gd)
        terms = np.stack([ad, d2, ad / gd, d2 / gd, l * l], -1)
    return np.where(ok[:, None], terms, 0.0), ok


def summary(sums, counts):
    """what Evaluator.summarize() reports of the depth accumulators"""
    n = int(counts[0])
    mean = lambda v: float(v) / n if n else math.nan
    return {"depth_n": n, "depth_missing": int(counts[4]), "depth_mae": mean(sums[0]), "depth_rmse": math.sqrt(mean(sums[1])) if n else math.nan,
            "depth_abs_rel": mean(sums[2]), "depth_sq_rel": mean(sums[3]), "depth_rmse_log": math.sqrt(mean(sums[4])) if n else math.nan,
            "depth_d1": mean(counts[1]), "depth_d2": mean(counts[2]), "depth_d3": mean(counts[3])}
