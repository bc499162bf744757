"""CPU references of pose tracking (csrc/pnr_icp.hip; the rule is include/pnr.h "pose tracking").

(a) accumulate_loops: the per-pixel rule as plain Python loops on numpy.float32 scalars -- the text of the header, step by step.
(b) accumulate32: the same in vectorised numpy float32, in the rule's operation order.  k_icp_accumulate must equal it bit for
    bit (code, residual).  Both take the ray and the projection from the CPU restatements of the three camera models
    (_pano_ref._rays / _project: _warp_ref.pinhole_rays32, _camera_ref.unproject32 / project32, _pano_ref.unproject32 /
    project32), which are pinned bit for bit against the ray and projection kernels.  `variant`: deliberately WRONG rules
    (test_icp_ref.py: its checks can fail).
(c) accumulate64: the same decisions in float64, and `excluded`: the pixels where float32 may legitimately decide differently,
    from a running first-order error bound (_warp_ref.E) carried through this rule's own operations.
(d) the sums: `terms` (the exact per-pixel products, in float64), `rows_device` and `combine` (the kernel's summation order,
    restated once for every ordered sum of the library in _reduce_ref.py: a thread's stride order, the wave's butterfly, the
    four waves, one row per workgroup, the rows in block order).
(e) solve: the Cholesky factorisation, the series and the pose update in Python floats (IEEE double), in the header's order.

A live frame is (model, cam, width, height); a model view is (model, cam, c2w (3, 4), width, height) with depth (height, width)
and normal (height, width, 3) float32 maps; pose12 is the live camera-to-world, 12 float32.
"""
import math

import numpy as np

import _camera_ref as cr
import _pano_ref as pr
import _reduce_ref as rr
import _tsdf_ref as tr
import _warp_ref as wr

PINHOLE, FISHEYE, EQUIRECT = tr.PINHOLE, tr.FISHEYE, tr.EQUIRECT
MATCH, NO_DEPTH, OUTSIDE, NO_MODEL, TOO_FAR, BACK_FACING = 0, 1, 2, 3, 4, 5
CODES = {"MATCH": MATCH, "NO_DEPTH": NO_DEPTH, "OUTSIDE": OUTSIDE, "NO_MODEL": NO_MODEL, "TOO_FAR": TOO_FAR, "BACK_FACING": BACK_FACING}
OK, TOO_FEW, DEGENERATE, STEP_TOO_LARGE = 0, 1, 2, 3
STATUS = {"OK": OK, "TOO_FEW": TOO_FEW, "DEGENERATE": DEGENERATE, "STEP_TOO_LARGE": STEP_TOO_LARGE}
SUMS, ROW, MAX_BLOCKS, SERIES_TERMS, MAX_ROT = 28, 29, 256, 8, 0.5
PIVOT = 2.0 ** -30
# sign: r = n . (p - m);  cross: c = n x qv;  origin: the twist about the world origin (c = p x n) with the update left as
# stated;  gt: BACK_FACING only for facing > 0;  floor: the model looked up at the floor pixel;  right: R' = R R_delta
VARIANTS = ("sign", "cross", "origin", "gt", "floor", "right")
ACC_VARIANTS, SOLVE_VARIANTS = ("sign", "cross", "origin", "gt", "floor"), ("right",)
U32 = 2.0 ** -24
INFLATE = wr.INFLATE
FMAX = np.finfo(np.float32).max
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def _views(live, model, w2c):
    ml, cam_l, wl, hl = live
    mm, cam_m, c2w_m, wm, hm = model
    c2w_m = np.asarray(c2w_m, np.float32).reshape(3, 4)
    w2c = tr.w2c32(c2w_m) if w2c is None else np.asarray(w2c, np.float32).reshape(3, 4)
    return (ml, cam_l, IDENTITY, wl, hl), (mm, cam_m, c2w_m, wm, hm), (mm, cam_m, w2c, wm, hm)


def _empty(R):
    return {"code": np.full(R, NO_DEPTH, np.uint8), "residual": np.zeros(R, np.float32), "J": np.zeros((R, 6), np.float32),
            "mq": np.full(R, -1, np.int64)}


# ------------------------------------------------------------------------------------------------ (a) loops
def accumulate_loops(live, depth_l, pose12, model, depth_m, normal_m, dist_max, w2c=None, variant=None):
    """the rule per pixel on numpy.float32 scalars; dict of code uint8, residual float32, J (R, 6) float32, mq (the model pixel)"""
    assert variant is None or variant in ACC_VARIANTS
    f = np.float32
    lview, mview, pview = _views(live, model, w2c)
    wl, hl, wm, hm = live[2], live[3], model[3], model[4]
    R = wl * hl
    P = np.asarray(pose12, np.float32).reshape(3, 4)
    depth_l = np.asarray(depth_l, np.float32).reshape(-1)
    depth_m = np.asarray(depth_m, np.float32).reshape(-1)
    normal_m = np.asarray(normal_m, np.float32).reshape(-1, 3)
    dist2 = f(dist_max) * f(dist_max)
    out = _empty(R)
    with np.errstate(all="ignore"):
        _, d_all, ok_all = pr._rays(np.float32, lview, np.arange(R, dtype=np.int64))
        for q in range(R):
            t = depth_l[q]
            if not (ok_all[q] and t > f(0) and t <= FMAX):                                    # 1
                continue
            x, y, z = t * d_all[q, 0], t * d_all[q, 1], t * d_all[q, 2]
            qv = [(P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z for k in range(3)]                # 2
            p = [qv[k] + P[k, 3] for k in range(3)]
            uv, _, valid, _ = pr._project(np.float32, pview, np.array([p], np.float32))       # 3
            out["code"][q] = OUTSIDE
            if not valid[0]:
                continue
            off = f(0.0) if variant == "floor" else f(0.5)
            a = min(int(np.floor(uv[0, 0] + off)), wm - 1)
            b = min(int(np.floor(uv[0, 1] + off)), hm - 1)
            a, b = max(a, 0), max(b, 0)                                                        # (the floor variant at u in [-0.5, 0))
            mq = b * wm + a
            out["mq"][q] = mq
            dm, n = depth_m[mq], normal_m[mq]                                                  # 4
            out["code"][q] = NO_MODEL
            if not (dm > f(0) and dm <= FMAX and np.all(np.abs(n) <= FMAX) and np.any(n != f(0))):
                continue
            o, dmr, okm = pr._rays(np.float32, mview, np.array([mq], np.int64))                # 5
            if not okm[0]:
                continue
            m = [f(o[k]) + dm * f(dmr[0, k]) for k in range(3)]
            e = [m[k] - p[k] for k in range(3)]
            out["code"][q] = TOO_FAR
            if not ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= dist2):
                continue
            facing = (n[0] * qv[0] + n[1] * qv[1]) + n[2] * qv[2]                              # 6
            out["code"][q] = BACK_FACING
            if (facing > f(0)) if variant == "gt" else (facing >= f(0)):
                continue
            out["code"][q] = MATCH                                                             # 7
            if variant == "sign":
                e = [-v for v in e]
            out["residual"][q] = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
            arm = p if variant == "origin" else qv
            c = [arm[1] * n[2] - arm[2] * n[1], arm[2] * n[0] - arm[0] * n[2], arm[0] * n[1] - arm[1] * n[0]]
            if variant == "cross":
                c = [n[1] * arm[2] - n[2] * arm[1], n[2] * arm[0] - n[0] * arm[2], n[0] * arm[1] - n[1] * arm[0]]
            out["J"][q] = c + [n[0], n[1], n[2]]
    return out


# ------------------------------------------------------------------------------------------------ (b), (c) vectorised
def _accumulate(f, live, depth_l, pose12, model, depth_m, normal_m, dist_max, w2c, variant):
    assert variant is None or variant in ACC_VARIANTS
    lview, mview, pview = _views(live, model, w2c)
    wl, hl, wm, hm = live[2], live[3], model[3], model[4]
    R = wl * hl
    P = np.asarray(pose12, np.float32).reshape(3, 4).astype(f)
    depth_l = np.asarray(depth_l, np.float32).reshape(-1).astype(f)
    depth_m = np.asarray(depth_m, np.float32).reshape(-1).astype(f)
    normal_m = np.asarray(normal_m, np.float32).reshape(-1, 3).astype(f)
    dist2 = f(np.float32(dist_max)) * f(np.float32(dist_max))
    with np.errstate(all="ignore"):
        _, d, ok = pr._rays(f, lview, np.arange(R, dtype=np.int64))                            # 1
        d = np.asarray(d, f)
        have = np.asarray(ok, bool) & (depth_l > 0) & (np.abs(depth_l) <= FMAX)
        t = np.where(have, depth_l, f(1.0)).astype(f)
        x, y, z = t * d[:, 0], t * d[:, 1], t * d[:, 2]
        qv = [((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z).astype(f) for k in range(3)]        # 2
        p = [(qv[k] + P[k, 3]).astype(f) for k in range(3)]
        uv, _, valid, _ = pr._project(f, pview, np.stack(p, -1).astype(f))                     # 3
        inside = have & valid
        off = f(0.0) if variant == "floor" else f(0.5)
        a = np.clip(np.floor(np.where(inside, uv[:, 0], 0) + off).astype(np.int64), 0, wm - 1)
        b = np.clip(np.floor(np.where(inside, uv[:, 1], 0) + off).astype(np.int64), 0, hm - 1)
        mq = b * wm + a
        dm, n = depth_m[mq], normal_m[mq]                                                      # 4
        om, dmr, okm = pr._rays(f, mview, mq)                                                  # 5
        dmr = np.asarray(dmr, f)
        known = inside & (dm > 0) & (np.abs(dm) <= FMAX) & np.all(np.abs(n) <= FMAX, -1) & np.any(n != 0, -1) & np.asarray(okm, bool)
        m = [(f(om[k]) + dm * dmr[:, k]).astype(f) for k in range(3)]
        e = [(m[k] - p[k]).astype(f) for k in range(3)]
        e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        near = known & (e2 <= dist2)
        facing = (n[:, 0] * qv[0] + n[:, 1] * qv[1]) + n[:, 2] * qv[2]                         # 6
        back = (facing > 0) if variant == "gt" else (facing >= 0)
        match = near & ~back
        if variant == "sign":                                                                  # 7
            e = [-v for v in e]
        r = (n[:, 0] * e[0] + n[:, 1] * e[1]) + n[:, 2] * e[2]
        arm = p if variant == "origin" else qv
        c = [arm[1] * n[:, 2] - arm[2] * n[:, 1], arm[2] * n[:, 0] - arm[0] * n[:, 2], arm[0] * n[:, 1] - arm[1] * n[:, 0]]
        if variant == "cross":
            c = [n[:, 1] * arm[2] - n[:, 2] * arm[1], n[:, 2] * arm[0] - n[:, 0] * arm[2], n[:, 0] * arm[1] - n[:, 1] * arm[0]]
        J = np.stack(c + [n[:, 0], n[:, 1], n[:, 2]], -1)
    code = np.full(R, NO_DEPTH, np.uint8)
    code[have] = OUTSIDE
    code[inside] = NO_MODEL
    code[known] = TOO_FAR
    code[near] = BACK_FACING
    code[match] = MATCH
    return {"code": code, "residual": np.where(match, r, 0).astype(f), "J": np.where(match[:, None], J, 0).astype(f),
            "mq": np.where(inside, mq, -1), "have": have, "inside": inside, "known": known, "uv": uv, "e2": e2, "facing": facing,
            "p": np.stack(p, -1), "m": np.stack(m, -1), "n": n, "qv": np.stack(qv, -1), "dist2": dist2}


def accumulate32(live, depth_l, pose12, model, depth_m, normal_m, dist_max, w2c=None, variant=None):
    """the rule in vectorised float32 (k_icp_accumulate, bit for bit): code, residual, J, mq and the intermediates"""
    return _accumulate(np.float32, live, depth_l, pose12, model, depth_m, normal_m, dist_max, w2c, variant)


def accumulate64(live, depth_l, pose12, model, depth_m, normal_m, dist_max, w2c=None, variant=None):
    """the same decisions in float64 on the same float32 inputs"""
    return _accumulate(np.float64, live, depth_l, pose12, model, depth_m, normal_m, dist_max, w2c, variant)


# ------------------------------------------------------------------------------------------------ (c) where float32 may differ
E = wr.E


def _project_E(view, X):
    """(u + 0.5, v + 0.5, signs) of the projection of the E points X in the E class: the second half of _pano_ref.chain_bound"""
    mt, cam_t, w2c, wt, ht = view
    Mt = np.asarray(w2c, np.float64).reshape(3, 4).tolist()
    pc = [((Mt[k][0] * X[0] + Mt[k][1] * X[1]) + Mt[k][2] * X[2]) + Mt[k][3] for k in range(3)]
    rng = ((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]).sqrt()
    if mt == PINHOLE:
        fx, fy, cx, cy = (float(v) for v in cam_t)
        u, v, signs = fx * (pc[0] / pc[2]) + cx, fy * (pc[1] / pc[2]) + cy, [pc[2]]
    elif mt == FISHEYE:
        xi, k1, k2, g1, g2, u0, v0 = (float(x) for x in cam_t)
        xs, ys, zs = pc[0] / rng, pc[1] / rng, pc[2] / rng
        den = zs + xi
        x, y = xs / den, ys / den
        r2 = x * x + y * y
        s = (1.0 + k1 * r2) + k2 * (r2 * r2)
        u, v, signs = (g1 * x) * s + u0, (g2 * y) * s + v0, [den, xi * zs + 1.0]
    else:
        lon0, dlon, lat0, dlat = (float(np.float32(x)) for x in cam_t)
        lam = pr._atan2pi_E(pc[0], pc[2])
        hh = (pc[0] * pc[0] + pc[2] * pc[2]).sqrt()
        psi = pr._atan2pi_E(pc[1], hh)
        u = (lam - lon0) / dlon - 0.5
        v = (psi - lat0) / dlat - 0.5
        u = E(u.v, u.e + U32 * (np.abs(u.v) + 2.0 / abs(dlon)))        # the wrap: one more rounding of a value of at most width
        signs = []
    return u + 0.5, v + 0.5, signs


def excluded(ref64, live, depth_l, pose12, model, depth_m, normal_m, w2c=None):
    """(R) bool: the pixels where the float32 rule may legitimately give another code than accumulate64's result `ref64`.  A bound
    on |float32 - float64| (first order in u = 2^-24, _warp_ref.E's rules, inflated by INFLATE for the neglected terms) is carried
    through this rule's own operations; a pixel is excluded where a value that decides lies within its bound of its threshold:
    the lens rim and the projection's domain (the signs), u + 0.5 and v + 0.5 against the integers (the nearest pixel and the
    image border), e . e against dist_max^2 and the facing product against 0.  Decisions on stored values (the depths, the
    normal) are the same in both."""
    lview, mview, pview = _views(live, model, w2c)
    wl, hl, wm, hm = live[2], live[3], model[3], model[4]
    R = wl * hl
    pix = np.arange(R, dtype=np.int64)
    P = np.asarray(pose12, np.float32).reshape(3, 4).astype(np.float64).tolist()
    with np.errstate(all="ignore"):
        _, d, signs = pr.ray_chain(lview, pix)
        t = np.asarray(depth_l, np.float64).reshape(-1)
        t = np.where(ref64["have"], t, 1.0)
        x, y, z = t * d[0], t * d[1], t * d[2]
        qv = [(P[k][0] * x + P[k][1] * y) + P[k][2] * z for k in range(3)]
        p = [qv[k] + P[k][3] for k in range(3)]
        up, vp, dom_signs = _project_E(pview, p)
        out = np.zeros(R, bool)
        for sgn in signs + dom_signs:
            out |= ~(sgn.e < wr.GUARD * np.abs(sgn.v))
        dom = np.ones(R, bool)
        for sgn in dom_signs:
            dom &= sgn.v > 0
        close = (up.v > -1.0) & (up.v < wm + 1.0) & (vp.v > -1.0) & (vp.v < hm + 1.0)       # nothing is decided far outside the image
        for a in (up, vp):
            out |= dom & close & ~(np.abs(a.v - np.round(a.v)) > INFLATE * a.e)
        out |= dom & ~np.isfinite(up.e + vp.e)
        # the model point of the float64 pixel; where the pixels differ the pixel is excluded above
        mq = np.maximum(ref64["mq"], 0)
        om, dm_, msigns = pr.ray_chain(mview, mq)
        dm = np.asarray(depth_m, np.float64).reshape(-1)[mq]
        n = np.asarray(normal_m, np.float64).reshape(-1, 3)[mq]
        e = [(om[k] + dm * dm_[k]) - p[k] for k in range(3)]
        e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        facing = (n[:, 0] * qv[0] + n[:, 1] * qv[1]) + n[:, 2] * qv[2]
        known = ref64["known"]
        for sgn in msigns:
            out |= known & ~(sgn.e < wr.GUARD * np.abs(sgn.v))
        out |= known & ~(np.abs(e2.v - float(ref64["dist2"])) > INFLATE * (e2.e + U32 * float(ref64["dist2"])))
        out |= known & (e2.v <= float(ref64["dist2"]) * 1.01) & ~(np.abs(facing.v) > INFLATE * facing.e)
    return out & ref64["have"]


# ------------------------------------------------------------------------------------------------ (d) the sums
def terms(out):
    """(M, 28) float64: the exact products of the MATCH pixels in pixel order (21 of A row by row, 6 of g, r r), and their indices"""
    idx = np.flatnonzero(out["code"] == MATCH)
    J = out["J"][idx].astype(np.float64)
    r = out["residual"][idx].astype(np.float64)
    cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)] + [r * r]
    return np.stack(cols, -1).reshape(-1, SUMS), idx


def blocks_for(n_pix, compute_units=256):
    """the grid of k_icp_accumulate on a device of that many compute units"""
    return rr.blocks_for(n_pix, MAX_BLOCKS, compute_units, 1)


def rows_device(out, n_pix, grid):
    """(grid, 28) float64 and (grid) int64: the rows a launch of `grid` workgroups writes, in the kernel's order of additions
    (_reduce_ref.rows_device; a pixel that is no MATCH adds nothing)"""
    T, idx = terms(out)
    full = np.zeros((n_pix, SUMS))
    full[idx] = T
    hit = np.zeros(n_pix, bool)
    hit[idx] = True
    return rr.rows_device(full, hit, grid)


def combine(rows, counts):
    """the 28 sums and the count of rows added in block order from 0.0"""
    return rr.combine(np.asarray(rows, np.float64).reshape(-1, SUMS)), int(np.sum(np.asarray(counts, np.int64)))


# ------------------------------------------------------------------------------------------------ (e) the solve
def series(s, n_terms=SERIES_TERMS):
    """(a, b) = (sin t / t, (1 - cos t) / t^2) at s = t^2: n_terms terms of each power series, Horner, in Python floats"""
    ca = [(-1.0 if k % 2 else 1.0) / float(math.factorial(2 * k + 1)) for k in range(n_terms)]
    cb = [(-1.0 if k % 2 else 1.0) / float(math.factorial(2 * k + 2)) for k in range(n_terms)]
    a, b = ca[-1], cb[-1]
    for k in range(n_terms - 2, -1, -1):
        a = a * s + ca[k]
        b = b * s + cb[k]
    return a, b


def apply_twist(pose12, x, variant=None):
    """the pose update of step 6 / 7 in Python floats: 12 numpy.float32"""
    P = [[float(v) for v in row] for row in np.asarray(pose12, np.float32).reshape(3, 4)]
    w2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    sa, sb = series(w2)
    K = [[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]]
    D = [[(1.0 + sb * (x[i] * x[i] - w2)) if i == j else (sa * K[i][j] + sb * (x[i] * x[j])) for j in range(3)] for i in range(3)]
    out = np.zeros((3, 4), np.float32)
    for i in range(3):
        for j in range(3):
            if variant == "right":
                out[i, j] = np.float32((P[i][0] * D[0][j] + P[i][1] * D[1][j]) + P[i][2] * D[2][j])
            else:
                out[i, j] = np.float32((D[i][0] * P[0][j] + D[i][1] * P[1][j]) + D[i][2] * P[2][j])
        out[i, 3] = np.float32(P[i][3] + x[3 + i])
    return out.reshape(12)


def solve(tot, count, pose12, min_matches=6, max_rot=MAX_ROT, max_trans=float("inf"), update=True, variant=None):
    """k_icp_solve after the combine: (pose12 float32 (12), history row [count, E, w2, v2, status] of Python floats)"""
    assert variant is None or variant in SOLVE_VARIANTS
    pose12 = np.asarray(pose12, np.float32).reshape(12).copy()
    max_rot, max_trans = float(np.float32(max_rot)), float(np.float32(max_trans))
    row = lambda w2, v2, st: [float(count), float(tot[27]), w2, v2, float(st)]
    if count < min_matches:
        return pose12, row(0.0, 0.0, TOO_FEW)
    if not update:
        return pose12, row(0.0, 0.0, OK)
    A = [[0.0] * 6 for _ in range(6)]
    n = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(tot[n])
            n += 1
    g = [float(v) for v in tot[21:27]]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > PIVOT * A[j][j]):
            return pose12, row(0.0, 0.0, DEGENERATE)
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = g[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    w2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    v2 = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
    if not (w2 <= max_rot * max_rot and v2 <= max_trans * max_trans):
        return pose12, row(w2, v2, STEP_TOO_LARGE)
    return apply_twist(pose12, x, variant), row(w2, v2, OK)


def step(live, depth_l, pose12, model, depth_m, normal_m, dist_max, grid=None, f=np.float32, w2c=None, variant=None, **solve_args):
    """one iteration: accumulate (float32, or float64 with f), the sums (in the kernel's order for a grid, else math.fsum per
    column), solve.  Returns (pose12, history row, the accumulate's dict)."""
    acc_v = variant if variant in ACC_VARIANTS else None
    out = _accumulate(f, live, depth_l, pose12, model, depth_m, normal_m, dist_max, w2c, acc_v)
    if grid is None:
        T, idx = terms(out)
        tot, count = [math.fsum(T[:, k]) for k in range(SUMS)], idx.size
    else:
        tot, count = combine(*rows_device(out, live[2] * live[3], grid))
    pose, row = solve(tot, count, pose12, variant=variant if variant in SOLVE_VARIANTS else None, **solve_args)
    return pose, row, out


def track(live, depth_l, pose12, model, depth_m, normal_m, iters, dist_max, grid=None, f=np.float32, w2c=None, variant=None, **solve_args):
    """fusion.track restated: (pose12, history (iters + 1, 5), the last accumulate's dict, the pose after every iteration)"""
    pose = np.asarray(pose12, np.float32).reshape(12).copy()
    hist, poses = [], []
    for _ in range(iters):
        pose, row, _ = step(live, depth_l, pose, model, depth_m, normal_m, dist_max, grid, f, w2c, variant, **solve_args)
        hist.append(row)
        poses.append(pose.copy())
    _, row, out = step(live, depth_l, pose, model, depth_m, normal_m, dist_max, grid, f, w2c, variant, update=False, **solve_args)
    hist.append(row)
    return pose, np.asarray(hist, np.float64), out, poses


# ------------------------------------------------------------------------------------------------ poses
def pose_error(pose12, truth12):
    """(rotation angle in radians, translation distance) between two camera-to-world poses, float64"""
    A, B = np.asarray(pose12, np.float64).reshape(3, 4), np.asarray(truth12, np.float64).reshape(3, 4)
    dR = A[:, :3] @ B[:, :3].T
    return float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(A[:, 3] - B[:, 3]))


def perturbed(c2w, rot, trans):
    """c2w (3, 4) float64 turned by the rotation vector `rot` about the camera's centre and moved by `trans`"""
    M = np.asarray(c2w, np.float64).reshape(3, 4)
    w = np.asarray(rot, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Rd = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    return np.concatenate([Rd @ M[:, :3], (M[:, 3] + np.asarray(trans, np.float64))[:, None]], 1)


# ------------------------------------------------------------------------------------------------ the room scene
ROOM = ((-2.0, -1.5, -2.5), (2.5, 1.2, 3.0))       # an axis-aligned box seen from inside: no symmetry, all six degrees pinned
_FISH = tuple(v * s for v, s in zip(cr.KITTI_FISHEYE, (1, 1, 1, 64 / 1400, 64 / 1400, 64 / 1400, 64 / 1400)))
TRUE_POSE = cr.pose(0.25, -0.1, (0.3, 0.1, -0.2))              # the live frame's camera-to-world
MODEL_POSE = cr.pose(0.2, -0.05, (0.25, 0.05, -0.3))           # the model view's: a few centimetres and degrees away
GUESS = (np.array([0.015, -0.02, 0.012]), np.array([0.03, -0.02, 0.025]))      # a rotation vector of 1.6 degrees, an offset of 4.4 cm


def cameras(scale=1):
    """name -> a package camera of the model at a small size (scale multiplies the image): pinhole 64 x 48, fisheye 64 x 64 (the
    KITTI-360-shaped lens), equirect 64 x 32 (the full sphere)"""
    from panopticnerf_amd import Equirect, Fisheye, Pinhole
    s = float(scale)
    f = list(_FISH)
    f[3], f[4], f[5], f[6] = f[3] * s, f[4] * s, (f[5] + 0.5) * s - 0.5, (f[6] + 0.5) * s - 0.5
    return {"pinhole": Pinhole(40.0 * s, 41.0 * s, 31.5 * s, 23.5 * s, int(64 * s), int(48 * s)),
            "fisheye": Fisheye(*f, int(64 * s), int(64 * s)), "equirect": Equirect(int(64 * s), int(32 * s))}


def live_of(camera):
    return (camera.word, tuple(camera.params), camera.width, camera.height)


def model_of(camera, c2w):
    return (camera.word, tuple(camera.params), np.asarray(c2w, np.float32).reshape(3, 4), camera.width, camera.height)


def room_maps(camera, c2w, room=ROOM):
    """(depth (h, w), normal (h, w, 3)) float32 numpy of the room seen by the camera at the float32 pose c2w: analytic, exact"""
    from panopticnerf_amd import synthetic
    d, n = synthetic.room_depth(camera, np.asarray(c2w, np.float32).astype(np.float64), room[0], room[1], normals=True)
    return d.numpy(), n.numpy()
