"""numpy restatements of the ray / convex-polytope rule of include/pnr.h ("a8b: convex bounding primitives"): hits32 in float32
in the rule's operation order (what k_convex_hits must reproduce bit for bit), hits64 the same in float64, kept_lists the kept
list of pnr_bbox_hits / pnr_convex_hits from either (insert_lists: the same by the kernels' literal insertion).

`variant` corrupts the rule on purpose (tests/test_convex_ref.py shows that the closed forms catch each one):
"swap" = entering and leaving exchanged, "strict" = hit <=> tmin < tmax, "noparallel" = the parallel-and-outside rule dropped."""
import numpy as np

U32 = 2.0 ** -24        # unit roundoff of float32


def _hits(rays, planes, offsets, dt, variant=None):
    rays, planes = np.asarray(rays, dt), np.asarray(planes, dt)
    offsets = np.asarray(offsets)
    R, M = rays.shape[0], offsets.size - 1
    o, d = rays[:, 0:3], rays[:, 3:6]
    tmin = np.repeat(rays[:, 6:7], M, 1).astype(dt)
    tmax = np.repeat(rays[:, 7:8], M, 1).astype(dt)
    bind_in = np.full((R, M), -1, np.int64)         # the plane that set tmin / tmax (-1: near / far)
    bind_out = np.full((R, M), -1, np.int64)
    ninf = dt(-np.inf)
    with np.errstate(all="ignore"):
        for m in range(M):
            for p in range(int(offsets[m]), int(offsets[m + 1])):
                n0, n1, n2, dd = planes[p]
                dn = (n0 * d[:, 0] + n1 * d[:, 1]) + n2 * d[:, 2]
                on = (n0 * o[:, 0] + n1 * o[:, 1]) + n2 * o[:, 2]
                s = dd - on
                q = s / dn
                leave, enter = dn > 0, dn < 0
                if variant == "swap":
                    leave, enter = enter, leave
                new = np.where(leave, np.fmin(tmax[:, m], q), tmax[:, m])
                if variant != "noparallel":
                    new = np.where((dn == 0) & (s < 0), ninf, new)
                bind_out[new != tmax[:, m], m] = p
                tmax[:, m] = new
                new = np.where(enter, np.fmax(tmin[:, m], q), tmin[:, m])
                bind_in[new != tmin[:, m], m] = p
                tmin[:, m] = new
        hit = (tmin < tmax) if variant == "strict" else (tmin <= tmax)
    return tmin, tmax, hit, bind_in, bind_out


def hits32(rays, planes, offsets, variant=None):
    """(tmin, tmax (R,M) float32, hit (R,M) bool, bind_in, bind_out (R,M) plane indices) of the rule in float32"""
    return _hits(rays, planes, offsets, np.float32, variant)


def hits64(rays, planes, offsets, variant=None):
    return _hits(rays, planes, offsets, np.float64, variant)


def kept_lists(tmin, tmax, hit, max_hits):
    """(hit_t (R,mh,2), hit_box (R,mh) int32, hit_count (R) int32): the max_hits nearest hits in ascending (t_in, primitive
    index) order, pads 0 / -1, the TRUE count.  A stable sort by t_in: what the kernels' insertion from the back produces (an
    entry moves in front of strictly larger t_in only, and the farthest falls off the end)."""
    R, M = hit.shape
    hit_t = np.zeros((R, max_hits, 2), tmin.dtype)
    hit_box = np.full((R, max_hits), -1, np.int32)
    cnt = hit.sum(1).astype(np.int32)
    if M:
        key = np.where(hit, tmin, np.inf)
        order = np.argsort(key, axis=1, kind="stable")[:, :max_hits]
        k = order.shape[1]
        ok = np.take_along_axis(hit, order, 1)
        hit_box[:, :k] = np.where(ok, order, -1)
        hit_t[:, :k, 0] = np.where(ok, np.take_along_axis(tmin, order, 1), 0)
        hit_t[:, :k, 1] = np.where(ok, np.take_along_axis(tmax, order, 1), 0)
    return hit_t, hit_box, cnt


def insert_lists(tmin, tmax, hit, max_hits):
    """kept_lists by the literal insertion of k_bbox_hits / k_convex_hits (slow: small cases)"""
    R, M = hit.shape
    hit_t = np.zeros((R, max_hits, 2), tmin.dtype)
    hit_box = np.full((R, max_hits), -1, np.int32)
    cnt = np.zeros(R, np.int32)
    for r in range(R):
        for m in range(M):
            if not hit[r, m]:
                continue
            n = min(int(cnt[r]), max_hits)
            pos = n
            while pos > 0 and hit_t[r, pos - 1, 0] > tmin[r, m]:
                pos -= 1
            if pos < max_hits:
                for k in range(n if n < max_hits else max_hits - 1, pos, -1):
                    hit_t[r, k] = hit_t[r, k - 1]
                    hit_box[r, k] = hit_box[r, k - 1]
                hit_t[r, pos] = (tmin[r, m], tmax[r, m])
                hit_box[r, pos] = m
            cnt[r] += 1
    return hit_t, hit_box, cnt


def t_bound(rays, planes, p, t):
    """Bound on |t32 - t64| when plane p (an index array; -1 = near / far: 0) sets the depth, t its float64 quotient.

    With u = 2^-24 and every float32 operation correctly rounded (first order in u):
      dn = (n0 d0 + n1 d1) + n2 d2: the first two products pass three roundings, the third two:  |dn^ - dn| <= 3u D,
          D = sum |n_i d_i|;     likewise |on^ - on| <= 3u O,  O = sum |n_i o_i|;
      s = dd - on^: one more rounding of a value of at most |dd| + O:        |s^ - s| <= 3u O + u (|dd| + O) = u (4 O + |dd|);
      q = s^ / dn^ rounded once:  |q^ - q| <= |s^ - s| / |dn| + |q| |dn^ - dn| / |dn| + u |q|
                                           <= u (4 O + |dd| + 3 |t| D) / |dn| + u |t|,   and u |t| <= u |t| D / |dn| as |dn| <= D,
                                           <= 4 u (O + |dd| + |t| D) / |dn|.
    The terms of second order are below 16 u times this: the factor (1 + 16 u).  The planes are the same float32 numbers in both
    evaluations and near / far are copied: no input rounding."""
    rays, planes = np.asarray(rays, np.float64), np.asarray(planes, np.float64)
    pl = planes[np.maximum(p, 0)]
    n, dd = pl[..., :3], pl[..., 3]
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    if n.ndim == 2:
        o, d = o[:, 0], d[:, 0]
    D, O = np.abs(n * d).sum(-1), np.abs(n * o).sum(-1)
    dn = np.abs((n * d).sum(-1))
    with np.errstate(all="ignore"):
        b = 4.0 * U32 * (O + np.abs(dd) + np.abs(t) * D) / dn * (1.0 + 16.0 * U32)
    return np.where(p < 0, 0.0, b)


def excluded(tmin64, tmax64, hit64, rel=1e-4):
    """Rays whose kept list float32 may legitimately order or decide differently: float64 sees a grazing interval (|t_out - t_in|
    within rel * max(1, |t|) of zero, hit or miss) or two entry depths of hit primitives closer than rel * max(1, t)."""
    with np.errstate(all="ignore"):
        scale = rel * np.maximum(1.0, np.abs(tmin64))
        graze = (np.abs(tmax64 - tmin64) < scale).any(1)
        key = np.sort(np.where(hit64, tmin64, np.inf), axis=1)
        gap = key[:, 1:] - key[:, :-1]
        close = (np.isfinite(key[:, 1:]) & (gap < rel * np.maximum(1.0, np.abs(key[:, 1:])))).any(1) if key.shape[1] > 1 else np.zeros(len(key), bool)
    return graze | close
