"""Plain high-precision references of the per-ray preamble (panopticnerf_amd/csrc/pnr_sampling.hip: k_bbox_hits, k_restrict_rays,
k_stratified, k_sample_labels, k_points, k_embed and the fused k_ray_setup), written from include/pnr.h and the comments of the
kernels.  Nothing here calls oracle/: tests/test_setup_ref.py holds the C oracle against these on the CPU, and
tests/test_gpu_setup_sweep.py holds the kernels against the C oracle bit for bit, which ties the kernels to float64.

`variant` corrupts a rule on purpose (test_setup_ref.py shows that the closed forms catch each one): "first" keeps the first
max_hits hits in table order instead of the nearest, "strict" closes an interval with < instead of <=, "hull0" takes the hull
from entry 0 only, "onesided" builds the linspace from the lower end only, "swapcs" exchanges the sin and cos columns.

Bounds (u = 2^-24, every float32 operation correctly rounded, first order in u with the second order in a factor 1 + 16 u).

t_bound: one slab quotient  t = (+-e - ol) * (1 / dl)  of box axis a, against the same expression in float64 on the same float32
inputs.  p_i = o_i - c_i is rounded once: |p^_i - p_i| <= u |p_i|.  ol = (r0 p0 + r1 p1) + r2 p2: the first two products pass
three roundings, the third two, and each carries its p's rounding:  |ol^ - ol| <= 4 u O,  O = sum |r_i p_i|.  dl likewise without
the input rounding:  |dl^ - dl| <= 3 u D,  D = sum |r_i d_i|.  s = +-e - ol^ is one more rounding of a value of at most e + O:
|s^ - s| <= u (5 O + e).  inv = 1 / dl^ rounded once: relative error u + 3 u D / |dl|.  t = s^ * inv rounded once.  Together
    |t^ - t| <= u (5 O + e) / |dl| + |t| u (3 D / |dl| + 2) <= 5 u (O + e + |t| D) / |dl|        as |dl| <= D.
An interval end is a max (min) over near (far) and three such quotients; interval_bounds explains how the bound of an end is
taken.  near / far are copied: their bound is 0.

stratified (strat_z, strat_sample), S = |near| + |far|:  t_i carries 2 u (step rounded, times i rounded; the upper half is one
fma from 1), 1 - t_i 3 u, near (1 - t) 4 u |near|, far t 3 u |far|, their sum u S more:  |z^ - z| <= 5 u S =: B.  With jitter:
lo and up are halves of a rounded sum of two such z (B + u S each), w = up - lo (2 B + 4 u S), m = w t_rand (2 B + 6 u S),
z = lo + m:  |z^ - z| <= 3 B + 8 u S = 23 u S.  lindisp: the same count on 1 / near, 1 / far (each one rounding more) gives the
denominator s to delta = 6 u (1 / |near| + 1 / |far|), and z = 1 / s rounded once:  |z^ - z| <= (z^2 delta + u |z|) / (1 - delta |z|) =: B_i;
with jitter 3 max_i B_i + 8 u max_i |z_i| by the same steps."""
import numpy as np

U32 = 2.0 ** -24
SECOND = 1.0 + 16.0 * U32


def fmin(a, b):
    """include/pnr.h "a8: min / max": a NaN operand loses, -0 orders below +0"""
    a, b = np.broadcast_arrays(a, b)
    first = (a < b) | ((a == b) & np.signbit(a))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(first, a, b)))


def fmax(a, b):
    a, b = np.broadcast_arrays(a, b)
    first = (a > b) | ((a == b) & ~np.signbit(a))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(first, a, b)))


# ------------------------------------------------------------------------------------------------------------ the slab test
def _axes(rays, box, dt):
    """per (ray, box, axis): ol, dl, e and the two quotients, in dtype dt and the rule's operation order"""
    rays, box = np.asarray(rays, np.float32).reshape(-1, 8).astype(dt), np.asarray(box, np.float32).reshape(-1, 15).astype(dt)
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    c, rot, e = box[None, :, 0:3], box[None, :, 3:12].reshape(1, -1, 3, 3), box[None, :, 12:15]
    p = (o - c)[:, :, None, :]                                      # (R, M, 1, 3)
    dd = np.broadcast_to(d[:, :, None, :], p.shape)
    with np.errstate(all="ignore"):
        ol = (rot[..., 0] * p[..., 0] + rot[..., 1] * p[..., 1]) + rot[..., 2] * p[..., 2]          # (R, M, 3)
        dl = (rot[..., 0] * dd[..., 0] + rot[..., 1] * dd[..., 1]) + rot[..., 2] * dd[..., 2]
        inv = dt(1.0) / dl
        t1, t2 = (-e - ol) * inv, (e - ol) * inv
    return p, dd, rot, np.broadcast_to(e, ol.shape), ol, dl, t1, t2


def _hits(rays, box, dt):
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    M = np.asarray(box).reshape(-1, 15).shape[0]
    *_, t1, t2 = _axes(rays, box, dt)
    tmin = np.repeat(rays[:, 6:7].astype(dt), M, 1)
    tmax = np.repeat(rays[:, 7:8].astype(dt), M, 1)
    with np.errstate(all="ignore"):
        for a in range(3):
            tmin = fmax(tmin, fmin(t1[..., a], t2[..., a]))
            tmax = fmin(tmax, fmax(t1[..., a], t2[..., a]))
        hit = tmin <= tmax
    return tmin, tmax, hit


def bbox_hits64(rays, box):
    """(t_in, t_out (R,M) float64, hit (R,M) bool) of the slab test in float64: every box, before any list is cut.  The true
    count is hit.sum(1)."""
    return _hits(rays, box, np.float64)


def bbox_hits32(rays, box):
    """the same in float32, one rounding per operation: the rule the kernels and the C oracle state"""
    return _hits(rays, box, np.float32)


def kept_lists(tmin, tmax, hit, max_hits, variant=None):
    """(hit_t (R,mh,2), hit_box (R,mh) int32, hit_count (R) int32): the max_hits nearest hits in ascending (t_in, box index)
    order, pads 0 / -1, the TRUE count."""
    R, M = hit.shape
    hit_t = np.zeros((R, max_hits, 2), tmin.dtype)
    hit_box = np.full((R, max_hits), -1, np.int32)
    cnt = hit.sum(1).astype(np.int32)
    if M:
        key = np.where(hit, tmin, np.inf)
        if variant == "first":          # corrupted: the first max_hits hits of the table, then sorted
            rank = np.cumsum(hit, 1)
            key = np.where(hit & (rank <= max_hits), tmin, np.inf)
            hit = hit & (rank <= max_hits)
        order = np.argsort(key, axis=1, kind="stable")[:, :max_hits]
        k = order.shape[1]
        ok = np.take_along_axis(hit, order, 1)
        hit_box[:, :k] = np.where(ok, order, -1)
        hit_t[:, :k, 0] = np.where(ok, np.take_along_axis(tmin, order, 1), 0)
        hit_t[:, :k, 1] = np.where(ok, np.take_along_axis(tmax, order, 1), 0)
    return hit_t, hit_box, cnt


def t_bound(O, e, t, D, dl):
    """bound on |float32 - float64| of one slab quotient (module docstring): 5 u (O + e + |t| D) / |dl|"""
    with np.errstate(all="ignore"):
        return 5.0 * U32 * (O + e + np.abs(t) * D) / np.abs(dl) * SECOND


def interval_bounds(rays, box):
    """(b_in, b_out (R,M) float64, degenerate (R) bool): bounds on |t_in32 - t_in64| and |t_out32 - t_out64| per (ray, box).

    t_in = max(near, q_0, q_1, q_2) with q_a the entering quotient of axis a and e_a its t_bound.  float32's maximum is attained
    at an axis a' with q^_a' >= q^_b >= q_b - e_b (b: float64's binder), so q_a' + e_a' >= t_in64 - e_b: b_in is the largest e_a
    over those candidates (near: 0), and symmetrically for t_out.  A ray with a non-finite quotient somewhere (dl = 0 in some
    box frame) is `degenerate`: its bounds are not meaningful and the caller counts it as unsafe."""
    p, dd, rot, e, ol, dl, t1, t2 = _axes(rays, box, np.float64)
    rays = np.asarray(rays, np.float64).reshape(-1, 8)
    with np.errstate(all="ignore"):
        O, D = np.abs(rot * p).sum(-1), np.abs(rot * dd).sum(-1)
        qi, qo = np.minimum(t1, t2), np.maximum(t1, t2)
        ei, eo = t_bound(O, e, qi, D, dl), t_bound(O, e, qo, D, dl)
        degenerate = ~(np.isfinite(t1) & np.isfinite(t2) & np.isfinite(ei) & np.isfinite(eo)).all((1, 2))
        tin = np.maximum(rays[:, 6:7], qi.max(-1))
        tout = np.minimum(rays[:, 7:8], qo.min(-1))
        eb_in = np.where(qi.max(-1) >= rays[:, 6:7], np.take_along_axis(ei, qi.argmax(-1)[..., None], -1)[..., 0], 0.0)
        eb_out = np.where(qo.min(-1) <= rays[:, 7:8], np.take_along_axis(eo, qo.argmin(-1)[..., None], -1)[..., 0], 0.0)
        b_in = np.where(qi + ei >= (tin - eb_in)[..., None], ei, 0.0).max(-1)
        b_out = np.where(qo - eo <= (tout + eb_out)[..., None], eo, 0.0).max(-1)
    return b_in, b_out, degenerate


def unsafe_rays(rays, box, max_hits):
    """Rays on which float32 may legitimately decide otherwise than float64: a decision's float64 margin is below the bounds of
    the two depths it compares.  Decisions: hit or miss of every box (t_out - t_in against b_in + b_out), the order of two
    neighbours among the first max_hits + 1 hits by t_in (which covers who falls off the end); degenerate rays."""
    tmin, tmax, hit = bbox_hits64(rays, box)
    b_in, b_out, deg = interval_bounds(rays, box)
    R, M = hit.shape
    bad = deg.copy()
    if M == 0:
        return bad
    with np.errstate(all="ignore"):
        margin = np.abs(tmax - tmin)
        bad |= (~(margin > b_in + b_out) & ~((margin == 0) & (b_in + b_out == 0))).any(1)
        key = np.where(hit, tmin, np.inf)
        order = np.argsort(key, axis=1, kind="stable")[:, : max_hits + 1]
        k, kb = np.take_along_axis(key, order, 1), np.take_along_axis(b_in, order, 1)
        if k.shape[1] > 1:
            gap, need = k[:, 1:] - k[:, :-1], kb[:, 1:] + kb[:, :-1]
            both = np.isfinite(k[:, 1:])
            bad |= (both & ~(gap > need) & ~((gap == 0) & (need == 0))).any(1)
    return bad


# ------------------------------------------------------------------------------------------------------------------ the hull
def restrict64(rays, hit_t, hit_count, variant=None):
    """rays (float64 copy) with near / far replaced by [min t_in, max t_out] over the min(hit_count, max_hits) kept entries;
    rays without a hit unchanged"""
    rays = np.asarray(rays, np.float64).reshape(-1, 8).copy()
    hit_t = np.asarray(hit_t, np.float64)
    mh = hit_t.shape[1]
    cnt = np.minimum(np.asarray(hit_count), mh)
    lo, hi = hit_t[:, 0, 0].copy(), hit_t[:, 0, 1].copy()
    if variant != "hull0":
        for h in range(1, mh):
            use = h < cnt
            lo = np.where(use, fmin(lo, hit_t[:, h, 0]), lo)
            hi = np.where(use, fmax(hi, hit_t[:, h, 1]), hi)
    rays[:, 6] = np.where(cnt > 0, lo, rays[:, 6])
    rays[:, 7] = np.where(cnt > 0, hi, rays[:, 7])
    return rays


def hull_loops(rays, hit_t, hit_count):
    """the hull rule as plain loops, float32 in and out (copies only: exact)"""
    out = np.array(rays, np.float32).reshape(-1, 8).copy()
    hit_t = np.asarray(hit_t, np.float32)
    mh = hit_t.shape[1]
    for r in range(out.shape[0]):
        cnt = min(int(hit_count[r]), mh)
        if cnt <= 0:
            continue
        lo, hi = hit_t[r, 0, 0], hit_t[r, 0, 1]
        for h in range(1, cnt):
            lo = np.float32(fmin(lo, hit_t[r, h, 0]))
            hi = np.float32(fmax(hi, hit_t[r, h, 1]))
        out[r, 6], out[r, 7] = lo, hi
    return out


# ---------------------------------------------------------------------------------------------------------------- the depths
def _linspace01(N, variant=None):
    """torch.linspace(0, 1, N) two-sided: the upper half counted down from 1, so that t[N - 1] == 1 exactly"""
    if N <= 1:
        return np.zeros(max(N, 0))
    i = np.arange(N, dtype=np.float64)
    step = 1.0 / (N - 1)
    if variant == "onesided":
        return step * i
    return np.where(i < N // 2, step * i, 1.0 - step * (N - 1 - i))


def _strat_z(near, far, N, lindisp, variant=None):
    t = _linspace01(N, variant)[None, :]
    near, far = near[:, None], far[:, None]
    with np.errstate(all="ignore"):
        if not lindisp:
            return near * (1.0 - t) + far * t
        return 1.0 / ((1.0 / near) * (1.0 - t) + (1.0 / far) * t)


def stratified64(rays, N, lindisp=False, t_rand=None, variant=None):
    """z (R,N) float64: the stratified depths, jittered inside their bins by t_rand (R,N) when given"""
    rays = np.asarray(rays, np.float64).reshape(-1, 8)
    z = _strat_z(rays[:, 6], rays[:, 7], N, lindisp, variant)
    if t_rand is None:
        return z
    mids = 0.5 * (z[:, 1:] + z[:, :-1])
    lo, up = np.concatenate([z[:, :1], mids], 1), np.concatenate([mids, z[:, -1:]], 1)
    return lo + (up - lo) * np.asarray(t_rand, np.float64).reshape(z.shape)


def stratified_bound(rays, N, lindisp=False, jitter=False):
    """(R,N) bound on |float32 - float64| of stratified64's depths (module docstring)"""
    rays = np.asarray(rays, np.float64).reshape(-1, 8)
    near, far = rays[:, 6], rays[:, 7]
    if not lindisp:
        S = (np.abs(near) + np.abs(far))[:, None] * np.ones((1, N))
        return (23.0 if jitter else 5.0) * U32 * S * SECOND
    z = np.abs(_strat_z(near, far, N, True))
    delta = 6.0 * U32 * (1.0 / np.abs(near) + 1.0 / np.abs(far))[:, None]
    B = (z * z * delta + U32 * z) / (1.0 - delta * z)
    if not jitter:
        return B * SECOND
    return (3.0 * B.max(1, keepdims=True) + 8.0 * U32 * z.max(1, keepdims=True)) * SECOND * np.ones((1, N))


def points64(rays, z):
    rays = np.asarray(rays, np.float64).reshape(-1, 8)
    return rays[:, None, 0:3] + rays[:, None, 3:6] * np.asarray(z, np.float64)[..., None]


def points_bound(rays, z):
    """2 roundings: the product d z, then the sum o + d z: u |d z| + u (|o| + |d z|)"""
    rays = np.asarray(rays, np.float64).reshape(-1, 8)
    m = np.abs(rays[:, None, 3:6] * np.asarray(z, np.float64)[..., None])
    return U32 * (2.0 * m + np.abs(rays[:, None, 0:3])) * SECOND


# ---------------------------------------------------------------------------------------------------------------- the labels
def labels_loops(z, hit_t, hit_box, hit_count, box_ids, variant=None):
    """label_hit as plain loops over float32 lists: among the min(hit_count, max_hits) kept intervals with t_in <= z <= t_out the
    one with the smallest t_in, ties to the earlier entry; its box's (semantic, instance) ids, (-1, -1) without one"""
    z, hit_t = np.asarray(z, np.float32), np.asarray(hit_t, np.float32)
    R, N = z.shape
    mh = hit_t.shape[1]
    ls, li = np.full((R, N), -1, np.int32), np.full((R, N), -1, np.int32)
    for r in range(R):
        cnt = min(int(hit_count[r]), mh)
        for i in range(N):
            zz, best, bt = z[r, i], -1, 0.0
            for h in range(cnt):
                ti, to = hit_t[r, h, 0], hit_t[r, h, 1]
                inside = (ti <= zz and zz < to) if variant == "strict" else (ti <= zz and zz <= to)
                if inside and (best < 0 or ti < bt):
                    best, bt = h, ti
            if best >= 0:
                ls[r, i], li[r, i] = box_ids[hit_box[r, best]]
    return ls, li


def labels_vec(z, hit_t, hit_box, hit_count, box_ids):
    """labels_loops vectorised (large cases; test_setup_ref.py holds the two equal)"""
    z, hit_t = np.asarray(z, np.float32), np.asarray(hit_t, np.float32)
    mh = hit_t.shape[1]
    use = (np.arange(mh)[None, :] < np.minimum(np.asarray(hit_count), mh)[:, None])[:, None, :]      # (R, 1, mh)
    ti, to = hit_t[:, None, :, 0], hit_t[:, None, :, 1]
    with np.errstate(invalid="ignore"):
        inside = use & (ti <= z[..., None]) & (z[..., None] <= to)
    key = np.where(inside, ti, np.inf)
    best = np.argmin(key, -1)                                       # first of equal minima: ties to the earlier entry
    found = inside.any(-1)
    m = np.take_along_axis(np.asarray(hit_box)[:, None, :].repeat(z.shape[1], 1), best[..., None], -1)[..., 0]
    ids = np.asarray(box_ids, np.int32).reshape(-1, 2)
    ls = np.where(found, ids[np.maximum(m, 0), 0], -1).astype(np.int32)
    li = np.where(found, ids[np.maximum(m, 0), 1], -1).astype(np.int32)
    return ls, li


# -------------------------------------------------------------------------------------------------------------- the embedder
def embed64(x, L, variant=None):
    """(n, 3 + 6 L) float64: x, then per band k sin(x 2^k) for x, y, z followed by cos(x 2^k) for x, y, z.  x is float32, so
    the argument x 2^k is the float32 product exactly."""
    x = np.asarray(x, np.float32).reshape(-1, 3).astype(np.float64)
    cols = [x]
    for k in range(L):
        a = x * 2.0 ** k
        cols += [np.cos(a), np.sin(a)] if variant == "swapcs" else [np.sin(a), np.cos(a)]
    return np.concatenate(cols, 1)
