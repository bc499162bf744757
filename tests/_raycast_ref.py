"""CPU references of volume ray casting (k_tsdf_raycast in csrc/pnr_fusion.hip; the rule is include/pnr.h "volume ray casting").

(a) raycast_loops: the rule as plain Python loops over pixels and samples on numpy.float32 scalars -- the text of the header,
    step by step.
(b) raycast32: the same in vectorised numpy float32, in the rule's operation order.  k_tsdf_raycast must equal it bit for bit.
    Both take the ray (step 1) from the CPU restatements of the three camera models that _splat_ref and _tsdf_ref build on
    (_pano_ref._rays: _warp_ref.pinhole_rays32, _camera_ref.unproject32, _pano_ref.unproject32), pinned bit for bit against
    the ray kernels.  `variant`: deliberately WRONG rules (test_raycast_ref.py: its checks can fail).
(c) raycast64: the same decisions in float64 ON THE FLOAT32 RAY (o, d as pnr_camera_ray rounds them -- what the ray kernels lose
    against float64 is the camera tests' subject, not this rule's), with the per-pixel quantities a float32 comparison needs.

A view is (model, cam, c2w (3, 4), width, height); a lattice is (lo32 (3), step32 (3), (res_x, res_y, res_z)) as _mesh_ref.lattice
makes it; tsdf and weight are flat float32 arrays in the order n = (iz res_y + iy) res_x + ix.  Results are dicts of arrays over
the pixels `pix` (None: all, row-major): depth float32, normal (., 3) float32, src int32, code uint8.
"""
import numpy as np

import _mesh_ref as mr
import _pano_ref as pr
import _tsdf_ref as tr

PINHOLE, FISHEYE, EQUIRECT = tr.PINHOLE, tr.FISHEYE, tr.EQUIRECT
HIT, NO_RAY, MISSED, NO_SURFACE = 0, 1, 2, 3
# sign: the crossing is + to - (the usual sign);  ge: observed means weight > min_weight;  unobserved_ok: a crossing counts
# whatever its two samples' observed flags;  no_clamp: the cell index runs to res - 1 (the far face gets a cell of its own,
# folded onto the face);  normal_sign: the normal is +gradient;  src_floor: src is the cell's own corner, not the nearest
VARIANTS = ("sign", "ge", "unobserved_ok", "no_clamp", "normal_sign", "src_floor")
U32 = 2.0 ** -24
INFLATE = 1.0 + 2.0 ** -4
FMAX = np.finfo(np.float32).max
BOX = ((-2.5, -1.0, 4.5), (3.0, 3.0, 8.0))         # test_gpu_tsdf.BOX: straddles _tsdf_ref.SPHERE's surface in front of every camera
# (res, box, trunc) of the sphere volumes the restatements and the kernel are compared on: the smallest lattice, an odd one, one
# of several cells a wave, and an anisotropic box; trunc is wide enough that each holds observed crossings
LATTICES = (((2, 2, 2), BOX, 3.0), ((2, 5, 9), BOX, 1.5), ((16, 16, 16), BOX, 0.9), ((12, 7, 5), ((-4.0, 0.5, 5.75), (4.0, 2.5, 6.25)), 0.6))


def lattice(lo, hi, res):
    lo32, step = mr.lattice(lo, hi, res)
    return lo32, step, tuple(int(r) for r in res)


def default_dt(step):
    """half the smallest |step|, a float32"""
    return np.float32(np.abs(np.asarray(step, np.float32)).min() * np.float32(0.5))


def default_max_steps(res, step, dt):
    diag = sum(((int(r) - 1) * float(s)) ** 2 for r, s in zip(res, step)) ** 0.5
    return min(int(diag / float(dt)) + 2, 2 ** 31 - 1)


def sphere_volume(lat, trunc, sphere=tr.SPHERE):
    """the analytic volume of a sphere seen from INSIDE, as depth fusion would leave it: phi = (|X - c| - R) / trunc, positive
    behind the surface; tsdf = max(phi, -1), weight = 1 where phi <= 1 and 0 (tsdf 0) deeper than trunc.  Flat float32 arrays."""
    lo, step, res = lat
    x, y, z = [((np.arange(res[a]).astype(np.float32) + np.float32(0.5)) * step[a] + lo[a]).astype(np.float64) for a in range(3)]
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    c, R = sphere
    phi = (np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - R) / float(trunc)
    seen = phi <= 1.0
    return np.where(seen, np.maximum(phi, -1.0), 0.0).astype(np.float32).reshape(-1), seen.astype(np.float32).reshape(-1)


def _pixels(view, pix):
    w, h = view[3], view[4]
    return np.arange(w * h, dtype=np.int64) if pix is None else np.asarray(pix, np.int64).reshape(-1)


def _rays32(view, pc):
    """o (3), d (R, 3) float32, ok (R): step 1, the bits of pnr_camera_ray"""
    o, d, ok = pr._rays(np.float32, view, pc)
    return np.asarray(o, np.float32), np.asarray(d, np.float32), np.asarray(ok, bool)


def _empty(R):
    return {"depth": np.zeros(R, np.float32), "normal": np.zeros((R, 3), np.float32), "src": np.full(R, -1, np.int32),
            "code": np.full(R, NO_RAY, np.uint8)}


# ------------------------------------------------------------------------------------------------ (a) loops
def _cell_scalar(f, g, res_k, variant):
    fl = np.fmin(np.fmax(np.floor(g), f(0.0)), f(2.0 ** 30))
    c = min(int(fl), res_k - (1 if variant == "no_clamp" else 2))
    return c, np.fmin(np.fmax(g - f(c), f(0.0)), f(1.0))


def _lerp(p, q, fr):
    return p + fr * (q - p)


def _sample_scalar(f, lat, tsdf, weight, min_weight, og, dg, t, variant):
    """step 5 at parameter t: (cell (3), fraction (3), corner values [8], observed, value)"""
    _, _, res = lat
    c, fr = [0, 0, 0], [f(0), f(0), f(0)]
    for k in range(3):
        c[k], fr[k] = _cell_scalar(f, og[k] + t * dg[k], res[k], variant)
    v, obs = [], True
    for k in range(8):
        ix, iy, iz = (min(c[a] + ((k >> a) & 1), res[a] - 1) for a in range(3))         # (+1 is inside the lattice under the rule's clamp)
        at = (iz * res[1] + iy) * res[0] + ix
        v.append(f(tsdf[at]))
        obs = obs and bool((weight[at] > min_weight) if variant == "ge" else (weight[at] >= min_weight))
    x = [_lerp(v[0], v[1], fr[0]), _lerp(v[2], v[3], fr[0]), _lerp(v[4], v[5], fr[0]), _lerp(v[6], v[7], fr[0])]
    val = _lerp(_lerp(x[0], x[1], fr[1]), _lerp(x[2], x[3], fr[1]), fr[2])
    return c, fr, v, obs, val


def raycast_loops(view, near, far, lat, tsdf, weight, min_weight=1.0, dt=None, max_steps=None, pix=None, variant=None):
    """The rule, one pixel and one sample at a time, on numpy.float32 scalars."""
    assert variant is None or variant in VARIANTS
    f = np.float32
    lo, step, res = lat
    dt = f(default_dt(step) if dt is None else dt)
    max_steps = default_max_steps(res, step, dt) if max_steps is None else int(max_steps)
    min_weight = f(min_weight)
    pc = _pixels(view, pix)
    o, d, ok = _rays32(view, pc)
    out = _empty(len(pc))
    with np.errstate(all="ignore"):
        for p in range(len(pc)):
            if not ok[p]:                                                               # 1
                continue
            og = [(o[k] - lo[k]) / step[k] - f(0.5) for k in range(3)]                  # 2
            dg = [d[p, k] / step[k] for k in range(3)]
            t_in, t_out, miss = f(near), f(far), False                                  # 3
            for k in range(3):
                top = f(res[k] - 1)
                if dg[k] == 0:
                    miss = miss or bool(og[k] < 0) or bool(og[k] > top)
                else:
                    ta, tb = (f(0.0) - og[k]) / dg[k], (top - og[k]) / dg[k]
                    t_in, t_out = np.fmax(t_in, np.fmin(ta, tb)), np.fmin(t_out, np.fmax(ta, tb))
            out["code"][p] = MISSED
            if miss or not t_in <= t_out:
                continue
            out["code"][p] = NO_SURFACE
            t_prev, v_prev, obs_prev, hit = f(0), f(0), False, None
            for n in range(max_steps):                                                  # 4
                t = t_in + f(n) * dt
                if not t <= t_out:
                    break
                _, _, _, obs, v = _sample_scalar(f, lat, tsdf, weight, min_weight, og, dg, t, variant)      # 5
                both = (obs_prev and obs) or (variant == "unobserved_ok" and n >= 1)    # 6
                cross = (v_prev > 0 and 0 >= v) if variant == "sign" else (v_prev < 0 and 0 <= v)
                if n >= 1 and both and cross:
                    r = v_prev / (v_prev - v)                                           # 7
                    hit = t_prev + (t - t_prev) * r
                    break
                t_prev, v_prev, obs_prev = t, v, obs
            if hit is None:
                continue
            out["code"][p], out["depth"][p] = HIT, hit
            c, fr, v, obs, _ = _sample_scalar(f, lat, tsdf, weight, min_weight, og, dg, hit, variant)
            s = [min(c[k] + (0 if variant == "src_floor" else int(fr[k] >= f(0.5))), res[k] - 1) for k in range(3)]
            out["src"][p] = (s[2] * res[1] + s[1]) * res[0] + s[0]
            if obs:
                gx = _lerp(_lerp(v[1] - v[0], v[3] - v[2], fr[1]), _lerp(v[5] - v[4], v[7] - v[6], fr[1]), fr[2]) / step[0]
                gy = _lerp(_lerp(v[2] - v[0], v[3] - v[1], fr[0]), _lerp(v[6] - v[4], v[7] - v[5], fr[0]), fr[2]) / step[1]
                gz = _lerp(_lerp(v[4] - v[0], v[5] - v[1], fr[0]), _lerp(v[6] - v[2], v[7] - v[3], fr[0]), fr[1]) / step[2]
                ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
                if ln > 0 and ln <= FMAX:
                    sg = f(1.0) if variant == "normal_sign" else f(-1.0)
                    out["normal"][p] = ((sg * gx) / ln, (sg * gy) / ln, (sg * gz) / ln)
    return out


# ------------------------------------------------------------------------------------------------ (b), (c) vectorised
def _sample(f, lat, tsdf, weight, min_weight, og, dg, t, variant):
    """step 5 for the rays given (og (3), dg (R, 3), t (R)): c (R, 3) int64, fr (R, 3), v [8] of (R), obs (R), value (R), g (R, 3)"""
    _, _, res = lat
    cs, frs, gs = [], [], []
    for k in range(3):
        g = og[k] + t * dg[:, k]
        fl = np.fmin(np.fmax(np.floor(g), f(0.0)), f(2.0 ** 30))
        c = np.minimum(fl.astype(np.int64), res[k] - (1 if variant == "no_clamp" else 2))
        cs.append(c)
        frs.append(np.fmin(np.fmax(g - c.astype(f), f(0.0)), f(1.0)))
        gs.append(g)
    v, obs = [], np.ones(t.shape, bool)
    for k in range(8):
        ix, iy, iz = (np.minimum(cs[a] + ((k >> a) & 1), res[a] - 1) for a in range(3))
        at = (iz * res[1] + iy) * res[0] + ix
        v.append(tsdf[at].astype(f))
        w = weight[at]
        obs &= (w > min_weight) if variant == "ge" else (w >= min_weight)
    x = [_lerp(v[0], v[1], frs[0]), _lerp(v[2], v[3], frs[0]), _lerp(v[4], v[5], frs[0]), _lerp(v[6], v[7], frs[0])]
    val = _lerp(_lerp(x[0], x[1], frs[1]), _lerp(x[2], x[3], frs[1]), frs[2])
    return np.stack(cs, -1), np.stack(frs, -1), v, obs, val, np.stack(gs, -1)


def _cast(f, view, near, far, lat, tsdf, weight, min_weight, dt, max_steps, pix, variant):
    assert variant is None or variant in VARIANTS
    lo32, step32, res = lat
    dt32 = np.float32(default_dt(step32) if dt is None else dt)
    max_steps = default_max_steps(res, step32, dt32) if max_steps is None else int(max_steps)
    lo, step, dt, min_weight = lo32.astype(f), step32.astype(f), f(dt32), np.float32(min_weight)
    flat = (lo, step, res)
    pc = _pixels(view, pix)
    o32, d32, ok = _rays32(view, pc)
    o, d = o32.astype(f), d32.astype(f)
    R = len(pc)
    out = _empty(R)
    info = {"n": np.full(R, -1, np.int64)}
    with np.errstate(all="ignore"):
        og = [(o[k] - lo[k]) / step[k] - f(0.5) for k in range(3)]
        dg = d / step[None, :]
        t_in, t_out, miss = np.full(R, f(near)), np.full(R, f(far)), np.zeros(R, bool)
        axis = np.full(R, -1)                                       # the axis that sets t_in (-1: near does)
        for k in range(3):
            top = f(res[k] - 1)
            z = dg[:, k] == 0
            miss |= z & bool((og[k] < 0) | (og[k] > top))
            ta, tb = (f(0.0) - og[k]) / dg[:, k], (top - og[k]) / dg[:, k]
            lo_t, hi_t = np.fmin(ta, tb), np.fmax(ta, tb)
            axis = np.where(~z & (lo_t > t_in), k, axis)
            t_in = np.where(z, t_in, np.fmax(t_in, lo_t))
            t_out = np.where(z, t_out, np.fmin(t_out, hi_t))
        enter = ok & ~miss & (t_in <= t_out)
        out["code"][ok] = MISSED
        out["code"][enter] = NO_SURFACE
        active = enter.copy()
        t_prev, v_prev, obs_prev = np.zeros(R, f), np.zeros(R, f), np.zeros(R, bool)
        depth = np.zeros(R, f)
        keep = {k: np.zeros(R, f) for k in ("t0", "t1", "v0", "v1")}
        for n in range(max_steps):
            t_all = t_in + f(n) * dt
            active &= t_all <= t_out
            at = np.nonzero(active)[0]
            if not at.size:
                break
            t = t_all[at]
            _, _, _, obs, v, _ = _sample(f, flat, tsdf, weight, min_weight, og, dg[at], t, variant)
            both = (obs_prev[at] & obs) | (variant == "unobserved_ok" and n >= 1)
            cross = ((v_prev[at] > 0) & (0 >= v)) if variant == "sign" else ((v_prev[at] < 0) & (0 <= v))
            hit = both & cross & (n >= 1)
            h = at[hit]
            r = v_prev[h] / (v_prev[h] - v[hit])
            depth[h] = t_prev[h] + (t[hit] - t_prev[h]) * r
            keep["t0"][h], keep["t1"][h], keep["v0"][h], keep["v1"][h] = t_prev[h], t[hit], v_prev[h], v[hit]
            info["n"][h] = n
            out["code"][h] = HIT
            active[h] = False
            t_prev[at], v_prev[at], obs_prev[at] = t, v, obs
        h = np.nonzero(out["code"] == HIT)[0]
        c, fr, v, obs, _, g = _sample(f, flat, tsdf, weight, min_weight, og, dg[h], depth[h], variant)
        s = [np.minimum(c[:, k] + (0 if variant == "src_floor" else (fr[:, k] >= f(0.5)).astype(np.int64)), res[k] - 1) for k in range(3)]
        out["src"][h] = ((s[2] * res[1] + s[1]) * res[0] + s[0]).astype(np.int32)
        gx = _lerp(_lerp(v[1] - v[0], v[3] - v[2], fr[:, 1]), _lerp(v[5] - v[4], v[7] - v[6], fr[:, 1]), fr[:, 2]) / step[0]
        gy = _lerp(_lerp(v[2] - v[0], v[3] - v[1], fr[:, 0]), _lerp(v[6] - v[4], v[7] - v[5], fr[:, 0]), fr[:, 2]) / step[1]
        gz = _lerp(_lerp(v[4] - v[0], v[5] - v[1], fr[:, 0]), _lerp(v[6] - v[2], v[7] - v[3], fr[:, 0]), fr[:, 1]) / step[2]
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        good = obs & (ln > 0) & (ln <= FMAX)
        sg = f(1.0) if variant == "normal_sign" else f(-1.0)
        nrm = np.stack([(sg * gx) / ln, (sg * gy) / ln, (sg * gz) / ln], -1)
        normal = np.zeros((R, 3), f)
        normal[h] = np.where(good[:, None], nrm, f(0.0))
    info.update(keep, og=np.asarray(og), dg=dg, t_in=t_in, axis=axis, depth=depth, normal=normal, corners=(h, v, g))
    if f is np.float32:
        out["depth"], out["normal"] = depth, normal
    return out, info


def raycast32(view, near, far, lat, tsdf, weight, min_weight=1.0, dt=None, max_steps=None, pix=None, variant=None, info=False):
    """The rule in vectorised numpy float32 (k_tsdf_raycast, bit for bit)."""
    out, inf = _cast(np.float32, view, near, far, lat, tsdf, weight, min_weight, dt, max_steps, pix, variant)
    return (out, inf) if info else out


def raycast64(view, near, far, lat, tsdf, weight, min_weight=1.0, dt=None, max_steps=None, pix=None):
    """The same decisions in float64 on the float32 ray.  Returns (out, info): out's code and src as raycast32's; info holds the
    float64 depth and normal, n = the hit's sample number (-1: none), and what depth_bound needs."""
    return _cast(np.float64, view, near, far, lat, tsdf, weight, min_weight, dt, max_steps, pix, None)


def depth_bound(lat, info, dt=None):
    """For the HIT pixels of raycast64's info: (bound (R) on |depth32 - depth64| where both pick the same crossing, in_doubt (R)).
    With u = 2^-24 and everything evaluated on the float64 run:
      coordinates.  og_k = (o_k - lo_k) / step_k - 0.5 is three roundings of numbers no larger than |og_k| + 0.5:
          e_og_k = 3 u (|og_k| + 0.5);  dg_k = d_k / step_k: u |dg_k|.
      the entry.  t_in is near (exact) or (c - og_k) / dg_k on the axis that sets it: e_in = (e_og_k + u |c - og_k|) / |dg_k|
          + 2 u |t_in| (the subtraction, the divisor's error and the division).
      a sample's parameter.  t_n = t_in + (float)n dt: e_t = e_in + u n dt + u |t_n|.
      its coordinates.  g_k = og_k + t dg_k: e_g_k = e_og_k + |dg_k| e_t + 2 u |t dg_k| + u |g_k|.
      its value.  The interpolant moves by at most D_k = the largest difference of two corners along axis k per unit of g_k, and
          the seven lerps round values no larger than vmax = the largest |corner| three times each:
          e_v = sum_k D_k e_g_k + 21 u vmax.  (D_k and vmax of the cell at t*, which lies between the two samples.)
      the hit.  r = v0 / (v0 - v1): e_r = (|v1| e_v + |v0| e_v) / (v0 - v1)^2 + 3 u |r|;
          t* = t0 + (t1 - t0) r: e = e_t0 + (e_t0 + e_t1 + u dt) |r| + dt e_r + 2 u |t*|.
    The whole is inflated by 1 + 2^-4 for the second-order terms.  in_doubt: a coordinate of one of the two samples within its
    e_g of an integer (the two runs may sit in different cells, whose D and observed flags differ)."""
    lo, step, res = lat
    dt = float(default_dt(step) if dt is None else np.float32(dt))
    h, v, g_star = info["corners"]
    R = len(info["n"])
    bound, doubt = np.zeros(R), np.zeros(R, bool)
    u = U32
    og, dg = info["og"], info["dg"][h]
    e_og = 3 * u * (np.abs(og) + 0.5)
    ax = info["axis"][h]
    t_in = info["t_in"][h]
    e_in = np.zeros(len(h))
    for k in range(3):
        on = ax == k
        num = np.maximum(np.abs(og[k]), np.abs(res[k] - 1 - og[k]))
        with np.errstate(all="ignore"):
            e_in = np.where(on, (e_og[k] + u * num) / np.abs(dg[:, k]) + 2 * u * np.abs(t_in), e_in)
    n = info["n"][h]
    t0, t1, v0, v1 = (info[k][h] for k in ("t0", "t1", "v0", "v1"))
    e_t = lambda t, m: e_in + u * m * dt + u * np.abs(t)
    e_t0, e_t1 = e_t(t0, n - 1), e_t(t1, n)
    V = np.stack(v, -1)                                             # (H, 8), index a + 2 b + 4 c
    vmax = np.abs(V).max(-1)
    pairs = {0: [(0, 1), (2, 3), (4, 5), (6, 7)], 1: [(0, 2), (1, 3), (4, 6), (5, 7)], 2: [(0, 4), (1, 5), (2, 6), (3, 7)]}
    e_v = 21 * u * vmax
    in_doubt = np.zeros(len(h), bool)
    for k in range(3):
        D = np.max([np.abs(V[:, b] - V[:, a]) for a, b in pairs[k]], 0)
        e_g = 0.0
        for t, et in ((t0, e_t0), (t1, e_t1)):
            g = og[k] + t * dg[:, k]
            e_gk = e_og[k] + np.abs(dg[:, k]) * et + 2 * u * np.abs(t * dg[:, k]) + u * np.abs(g)
            in_doubt |= np.abs(g - np.rint(g)) <= INFLATE * e_gk
            e_g = np.maximum(e_g, e_gk)
        e_v = e_v + D * e_g
    r = v0 / (v0 - v1)
    e_r = (np.abs(v1) + np.abs(v0)) * e_v / (v0 - v1) ** 2 + 3 * u * np.abs(r)
    bound[h] = INFLATE * (e_t0 + (e_t0 + e_t1 + u * dt) * np.abs(r) + dt * e_r + 2 * u * np.abs(info["depth"][h]))
    doubt[h] = in_doubt
    return bound, doubt
