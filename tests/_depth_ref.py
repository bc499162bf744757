"""CPU references of the depth front end (csrc/pnr_depth.hip; the rule is include/pnr.h "depth front end").

(a) filter_loops / normals_loops: each rule per pixel as plain Python loops on numpy.float32 scalars -- the text of the header.
(b) filter32 / normals32: the same in vectorised numpy float32, in the rule's operation order.  k_depth_filter and k_depth_normals
    must equal them bit for bit.  The ray comes from the CPU restatements of the three camera models (_pano_ref._rays), which are
    pinned bit for bit against the ray kernels.  `variant`: deliberately WRONG rules (test_depth_ref.py: its checks can fail).
(c) filter64 / normals64: the same decisions in float64 on the same float32 inputs, and `excluded`: the pixels where the float32
    normals may legitimately get another code, from a running first-order error bound (_warp_ref.E) carried through the rule's own
    operations, as _icp_ref.excluded does.
(d) view / odometry: depth.view and fusion.odometry restated on (a)-(c) and _icp_ref.track.

A view is _icp_ref's (model, cam, c2w (3, 4), width, height); images are (height, width) float32 numpy.
"""
import math

import numpy as np

import _icp_ref as ir
import _pano_ref as pr
import _warp_ref as wr

OK, NO_DEPTH, NO_NEIGHBOUR, DEGENERATE, GRAZING = 0, 1, 2, 3, 4
CODES = {"OK": OK, "NO_DEPTH": NO_DEPTH, "NO_NEIGHBOUR": NO_NEIGHBOUR, "DEGENERATE": DEGENERATE, "GRAZING": GRAZING}
MAX_RADIUS = 8
# order: the window summed column-major;  gate: a neighbour is used with u >= 0;  support: the count leaves out the centre;
# sign: the normal is never flipped;  world: differences of vertex = o + v;  onesided: never the central difference
FILTER_VARIANTS, NORMALS_VARIANTS = ("order", "gate", "support"), ("sign", "world", "onesided")
VARIANTS = FILTER_VARIANTS + NORMALS_VARIANTS
FMAX = np.finfo(np.float32).max
U32, INFLATE, E = wr.U32, wr.INFLATE, wr.E
FILTER_DEFAULTS = dict(radius=3, sigma_space=1.5, sigma_range=(0.0, 0.03), min_support=1)
NORMALS_DEFAULTS = dict(jump=(0.0, 0.05), min_cos=0.1)


def spatial_weights(radius, sigma_space):
    """g[0 .. radius] float32: exp(-k^2 / (2 sigma_space^2)) in float64, rounded once (ops.depth_filter_params)"""
    return np.array([math.exp(-(k * k) / (2.0 * float(sigma_space) * float(sigma_space))) for k in range(radius + 1)], np.float64).astype(np.float32)


def _valid(t):
    return (t > 0) & (np.abs(t) <= FMAX)


def _window(radius, variant):
    offs = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    if variant == "order":
        offs = [(dy, dx) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1)]
    return offs


# ------------------------------------------------------------------------------------------------ the filter
def filter_loops(depth, radius=3, sigma_space=1.5, sigma_range=(0.0, 0.03), min_support=1, variant=None):
    """the rule per pixel on numpy.float32 scalars: (out float32, support int16), (height, width) each"""
    assert variant is None or variant in FILTER_VARIANTS
    f = np.float32
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    g = spatial_weights(radius, sigma_space)
    sa, sb = f(sigma_range[0]), f(sigma_range[1])
    out, sup = np.zeros((h, w), np.float32), np.zeros((h, w), np.int16)
    with np.errstate(all="ignore"):
        for j in range(h):
            for i in range(w):
                c = depth[j, i]
                if not (c > f(0) and c <= FMAX):                                               # 1
                    continue
                sigma = sa + sb * c                                                            # 2
                acc, ws, count = f(0), f(0), 0
                for dy, dx in _window(radius, variant):                                        # 3
                    jj, ii = j + dy, i + dx
                    if not (0 <= jj < h and 0 <= ii < w):
                        continue
                    t = depth[jj, ii]
                    if not (t > f(0) and t <= FMAX):
                        continue
                    x = (t - c) / sigma
                    u = f(1) - x * x
                    if not ((u >= f(0)) if variant == "gate" else (u > f(0))):
                        continue
                    wgt = (g[abs(dy)] * g[abs(dx)]) * (u * u)
                    acc = acc + wgt * t
                    ws = ws + wgt
                    if not (variant == "support" and dy == 0 and dx == 0):
                        count += 1
                if count >= min_support:                                                       # 4
                    out[j, i] = acc / ws
                sup[j, i] = count
    return out, sup


def _filter(f, depth, radius, sigma_space, sigma_range, min_support, variant):
    assert variant is None or variant in FILTER_VARIANTS
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    g = spatial_weights(radius, sigma_space).astype(f)
    sa, sb = f(np.float32(sigma_range[0])), f(np.float32(sigma_range[1]))
    r = radius
    pad = np.zeros((h + 2 * r, w + 2 * r), f)                      # beyond the image: 0, which is no valid depth
    pad[r:r + h, r:r + w] = depth.astype(f)
    c = depth.astype(f)
    with np.errstate(all="ignore"):
        cv = _valid(c)
        sigma = (sa + sb * c).astype(f)
        acc, ws, count = np.zeros((h, w), f), np.zeros((h, w), f), np.zeros((h, w), np.int64)
        for dy, dx in _window(r, variant):
            t = pad[r + dy:r + dy + h, r + dx:r + dx + w]
            x = ((t - c) / sigma).astype(f)
            u = (f(1) - x * x).astype(f)
            used = cv & _valid(t) & ((u >= 0) if variant == "gate" else (u > 0))
            wgt = ((g[abs(dy)] * g[abs(dx)]) * (u * u)).astype(f)
            acc = np.where(used, acc + wgt * t, acc).astype(f)
            ws = np.where(used, ws + wgt, ws).astype(f)
            if not (variant == "support" and dy == 0 and dx == 0):
                count = count + used
        out = np.where(cv & (count >= min_support), acc / ws, 0).astype(f)
    return out, np.where(cv, count, 0).astype(np.int16)


def filter32(depth, radius=3, sigma_space=1.5, sigma_range=(0.0, 0.03), min_support=1, variant=None):
    """the rule in vectorised float32 (k_depth_filter, bit for bit): (out float32, support int16)"""
    return _filter(np.float32, depth, radius, sigma_space, sigma_range, min_support, variant)


def filter64(depth, radius=3, sigma_space=1.5, sigma_range=(0.0, 0.03), min_support=1, variant=None):
    """the same in float64 on the same float32 inputs and float32 weights"""
    return _filter(np.float64, depth, radius, sigma_space, sigma_range, min_support, variant)


# ------------------------------------------------------------------------------------------------ the normals
def _scalars(f, jump, min_cos):
    """jump_a, jump_b and mc2 as the entry point receives them: float32 roundings of the host's doubles"""
    return f(np.float32(jump[0])), f(np.float32(jump[1])), f(np.float32(float(min_cos) * float(min_cos)))


def normals_loops(view, depth, jump=(0.0, 0.05), min_cos=0.1, variant=None):
    """the rule per pixel on numpy.float32 scalars: dict of normal (R, 3), vertex (R, 3) float32 and code uint8"""
    assert variant is None or variant in NORMALS_VARIANTS
    f = np.float32
    m, cam, c2w, w, h = view
    R = w * h
    depth = np.asarray(depth, np.float32).reshape(-1)
    ja, jb, mc2 = _scalars(f, jump, min_cos)
    out = {"normal": np.zeros((R, 3), np.float32), "vertex": np.zeros((R, 3), np.float32), "code": np.full(R, NO_DEPTH, np.uint8)}
    with np.errstate(all="ignore"):
        o, d_all, ok_all = pr._rays(np.float32, view, np.arange(R, dtype=np.int64))
        o = [f(o[k]) for k in range(3)]
        have = lambda q: bool(ok_all[q]) and depth[q] > f(0) and depth[q] <= FMAX
        vec = lambda q: [depth[q] * d_all[q, k] for k in range(3)]
        for j in range(h):
            for i in range(w):
                q = j * w + i
                if not have(q):                                                                # 1
                    continue
                t, v = depth[q], vec(q)
                vertex = [o[k] + v[k] for k in range(3)]
                out["vertex"][q] = vertex
                thr = ja + jb * t
                D, missing = [], False
                for (di, dj) in ((1, 0), (0, 1)):                                              # 2, 3
                    side = []
                    for sgn in (-1, 1):
                        ii, jj = i + sgn * di, j + sgn * dj
                        qq = jj * w + ii
                        usable = 0 <= ii < w and 0 <= jj < h and have(qq) and np.abs(depth[qq] - t) <= thr
                        if not usable:
                            side.append(None)
                        elif variant == "world":
                            side.append([o[k] + depth[qq] * d_all[qq, k] for k in range(3)])
                        else:
                            side.append(vec(qq))
                    here = vertex if variant == "world" else v
                    lo, hi = side
                    if lo is None and hi is None:
                        missing = True
                        D.append([f(0)] * 3)
                        continue
                    if variant == "onesided" and lo is not None and hi is not None:
                        lo = None
                    lo, hi = (here if lo is None else lo), (here if hi is None else hi)
                    D.append([hi[k] - lo[k] for k in range(3)])
                out["code"][q] = NO_NEIGHBOUR
                if missing:
                    continue
                (ax, ay, az), (bx, by, bz) = D                                                 # 4
                c = [ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx]
                cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                ln = np.sqrt(cc)
                out["code"][q] = DEGENERATE
                if not (ln > f(0) and ln <= FMAX):
                    continue
                s = (c[0] * v[0] + c[1] * v[1]) + c[2] * v[2]                                  # 5
                vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                out["code"][q] = GRAZING
                if s * s < (mc2 * cc) * vv:
                    continue
                out["code"][q] = OK                                                            # 6
                n = [c[k] / ln for k in range(3)]
                if s > f(0) and variant != "sign":
                    n = [-x for x in n]
                out["normal"][q] = n
    return out


def _shift(a, di, dj, fill):
    """a[j + dj, i + di] per pixel (i, j) of an (h, w, ...) array, `fill` beyond the image"""
    out = np.full_like(a, fill)
    h, w = a.shape[:2]
    src = a[max(dj, 0):h + min(dj, 0), max(di, 0):w + min(di, 0)]
    out[max(-dj, 0):h + min(-dj, 0), max(-di, 0):w + min(-di, 0)] = src
    return out


def _normals(f, view, depth, jump, min_cos, variant):
    assert variant is None or variant in NORMALS_VARIANTS
    m, cam, c2w, w, h = view
    R = w * h
    depth = np.asarray(depth, np.float32).reshape(h, w).astype(f)
    ja, jb, mc2 = _scalars(f, jump, min_cos)
    with np.errstate(all="ignore"):
        o, d, ok = pr._rays(f, view, np.arange(R, dtype=np.int64))
        o = np.asarray(o, np.float32).astype(f) if f is np.float32 else np.asarray(c2w, np.float32).astype(f).reshape(3, 4)[:, 3]
        d = np.asarray(d, f).reshape(h, w, 3)
        have = np.asarray(ok, bool).reshape(h, w) & _valid(depth)                              # 1
        t = np.where(have, depth, 0).astype(f)
        v = np.where(have[..., None], t[..., None] * d, 0).astype(f)
        vertex = np.where(have[..., None], o + v, 0).astype(f)
        thr = (ja + jb * t).astype(f)
        arm = vertex if variant == "world" else v
        D, both_missing, used = [], np.zeros((h, w), bool), []
        for (di, dj) in ((1, 0), (0, 1)):                                                      # 2, 3
            side = []
            for sgn in (-1, 1):
                hv, tn, an = _shift(have, sgn * di, sgn * dj, False), _shift(t, sgn * di, sgn * dj, 0), _shift(arm, sgn * di, sgn * dj, 0)
                usable = have & hv & (np.abs(tn - t) <= thr)
                side.append((usable, an))
                used.append(usable)
            (ul, al), (uh, ah) = side
            both_missing |= ~(ul | uh)
            if variant == "onesided":
                ul = ul & ~uh
            lo, hi = np.where(ul[..., None], al, arm), np.where(uh[..., None], ah, arm)
            D.append((hi - lo).astype(f))
        a, b = D                                                                               # 4
        c = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f)
        cc = ((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]).astype(f)
        ln = np.sqrt(cc).astype(f)
        s = ((c[..., 0] * v[..., 0] + c[..., 1] * v[..., 1]) + c[..., 2] * v[..., 2]).astype(f)   # 5
        vv = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(f)
        lhs, rhs = (s * s).astype(f), ((mc2 * cc) * vv).astype(f)
        near = have & ~both_missing
        solid = near & (ln > 0) & (np.abs(ln) <= FMAX)
        good = solid & ~(lhs < rhs)
        n = (c / ln[..., None]).astype(f)                                                      # 6
        if variant != "sign":
            n = np.where((s > 0)[..., None], -n, n)
    code = np.full((h, w), NO_DEPTH, np.uint8)
    code[have] = NO_NEIGHBOUR
    code[near] = DEGENERATE
    code[solid] = GRAZING
    code[good] = OK
    return {"normal": np.where(good[..., None], n, 0).astype(f).reshape(R, 3), "vertex": vertex.reshape(R, 3), "code": code.reshape(R),
            "have": have.reshape(R), "near": near.reshape(R), "solid": solid.reshape(R), "used": [u.reshape(R) for u in used], "s": s.reshape(R)}


def normals32(view, depth, jump=(0.0, 0.05), min_cos=0.1, variant=None):
    """the rule in vectorised float32 (k_depth_normals, bit for bit): normal, vertex, code and the intermediates"""
    return _normals(np.float32, view, depth, jump, min_cos, variant)


def normals64(view, depth, jump=(0.0, 0.05), min_cos=0.1, variant=None):
    """the same decisions in float64 on the same float32 inputs"""
    return _normals(np.float64, view, depth, jump, min_cos, variant)


# ------------------------------------------------------------------------------------------------ (c) where float32 may differ
def excluded(ref64, view, depth, jump=(0.0, 0.05), min_cos=0.1):
    """(R) bool: the pixels where the float32 rule may legitimately give another code than normals64's result `ref64`.  A bound on
    |float32 - float64| (first order in u = 2^-24, _warp_ref.E's rules, inflated by INFLATE) is carried through this rule's own
    operations; a pixel is excluded where a value that decides lies within its bound of its threshold: the lens rim (the ray's
    signs) of the pixel or of a neighbour, |t_nb - t| against the jump threshold, cc against 0, and s s against (mc2 cc) vv.  The
    decisions on a stored depth alone are the same in both."""
    m, cam, c2w, w, h = view
    R = w * h
    pix = np.arange(R, dtype=np.int64)
    ja, jb, mc2 = (float(x) for x in _scalars(np.float32, jump, min_cos))
    img = lambda x: np.asarray(x).reshape(h, w)
    with np.errstate(all="ignore"):
        _, d, signs = pr.ray_chain(view, pix)
        rim = np.zeros(R, bool)
        for sgn in signs:
            rim |= ~(sgn.e < wr.GUARD * np.abs(sgn.v))
        rim = img(rim)
        have = img(ref64["have"])
        t = np.where(have, np.asarray(depth, np.float64).reshape(h, w), 1.0)
        v = [E(t) * E(img(d[k].v), img(d[k].e)) for k in range(3)]
        thr = E(ja) + E(jb) * E(t)
        out = rim.copy()
        D = []
        k = 0
        for (di, dj) in ((1, 0), (0, 1)):
            side = []
            for sgn in (-1, 1):
                inside = _shift(np.ones((h, w), bool), sgn * di, sgn * dj, False)
                hv, tn = _shift(have, sgn * di, sgn * dj, False), _shift(t, sgn * di, sgn * dj, 1.0)
                out |= have & inside & _shift(rim, sgn * di, sgn * dj, False)
                diff = E(tn) - E(t)
                out |= have & hv & ~(np.abs(np.abs(diff.v) - thr.v) > INFLATE * (diff.e + thr.e))
                usable = img(ref64["used"][k])
                k += 1
                side.append((usable, [E(_shift(c.v, sgn * di, sgn * dj, 0.0), _shift(np.array(c.e), sgn * di, sgn * dj, 0.0)) for c in v]))
            (ul, al), (uh, ah) = side
            lo = [E(np.where(ul, al[c].v, v[c].v), np.where(ul, al[c].e, v[c].e)) for c in range(3)]
            hi = [E(np.where(uh, ah[c].v, v[c].v), np.where(uh, ah[c].e, v[c].e)) for c in range(3)]
            D.append([hi[c] - lo[c] for c in range(3)])
        a, b = D
        c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        near = img(ref64["near"])
        out |= near & ~(cc.v > INFLATE * cc.e)
        s = (c[0] * v[0] + c[1] * v[1]) + c[2] * v[2]
        vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        lhs, rhs = s * s, (E(mc2) * cc) * vv
        out |= near & ~(np.abs(lhs.v - rhs.v) > INFLATE * (lhs.e + rhs.e))
    return (out & have).reshape(R)


# ------------------------------------------------------------------------------------------------ (d) depth.view, fusion.odometry
def view_maps(view, depth, filter=None, f=np.float32, **normals_args):
    """depth.view restated: (the filtered depth (h, w) float32, the normals' dict).  With f = float64 the NORMALS are the float64
    restatement's; the filtered image is the float32 one either way (it is the data both see)."""
    m, cam, c2w, w, h = view
    depth = np.asarray(depth, np.float32).reshape(h, w)
    if filter is not None:
        depth = filter32(depth, **dict(FILTER_DEFAULTS, **filter))[0]
    return depth, _normals(f, view, depth, normals_args.get("jump", (0.0, 0.05)), normals_args.get("min_cos", 0.1), None)


def compose(a, b):
    """fusion._compose: a o b of two (3, 4) float64 poses, in its operation order"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = (a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :]) + a[:, 2:3] * b[2:3, :]
    return np.concatenate([out[:, :3], out[:, 3:] + a[:, 3:]], 1)


def odometry(camera, depths, c2w0=None, filter=None, guess="identity", iters=10, dist_max=0.25, grid=None, f=np.float32, w2c=None, **solve_args):
    """fusion.odometry restated on view_maps and _icp_ref.track: (poses (F, 3, 4) float32, relative (F - 1, 3, 4) float32,
    history (F - 1, iters + 1, 5)).  grid: the accumulate's workgroups on the device (None: math.fsum per column); w2c: the
    model views' world-to-camera as the package inverts the identity (None: _icp_ref's own)"""
    live = ir.live_of(camera)
    model = ir.model_of(camera, ir.IDENTITY)
    views = [view_maps(model, d, filter, f) for d in depths]
    first = np.eye(4)[:3] if c2w0 is None else np.asarray(c2w0, np.float32).reshape(-1)[:12].reshape(3, 4).astype(np.float64)
    absolute, relative, history = [first], [], []
    start = ir.IDENTITY.reshape(12).copy()
    for k in range(1, len(views)):
        dm, nm = views[k - 1]
        pose, hist, _, _ = ir.track(live, views[k][0], start, model, dm, nm["normal"].astype(np.float32), iters, dist_max, grid=grid, f=f, w2c=w2c, **solve_args)
        rel = np.asarray(pose, np.float32).reshape(3, 4)
        relative.append(rel)
        history.append(hist)
        absolute.append(compose(absolute[-1], rel.astype(np.float64)))
        if guess == "velocity":
            start = rel.reshape(12).copy()
    return np.stack(absolute).astype(np.float32), np.asarray(relative, np.float32).reshape(-1, 3, 4), np.asarray(history, np.float64).reshape(-1, iters + 1, 5)


# ------------------------------------------------------------------------------------------------ inputs the tests share
STEP = (np.array([0.008, -0.022, 0.004]), np.array([0.05, -0.02, 0.036]))      # between frames of a sequence: 1.4 degrees, 6.5 cm


def dirty(depth, seed, share=16):
    """a copy with one pixel in `share` replaced by 0, a negative, NaN or Inf in turn"""
    depth = np.array(depth, np.float32)
    flat = depth.reshape(-1)
    g = np.random.default_rng(seed)
    k = max(flat.size // share, min(flat.size, 4) if flat.size > 1 else 0)
    if k:
        flat[g.choice(flat.size, k, replace=False)] = np.resize(np.array([0.0, -1.5, np.nan, np.inf], np.float32), k)
    return depth


def noisy(depth, seed, rel=0.005, speckle=0):
    """multiplicative Gaussian noise of relative sigma `rel` on the valid pixels, and `speckle` isolated wrong pixels"""
    g = np.random.default_rng(seed)
    depth = np.asarray(depth, np.float32)
    out = np.where(depth > 0, depth * (1.0 + rel * g.standard_normal(depth.shape)), 0).astype(np.float32)
    if speckle:
        flat = out.reshape(-1)
        flat[g.choice(flat.size, speckle, replace=False)] *= np.float32(1.6)
    return out


def room_sequence(camera, n):
    """(truths, depths): n float32 poses that move by STEP from _icp_ref.TRUE_POSE, and the room's exact depth image at each"""
    base = np.asarray(ir.TRUE_POSE, np.float32)
    truths = [ir.perturbed(base, STEP[0] * k, STEP[1] * k).astype(np.float32) for k in range(n)]
    return truths, [ir.room_maps(camera, t)[0] for t in truths]


def angles(normal, truth, mask):
    """degrees between two (R, 3) fields of unit normals on the pixels of `mask`, float64"""
    a, b = np.asarray(normal, np.float64).reshape(-1, 3)[mask], np.asarray(truth, np.float64).reshape(-1, 3)[mask]
    return np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))
