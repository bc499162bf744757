"""CPU references of cross-view reprojection (csrc/pnr_warp.hip; the rule is include/pnr.h "cross-view reprojection").

(a) reproject32: the rule in numpy float32, in EXACTLY the kernel's operation order, on _camera_ref.unproject32 /
    _camera_ref.project32 (the fisheye ray and the projection, already pinned bit for bit) plus the two pieces those do not
    have: the pinhole ray and p_cam.z.  k_reproject must equal it bit for bit, counters included.
(b) reproject64: the same rule in float64 on unproject64 / project64.  tests/test_warp_ref.py pins it with closed forms and
    corrupted variants (`variant`) before (a) is measured against it.
(c) chain_bound: a running first-order bound on |float32 - float64| of the chain's u, v and expected depth, per pixel; it
    says which pixels may legitimately decide differently in (a) and (b) (`excluded`).

Views are passed as (model, cam, pose, width, height): model _camera_ref.PINHOLE / FISHEYE, cam the 4 or 7 parameters, pose
the source's c2w or the target's w2c (3, 4).  Maps are flat or (height, width) arrays indexed by the linear pixel index.
"""
import numpy as np

import _camera_ref as cr

PINHOLE, FISHEYE = cr.PINHOLE, cr.FISHEYE
NOTHING, LEFT_VIEW, UNKNOWN, OCCLUDED = -1, -2, -3, -4
VARIANTS = ("depth_swap", "floor", "one_sided", "c2w")        # deliberately WRONG rules (test_warp_ref.py: the checks can fail)
U32 = 2.0 ** -24        # unit roundoff of float32


def pinhole_rays32(cam, c2w, width, height, pix=None):
    """o (3,), d (R, 3) float32 of pnr_pinhole_ray: d = R ((i - cx)/fx, (j - cy)/fy, 1), not normalised"""
    f = np.float32
    fx, fy, cx, cy = (f(v) for v in cam)
    M = np.asarray(c2w, dtype=np.float32).reshape(3, 4)
    i, j = cr.pixel_grid(width, height, pix)
    x = (i.astype(np.float32) - cx) / fx
    y = (j.astype(np.float32) - cy) / fy
    d = np.stack([(M[k, 0] * x + M[k, 1] * y) + M[k, 2] for k in range(3)], -1)
    return M[:, 3].copy(), d.astype(np.float32)


def _flat(a, dtype, n, what):
    if a is None:
        return None
    a = np.asarray(a, dtype=dtype).reshape(-1)
    assert a.size == n, "%s: %d values for %d pixels" % (what, a.size, n)
    return a


def _reproject(dt_, src, depth_src, tgt, depth_tgt, tol, pix, label_src, label_tgt, n_classes, variant):
    f = dt_
    ms, cam_s, c2w, ws, hs = src
    mt, cam_t, w2c, wt, ht = tgt
    assert variant is None or variant in VARIANTS
    if variant == "c2w":                     # the target's camera-to-world used where world-to-camera belongs
        w2c = cr.invert_pose(w2c)
    depth_src = _flat(depth_src, f, ws * hs, "depth_src")
    depth_tgt = _flat(depth_tgt, f, wt * ht, "depth_tgt")
    p = np.arange(ws * hs, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64).reshape(-1)
    R = p.size
    inside_src = (p >= 0) & (p < ws * hs)
    pc = np.where(inside_src, p, 0)
    fmax = np.finfo(np.float32).max
    with np.errstate(all="ignore"):
        # 1: the ray
        if f is np.float32:
            if ms == PINHOLE:
                o, d = pinhole_rays32(cam_s, c2w, ws, hs, pc)
                ok = np.ones(R, bool)
            else:
                rays, valid = cr.unproject32(cam_s, c2w, ws, hs, 0.0, 0.0, pix=pc)
                o, d, ok = np.asarray(c2w, np.float32).reshape(3, 4)[:, 3], rays[:, 3:6], valid != 0
        else:
            M = np.asarray(c2w, np.float64).reshape(3, 4)
            o = M[:, 3]
            if ms == PINHOLE:
                fx, fy, cx, cy = (float(v) for v in cam_s)
                i, j = cr.pixel_grid(ws, hs, pc)
                d = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones(R)], -1) @ M[:, :3].T
                ok = np.ones(R, bool)
            else:
                d, ok, _ = cr.unproject64(cam_s, ws, hs, pix=pc, c2w=c2w)
        # 2: the depth
        t = depth_src[pc]
        have = inside_src & ok & (t > 0) & (np.abs(t) <= fmax)
        t = np.where(have, t, f(1.0)).astype(f)
        # 3: the point
        X = np.stack([o[k] + t * d[:, k] for k in range(3)], -1).astype(f)
        # 4: into the target
        if f is np.float32:
            uv, rng, valid = cr.project32(mt, cam_t, w2c, wt, ht, X)
            Mt = np.asarray(w2c, np.float32).reshape(3, 4)
            z = ((Mt[2, 0] * X[:, 0] + Mt[2, 1] * X[:, 1]) + Mt[2, 2] * X[:, 2]) + Mt[2, 3]
            half = f(0.5)
        else:
            uv, rng, valid = cr.project64(mt, cam_t, w2c, wt, ht, X)
            Mt = np.asarray(w2c, np.float64).reshape(3, 4)
            z = X @ Mt[2, :3] + Mt[2, 3]
            half = 0.5
        valid = valid != 0
        # 5: the nearest pixel
        off = f(0.0) if variant == "floor" else half
        iu = np.minimum(np.floor(np.where(valid, uv[:, 0], 0) + off).astype(np.int64), wt - 1)
        iv = np.minimum(np.floor(np.where(valid, uv[:, 1], 0) + off).astype(np.int64), ht - 1)
        q = iv * wt + iu
        code = np.where(valid, q, LEFT_VIEW)
        # 6: the depth test, in the target's convention
        e = z if (mt == PINHOLE) != (variant == "depth_swap") else rng
        e = e.astype(f)
        dt = thr = None
        if depth_tgt is not None:
            dt = depth_tgt[np.where(valid, q, 0)]
            known = (dt > 0) & (np.abs(dt) <= fmax)
            thr = f(np.float32(tol[0])) + f(np.float32(tol[1])) * e            # the float32 tolerances in both evaluations
            diff = (e - dt) if variant == "one_sided" else np.abs(e - dt)
            code = np.where(valid & ~known, UNKNOWN, code)
            code = np.where(valid & known & ~(diff <= thr), OCCLUDED, code)
        code = np.where(have, code, NOTHING).astype(np.int32)
        uv = np.where(have[:, None], uv, 0).astype(f)
    out = {"match": code, "uv": uv, "have": have, "e": e, "dt": dt, "thr": thr, "rng": rng, "z": z,
           "stats": np.array([(code >= 0).sum()] + [(code == c).sum() for c in (-1, -2, -3, -4)], np.int64)}
    if label_src is not None:
        ls = _flat(label_src, np.int64, ws * hs, "label_src")[pc]
        lt = _flat(label_tgt, np.int64, wt * ht, "label_tgt")[np.maximum(code, 0)]
        use = (code >= 0) & (ls >= 0) & (ls < n_classes) & (lt >= 0) & (lt < n_classes)
        agree = np.zeros((n_classes, n_classes), np.int64)
        np.add.at(agree, (ls[use], lt[use]), 1)
        out["agree"] = agree
    return out


def reproject32(src, depth_src, tgt, depth_tgt=None, tol=(0.0, 0.02), pix=None, label_src=None, label_tgt=None, n_classes=0,
                variant=None):
    """The rule in float32: dict of match (R) int32, uv (R, 2) float32, stats (5) int64, agree (n_classes^2) int64 with labels
    (and the intermediate e, dt, thr, have)."""
    return _reproject(np.float32, src, depth_src, tgt, depth_tgt, tol, pix, label_src, label_tgt, n_classes, variant)


def reproject64(src, depth_src, tgt, depth_tgt=None, tol=(0.0, 0.02), pix=None, label_src=None, label_tgt=None, n_classes=0,
                variant=None):
    return _reproject(np.float64, src, depth_src, tgt, depth_tgt, tol, pix, label_src, label_tgt, n_classes, variant)


# ------------------------------------------------------------------------------------------------ the float32 error of the chain
GUARD = 2.0 ** -8       # no claim where a divisor's or radicand's bound exceeds this share of its magnitude
INFLATE = 1.0 + 2.0 ** -4


class E:
    """A float64 value `v` of the chain with a bound `e` on |float32 value - v|, carried through the chain's own operations
    (a running error analysis, first order in u = 2^-24): with every float32 operation correctly rounded,
        a + b:    e = ea + eb + u |a + b|                 a * b:   e = |a| eb + |b| ea + u |a b|
        a / b:    e = (ea + |a / b| eb) / |b| + u |a / b|   sqrt a:  e = ea / (2 sqrt a) + u sqrt a
    Inputs that are the same float32 numbers in both evaluations (camera words, poses, depth, pixel indices) enter with e = 0.
    The neglected terms are products of two relative errors.  Where a divisor's or radicand's bound exceeds GUARD = 2^-8 of
    its magnitude no claim is made (e = inf); elsewhere each neglected term is below 2^-8 of a kept one (at typical pixels
    2^-18: the relative bounds are tens of u), and `excluded` inflates the bound by INFLATE = 1 + 2^-4 as their allowance.
    Cheap (one array per value) but blind to correlation: an error that enters twice is counted twice, |.| each time."""
    __array_ufunc__ = None          # ndarray (op) E defers to E's reflected operator

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @classmethod
    def of(cls, x):
        return x if isinstance(x, cls) else cls(x)

    def __add__(self, o):
        o = self.of(o)
        v = self.v + o.v
        return E(v, self.e + o.e + U32 * np.abs(v))

    __radd__ = __add__

    def __neg__(self):
        return E(-self.v, self.e)

    def __sub__(self, o):
        return self + (-self.of(o))

    def __rsub__(self, o):
        return self.of(o) + (-self)

    def __mul__(self, o):
        o = self.of(o)
        with np.errstate(all="ignore"):
            v = self.v * o.v
            return E(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U32 * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            e = (self.e + np.abs(v) * o.e) / np.abs(o.v) + U32 * np.abs(v)
            e = np.where(o.e >= GUARD * np.abs(o.v), np.inf, e)
        return E(v, e)

    def sqrt(self):
        with np.errstate(all="ignore"):
            v = np.sqrt(np.maximum(self.v, 0.0))
            e = np.where(self.e > 0, self.e / (2.0 * v), 0.0) + U32 * v
            e = np.where((self.e >= GUARD * np.abs(self.v)) & (self.e > 0), np.inf, e)
        return E(v, e)

    def select(self, cond, other):
        """where(cond, self, the exact constant `other`)"""
        return E(np.where(cond, self.v, other), np.where(cond, self.e, 0.0))

    @staticmethod
    def root(r, f, fp):
        """the Newton fixed point r of f, given f evaluated at the exact r (see ray_chain)"""
        with np.errstate(all="ignore"):
            return E(r, f.e / np.abs(fp) + U32 * np.abs(r))

    def bound(self):
        return self.e


class S:
    """The same first-order bound with the correlations kept: a float64 value `v` and its sensitivity `g[k]` to the rounding
    error of every earlier operation k (forward differentiation with respect to the rounding errors).  Operation k commits an
    absolute error of at most S.src[k] = u |its result|; the float32 value differs from v by sum_k g[k] delta_k to first
    order, so |float32 - v| <= sum_k |g[k]| S.src[k]: the exact first-order worst case, never above E's bound.  About a
    hundred arrays per value: used on the pixels E's bound cannot settle.  One chain at a time (S.src is shared): call
    S.begin() first."""
    __array_ufunc__ = None
    src = []

    @classmethod
    def begin(cls):
        cls.src = []

    def __init__(self, v, g=None):
        self.v = np.asarray(v, np.float64)
        self.g = {} if g is None else g

    @classmethod
    def of(cls, x):
        return x if isinstance(x, cls) else cls(x)

    def _rounded(self):
        S.src.append(U32 * np.abs(self.v))
        self.g[len(S.src) - 1] = 1.0
        return self

    @staticmethod
    def _lin(a, ca, b, cb):
        g = {k: ca * x for k, x in a.items()}
        for k, x in b.items():
            g[k] = g[k] + cb * x if k in g else cb * x
        return g

    def __add__(self, o):
        o = self.of(o)
        return S(self.v + o.v, self._lin(self.g, 1.0, o.g, 1.0))._rounded()

    __radd__ = __add__

    def __neg__(self):
        return S(-self.v, {k: -x for k, x in self.g.items()})

    def __sub__(self, o):
        return self + (-self.of(o))

    def __rsub__(self, o):
        return self.of(o) + (-self)

    def __mul__(self, o):
        o = self.of(o)
        with np.errstate(all="ignore"):
            return S(self.v * o.v, self._lin(self.g, o.v, o.g, self.v))._rounded()

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            return S(v, self._lin(self.g, 1.0 / o.v, o.g, -v / o.v))._rounded()

    def sqrt(self):
        with np.errstate(all="ignore"):
            v = np.sqrt(np.maximum(self.v, 0.0))
            return S(v, {k: x / (2.0 * v) for k, x in self.g.items()})._rounded()

    def select(self, cond, other):
        return S(np.where(cond, self.v, other), {k: np.where(cond, x, 0.0) for k, x in self.g.items()})

    @staticmethod
    def root(r, f, fp):
        with np.errstate(all="ignore"):
            return S(r, {k: -x / fp for k, x in f.g.items()})._rounded()

    def bound(self):
        with np.errstate(all="ignore"):
            b = np.zeros(self.v.shape)
            for k, x in self.g.items():
                b = b + np.abs(x) * S.src[k]
        return b


def ray_chain(N, model, cam, c2w, width, height, pix):
    """(o (3) floats, d (3) N, disc) of the source ray in the number class N (E or S), in the kernel's operation order.
    Fisheye: the float32 Newton iterate is a fixed point of r <- r - f(r) / f'(r) (tests/test_camera_ref.py: the float32 floor
    is reached from 4 of the 8 steps on).  With e_n the error of r_n against the root of the exact f, the float32 step gives
        r_(n+1) - root = e_n - (e_n + df / f')(1 + eta) + rounding = -df / f' + rounding + (second order),
    where df is the error of EVALUATING f = r ((1 + k1 r^2) + k2 r^4) - rd at r_n -- its own roundings with r taken as exact,
    and the error rd carries -- and eta (a few u, and Newton's contraction f'' e_n / f') multiplies errors only.  So the
    iterate's error is that of f at the exact r, divided by -f', plus the rounding u |r| of the last subtraction: N.root."""
    M = np.asarray(c2w, np.float64).reshape(3, 4).tolist()          # python floats: float (op) N defers to N
    i, j = cr.pixel_grid(width, height, pix)
    i, j = i.astype(np.float64), j.astype(np.float64)
    o = [M[k][3] for k in range(3)]
    if model == PINHOLE:
        fx, fy, cx, cy = (float(v) for v in cam)
        x, y = (N(i) - cx) / fx, (N(j) - cy) / fy
        return o, [(M[k][0] * x + M[k][1] * y) + M[k][2] for k in range(3)], None
    xi, k1, k2, g1, g2, u0, v0 = (float(v) for v in cam)
    x, y = (N(i) - u0) / g1, (N(j) - v0) / g2
    rd = (x * x + y * y).sqrt()
    r = cr.undistort64(cam, rd.v)
    re = N(r)                                               # r as an exact input of f
    r2 = re * re
    f = re * ((1.0 + k1 * r2) + k2 * (r2 * r2)) - rd
    fp = 1.0 + 3.0 * k1 * r * r + 5.0 * k2 * r ** 4
    sc = (N.root(r, f, fp) / rd).select(rd.v > 0, 1.0)
    x, y = x * sc, y * sc
    r2 = x * x + y * y
    disc = 1.0 + (1.0 - N(xi) * xi) * r2
    lam = (xi + disc.sqrt()) / (r2 + 1.0)
    dc = [lam * x, lam * y, lam - xi]
    return o, [(M[k][0] * dc[0] + M[k][1] * dc[1]) + M[k][2] * dc[2] for k in range(3)], disc


def chain(N, src, depth_src, tgt, pix):
    """(u + 0.5, v + 0.5, e, signs) of the whole chain in the number class N; signs: the values whose sign decides validity
    (the lens rim's disc, the projection's domain) -- where one of them is not clear of zero the decision itself may differ."""
    ms, cam_s, c2w, ws, hs = src
    mt, cam_t, w2c, wt, ht = tgt
    o, d, disc = ray_chain(N, ms, cam_s, c2w, ws, hs, pix)
    t = np.asarray(depth_src, np.float64).reshape(-1)[pix]
    with np.errstate(all="ignore"):
        t = np.where((t > 0) & np.isfinite(t), t, 1.0)
        X = [o[k] + t * d[k] for k in range(3)]
        Mt = np.asarray(w2c, np.float64).reshape(3, 4).tolist()
        pc = [((Mt[k][0] * X[0] + Mt[k][1] * X[1]) + Mt[k][2] * X[2]) + Mt[k][3] for k in range(3)]
        rng = ((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]).sqrt()
        if mt == PINHOLE:
            fx, fy, cx, cy = (float(v) for v in cam_t)
            u = fx * (pc[0] / pc[2]) + cx
            v = fy * (pc[1] / pc[2]) + cy
            e, signs = pc[2], [pc[2]]
        else:
            xi, k1, k2, g1, g2, u0, v0 = (float(v) for v in cam_t)
            xs, ys, zs = pc[0] / rng, pc[1] / rng, pc[2] / rng
            den = zs + xi
            x, y = xs / den, ys / den
            r2 = x * x + y * y
            s = (1.0 + k1 * r2) + k2 * (r2 * r2)
            u = (g1 * x) * s + u0
            v = (g2 * y) * s + v0
            e, signs = rng, [den, xi * zs + 1.0]
        return u + 0.5, v + 0.5, e, signs + ([disc] if disc is not None else [])


def chain_bound(src, depth_src, tgt, pix=None, N=E, rough=None):
    """Per source pixel: bounds (du, dv, de) on |float32 - float64| of u + 0.5, v + 0.5 (the addition included) and of the
    expected depth e.  inf where a decision before them (the lens rim, the projection's domain) may already differ, 0 where
    the point is clearly outside the domain (both evaluations leave the view; nothing more is decided).  N = S: the tight
    bound; `rough` = E's (du, dv, de) for the same pixels supplies the inf / 0 flags."""
    ws, hs = src[3], src[4]
    pix = np.arange(ws * hs, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64).reshape(-1)
    if N is S:
        S.begin()
    u, v, e, signs = chain(N, src, depth_src, tgt, pix)
    with np.errstate(all="ignore"):
        out = [a.bound() for a in (u, v, e)]
        if N is E:
            edge = np.zeros(pix.shape, bool)
            dom = np.ones(pix.shape, bool)
            for sgn in signs:
                edge |= ~(sgn.e < GUARD * np.abs(sgn.v))
            for sgn in signs[: 1 if tgt[0] == PINHOLE else 2]:
                dom &= sgn.v > 0
            return tuple(np.where(edge, np.inf, np.where(dom, b, 0.0)) for b in out)
        flag = [np.isfinite(r) & (r > 0) for r in rough]
        return tuple(np.where(fl, np.minimum(b, r), r) for b, r, fl in zip(out, rough, flag))


def near_decision(ref64, tgt, tol, du, dv, de, inflate=INFLATE):
    """Pixels (of those float64 can reproject) where float32 may legitimately decide differently under the bounds given:
    u + 0.5 or v + 0.5 of the float64 evaluation lies within its bound of an integer (the nearest pixel, and the image border
    at 0 / width / height, are decided there), or |e - dt| lies within its bound of the threshold -- the depth test's own
    float32 roundings (e - dt, tol_rel * e, the sum: u times each value) added."""
    mt, _, _, wt, ht = tgt
    uv = ref64["uv"]
    with np.errstate(all="ignore"):
        out = np.zeros(len(uv), bool)
        for k, dk in ((0, du), (1, dv)):
            a = uv[:, k] + 0.5
            out |= ~(np.abs(a - np.round(a)) > inflate * dk)
        # far outside the image nothing is decided at the other integers; a non-finite bound still excludes
        out &= ((uv[:, 0] > -1.0) & (uv[:, 0] < wt) & (uv[:, 1] > -1.0) & (uv[:, 1] < ht)) | ~np.isfinite(du) | ~np.isfinite(dv)
        if ref64["dt"] is not None:
            e, dt, thr = ref64["e"], ref64["dt"], ref64["thr"]
            diff = np.abs(e - dt)
            margin = de * (1.0 + tol[1]) + U32 * (diff + np.abs(tol[1] * e) + np.abs(thr))
            out |= (ref64["match"] != LEFT_VIEW) & np.isfinite(dt) & (dt > 0) & ~(np.abs(diff - thr) > inflate * margin)
    return out & ref64["have"]


def excluded(ref64, src, depth_src, tgt, tol, pix=None):
    """The excluded set of a float32-against-float64 comparison, in two passes: E's cheap bound on every pixel, then S's exact
    first-order bound on the pixels the first pass could not clear.  Returns (excluded (R) bool, E's du)."""
    ws, hs = src[3], src[4]
    pix = np.arange(ws * hs, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64).reshape(-1)
    rough = chain_bound(src, depth_src, tgt, pix)
    out = near_decision(ref64, tgt, tol, *rough)
    k = np.flatnonzero(out)
    for a in range(0, k.size, 65536):                      # S carries ~100 arrays per value: in pieces
        kk = k[a:a + 65536]
        tight = chain_bound(src, depth_src, tgt, pix[kk], N=S, rough=[r[kk] for r in rough])
        sub = {key: (val[kk] if isinstance(val, np.ndarray) and val.shape[:1] == out.shape else val) for key, val in ref64.items()}
        out[kk] = near_decision(sub, tgt, tol, *tight)
    return out, rough[0]


# ------------------------------------------------------------------------------------------------ analytic scenes
def sphere_depth(model, cam, c2w, width, height, centre, radius):
    """(height, width) float32 depth image of a camera INSIDE a sphere, in the model's own convention (pinhole: z-depth,
    i.e. the parameter of the z_cam = 1 ray; fisheye: range along the unit ray); 0 outside the lens.  Smooth and analytic."""
    M = np.asarray(c2w, np.float64).reshape(3, 4)
    if model == PINHOLE:
        fx, fy, cx, cy = (float(v) for v in cam)
        i, j = cr.pixel_grid(width, height)
        d = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones(i.size)], -1) @ M[:, :3].T
        ok = np.ones(i.size, bool)
    else:
        d, ok, _ = cr.unproject64(cam, width, height, c2w=c2w)
    oc = M[:, 3] - np.asarray(centre, np.float64)
    a, b, c = (d * d).sum(-1), d @ oc, oc @ oc - radius * radius
    assert c < 0, "the camera must stand inside the sphere"
    with np.errstate(all="ignore"):
        t = (-b + np.sqrt(b * b - a * c)) / a
    return np.where(ok, t, 0.0).astype(np.float32).reshape(height, width)
