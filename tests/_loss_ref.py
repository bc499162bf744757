"""Float64 reference of the loss wrapper (pnr_losses, pnr_ce3d), its float32 restatement in the kernels' op
order, the per-element bounds, and the case list shared by tests/test_loss_ref.py (CPU) and tests/test_gpu_loss_sweep.py (GPU).

losses64 / ce3d64 are written from the contract in include/pnr.h 8f-1 with closed-form gradients (plain numpy, no autograd);
tests/test_loss_ref.py pins them against the torch oracle run in float64, finite differences and hand-made answers.  Labels
outside [0, n) are "ignored"; a target depth that is not > 0 (0, -0.0, negative, NaN) is "no depth".  The loss weights and
fix_eps cross the ABI as floats, so the reference rounds them to float32 first: they are inputs, not arithmetic.

losses32 / ce3d32 restate the kernels in numpy float32, in their op order: inside a ray the 16 lanes' strided partial sums and
the xor butterfly 8, 4, 2, 1; across rays the 16 rays of a block in order, k_loss_final's lane-strided walk and its 64-lane
butterfly; for ce3d the online log-sum-exp with its two branches, the wave butterfly, the 4 waves in order and the final in
double.  They show what float32 rounding alone costs; numpy's expf / logf are not the device's, so nothing compares them with
the GPU bit for bit.  `reassoc=False` forms the cross-entropy as (mx + log den) - x_label, the order the kernels had before the
value was made invariant under a common shift of the logits.

Bounds.  Every bound is k * u * cond with u = 2^-24, cond computed per element from the float64 reference, and k one small
integer per quantity (K below; how it is fixed is in the docstring of test_gpu_loss_sweep.py).  The conditions:

  ce_ray     per-ray cross-entropy v = log den + (mx - x_label):  max(1, v).  v is a sum of log den in [0, log n] (absolute
             error a few u from the sum and logf) and of mx - x_label, one rounding of an exact difference; neither depends
             on a common shift of the row, so the condition does not either.
  ce_grad    s (p_c - [c = label]), s = |w| / n:  s (p_c (1 + |x_c - mx|) + [c = label]).  p_c = exp(x_c - mx) / den carries
             the rounding of its argument (u |x_c - mx|, relative to p_c) and a few u from expf, den and the division; the
             subtraction from 1 rounds at the size of the result, at most s.  Plus s 2^-126 absolute: a p_c below float32's
             smallest normal number may be flushed to zero.
  nll_ray    -log(p + eps):  max(1, |log(p + eps)|)  (p + eps rounds by u relative, which moves the log by u; logf by u |log|).
  nll_grad   -w / ((p + eps) n):  |g|  (three roundings, all relative).
  rgb_ray    sum of three squares of one-rounding differences:  the value (relative).
  rgb_grad   k (rgb - rgb_gt):  |g|.
  depth_ray  |d| or d^2 with d one rounding of a difference:  the value.
  depth_grad depth_l2: 2 w d / n_d:  |g|.  L1: +-fl(w / n_d) or 0, compared BIT FOR BIT with numpy float32 -- that is how
             the count n_d is verified exactly (the kernel does not return it).  A fixed-field (or probability-map) entry with
             fl(p + eps) == 1 has the gradient -fl(w / n) exactly and is compared bit for bit in the same way: the label counts.
  a mean     the mean of its rays' bounds, plus k_sum * u * mean |per-ray value|, with k_sum = the number of float32 roundings
             on the longest path of the reduction (up to 15 in the block, the lane's walk over ceil(blocks / 64) partials, up
             to 6 butterfly steps; an addition to an exact zero does not round, so one ray alone has none) + 1 for the
             division: the plain worst-case bound of a fixed-order sum.
  ce3d       per sample as ce_ray (k_ce3d adds the n terms of den one after the other where ce_row's 16 lanes split them, so
             its error grows with n and its k is larger); its mean as above with k_sum <= 10 (up to 6 butterfly steps, 3 waves, the rounding of the
             double mean to float; the final sum is in double).
  total      sum |w_x| * bound_x + 8 u sum |w_x term_x|  (six products, six additions).

No bound is looser than the bars of test_gpu_losses.py: 2e-5 * max(1, |term|) for a value, 1e-6 + 2e-5 * max |ref| over a
gradient map -- `violations` caps every bound by them."""
import zlib

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126             # float32's smallest normal number: below it expf may flush to zero
F32 = np.float32
KEYS = ("rgb", "depth", "semantic", "fix_semantic", "instance", "fix_instance")
WEIGHTS = {"rgb": 1.0, "depth": 0.1, "semantic": 0.7, "fix_semantic": 0.3, "instance": 0.5, "fix_instance": 0.2}
FIX_EPS = 1e-5
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
OFFSETS = (0.0, 80.0, -80.0, 1e3, -1e3, 3e4)
LS_RAYS, LS_THREADS = 16, 256

# k per quantity = max(4, ceil(4 * rho)), rho = the worst error / (u * cond) of losses32 / ce3d32 and of the float32 torch graph
# against float64 over loss_cases() and ce3d_cases(); test_loss_ref.py::test_float32_restatements_sit_at_a_quarter_of_the_bounds
# keeps it true.  The table with rho is in the docstring of test_gpu_loss_sweep.py.
K = {"ce_ray": 13, "ce_grad": 26, "nll_ray": 10, "nll_grad": 11, "rgb_ray": 17, "rgb_grad": 12, "depth_ray": 12, "depth_grad": 11,
     "ce3d_ray": 43}
K_TOTAL = 8


def _log2ceil(n):
    return int(n - 1).bit_length()


def k_sum(R):
    """float32 roundings on the longest path of pnr_losses' reduction over R rays (adding to an exact 0 is no rounding)"""
    blocks = -(-int(R) // LS_RAYS)
    return (min(int(R), LS_RAYS) - 1) + (-(-blocks // 64) - 1) + _log2ceil(min(blocks, 64)) + 1


def k_sum_ce3d(S):
    """... of pnr_ce3d's over S samples: the wave butterfly, the block's waves in order, the float of the double mean"""
    return _log2ceil(min(int(S), 64)) + (min(-(-int(S) // 64), LS_THREADS // 64) - 1) + 1


def _np(x, dtype=np.float64):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(dtype)


def _dtype(dtype):
    s = str(dtype)
    return np.float32 if "32" in s else np.float64


def _labels(lab, n):
    """int64 labels with everything outside [0, n) set to -1"""
    lab = _np(lab, np.int64)
    return np.where((lab >= 0) & (lab < n), lab, -1)


# ------------------------------------------------------------------------------------------------------------- float64
def losses64(maps, targets, weights, C, K_, depth_l2=False, fix_eps=FIX_EPS, maps_are_prob=False, dtype=np.float64):
    """maps: any subset of rgb (R,3), depth (R), semantic / fix_semantic (R,C), instance / fix_instance (R,K_); targets: rgb, depth,
    semantic (R) int, instance (R) int (a map without its target is skipped, as in pnr_losses).  Returns a dict:
      losses (8,): the six means (0 where absent), the weighted total, 0;   counts: {depth, semantic, instance};
      grads[key]: d total / d map, zero rows on ignored rays;   per_ray[key] (R,): the ray's term, 0 where ignored;
      n[key]: the divisor of the mean;   unit_ray[key] (R,), unit_grad[key]: u * cond per element (module docstring);
      kind[key]: which row of K applies;   bound[key], bound['total']: the bounds of the means and of the total;
      exact[key]: (mask, float32 values) of gradient entries known bit for bit."""
    dt = _dtype(dtype)
    m = {k: _np(v, dt) for k, v in maps.items() if v is not None and k in KEYS}
    w = {k: float(F32(weights.get(k, 0.0))) for k in KEYS}
    eps = float(F32(fix_eps))
    R = next(iter(m.values())).shape[0]
    ref = {"losses": np.zeros(8, dt), "counts": {"depth": 0, "semantic": 0, "instance": 0}, "grads": {}, "per_ray": {}, "n": {},
           "unit_ray": {}, "unit_grad": {}, "kind": {}, "bound": {}, "exact": {}, "R": R}

    def put(key, kind, pr, n, g, ur, ug):
        ref["per_ray"][key], ref["n"][key], ref["grads"][key] = pr, n, g
        ref["unit_ray"][key], ref["unit_grad"][key], ref["kind"][key] = ur, ug, kind

    if "rgb" in m and targets.get("rgb") is not None:
        d = m["rgb"] - _np(targets["rgb"], dt)
        pr = (d * d).sum(1)
        g = w["rgb"] * 2.0 * d / (3.0 * R)
        put("rgb", "rgb", pr, 3 * R, g, U * pr, U * np.abs(g))
    if "depth" in m and targets.get("depth") is not None:
        gt = _np(targets["depth"], dt)
        valid = gt > 0                                  # False for 0, -0.0, negatives and NaN
        nd = int(valid.sum())
        ref["counts"]["depth"] = nd
        d = np.where(valid, m["depth"] - np.where(valid, gt, 0), 0.0)
        if depth_l2:
            pr, g = d * d, w["depth"] * 2.0 * d / max(nd, 1)
        else:
            pr, g = np.abs(d), w["depth"] * np.sign(d) / max(nd, 1)
            ref["exact"]["depth"] = (np.ones(R, bool), (np.sign(d).astype(F32) * (F32(w["depth"]) / F32(max(nd, 1)))).astype(F32))
        put("depth", "depth", pr, max(nd, 1), g, U * pr, U * np.abs(g))
    for key, fkey, n_cls in (("semantic", "fix_semantic", C), ("instance", "fix_instance", K_)):
        if targets.get(key) is None or n_cls == 0 or not (key in m or fkey in m):
            continue
        lab = _labels(targets[key], n_cls)
        valid = lab >= 0
        cnt = int(valid.sum())
        ref["counts"][key] = cnt
        n = max(cnt, 1)
        rows, cols = np.nonzero(valid)[0], lab[valid]

        def nll(mk):
            p = m[mk][rows, cols] + eps
            pr, g, ur = np.zeros(R, dt), np.zeros((R, n_cls), dt), np.zeros(R)
            pr[rows] = -np.log(p)
            g[rows, cols] = -w[mk] / (p * n)
            ur[rows] = U * np.maximum(1.0, np.abs(np.log(p)))
            one = np.zeros((R, n_cls), bool)
            one[rows, cols] = (m[mk][rows, cols].astype(F32) + F32(eps)) == F32(1.0)
            ref["exact"][mk] = (one, np.where(one, -(F32(w[mk]) / F32(n)), F32(0)).astype(F32))
            put(mk, "nll", pr, n, g, ur, U * np.abs(g))

        if key in m and maps_are_prob:
            nll(key)
        elif key in m:
            x = m[key]
            mx = x.max(1, keepdims=True)
            e = np.exp(x - mx)
            den = e.sum(1, keepdims=True)
            p = e / den
            hot = np.zeros((R, n_cls), dt)
            hot[rows, cols] = 1.0
            pr, ur = np.zeros(R, dt), np.zeros(R)
            pr[rows] = np.log(den[rows, 0]) + (mx[rows, 0] - x[rows, cols])
            ur[rows] = U * np.maximum(1.0, pr[rows])
            s = w[key] / n
            g = np.where(valid[:, None], s * (p - hot), 0.0)
            ug = np.where(valid[:, None], abs(s) * (U * (p * (1.0 + np.abs(x - mx)) + hot) + TINY), 0.0)
            put(key, "ce", pr, n, g, ur, ug)
        if fkey in m:
            nll(fkey)
    total, tb = 0.0, 0.0
    for i, key in enumerate(KEYS):
        if key not in ref["per_ray"]:
            continue
        n, pr = ref["n"][key], ref["per_ray"][key]
        term = pr.sum() / n
        ref["losses"][i] = term
        b = K[ref["kind"][key] + "_ray"] * ref["unit_ray"][key].sum() / n + k_sum(R) * U * np.abs(pr).sum() / n
        ref["bound"][key] = float(b)
        total += w[key] * term
        tb += abs(w[key]) * b + K_TOTAL * U * abs(w[key] * term)
    ref["losses"][6] = total
    ref["bound"]["total"] = float(tb)
    return ref


def ce3d64(raw_cm, first_channel, n, label, dtype=np.float64):
    """raw_cm (channels, >= S) channel-major logits, label (S) int.  Returns a dict: mean, count, per_sample (S,) (0 where
    unlabelled), unit (S,) = u * cond per sample, bound = the bound of the mean.  Only the rows [first_channel, +n) and the
    first S columns are read."""
    dt = _dtype(dtype)
    lab = _labels(label, n).reshape(-1)
    S = lab.shape[0]
    raw = raw_cm.detach().cpu().numpy() if hasattr(raw_cm, "detach") else np.asarray(raw_cm)
    x = raw[first_channel:first_channel + n, :S].astype(dt).T
    valid = lab >= 0
    rows, cols = np.nonzero(valid)[0], lab[valid]
    mx = x[rows].max(1)
    den = np.exp(x[rows] - mx[:, None]).sum(1)
    ps, unit = np.zeros(S, dt), np.zeros(S)
    ps[rows] = np.log(den) + (mx - x[rows, cols])
    unit[rows] = U * np.maximum(1.0, ps[rows])
    cnt = int(valid.sum())
    c = max(cnt, 1)
    return {"mean": ps.sum() / c, "count": cnt, "per_sample": ps, "unit": unit,
            "bound": float(K["ce3d_ray"] * unit.sum() / c + k_sum_ce3d(S) * U * np.abs(ps).sum() / c)}


# ------------------------------------------------------------------------------------------------------------- float32
def _butterfly(v):
    """xor butterfly width/2 .. 1 over the last axis (every lane ends with the same value; lane 0 is returned)"""
    width = v.shape[-1]
    idx = np.arange(width)
    d = width // 2
    while d >= 1:
        v = v + v[..., idx ^ d]
        d //= 2
    return v[..., 0]


def _strided(e, width):
    """(R, n) -> (R,): lane l adds columns l, l + width, ... in order, then the butterfly"""
    R, n = e.shape
    T = -(-n // width)
    pad = np.zeros((R, T * width), e.dtype)
    pad[:, :n] = e
    pad = pad.reshape(R, T, width)
    acc = np.zeros((R, width), e.dtype)
    for t in range(T):
        acc = acc + pad[:, t]
    return _butterfly(acc)


def _reduce_rays32(t):
    """k_loss_maps' block sums (16 rays in order) and k_loss_final's walk + butterfly, float32"""
    R = t.shape[0]
    nb = -(-R // LS_RAYS)
    pad = np.zeros(nb * LS_RAYS, F32)
    pad[:R] = t
    pad = pad.reshape(nb, LS_RAYS)
    part = np.zeros(nb, F32)
    for r in range(LS_RAYS):
        part = part + pad[:, r]
    return _strided(part[None, :], 64)[0]


def losses32(maps, targets, weights, C, K_, depth_l2=False, fix_eps=FIX_EPS, maps_are_prob=False, reassoc=True):
    """pnr_losses in numpy float32, in the kernels' op order.  Returns {losses (8,) float32, grads, per_ray}."""
    m = {k: _np(v, F32) for k, v in maps.items() if v is not None and k in KEYS}
    w = {k: F32(weights.get(k, 0.0)) for k in KEYS}
    eps = F32(fix_eps)
    R = next(iter(m.values())).shape[0]
    out = {"losses": np.zeros(8, F32), "grads": {}, "per_ray": {}}
    n_of = {}
    one, two, three = F32(1), F32(2), F32(3)
    with np.errstate(all="ignore"):
        if "rgb" in m and targets.get("rgb") is not None:
            k = w["rgb"] * two / (three * F32(R))
            d = m["rgb"] - _np(targets["rgb"], F32)
            dd = d * d
            out["per_ray"]["rgb"] = (dd[:, 0] + dd[:, 1]) + dd[:, 2]
            out["grads"]["rgb"] = k * d
            n_of["rgb"] = three * F32(R)
        if "depth" in m and targets.get("depth") is not None:
            gt = _np(targets["depth"], F32)
            valid = gt > 0
            nd = F32(max(int(valid.sum()), 1))
            d = np.where(valid, m["depth"] - gt, F32(0)).astype(F32)
            if depth_l2:
                pr, g = d * d, w["depth"] * two * d / nd
            else:
                pr, g = np.abs(d), w["depth"] * np.sign(d).astype(F32) / nd
            out["per_ray"]["depth"], out["grads"]["depth"], n_of["depth"] = pr.astype(F32), g.astype(F32), nd
        for key, fkey, n_cls in (("semantic", "fix_semantic", C), ("instance", "fix_instance", K_)):
            if targets.get(key) is None or n_cls == 0 or not (key in m or fkey in m):
                continue
            lab = _labels(targets[key], n_cls)
            valid = lab >= 0
            n = F32(max(int(valid.sum()), 1))
            rows, cols = np.nonzero(valid)[0], lab[valid]

            def nll(mk):
                p = m[mk][rows, cols] + eps
                pr, g = np.zeros(R, F32), np.zeros((R, n_cls), F32)
                pr[rows] = -np.log(p)
                g[rows, cols] = -w[mk] / (p * n)
                out["per_ray"][mk], out["grads"][mk], n_of[mk] = pr, g, n

            if key in m and maps_are_prob:
                nll(key)
            elif key in m:
                x = m[key]
                mx = x.max(1, keepdims=True)                 # a maximum is exact: its order does not matter
                e = np.exp(x - mx)
                den = _strided(e, 16)
                hot = np.zeros((R, n_cls), F32)
                hot[rows, cols] = 1
                g = np.where(valid[:, None], (w[key] / n) * (e / den[:, None] - hot), F32(0)).astype(F32)
                pr = np.zeros(R, F32)
                xl = x[rows, cols]
                pr[rows] = np.log(den[rows]) + (mx[rows, 0] - xl) if reassoc else (mx[rows, 0] + np.log(den[rows])) - xl
                out["per_ray"][key], out["grads"][key], n_of[key] = pr, g, n
            if fkey in m:
                nll(fkey)
        total = F32(0)
        for i, key in enumerate(KEYS):
            if key in out["per_ray"]:
                v = _reduce_rays32(out["per_ray"][key]) / n_of[key]
                out["losses"][i] = v
                total = total + w[key] * v
            else:
                total = total + w[key] * F32(0)
        out["losses"][6] = total
    return out


def ce3d32(logits, label, reassoc=True):
    """pnr_ce3d in numpy float32: logits (S, n) float32, label (S).  Returns (mean float32, count, per_sample float32)."""
    x = _np(logits, F32)
    S, n = x.shape
    lab = _labels(label, n).reshape(-1)
    valid = lab >= 0
    mx, den = np.full(S, -np.inf, F32), np.zeros(S, F32)
    with np.errstate(all="ignore"):
        for c in range(n):                                  # the online log-sum-exp and its two branches
            v = x[:, c]
            d = v - mx
            e = np.exp(-np.abs(d))
            den = np.where(d <= 0, den + e, den * e + F32(1)).astype(F32)
            mx = np.maximum(mx, v)
        at = x[np.arange(S), np.where(valid, lab, 0)]
        ce = np.log(den) + (mx - at) if reassoc else (mx + np.log(den)) - at
    ce = np.where(valid, ce, F32(0)).astype(F32)
    nb = -(-S // LS_THREADS)

    def blocks(v):
        pad = np.zeros(nb * LS_THREADS, F32)
        pad[:S] = v
        wave = _butterfly(pad.reshape(nb, LS_THREADS // 64, 64))
        part = np.zeros(nb, F32)
        for i in range(LS_THREADS // 64):
            part = part + wave[:, i]
        return part
    s = _strided(blocks(ce).astype(np.float64)[None, :], 64)[0]
    cnt = _strided(blocks(valid.astype(F32)).astype(np.float64)[None, :], 64)[0]
    return F32(s / (cnt if cnt > 0 else 1.0)), int(cnt), ce


# -------------------------------------------------------------------------------------------------------------- checks
def _legacy_value(term):
    return 2e-5 * max(1.0, abs(float(term)))


def _items(got, ref, exact):
    """(quantity, name, err array, unit array, cap, k): the test is err <= min(k * unit, cap)"""
    gl = np.asarray(got["losses"], np.float64)
    for i, key in enumerate(KEYS):
        if key in ref["per_ray"]:
            term = ref["losses"][i]
            yield "mean", key, np.abs(gl[i] - term), np.float64(ref["bound"][key]), _legacy_value(term), 1
            pr = got.get("per_ray", {}).get(key)
            if pr is not None:
                q = ref["kind"][key] + "_ray"
                yield q, key, np.abs(np.asarray(pr, np.float64) - ref["per_ray"][key]), ref["unit_ray"][key], np.inf, K[q]
        else:
            yield "absent", key, np.abs(gl[i]), np.float64(0.0), 0.0, 1
    yield "total", "total", np.abs(gl[6] - ref["losses"][6]), np.float64(ref["bound"]["total"]), _legacy_value(ref["losses"][6]), 1
    yield "absent", "losses[7]", np.abs(gl[7]), np.float64(0.0), 0.0, 1
    for key, g in got.get("grads", {}).items():
        if g is None or key not in ref["grads"]:
            continue
        g = _np(g, np.float32)
        rg = ref["grads"][key]
        q = ref["kind"][key] + "_grad"
        yield q, key, np.abs(g.astype(np.float64) - rg), ref["unit_grad"][key], 1e-6 + 2e-5 * np.abs(rg).max(), K[q]
        if exact and key in ref["exact"]:
            mask, val = ref["exact"][key]
            bad = mask & (g.view(np.uint32) != val.view(np.uint32)) & ~((g == 0) & (val == 0))
            yield "exact", key, bad.astype(np.float64), np.zeros(bad.shape), 0.0, 1


def worst(got, ref, into=None, exact=False):
    """quantity -> the largest err / unit (the figure k is compared with; for 'mean' and 'total' err / bound)"""
    into = {} if into is None else into
    for q, _, err, unit, _, _ in _items(got, ref, exact):
        err, unit = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(unit, np.float64))
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, np.where(unit > 0, err / unit, np.inf))
        ratio = np.where(np.isnan(err), np.inf, ratio)
        into[q] = max(into.get(q, 0.0), float(ratio.max()) if ratio.size else 0.0)
    return into


def violations(got, ref, exact=False, scale=1.0):
    """every (quantity, map) whose error leaves its bound, as strings; `scale` shrinks every bound (1/4: where float32 sits)"""
    bad = []
    for q, name, err, unit, cap, k in _items(got, ref, exact):
        bound = np.minimum(k * np.asarray(unit, np.float64), cap) * scale
        fail = ~(np.asarray(err, np.float64) <= bound)
        if fail.any():
            i = int(np.argmax(np.where(fail, np.nan_to_num(np.asarray(err, np.float64), nan=np.inf), -1)))
            e, b = np.broadcast_arrays(np.asarray(err, np.float64), bound)
            bad.append(f"{q}:{name} err {e.reshape(-1)[i]:.3e} > bound {b.reshape(-1)[i]:.3e} at {i} ({int(fail.sum())} elements)")
    return bad


def ce3d_violations(mean, count, ref, scale=1.0):
    bad = []
    if int(count) != ref["count"]:
        bad.append(f"count {count} != {ref['count']}")
    bound = min(ref["bound"], _legacy_value(ref["mean"])) * scale
    if not abs(float(mean) - ref["mean"]) <= bound:
        bad.append(f"mean {float(mean)!r} vs {ref['mean']!r}: err {abs(float(mean) - ref['mean']):.3e} > bound {bound:.3e}")
    return bad


# --------------------------------------------------------------------------------------------------------------- cases
_KC = (0, 1, 15, 16, 17, 33)
EDGE_LABELS = lambda n: [-1, -7, n, n + 5, 255, INT_MAX, INT_MIN]      # noqa: E731  (255 >= n in every case that uses them)
R_BIG = 3 * 262144 + 77                                                # >= 3 trips of k_loss_count's 1024 x 256 grid-stride loop


def loss_cases():
    c = []
    add = lambda **kw: c.append(dict({"l2": False, "prob": False, "offset": None, "edge": None}, **kw))    # noqa: E731
    for l2 in (False, True):
        for prob in (False, True):
            for C in range(1, 131):
                add(id=f"sweep-C{C}-l2{int(l2)}-p{int(prob)}", group="sweep", R=157, C=C, K=_KC[C % 6], l2=l2, prob=prob)
    for C, K_ in ((45, 32), (17, 1)):
        for R in range(1, 18):
            add(id=f"smallR-{R}-C{C}", group="smallR", R=R, C=C, K=K_, l2=bool(R & 1))
    for R in (255, 256, 257, 1023, 1024, 1025, 2049 + 16 * 64 * 2):
        add(id=f"Redge-{R}", group="Redge", R=R, C=19, K=5)
    add(id="big", group="big", R=R_BIG, C=3, K=2, edge="plant")
    for C in range(1, 131):                                  # every ray of the sweep row with one of the offsets
        add(id=f"shiftmix-C{C}", group="shiftmix", R=157, C=C, K=_KC[C % 6], offset="mix")
    for off in OFFSETS:                                      # one offset for the whole batch; R = 1, 2: the mean IS the ray's value
        for C in (1, 3, 16, 17, 45, 130):
            for R in (1, 2, 157):
                add(id=f"shift{off:g}-C{C}-R{R}", group="shift", R=R, C=C, K=_KC[C % 6], offset=off)
    for l2 in (False, True):
        for prob in (False, True):
            add(id=f"edge-l2{int(l2)}-p{int(prob)}", group="edge", R=157, C=19, K=17, l2=l2, prob=prob, edge="rays")
    add(id="nolabel", group="edge", R=157, C=19, K=17, edge="nolabel")
    add(id="nodepth", group="edge", R=157, C=19, K=17, edge="nodepth")
    return c


def _softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def loss_inputs(case):
    """Seeded float32 maps and targets of a case.  Logits are 3 N(0,1) on a grid of 2^-8, so adding any of OFFSETS is exact in
    float32 and the shifted row has the same float64 answer as the row itself."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    R, C, K_, prob, edge = case["R"], case["C"], case["K"], case["prob"], case["edge"]
    maps = {"rgb": rng.random((R, 3)).astype(F32), "depth": (rng.random(R) * 20).astype(F32)}
    tg = {"rgb": rng.random((R, 3)).astype(F32), "depth": (rng.random(R) * 20 - 4).astype(F32)}        # ~20 % not > 0
    off = case["offset"]
    offs = None if off is None else (np.asarray(OFFSETS, F32)[np.arange(R) % len(OFFSETS)] if off == "mix" else np.full(R, off, F32))
    for key, fkey, n in (("semantic", "fix_semantic", C), ("instance", "fix_instance", K_)):
        if n == 0:
            continue
        if prob:
            maps[key] = (_softmax(rng.normal(size=(R, n))) * rng.random((R, 1))).astype(F32)
        else:
            x = (np.round(rng.normal(size=(R, n)) * 3 * 256) / 256).astype(F32)
            maps[key] = x if offs is None else (x + offs[:, None]).astype(F32)
        maps[fkey] = (_softmax(rng.normal(size=(R, n))) * rng.random((R, 1))).astype(F32)
        tg[key] = rng.integers(-1, n, R).astype(np.int32)
    eps = F32(FIX_EPS)
    if edge == "plant":                                      # fl(p + eps) == 1 on every labelled ray: g_fix tells the label count exactly
        for key, fkey, n in (("semantic", "fix_semantic", C), ("instance", "fix_instance", K_)):
            v = (tg[key] >= 0) & (tg[key] < n)
            maps[fkey][np.nonzero(v)[0], tg[key][v]] = F32(1) - eps
    elif edge == "rays":
        for key, fkey, n, r0 in (("semantic", "fix_semantic", C, 0), ("instance", "fix_instance", K_, 3)):
            t = tg[key]
            t[7:20] = np.arange(7, 20) % n                   # the rays with hand-made maps carry a label (set before the bad ones)
            t[r0:r0 + 7] = np.array(EDGE_LABELS(n), np.int64).astype(np.int32)
            if not prob:
                x = maps[key]
                x[10], x[11], x[12] = 0.0, 80.0, -80.0       # all equal, at three levels
                x[13] = rng.choice(np.array([-80.0, 80.0], F32), n)
                x[14, 14 % n] = 50.0                         # one dominant class: the label's; ray 15: another one's
                x[15, (15 + 1) % n] = 50.0
            for mk in (fkey,) + ((key,) if prob else ()):
                maps[mk][16, t[16]] = 0.0                    # probability 0: -log(eps), gradient -w / (eps n)
                maps[mk][17, t[17]] = 1.0
                maps[mk][18, t[18]] = F32(1) - eps           # fl(p + eps) == 1: the exact-count entry
        tg["depth"][20:24] = np.array([0.0, -0.0, -3.0, np.nan], F32)
        tg["depth"][24] = 7.5
        maps["depth"][24] = 7.5                              # depth == depth_gt: L1 gradient 0
        tg["rgb"][25] = maps["rgb"][25]
    elif edge == "nolabel":
        tg["semantic"][:] = -1
        tg["instance"][:] = np.array([-7, K_, INT_MIN, K_ + 5, INT_MAX], np.int64).astype(np.int32)[np.arange(R) % 5]
    elif edge == "nodepth":
        tg["depth"][:] = np.array([0.0, -0.0, -3.0, np.nan], F32)[np.arange(R) % 4]
    return maps, tg


def ce3d_cases():
    c = []
    add = lambda **kw: c.append(dict({"S": 1000, "fc": 0, "rows": None, "offset": None, "labels": None}, **kw))    # noqa: E731
    for n in range(1, 131):
        for fc in (0, 4, 4 + n):
            add(id=f"sweep-n{n}-fc{fc}", group="sweep", n=n, fc=fc)
    for S in (1, 63, 64, 65, 255, 256, 257, 64 * 256 + 1, 3 * 64 * 256 + 5):
        add(id=f"S{S}", group="S", n=19, S=S, fc=4)
    for n in (1, 16, 17, 45):
        add(id=f"one-n{n}", group="one", n=n, labels="one")
    for rows in ("ascending", "descending", "equal"):
        add(id=f"rows-{rows}", group="rows", n=45, rows=rows)
    for off in OFFSETS:
        for n in (1, 3, 16, 17, 45, 130):
            add(id=f"shift{off:g}-n{n}", group="shift", n=n, S=300, offset=off)
        for n in (3, 17, 45):                                # one labelled sample: the mean IS its value
            add(id=f"shift{off:g}-one-n{n}", group="shift", n=n, S=300, offset=off, labels="one")
    add(id="shiftmix", group="shift", n=19, offset="mix")
    add(id="edge-labels", group="labels", n=19, labels="edge")
    add(id="nolabel", group="labels", n=19, labels="none")
    return c


def ce3d_inputs(case):
    """logits (S, n) float32 (on the 2^-8 grid), label (S,) int32"""
    rng = np.random.default_rng(zlib.crc32(("ce3d-" + case["id"]).encode()))
    S, n = case["S"], case["n"]
    x = (np.round(rng.normal(size=(S, n)) * 3 * 256) / 256).astype(F32)
    if case["rows"] == "ascending":                           # the running maximum moves at every step: the rescale branch
        x = np.sort(x, 1)
    elif case["rows"] == "descending":                        # ... never after the first
        x = np.sort(x, 1)[:, ::-1].copy()
    elif case["rows"] == "equal":
        x[:] = x[:, :1]
    off = case["offset"]
    if off is not None:
        offs = np.asarray(OFFSETS, F32)[np.arange(S) % len(OFFSETS)] if off == "mix" else np.full(S, off, F32)
        x = (x + offs[:, None]).astype(F32)
    lab = rng.integers(-1, n, S).astype(np.int32)
    if case["labels"] == "one":
        lab[:] = -1
        lab[S * 3 // 4 + 27] = n - 1
    elif case["labels"] == "edge":
        lab = np.array(EDGE_LABELS(n) + list(range(n)), np.int64).astype(np.int32)[rng.integers(0, 7 + n, S)]
    elif case["labels"] == "none":
        lab = np.array(EDGE_LABELS(n), np.int64).astype(np.int32)[np.arange(S) % 7]
    return x, lab
