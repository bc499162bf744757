"""Test support: probe networks that make an MLP forward WITHOUT saved activations (the fp32 inference kernel, k_mlp_fused<fp32>
behind pnr_mlp_forward) read out its own internal regions exactly, and the layer-local float64 check of tests/_mlp32_ref.py run
on what they return.  Not part of the product package.

A probe is a descriptor and a parameter set in which a selector / identity row multiplies ONE activation by 1 and every other by
0, with bias 0: every partial sum of such a row is exact in any summation order (0 + x = x, x + 0 = x), so the output row IS the
internal value, bit for bit, as long as that value is a normal number (or 0).  The regions are named as in
_mlp32_ref.acts_regions:

  X_D, F    the case's own trunk, appearance branch unchanged, ONE head_depth-1 head semantic_linears.0 = I_W (n_sem = W) on the
            trunk output / on the feature: raw[4:4 + W].  rgb and sigma of these launches are the real launch's, bit for bit.
  X_l       1 < l < D: the depth-l prefix of the same trunk (skip = -1 while the skip layer lies outside it), same identity head.
  X_1       a D = 2 network whose pts_linears.1 = I_W: relu(X_1) = X_1.
  SH_*      head_depth 2, the case's own *.0 Linear, *.1 = I_H, n = H; both heads in one launch.
  EX        D = 2, skip = -1, pts_linears.0 rows 2c = +e_c, 2c + 1 = -e_c (ex <= 63 <= W / 2 columns: one launch),
            pts_linears.1 = I_W: column c = row 2c - row 2c + 1 (one of the two is 0).
  ED        views_linears.0 rows 0 / 1 = +e_{W + c} / -e_{W + c}, rgb_linear rows e_0, e_1: column c = raw[0] - raw[1], one
            column per launch.
  G         rgb_linear rows e_i, e_j, e_k: three columns per launch, H / 3 launches (full_G).

probes(prec="bf16") builds the same networks for the bf16 inference kernels, where the read-out is the bf16 activation the next
Linear reads (tests/_mlp_probe_bf16.py).

Everything sits behind launch(desc, params, rays, z) -> raw (S, channels): the same code runs against _mlp32_ref.forward32 on the
CPU (tests/test_mlp_probe.py) and against the kernel on the GPU (tests/test_gpu_mlp_fp32_infer_sweep.py).

check(): EX / ED through _mlp32_ref.check_inputs, every nn.Linear through _mlp32_ref.check_linear (with full_G the assembled acts
buffer goes through check_forward as it stands).  Without G, rgb is checked with the two-step bound from the kernel's F and ED:
    E_G = f32_bound(r_G, m_G, W + ed + 2),        r_G = relu(float64 views_linears.0 on [F, ED]),  m_G its |w| |x| + |b|
    |rgb_k - rgb64| <= |W_rgb| E_G + f32_bound(rgb64, |W_rgb| (r_G + E_G) + |b|, H + 2),      rgb64 = W_rgb r_G + b
(ReLU is 1-Lipschitz, so the kernel's G is within E_G of r_G; the second term is check_linear's bound on the kernel's own G, whose
magnitude is at most r_G + E_G).  No measured number enters.

kernel_order / layer32: one Linear restated in numpy float32 in the order k_mlp_fused<fp32> accumulates it -- the bias first
(load_bias), then one v_mfma_f32_32x32x2_f32 per lane-vector slot v, whose two k values are the slots (hi = 0, v) and (hi = 1, v) of
pnr_mlp_layout.h (pnr_seg_col), each step one fused multiply-add (fma32: exact, no double rounding)."""
import numpy as np
import torch

import _mlp32_ref as m32
from panopticnerf_amd import ops

TINY = 2.0 ** -126


class Probe:
    def __init__(self, region, desc, params, store, same_rgbs=False):
        self.region, self.desc, self.params, self.store, self.same_rgbs = region, desc, params, store, same_rgbs


def _lin(prefix, w, b=None):
    return {prefix + ".weight": w, prefix + ".bias": torch.zeros(w.shape[0]) if b is None else b}


def _take(params, prefix):
    return {prefix + ".weight": params[prefix + ".weight"], prefix + ".bias": params[prefix + ".bias"]}


def probes(desc, params, full_G=False, need=None, prec="fp32"):
    """the probe launches of one case; need: region names to read (None: all, G only with full_G); prec: the precision of the
    probe descriptors (every probe matrix holds only 0 and +-1, exact in bf16 too: tests/_mlp_probe_bf16.py)"""
    g = m32.dims(desc)
    W, H, D, skip, ex, ed = g["W"], g["H"], g["D"], g["skip"], g["ex"], g["ed"]
    tapname = "feature" if g["tap"] else "trunk"
    want = lambda r: need is None or r in need                                       # noqa: E731

    def mk(D_, skip_, C=0, K=0, tap="trunk", depth=1):
        return ops.make_desc(D_, W, skip_, desc.xyz_L, desc.dir_L, C, K, H, prec, tap, depth)

    base = {}
    for nm in ("alpha_linear", "feature_linear", "views_linears.0", "rgb_linear"):
        base.update(_take(params, nm))
    trunk = lambda l: {k: v for i in range(l) for k, v in _take(params, "pts_linears.%d" % i).items()}      # noqa: E731
    id_head = _lin("semantic_linears.0", torch.eye(W))
    two = dict(_lin("pts_linears.1", torch.eye(W)), **base)                          # the D = 2 carriers: pts_linears.0 is the probe's
    out = []

    def region_store(name, c0, n):
        def store(X, raw):
            X[name] = raw[:, c0:c0 + n].clone()
        return store

    for reg, tap in (("X%d" % D, "trunk"), ("F", "feature")):
        if want(reg):
            out.append(Probe(reg, mk(D, skip, W, 0, tap, 1), dict(trunk(D), **base, **id_head), region_store(reg, 4, W), same_rgbs=True))
    for l in range(2, D):
        if want("X%d" % l):
            out.append(Probe("X%d" % l, mk(l, skip if skip < l - 1 else -1, W), dict(trunk(l), **base, **id_head),
                             region_store("X%d" % l, 4, W)))
    if want("X1"):
        out.append(Probe("X1", mk(2, -1, W), dict(_take(params, "pts_linears.0"), **two, **id_head), region_store("X1", 4, W)))
    hs = [h for h in m32.heads(desc) if want(h[3])]
    if g["deep"] and hs:
        hp, stores = {}, []
        for i, (nm, _, _, sh) in enumerate(hs):
            hp.update(_take(params, nm + ".0"))
            hp.update(_lin(nm + ".1", torch.eye(H)))
            stores.append(region_store(sh, 4 + i * H, H))
        C, K = (H if any(h[0] == "semantic_linears" for h in hs) else 0), (H if any(h[0] == "instance_linears" for h in hs) else 0)

        def store_heads(X, raw, stores=stores):
            for s in stores:
                s(X, raw)
        out.append(Probe("SH", mk(D, skip, C, K, tapname, 2), dict(trunk(D), **base, **hp), store_heads))
    if want("EX"):
        w0 = torch.zeros(W, ex)
        for c in range(ex):
            w0[2 * c, c], w0[2 * c + 1, c] = 1.0, -1.0

        def store_ex(X, raw):
            X["EX"] = raw[:, 4:4 + 2 * ex:2] - raw[:, 5:5 + 2 * ex:2]
        out.append(Probe("EX", mk(2, -1, W), dict(_lin("pts_linears.0", w0), **two, **id_head), store_ex))
    if want("ED"):
        w_rgb = torch.zeros(3, H)
        w_rgb[0, 0] = w_rgb[1, 1] = 1.0
        for c in range(ed):
            wv = torch.zeros(H, W + ed)
            wv[0, W + c], wv[1, W + c] = 1.0, -1.0

            def store_ed(X, raw, c=c):
                if "ED" not in X:
                    X["ED"] = torch.zeros((raw.shape[0], ed), dtype=raw.dtype, device=raw.device)
                X["ED"][:, c] = raw[:, 0] - raw[:, 1]
            p = dict(_take(params, "pts_linears.0"), **two)
            p.update(_lin("views_linears.0", wv))
            p.update(_lin("rgb_linear", w_rgb))
            out.append(Probe("ED", mk(2, -1), p, store_ed))
    if full_G and want("G"):
        for i0 in range(0, H, 3):
            n = min(3, H - i0)
            w_rgb = torch.zeros(3, H)
            for j in range(n):
                w_rgb[j, i0 + j] = 1.0

            def store_g(X, raw, i0=i0, n=n):
                if "G" not in X:
                    X["G"] = torch.zeros((raw.shape[0], H), dtype=raw.dtype, device=raw.device)
                X["G"][:, i0:i0 + n] = raw[:, 0:n]
            p = dict(trunk(D), **base)
            p.update(_lin("rgb_linear", w_rgb))
            out.append(Probe("G", mk(D, skip), p, store_g))
    return out


def read_out(launch, probe_list, rays, z, real=None):
    """region -> (S, width) as the launches return it; real: the case's own raw, whose first four channels every launch that keeps
    the trunk and the appearance branch must reproduce bit for bit"""
    X = {}
    for pr in probe_list:
        raw = launch(pr.desc, pr.params, rays, z)
        pr.store(X, raw)
        if pr.same_rgbs and real is not None:
            assert torch.equal(raw[:, :4], real[:, :4]), "%s probe: rgb / sigma differ from the real launch" % pr.region
    return X


def assemble_acts(desc, S, X):
    """the regions in the acts layout of include/pnr.h (acts_regions), flat"""
    reg, total = m32.acts_regions(desc, S)
    acts = torch.zeros(total, dtype=torch.float32, device=next(iter(X.values())).device)
    for nm, (o, w) in reg.items():
        acts[o:o + S * w] = X[nm].reshape(-1)
    return acts


def assert_normal(desc, params, rays, z):
    """readouts are exact for normal numbers: no activation of the float64 reference may be subnormal"""
    X, raw = m32.chain64(desc, params, rays.cpu(), z.cpu())
    for nm, x in list(X.items()) + [("raw", raw)]:
        a = x.abs()
        assert not ((a > 0) & (a < TINY)).any(), "%s: a subnormal activation (choose another seed)" % nm


def check_rgb_two_step(rep, desc, net, X, raw):
    x = torch.cat([X["F"], X["ED"]], 1).double()
    wv, bv, wr, br = net.w["views_linears.0"], net.b["views_linears.0"], net.w["rgb_linear"], net.b["rgb_linear"]
    rG, mG = (x @ wv.t() + bv).clamp(min=0), x.abs() @ wv.abs().t() + bv.abs()
    EG = m32.f32_bound(rG, mG, x.shape[1] + 2)
    rgb64 = rG @ wr.t() + br
    bound = EG @ wr.abs().t() + m32.f32_bound(rgb64, (rG + EG) @ wr.abs().t() + br.abs(), wr.shape[1] + 2)
    ratio = (raw[:, 0:3].double() - rgb64).abs() / bound
    rep.note("fp32 raw rgb (two-step)", ratio.max())
    rep.note("two-step rgb bound / (1e-4 max(1, |rgb|))", (bound / (1e-4 * rgb64.abs().clamp(min=1.0))).max())
    if not (ratio <= 1).all():
        rep.fail("raw[rgb_linear]", "%d of %d rgb values beyond the two-step bound (worst ratio %.3g)"
                 % (int((~(ratio <= 1)).sum()), ratio.numel(), ratio.max().item()))


def regions_of(desc, only):
    need = set()
    for name, src, dst, _ in m32.linears(desc):
        if name in only:
            need.update(src)
            if isinstance(dst, str):
                need.add(dst)
    return need


def check(rep, launch, desc, params, rays, z, full_G=False, only=None, trig_bound=None, real=None):
    """the layer-local check of one case through `launch`.  only: names of the nn.Linears to check (their regions alone are read
    out; gamma is then not checked).  Returns (X regions, the case's own raw)."""
    S = z.numel()
    assert_normal(desc, params, rays, z)
    real = launch(desc, params, rays, z) if real is None else real
    need = None if only is None else regions_of(desc, only)
    X = read_out(launch, probes(desc, params, full_G, need), rays, z, real)
    if only is None and full_G:
        m32.check_forward(rep, desc, params, rays, z, real, assemble_acts(desc, S, X), trig_bound)
        return X, real
    if only is None:
        m32.check_inputs(rep, desc, rays, z, X, trig_bound)
    net = m32.Net(desc, params, real.device)
    for name, src, dst, relu in m32.linears(desc):
        if only is not None and name not in only:
            continue
        if "G" not in X and name == "views_linears.0":
            continue
        if "G" not in X and name == "rgb_linear":
            check_rgb_two_step(rep, desc, net, X, real)
            continue
        m32.check_linear(rep, net, X, real, name, src, dst, relu)
    return X, real


# ------------------------------------------------------------------------------------- the kernel's own accumulation order
def seg_col(kind, L, hi, v):
    """pnr_seg_col of pnr_mlp_layout.h: the canonical column of lane-vector slot (hi, v); -1 = pad.  kind: 'gx', 'gd', 'feat'"""
    if kind == "feat":
        r = v & 15
        return (v >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi
    nfh = 5 if kind == "gx" else 2
    if v == 0:
        return 2 if hi else 0
    if v == 1:
        return -1 if hi else 1
    fp, j = divmod(v - 2, 6)
    f = hi * nfh + fp
    if fp >= nfh or f >= L:
        return -1
    return 3 + 6 * f + j


def kernel_order(kind, L=0, width=0):
    """the columns of one input segment in the order the fp32 kernel adds them: slot v = 0, 1, ..., within it hi = 0 then 1"""
    vl = 32 if kind == "gx" else 16 if kind == "gd" else width // 2
    return [c for v in range(vl) for c in (seg_col(kind, L, 0, v), seg_col(kind, L, 1, v)) if c >= 0]


def fma32(a, b, c):
    """fl32(a b + c) of float32 arrays with ONE rounding: the float64 sum of the exact product and c, its rounding error by TwoSum,
    and the float32 rounding corrected where the float64 sum sits on a float32 midpoint that the exact sum does not"""
    p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (d != 0) & (np.abs(d) == np.abs(other.astype(np.float64) - s))
    return np.where(tie & (err != 0) & (np.sign(err) == np.sign(d)), other, r).astype(np.float32)


def layer32(segments, w, b, relu=True):
    """segments: [(x (S, n) float32, order)] in the weight's column order; w (n_out, sum n), b (n_out,): the Linear as one fmaf chain
    per element from the bias, in the kernel's order"""
    w, b = np.asarray(w, np.float32), np.asarray(b, np.float32)
    acc = np.broadcast_to(b, (segments[0][0].shape[0], w.shape[0])).astype(np.float32)
    k0 = 0
    for x, order in segments:
        x = np.asarray(x, np.float32)
        for c in order:
            acc = fma32(x[:, c, None], w[None, :, k0 + c], acc)
        k0 += x.shape[1]
    return np.maximum(acc, np.float32(0)) if relu else acc
