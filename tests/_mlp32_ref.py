"""Test support: a float64, LAYER-LOCAL reference of the fp32 parity mode of the training MLP (pnr_mlp_forward_train_fp32,
pnr_mlp_backward_fp32: k_f32_inputs, k_f32_gemm, k_f32_slab_sum, k_f32_colsum), a numpy float32 restatement of the kernels' GEMM
order, and the two size ledgers of include/pnr.h.  Not part of the product package.  Report, check_f32, U and C_ACC are
_mlp_ref.py's.

Layer-local forward: every Linear of the reference reads the KERNEL's own saved fp32 input region(s) (the acts layout of
include/pnr.h) and the fp32 parameters, computes in float64 and compares per element:
    |k - r64| <= C_ACC (K + 2) u m + ulp(r64),   m = |b| + sum |w x| over both segments of a concatenated layer,
K the full reduction length (the recursive-summation bound, any order; u = 2^-24), + 2 for the bias add and the `beta` add of
the two-launch skip / views layers.  A ReLU output is that value clamped at 0, and exactly 0 where r64 is below minus the bound.
The raw rows (rgb, sigma, logits) are checked the same way from G / X_D / the tap / SH.

gamma(x), gamma(d): the identity columns of EX are o + d z, one multiply and one add in float32 (the build has contraction off):
bit for bit.  Those of ED are d / ||d||: within 8 u relative of float64 (three products, two sums, sqrt, division, as derived in
_mlp_ref.py).  Every band is sin / cos in float64 of 2^k times the kernel's OWN stored identity column -- that argument is exact
in float32 -- so only the error of the device sinf / cosf is left.  Nothing in the project fixes it: TRIG_MEASURED is the worst
|kernel - float64| an MI355X gave over the cases of test_gpu_mlp_fp32_sweep.py (far points at band 9 included), and TRIG_BOUND
is 4 x that, floored at 2 u, never looser than test_embed's 2e-6.

Backward: the intermediate dYs stay inside the kernel's workspace.  The reference runs the whole backward in float64 from d_raw,
the parameters and the kernel's saved activations (gates = saved X > 0 on both sides) and compares every dW and db per element:
  * output Linears (rgb_linear, alpha_linear, the logit Linears): dY is d_raw itself,
        |k - r64| <= C_ACC (min(S, 2048) + n_slab) u sum_s |dy x| + ulp      (one slab's chain, then the slabs' sum);
  * every other Linear: the running error of a chain of linear maps with fixed gates.  The same backward with |W|, |d_raw| and the
    same gates gives |dY|_abs; a computed dY is off by at most C_ACC P u |dY|_abs, P the sum of the reduction lengths, plus one per
    accumulate, of the data-gradient GEMMs on the longest path from d_raw to that dY (path_lengths: from the descriptor), so
        |k - r64| <= C_ACC (P + min(S, 2048) + n_slab) u A + ulp,   A = |dY|_abs^T |X|  (sum_s |dY|_abs for a bias).
No measured number enters these bounds."""
import numpy as np
import torch

from _mlp_ref import C_ACC, U, Report, check_f32  # noqa: F401  (Report: re-exported for the tests)

KSLAB = 2048                    # samples per weight-gradient partial (pnr_mlp_fp32_train.hip)
TRIG_MEASURED = 6.96e-8         # worst |kernel - float64| of a band value on an MI355X (1.17 u; the sweep's docstring table)
TRIG_BOUND = max(4.0 * TRIG_MEASURED, 2.0 * U)
assert TRIG_BOUND <= 2e-6       # test_embed's bar


# ------------------------------------------------------------------------------------------------------- the architecture
def dims(desc):
    return dict(ex=3 + 6 * desc.xyz_L, ed=3 + 6 * desc.dir_L, W=desc.W, H=desc.W // 2, D=desc.D, deep=desc.head_depth != 1,
                C=desc.n_sem, K=desc.n_inst, tap=bool(desc.head_tap), skip=desc.skip)


def heads(desc):
    """[(nn.Module name, first raw channel, n, hidden region)] of the heads that exist"""
    return [(nm, c0, n, sh) for nm, c0, n, sh in (("semantic_linears", 4, desc.n_sem, "SH_sem"),
                                                  ("instance_linears", 4 + desc.n_sem, desc.n_inst, "SH_inst")) if n]


def linears(desc):
    """Every nn.Linear in forward order: (name, input regions (concatenated in this order), output, relu).  output: an acts region
    or ('raw', first channel, n)."""
    g = dims(desc)
    D, tap = g["D"], "F" if g["tap"] else "X%d" % g["D"]
    out = []
    for l in range(D):
        src = ["EX"] if l == 0 else (["EX", "X%d" % l] if l - 1 == g["skip"] else ["X%d" % l])
        out.append(("pts_linears.%d" % l, src, "X%d" % (l + 1), True))
    out.append(("alpha_linear", ["X%d" % D], ("raw", 3, 1), False))
    out.append(("feature_linear", ["X%d" % D], "F", False))
    out.append(("views_linears.0", ["F", "ED"], "G", True))
    out.append(("rgb_linear", ["G"], ("raw", 0, 3), False))
    for nm, c0, n, sh in heads(desc):
        if g["deep"]:
            out.append((nm + ".0", [tap], sh, True))
            out.append((nm + ".1", [sh], ("raw", c0, n), False))
        else:
            out.append((nm + ".0", [tap], ("raw", c0, n), False))
    return out


def acts_regions(desc, S):
    """(name -> (float offset, width), total floats): the acts layout as include/pnr.h documents it"""
    g = dims(desc)
    order = [("EX", g["ex"]), ("ED", g["ed"])] + [("X%d" % (l + 1), g["W"]) for l in range(g["D"])] + [("F", g["W"]), ("G", g["H"])]
    if g["deep"]:
        order += [(sh, g["H"]) for _, _, _, sh in heads(desc)]
    reg, o = {}, 0
    for nm, w in order:
        reg[nm] = (o, w)
        o += S * w
    return reg, o


def read_acts(desc, S, acts):
    reg, total = acts_regions(desc, S)
    assert acts.numel() == total, (acts.numel(), total)
    return {nm: acts[o:o + S * w].view(S, w) for nm, (o, w) in reg.items()}


def wgrad_launches(desc):
    """(n_out, k, has bias) of every weight-gradient GEMM of one backward, from the nn.Linear shapes: one launch per input segment
    of a Linear, the bias with the segment that is not an embedding"""
    width = dict((nm, w) for nm, (_, w) in acts_regions(desc, 1)[0].items())
    out = []
    for name, src, dst, _ in linears(desc):
        n_out = width[dst] if isinstance(dst, str) else dst[2]
        for s in src:
            out.append((n_out, width[s], len(src) == 1 or s not in ("EX", "ED")))
    return out


def n_slabs(S):
    return -(-S // KSLAB)


def workspace_bytes(desc, S):
    """the ledger of pnr_mlp_backward_fp32_workspace_bytes: dH a/b, dF [S][W], dG, dSH [S][W/2], then n_slab blocks of the widest
    launch's partials"""
    g = dims(desc)
    return 4 * (S * (3 * g["W"] + 2 * g["H"]) + n_slabs(S) * max(n * k + (n if b else 0) for n, k, b in wgrad_launches(desc)))


def parent_workspace_bytes(desc, S):
    """what the library returned before the head_depth-1 Linears were counted (the size of the guard the GPU sweep puts behind its
    workspace comes from the difference)"""
    g = dims(desc)
    return 4 * (S * (3 * g["W"] + 2 * g["H"]) + n_slabs(S) * (g["W"] * (g["W"] + max(g["ex"], g["ed"])) + g["W"]) + 16)


def path_lengths(desc):
    """Linear name -> P of its dY (module docstring)"""
    g = dims(desc)
    W, H, D = g["W"], g["H"], g["D"]
    P = {"rgb_linear": 0, "alpha_linear": 0, "views_linears.0": 3}
    into_f, into_h = [3 + H], []                      # path lengths of the GEMMs that write / accumulate d F and d h
    for nm, _, n, _ in heads(desc):
        if g["deep"]:
            P[nm + ".1"], P[nm + ".0"] = 0, n
            (into_f if g["tap"] else into_h).append(n + H)
        else:
            P[nm + ".0"] = 0
            (into_f if g["tap"] else into_h).append(n)
    P["feature_linear"] = max(into_f) + len(into_f) - 1
    into_h += [P["feature_linear"] + W, 1]
    p = max(into_h) + len(into_h) - 1
    for l in range(D - 1, -1, -1):
        P["pts_linears.%d" % l] = p
        p += W
    return P


class Net:
    """the fp32 parameters in float64 on `device`"""

    def __init__(self, desc, params, device):
        self.desc = desc
        self.w = {k[:-7]: v.detach().to(device, torch.float64) for k, v in params.items() if k.endswith(".weight")}
        self.b = {k[:-5]: v.detach().to(device, torch.float64) for k, v in params.items() if k.endswith(".bias")}


# ------------------------------------------------------------------------------------------------------------- forward
def f32_bound(r64, m, K_eff):
    _, e = torch.frexp(r64)
    return C_ACC * K_eff * U * m + torch.exp2((e - 24).clamp(min=-149).to(r64.dtype))


def points32(rays, z):
    """o + d z in float32, a separate multiply and add: numpy, (R, 8), (R, N) -> (R N, 3)"""
    rays, z = np.asarray(rays, np.float32), np.asarray(z, np.float32)
    return (rays[:, None, 0:3] + (rays[:, None, 3:6] * z[:, :, None]).astype(np.float32)).astype(np.float32).reshape(-1, 3)


def check_inputs(rep, desc, rays, z, X, trig_bound=None):
    trig_bound = TRIG_BOUND if trig_bound is None else trig_bound
    dev = X["EX"].device
    N = z.shape[1]
    p32 = torch.from_numpy(points32(rays.cpu().numpy(), z.cpu().numpy())).to(dev)
    if not torch.equal(X["EX"][:, :3], p32):
        rep.fail("EX", "%d identity columns differ from fl(o + fl(d z))" % int((X["EX"][:, :3] != p32).sum()))
    d = rays[:, 3:6].to(dev).double()
    vd = (d / d.norm(dim=1, keepdim=True)).repeat_interleave(N, 0)
    rel = (X["ED"][:, :3].double() - vd).abs() / (8 * U * vd.abs()).clamp(min=1e-300)
    rel = torch.where(vd == 0, (X["ED"][:, :3] != 0).double() * 2, rel)
    rep.note("ED identity / (8 u |v|)", rel.max())
    if not (rel <= 1).all():
        rep.fail("ED", "%d unit-direction columns beyond 8 u relative (worst %.3g)" % (int((rel > 1).sum()), rel.max().item()))
    for nm, L in (("EX", desc.xyz_L), ("ED", desc.dir_L)):
        x = X[nm][:, :3].double()
        for k in range(L):
            ref = torch.cat([torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)], 1)
            err = (X[nm][:, 3 + 6 * k: 9 + 6 * k].double() - ref).abs()
            rep.note("trig abs", err.max())
            rep.note("trig", err.max() / trig_bound)
            if not (err <= trig_bound).all():
                rep.fail(nm, "band %d: %d values beyond %.3g of float64 sin / cos (worst %.3g)"
                         % (k, int((~(err <= trig_bound)).sum()), trig_bound, err.max().item()))


def check_linear(rep, net, X, raw, name, src, dst, relu):
    """one nn.Linear of linears(): float64 on the kernel's own input region(s) X[s] against the kernel's output region / raw rows"""
    x = torch.cat([X[s] for s in src], 1).double()
    w, b = net.w[name], net.b[name]
    r, m, K = x @ w.t() + b, x.abs() @ w.abs().t() + b.abs(), x.shape[1]
    k = X[dst] if isinstance(dst, str) else raw[:, dst[1]: dst[1] + dst[2]]
    region = dst if isinstance(dst, str) else "raw[%s]" % name
    if relu:
        dead = r < -f32_bound(r, m, K + 2)
        if (k < 0).any() or (k[dead] != 0).any():
            rep.fail(region, "ReLU output negative, or non-zero where the pre-activation is below minus its bound")
        r = r.clamp(min=0)
    check_f32(rep, region, k, r, m, K + 2, key="fp32 " + ("raw" if region.startswith("raw") else region.rstrip("0123456789")))


def check_forward(rep, desc, params, rays, z, raw, acts, trig_bound=None):
    """raw: an (S, channels) view of the kernel's image (any strides); acts: the flat fp32 buffer; rays (R, 8), z (R, N)"""
    S = z.numel()
    net = Net(desc, params, acts.device)
    X = read_acts(desc, S, acts)
    check_inputs(rep, desc, rays, z, X, trig_bound)
    for name, src, dst, relu in linears(desc):
        check_linear(rep, net, X, raw, name, src, dst, relu)
    return rep


# ------------------------------------------------------------------------------------------------------------ backward
def dy_chain(desc, Wt, gate, dr):
    """Linear name -> dY (S, n_out) float64 for the upstream dr (S, channels); Wt: name -> weight (or |weight|); gate: region ->
    (S, width) 0 / 1"""
    g = dims(desc)
    W, D = g["W"], g["D"]
    Y = {"rgb_linear": dr[:, 0:3], "alpha_linear": dr[:, 3:4]}
    Y["views_linears.0"] = (dr[:, 0:3] @ Wt["rgb_linear"]) * gate["G"]
    dF = Y["views_linears.0"] @ Wt["views_linears.0"][:, :W]
    dH = 0.0
    for nm, c0, n, sh in heads(desc):
        if g["deep"]:
            Y[nm + ".1"] = dr[:, c0:c0 + n]
            Y[nm + ".0"] = (dr[:, c0:c0 + n] @ Wt[nm + ".1"]) * gate[sh]
        else:
            Y[nm + ".0"] = dr[:, c0:c0 + n]
        t = Y[nm + ".0"] @ Wt[nm + ".0"]
        if g["tap"]:
            dF = dF + t
        else:
            dH = dH + t
    Y["feature_linear"] = dF
    dy = (dH + dF @ Wt["feature_linear"] + dr[:, 3:4] @ Wt["alpha_linear"]) * gate["X%d" % D]
    for l in range(D - 1, -1, -1):
        Y["pts_linears.%d" % l] = dy
        if l:
            w = Wt["pts_linears.%d" % l]
            dy = (dy @ w[:, w.shape[1] - W:]) * gate["X%d" % l]
    return Y


def backward64(desc, net, X, dr):
    """parameter name -> (r64, A) for every weight and bias; X: region -> (S, width) float64 saved activations; dr (S, ch) float64"""
    gate = {nm: (x > 0).double() for nm, x in X.items()}
    Y = dy_chain(desc, net.w, gate, dr)
    Ya = dy_chain(desc, {k: v.abs() for k, v in net.w.items()}, gate, dr.abs())
    out = {}
    for name, src, _, _ in linears(desc):
        x = torch.cat([X[s] for s in src], 1)
        out[name + ".weight"] = (Y[name].t() @ x, Ya[name].t() @ x.abs())
        out[name + ".bias"] = (Y[name].sum(0), Ya[name].sum(0))
    return out


def check_backward(rep, desc, params, acts, d_raw, grads, S):
    """d_raw: (S, channels) view; grads: parameter name -> the kernel's gradient"""
    net = Net(desc, params, acts.device)
    X = {nm: x.double() for nm, x in read_acts(desc, S, acts).items()}
    P = path_lengths(desc)
    ref = backward64(desc, net, X, d_raw.double())
    assert set(ref) == set(params), set(ref) ^ set(params)
    for pname, (r, A) in ref.items():
        k = grads.get(pname)
        if k is None or tuple(k.shape) != tuple(r.shape):
            rep.fail(pname, "missing from the kernel's gradients, or of another shape")
            continue
        lin = pname.rsplit(".", 1)[0]
        kind = "output" if P[lin] == 0 else "chain"
        check_f32(rep, pname, k.to(r.device), r, A, P[lin] + min(S, KSLAB) + n_slabs(S), key="fp32 d%s (%s)" % (pname.rsplit(".", 1)[1], kind))
    return rep


def chain64(desc, params, rays, z):
    """the whole forward in float64 from float64 points (no kernel buffer): (X regions, raw (S, ch)), for the autograd pin"""
    net = Net(desc, params, "cpu")
    rays, z = rays.double(), z.double()
    N = z.shape[1]
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    d = rays[:, 3:6]
    vd = (d / d.norm(dim=1, keepdim=True)).repeat_interleave(N, 0)
    emb = lambda x, L: torch.cat([x] + [f(x * 2.0 ** k) for k in range(L) for f in (torch.sin, torch.cos)], 1)   # noqa: E731
    X = {"EX": emb(pts, desc.xyz_L), "ED": emb(vd, desc.dir_L)}
    raw = torch.zeros((pts.shape[0], 4 + desc.n_sem + desc.n_inst), dtype=torch.float64)
    for name, src, dst, relu in linears(desc):
        y = torch.cat([X[s] for s in src], 1) @ net.w[name].t() + net.b[name]
        y = y.clamp(min=0) if relu else y
        if isinstance(dst, str):
            X[dst] = y
        else:
            raw[:, dst[1]: dst[1] + dst[2]] = y
    return X, raw


# ------------------------------------------------------------------------------ float32 restatement of the kernels' order
def fma_chain(A, B, k_hi=None):
    """(M, K) x (K, N) float32 -> (M, N): one fmaf chain per element in ascending k from 0.0f, each step the float64 product plus
    the accumulator rounded to float32 (the product of two float32 is exact in float64)"""
    A64, B64 = np.asarray(A, np.float32).astype(np.float64), np.asarray(B, np.float32).astype(np.float64)
    acc = np.zeros((A64.shape[0], B64.shape[1]), np.float32)
    for k in range(A64.shape[1] if k_hi is None else k_hi):
        acc = (A64[:, k, None] * B64[None, k, :] + acc).astype(np.float32)
    return acc


def slab_sum32(parts):
    s = np.zeros_like(parts[0])
    for p in parts:                                   # ascending slab order
        s = (s + p).astype(np.float32)
    return s


def colsum32(dy):
    """k_f32_colsum of one slab: 256 strided sums, then the tree red[t] += red[t + w], w = 128 .. 1.  dy (rows, n_out) float32"""
    red = np.zeros((256, dy.shape[1]), np.float32)
    for r in range(0, dy.shape[0], 256):              # thread t adds rows t, t + 256, ... in this order
        n = min(256, dy.shape[0] - r)
        red[:n] = (red[:n] + dy[r:r + n]).astype(np.float32)
    w = 128
    while w:
        red[:w] = (red[:w] + red[w:2 * w]).astype(np.float32)
        w >>= 1
    return red[0]


def forward32(desc, params, rays, z, corrupt=None):
    """(raw (S, ch), acts flat) float32 numpy, as the kernels' order gives them; band values are float64 sin / cos of the stored
    argument rounded once.  corrupt: 'ktile' (pts_linears.0 loses the reduction rows from the last multiple of 16 on),
    'skip_bias' (no bias in the skip layer's second launch), 'skip_order' (the skip layer reads [X, EX]), 'band_swap' (band 1 of gamma(x) stored as cos | sin)."""
    g = dims(desc)
    p = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in params.items()}
    rays, z = np.asarray(rays, np.float32), np.asarray(z, np.float32)
    S, N = z.size, z.shape[1]
    d = rays[:, 3:6]
    nrm = np.sqrt((d.astype(np.float64) ** 2).sum(1)).astype(np.float32)          # (the identity columns only need 8 u)
    vd = np.repeat((d / nrm[:, None]).astype(np.float32), N, 0)

    def emb(x, L, swap=False):
        cols = [x]
        for k in range(L):
            a = (x * np.float32(2.0 ** k)).astype(np.float64)
            sc = [np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)]
            cols += sc[::-1] if (swap and k == 1) else sc
        return np.concatenate(cols, 1)

    X = {"EX": emb(points32(rays, z), desc.xyz_L, corrupt == "band_swap"), "ED": emb(vd, desc.dir_L)}
    raw = np.zeros((S, 4 + desc.n_sem + desc.n_inst), np.float32)
    for name, src, dst, relu in linears(desc):
        w, b = p[name + ".weight"], p[name + ".bias"]
        k1 = X[src[0]].shape[1]
        is_skip = name.startswith("pts") and len(src) == 2
        if is_skip and corrupt == "skip_order":
            W = g["W"]
            v = fma_chain(X[src[1]], w[:, :W].T)
            v = (fma_chain(X[src[0]], w[:, W:].T) + v).astype(np.float32)
        else:
            v = fma_chain(X[src[0]], w[:, :k1].T, k_hi=k1 // 16 * 16 if (corrupt == "ktile" and name == "pts_linears.0") else None)
            if len(src) == 2:
                v = (fma_chain(X[src[1]], w[:, k1:].T) + v).astype(np.float32)            # second launch: acc + *c
        if not (is_skip and corrupt == "skip_bias"):
            v = (v + b).astype(np.float32)
        v = np.maximum(v, np.float32(0)) if relu else v
        if isinstance(dst, str):
            X[dst] = v
        else:
            raw[:, dst[1]: dst[1] + dst[2]] = v
    reg, total = acts_regions(desc, S)
    acts = np.zeros(total, np.float32)
    for nm, (o, wd) in reg.items():
        acts[o:o + S * wd] = X[nm].reshape(-1)
    return raw, acts


def backward32(desc, params, acts, d_raw, corrupt=None):
    """parameter name -> float32 gradient in the kernels' order (linear_dgrad / linear_wgrad of pnr_mlp_backward_fp32).  d_raw
    (S, ch).  corrupt: 'gate' (the top trunk dY is gated by X_{D-1}), 'drop_sample' (the last slab misses its last sample),
    'slab_twice' (the last partial is added twice), 'views_row' (row 1 of views_w's direction columns is row 2's)."""
    g = dims(desc)
    W, H, D = g["W"], g["H"], g["D"]
    p = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in params.items()}
    d_raw = np.asarray(d_raw, np.float32)
    S = d_raw.shape[0]
    reg, _ = acts_regions(desc, S)
    X = {nm: np.asarray(acts[o:o + S * w], np.float32).reshape(S, w) for nm, (o, w) in reg.items()}
    grads = {}

    def dgrad(dy, w, koff, k, prev=None, gate=None):
        v = fma_chain(dy, w[:, koff:koff + k])
        if prev is not None:
            v = (v + prev).astype(np.float32)
        return v * (gate > 0) if gate is not None else v

    def wgrad(name, dy, x, koff, bias):
        bounds = [(lo, min(S, lo + KSLAB)) for lo in range(0, S, KSLAB)]
        if corrupt == "drop_sample":
            bounds[-1] = (bounds[-1][0], bounds[-1][1] - 1)
        parts = [fma_chain(dy[lo:hi].T, x[lo:hi]) for lo, hi in bounds]
        bparts = [colsum32(dy[lo:hi]) for lo, hi in bounds]
        if corrupt == "slab_twice":
            parts, bparts = parts + parts[-1:], bparts + bparts[-1:]
        dw = grads.setdefault(name + ".weight", np.zeros_like(p[name + ".weight"]))
        dw[:, koff:koff + x.shape[1]] = slab_sum32(parts)
        if bias:
            grads[name + ".bias"] = slab_sum32(bparts)

    dr = lambda c0, n: d_raw[:, c0:c0 + n]                                           # noqa: E731
    h, F, G = X["X%d" % D], X["F"], X["G"]
    wgrad("rgb_linear", dr(0, 3), G, 0, True)
    dG = dgrad(dr(0, 3), p["rgb_linear.weight"], 0, H, gate=G)
    wgrad("views_linears.0", dG, F, 0, True)
    wgrad("views_linears.0", dG, X["ED"], W, False)
    if corrupt == "views_row":
        grads["views_linears.0.weight"][1, W:] = grads["views_linears.0.weight"][2, W:]
    dF = dgrad(dG, p["views_linears.0.weight"], 0, W)
    dH = None
    tap = F if g["tap"] else h
    for nm, c0, n, sh in heads(desc):
        if g["deep"]:
            wgrad(nm + ".1", dr(c0, n), X[sh], 0, True)
            dSH = dgrad(dr(c0, n), p[nm + ".1.weight"], 0, H, gate=X[sh])
            wgrad(nm + ".0", dSH, tap, 0, True)
            dy = dSH
        else:
            wgrad(nm + ".0", dr(c0, n), tap, 0, True)
            dy = dr(c0, n)
        if g["tap"]:
            dF = dgrad(dy, p[nm + ".0.weight"], 0, W, prev=dF)
        else:
            dH = dgrad(dy, p[nm + ".0.weight"], 0, W, prev=dH)
    wgrad("feature_linear", dF, h, 0, True)
    wgrad("alpha_linear", dr(3, 1), h, 0, True)
    dH = dgrad(dF, p["feature_linear.weight"], 0, W, prev=dH)
    dY = dgrad(dr(3, 1), p["alpha_linear.weight"], 0, W, prev=dH, gate=X["X%d" % (D - 1)] if corrupt == "gate" else h)
    for l in range(D - 1, -1, -1):
        name = "pts_linears.%d" % l
        if l == 0:
            wgrad(name, dY, X["EX"], 0, True)
            break
        hoff = g["ex"] if l - 1 == g["skip"] else 0
        if hoff:
            wgrad(name, dY, X["EX"], 0, False)
        wgrad(name, dY, X["X%d" % l], hoff, True)
        dY = dgrad(dY, p[name + ".weight"], hoff, W, gate=X["X%d" % l])
    return grads


def localise(d_raw, kind):
    """d_raw (S, ch) with every row zeroed outside the last slab ('slab') or outside the last 64-row tile of the last slab ('tile'):
    A of the bounds then holds those samples only, and an error in the tail is far above the bound"""
    S = d_raw.shape[0]
    lo = (n_slabs(S) - 1) * KSLAB
    if kind == "tile":
        lo += (S - lo - 1) // 64 * 64
    out = d_raw.clone() if isinstance(d_raw, torch.Tensor) else d_raw.copy()
    out[:lo] = 0
    return out
