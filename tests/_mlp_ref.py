"""Test support: a float64, LAYER-LOCAL reference of the bf16 training MLP (k_mlp_fused<TRAIN> / k_mlp_pp<TRAIN>, k_mlp_bwd,
k_wgrad + k_wgrad_reduce), and the one comparison every check uses.  Not part of the product package.

Layer-local: every layer of the reference reads the KERNEL's own saved bf16 input of that layer (acts) or its own stored
upstream gradient (dys), so kernel and reference see the same ReLU gates and the same rounded operands.  What is left between
them is the order of the fp32 accumulation and one rounding to bf16, which is bounded below from first principles.
The forward half (check_forward) works on feature-ordered regions, whoever produced them: check_training hands it Buffers.feat(...),
the inference sweep (tests/_mlp_probe_bf16.py, test_gpu_mlp_bf16_infer_sweep.py) the regions its probe networks read out.

Bounds (u = 2^-24, the unit roundoff of fp32; C_ACC = 2):
  * A fp32 sum of K exact products plus an fp32 bias (bf16 x bf16 products are exact in fp32) differs from the exact sum by at
    most K u m, m = |b| + sum |w x| (the standard recursive-summation bound, any order).  C_ACC = 2 also covers an accumulator
    that truncates instead of rounding to nearest.  K is the reduction length the kernel runs: the padded k-segments
    (pnr_mlp_plan.h), e.g. 32 slots for the [rgb, sigma] gradient block, 64 for a head's logit gradients.
  * bf16 outputs: the kernel value is RNE(acc) (v_cvt_pk_bf16_f32), |acc - r64| <= delta = C_ACC K u m.  So it must lie in
    [RNE(r64 - delta), RNE(r64 + delta)] (one of the two bf16 neighbours of r64 whenever delta < ulp / 2) and equal RNE(r64)
    unless a rounding midpoint lies within delta of r64.
    ReLU outputs are that value clamped at 0; the gate bit must be [saved X > 0] exactly; a gated dY is exactly 0 where the
    gate is 0.
  * fp32 outputs (raw, dW, db): |k - r64| <= C_ACC K_eff u m + ulp(r64).  For the weight gradients K_eff = slab + n_slabs:
    k_wgrad sums one slab of samples per (job, slab) partial, k_wgrad_reduce adds the n_slabs partials (pnr_mlp_wgrad.hip).
  * gamma(x), gamma(d): r64 = sin / cos of 2^f p in float64, p the fp32 sample point (the C oracle's pnr_points, asserted bit for bit
    equal to k_points -- the same separate multiply and add the training forward runs -- by the GPU sweep, and through the xyz slots
    here; so the base-band argument 2^f p is the kernel's exactly) or the float64 unit view direction.  The kernel's fp32 value differs by E_j:
      - sincos_cw at the half-wave's base band: two FMA roundings in the Cody-Waite reduction (<= u each, |r| <= pi/4 + eps),
        the C2 tail's own rounding (|k| |C2| u <= 1e-11 for |x| <= 2^13), five roundings in the polynomial and its sign
        selection (<= 1 each for values <= 1: 5 u) and the minimax truncation of the two polynomials on
        |r| <= pi/4 + 1e-6 (< 1e-8 < u: evaluated in float64 by tests/test_mlp_ref.py::test_sincos_polynomials_truncation): E_0 = 8 u;
      - each double-angle step of embed_next_band: s' = 2 s c, c' = 1 - 2 s^2 has |d c'/d s| = 4 |s| <= 4, so an error E grows
        to at most 4 E, plus one rounding each (2 u): E_{j+1} = 4 E_j + 2 u (the kernel comment's "doubles per octave" is the
        phase part; the amplitude part can grow 4x);
      - gamma(d) only: the kernel normalises d in fp32 (three products, two sums, sqrt, division: <= 8 u relative), and sin / cos
        are 1-Lipschitz, so the argument's error 2^f * 8 u adds to E_j;  the xyz slots of gamma(d) compare with delta = 8 u.
"""
import torch

from panopticnerf_amd import ops
from _wgrad_ref import _inverse, embed_slots, feat_slots, pad_samples, saved_rows

U = 2.0 ** -24
C_ACC = 2.0


# ----------------------------------------------------------------------------------------------------------------- layout
def names(desc):
    """(acts region names in train_layout order, gate region names by acts index, dys region names)"""
    D = desc.D
    acts = ["EX", "ED"] + ["X%d" % (l + 1) for l in range(D)] + ["F", "G", "SH_sem", "SH_inst"]
    gates = {2 + l: "gate_X%d" % (l + 1) for l in range(D)}
    gates.update({3 + D: "gate_G", 4 + D: "gate_SH_sem", 5 + D: "gate_SH_inst"})
    dys = ["DY_views", "DY_feature", "DY_sem0", "DY_inst0"] + ["DY_%d" % l for l in range(D)] + ["dRGBS", "dSEM", "dINST"]
    return acts, gates, dys


def widths(desc):
    D, W, H = desc.D, desc.W, desc.W // 2
    return [64, 32] + [W] * D + [W, H, H, H], [H, W, H, H] + [W] * D + [32, 64, 64]


def gate_offsets(desc, S):
    """acts index -> element offset of its gate-bit region: the regions follow the last bf16 region, each on a 64-element line
    (pnr_train_layout); the last one must end where train_layout's acts total says."""
    D, W = desc.D, desc.W
    ao, _ = ops.train_layout(desc, S)
    Sp = pad_samples(S)
    al = lambda o: (o + 63) // 64 * 64
    o, g = al(ao[5 + D] + Sp * (W // 2)), {}
    for i, w in [(2 + l, W) for l in range(D)] + [(3 + D, W // 2), (4 + D, W // 2), (5 + D, W // 2)]:
        g[i] = o
        o = al(o + Sp * w // 16)
    assert o == ao[6 + D], (o, ao[6 + D])
    return g


def decode_gates(acts, off, S, w):
    """(S, w) bool gate bits of a ReLU output region, FEATURE order.  Per sample w/32 dwords; lane (n, hi) owns dwords
    hi*(w/64) ..; dword j covers blocks 2j, 2j+1; bit 8*(fb&1) + p <-> slot fb*32 + hi*16 + 2p, bit 16 + 8*(fb&1) + p <-> + 1
    (pnr_mlp_layout.h)."""
    Sp, nd = pad_samples(S), w // 32
    words = acts.view(torch.int16)[off: off + Sp * w // 16].view(torch.int32).view(Sp, nd)[:S]
    dw, bit = torch.empty(w, dtype=torch.long), torch.empty(w, dtype=torch.long)
    for fb in range(w // 32):
        for hi in (0, 1):
            for r in range(16):
                s = fb * 32 + hi * 16 + r
                dw[s] = hi * (w // 64) + fb // 2
                bit[s] = (16 if r & 1 else 0) + 8 * (fb & 1) + r // 2
    dw, bit = dw.to(acts.device), bit.to(acts.device)
    bits = ((words[:, dw].to(torch.int64) >> bit) & 1).bool()               # slot order
    return bits.index_select(1, _inverse(feat_slots(w, str(acts.device)), w))


def encode_gates(acts, off, S, w, gates_feat):
    """inverse of decode_gates for rows < S (padding rows: 0).  Test-buffer construction only."""
    Sp, nd = pad_samples(S), w // 32
    slot = gates_feat.index_select(1, feat_slots(w, str(acts.device))).to(torch.int64)        # feature -> slot order
    words = torch.zeros((Sp, nd), dtype=torch.int64, device=acts.device)
    for fb in range(w // 32):
        for hi in (0, 1):
            for r in range(16):
                s = fb * 32 + hi * 16 + r
                words[:S, hi * (w // 64) + fb // 2] |= slot[:, s] << ((16 if r & 1 else 0) + 8 * (fb & 1) + r // 2)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    acts.view(torch.int16)[off: off + Sp * w // 16].view(torch.int32).view(Sp, nd)[:] = words
    return acts


# ---------------------------------------------------------------------------------------------------------- comparison
def bf16_neighbours(r):
    """float64 r -> (RNE(r) to bf16, lower neighbour, upper neighbour, midpoint between them), all float64 (exact: no double
    rounding through fp32)."""
    m, e = torch.frexp(r)
    sc = m * 256.0                                   # 8 significand bits
    scale = torch.exp2((e - 8).to(r.dtype))           # (torch.ldexp's integer power of 2 is not exact on every device)
    lo, hi = torch.floor(sc), torch.ceil(sc)
    return torch.round(sc) * scale, lo * scale, hi * scale, (lo + 0.5) * scale


class Report:
    """Failures and the worst error / bound per (quantity): the measured headroom comes from here."""

    def __init__(self):
        self.worst, self.fails, self.ledger = {}, [], {}

    def note(self, key, ratio):
        self.worst[key] = max(self.worst.get(key, 0.0), float(ratio))

    def fail(self, region, msg):
        self.fails.append("%s: %s" % (region, msg))

    def check(self):
        assert not self.fails, "\n".join(self.fails[:12])


def check_bf16(rep, region, k, r64, delta, relu=False, gate=None, s0=0):
    """k: kernel bf16 values (any float dtype), r64 / delta float64, same shape.  gate (bool) or None.
    The kernel value is RNE(acc) with |acc - r64| <= delta; RNE is monotone, so it must lie in [RNE(r64 - delta), RNE(r64 + delta)]
    -- one of the two neighbours of r64 while delta < ulp / 2, more where cancellation leaves |r64| far below m -- and it must equal
    RNE(r64) unless r64 lies within delta of a rounding midpoint."""
    k = k.double()
    rne = bf16_neighbours(r64)[0]
    lo, hi = bf16_neighbours(r64 - delta)[0], bf16_neighbours(r64 + delta)[0]
    if relu:
        rne, lo, hi = rne.clamp(min=0), lo.clamp(min=0), hi.clamp(min=0)
    ok = (k == rne) | ((k >= lo) & (k <= hi))
    if gate is not None:
        ok = torch.where(gate, ok, k == 0)
    excused = ok & (k != rne)
    if excused.any():           # error / bound: how far acc must have been from r64 to round to k, relative to delta
        _, e = torch.frexp(k)
        need = ((k - r64).abs() - torch.exp2((e - 9).to(k.dtype))).clamp(min=0)
        rep.note("bf16 " + region.rstrip("0123456789"), (need / delta.clamp(min=1e-300))[excused].max())
    if not ok.all():
        i = torch.nonzero(~ok)[0].tolist()
        rep.fail(region, "%d of %d bf16 values off (first at sample %d col %d: kernel %r, r64 %r, delta %.3g)"
                 % (int((~ok).sum()), ok.numel(), i[0] + s0, i[1], k[tuple(i)].item(), r64[tuple(i)].item(), delta[tuple(i)].item()))


def check_f32(rep, region, k, r64, m, K_eff, key=None):
    k = k.double()
    _, e = torch.frexp(r64)
    ulp = torch.exp2((e - 24).clamp(min=-149).to(r64.dtype))
    bound = C_ACC * K_eff * U * m + ulp
    ratio = (k - r64).abs() / bound
    rep.note(key or ("fp32 " + region), ratio.max() if ratio.numel() else 0.0)
    bad = ~(ratio <= 1.0)
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        rep.fail(region, "%d of %d fp32 values off (first at %s: kernel %r, r64 %r, bound %.3g)"
                 % (int(bad.sum()), bad.numel(), i, k[tuple(i)].item(), r64[tuple(i)].item(), bound[tuple(i)].item()))


# ------------------------------------------------------------------------------------------------------ the network math
class Net:
    """desc + fp32 parameters (nn.Linear names) -> bf16-rounded float64 weights, float64 biases, on `device`."""

    def __init__(self, desc, params, device):
        self.desc, self.dev = desc, device
        self.D, self.W, self.H, self.skip = desc.D, desc.W, desc.W // 2, desc.skip
        self.C, self.K, self.tap, self.depth = desc.n_sem, desc.n_inst, desc.head_tap, (1 if desc.head_depth == 1 else 2)
        self.Lx, self.Ld = desc.xyz_L, desc.dir_L
        self.w = {k[:-7]: v.detach().to(device, torch.float32).to(torch.bfloat16).double()
                  for k, v in params.items() if k.endswith(".weight")}
        self.b = {k[:-5]: v.detach().to(device, torch.float64) for k, v in params.items() if k.endswith(".bias")}
        self.sem = ("semantic_linears.1", "semantic_linears.0") if self.depth == 2 else (None, "semantic_linears.0")
        self.inst = ("instance_linears.1", "instance_linears.0") if self.depth == 2 else (None, "instance_linears.0")

    def lin(self, name, x, cols=None):
        """-> (r64 = b + W x, m = |b| + |W| |x|, K) of a Linear; cols: a column slice of W (a k-segment)."""
        w = self.w[name] if cols is None else self.w[name][:, cols]
        return x @ w.t() + self.b[name], x.abs() @ w.abs().t() + self.b[name].abs(), x.shape[1]

    # forward: region -> (weight name, inputs)
    def fwd_inputs(self, region, X):
        D = self.D
        if region.startswith("X"):
            l = int(region[1:]) - 1
            if l == 0:
                return "pts_linears.0", X["EX"]
            if l - 1 == self.skip:
                return "pts_linears.%d" % l, torch.cat([X["EX"], X["X%d" % l]], 1)
            return "pts_linears.%d" % l, X["X%d" % l]
        if region == "F":
            return "feature_linear", X["X%d" % D]
        if region == "G":
            return "views_linears.0", torch.cat([X["F"], X["ED"]], 1)
        return {"SH_sem": "semantic_linears.0", "SH_inst": "instance_linears.0"}[region], X["F"] if self.tap else X["X%d" % D]

    def fwd(self, region, X):
        """r64, m, K of a saved hidden region, or of 'raw' (S, 4 + C + K) fp32 rows."""
        if region != "raw":
            name, x = self.fwd_inputs(region, X)
            return self.lin(name, x)
        parts = [self.lin(name, X[src]) for name, _, _, src in self.raw_parts()]
        K = torch.tensor([float(p[2]) for p in parts for _ in range(p[0].shape[1])], dtype=torch.float64, device=self.dev)
        return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), K

    def raw_parts(self):
        """[(Linear name, first raw channel, rows, input region)] of the fp32 rows, in channel order"""
        xd = "X%d" % self.D
        tap = "F" if self.tap else xd
        out = [("rgb_linear", 0, 3, "G"), ("alpha_linear", 3, 1, xd)]
        for (last, first), c0, n, sh in ((self.sem, 4, self.C, "SH_sem"), (self.inst, 4 + self.C, self.K, "SH_inst")):
            if n:
                out.append((last, c0, n, sh) if self.depth == 2 else (first, c0, n, tap))
        return out

    def regions_fwd(self):
        out = ["X%d" % (l + 1) for l in range(self.D)] + ["F", "G"]
        if self.depth == 2:
            out += (["SH_sem"] if self.C else []) + (["SH_inst"] if self.K else [])
        return out

    # backward: dY region -> list of (weight name, columns of W, upstream dY), K (the kernel's padded k length), gate region
    def bwd_terms(self, region, Y):
        D, W, H = self.D, self.W, self.H
        head = []
        if region in ("DY_feature", "DY_%d" % (D - 1)):
            if self.C:
                head.append((self.sem[1], None, Y["DY_sem0"] if self.depth == 2 else Y["dSEM"][:, :self.C]))
            if self.K:
                head.append((self.inst[1], None, Y["DY_inst0"] if self.depth == 2 else Y["dINST"][:, :self.K]))
        if region == "DY_views":
            return [("rgb_linear", None, Y["dRGBS"][:, :3])], 32, "G"
        if region == "DY_sem0":
            return [("semantic_linears.1", None, Y["dSEM"][:, :self.C])], 64, "SH_sem"
        if region == "DY_inst0":
            return [("instance_linears.1", None, Y["dINST"][:, :self.K])], 64, "SH_inst"
        if region == "DY_feature":
            t = [("views_linears.0", slice(0, W), Y["DY_views"])]
            return (t + head, 3 * H, None) if self.tap else (t, H, None)
        if region == "DY_%d" % (D - 1):
            t = [("feature_linear", None, Y["DY_feature"]), ("alpha_linear", None, Y["dRGBS"][:, 3:4])]
            return (t, W + 32, "X%d" % D) if self.tap else (t + head, W + 32 + 2 * H, "X%d" % D)
        l = int(region[3:]) + 1                       # DY_{l-1} = gate(X_l) (W_l[:, h columns]^T DY_l)
        cols = slice(self.w["pts_linears.%d" % l].shape[1] - W, None)
        return [("pts_linears.%d" % l, cols, Y["DY_%d" % l])], W, "X%d" % l

    def bwd(self, region, Y):
        terms, K, gate = self.bwd_terms(region, Y)
        r = m = 0.0
        for name, cols, dy in terms:
            w = self.w[name] if cols is None else self.w[name][:, cols]
            r = r + dy @ w
            m = m + dy.abs() @ w.abs()
        return r, m, K, gate

    def regions_bwd(self):
        D = self.D
        out = ["DY_views"]
        if self.depth == 2:
            out += (["DY_sem0"] if self.C else []) + (["DY_inst0"] if self.K else [])
        return out + ["DY_feature"] + ["DY_%d" % l for l in range(D - 1, -1, -1)]

    # weight gradients: parameter name -> (dY, X) pairs (columns concatenated)
    def wgrad_terms(self, X, Y):
        D, C, K = self.D, self.C, self.K
        tapx = X["F"] if self.tap else X["X%d" % D]
        t = {}
        for l in range(D):
            t["pts_linears.%d" % l] = (Y["DY_%d" % l], self.fwd_inputs("X%d" % (l + 1), X)[1])
        t["feature_linear"] = (Y["DY_feature"], X["X%d" % D])
        t["views_linears.0"] = (Y["DY_views"], torch.cat([X["F"], X["ED"]], 1))
        t["rgb_linear"] = (Y["dRGBS"][:, :3], X["G"])
        t["alpha_linear"] = (Y["dRGBS"][:, 3:4], X["X%d" % D])
        if C:
            if self.depth == 2:
                t["semantic_linears.0"] = (Y["DY_sem0"], tapx)
                t["semantic_linears.1"] = (Y["dSEM"][:, :C], X["SH_sem"])
            else:
                t["semantic_linears.0"] = (Y["dSEM"][:, :C], tapx)
        if K:
            if self.depth == 2:
                t["instance_linears.0"] = (Y["DY_inst0"], tapx)
                t["instance_linears.1"] = (Y["dINST"][:, :K], X["SH_inst"])
            else:
                t["instance_linears.0"] = (Y["dINST"][:, :K], tapx)
        return t


# ------------------------------------------------------------------------------------------------------------- embedding
def _band_err(j):
    e = 8 * U
    for _ in range(j):
        e = 4 * e + 2 * U
    return e


def embed_ref(p, nf, dir_arg_err=0.0):
    """p (S, 3) float64 -> (values, delta) (S, 6 nf + 3) in canonical column order with ALL 2 nf bands (the kernel computes
    every band; pnr_seg_col hides those >= L from the weights).  delta: the E_j of the header.
    dir_arg_err: relative error of p itself (gamma(d): the fp32 normalisation), added as 2^f * it to band f."""
    S = p.shape[0]
    vals, dl = [p], [torch.zeros_like(p)]
    for f in range(2 * nf):
        a = p * 2.0 ** f
        vals += [torch.sin(a), torch.cos(a)]
        e = _band_err(f % nf)
        dl += [torch.full((S, 6), e, dtype=torch.float64, device=p.device)]
    v = torch.cat([vals[0]] + [torch.cat([vals[1 + 2 * f], vals[2 + 2 * f]], 1) for f in range(2 * nf)], 1)
    dl = torch.cat(dl, 1)
    if dir_arg_err:
        dl[:, :3] += dir_arg_err
        for f in range(2 * nf):
            dl[:, 3 + 6 * f: 9 + 6 * f] += 2.0 ** f * dir_arg_err
    return v, dl


def embed_slot_ref(p, nf, dir_arg_err=0.0):
    """(values, delta) of a saved EX (nf = 5, 64 slots) / ED (nf = 2, 32 slots) region in SLOT order; pads are exactly 0."""
    v, dl = embed_ref(p, nf, dir_arg_err)
    idx = embed_slots(nf, 2 * nf, str(p.device))               # every band's slot
    ok = idx >= 0
    vs = torch.zeros((p.shape[0], idx.numel()), dtype=torch.float64, device=p.device)
    ds = torch.zeros_like(vs)
    vs[:, ok], ds[:, ok] = v[:, idx[ok]], dl[:, idx[ok]]
    return vs, ds


def unit_dirs64(rays):
    d = rays[:, 3:6].double()
    return d / d.norm(dim=1, keepdim=True)


# ----------------------------------------------------------------------------------------------------- reading buffers
class Buffers:
    """The kernel's training buffers as FEATURE-ordered bf16 tensors (S, width); embeddings also in slot order."""

    def __init__(self, desc, S, acts, dys=None):
        self.desc, self.S = desc, S
        self.ao, self.do = ops.train_layout(desc, S)
        self.go = gate_offsets(desc, S)
        self.acts, self.dys = acts, dys
        self.an, self.gn, self.dn = names(desc)
        self.aw, self.dw = widths(desc)
        dev = str(acts.device)
        self.ex_can = _inverse(embed_slots(5, desc.xyz_L, dev), 3 + 6 * desc.xyz_L)
        self.ed_can = _inverse(embed_slots(2, desc.dir_L, dev), 3 + 6 * desc.dir_L)

    def slots(self, name, pad=False):
        if name in self.an:
            i = self.an.index(name)
            return saved_rows(self.acts, self.ao[i], pad_samples(self.S) if pad else self.S, self.aw[i])
        i = self.dn.index(name)
        return saved_rows(self.dys, self.do[i], pad_samples(self.S) if pad else self.S, self.dw[i])

    def feat(self, name):
        t = self.slots(name)
        if name == "EX":
            return t.index_select(1, self.ex_can)
        if name == "ED":
            return t.index_select(1, self.ed_can)
        return t.index_select(1, _inverse(feat_slots(t.shape[1], str(t.device)), t.shape[1]))

    def gate(self, name):
        i = self.an.index(name)
        return decode_gates(self.acts, self.go[i], self.S, self.aw[i])


def wgrad_slabs(desc, S):
    """(most samples one k_wgrad slab can hold, slab count) of pnr_mlp_wgrad for S samples, from the library's own workspace
    arithmetic rather than a restatement of its slab heuristic: the workspace is a 1 KiB head plus n_slabs equal per-slab
    blocks of partial sums, and S = 1 is one slab.  n_slabs = ceil(S / slab) gives slab < S / (n_slabs - 1)."""
    import ctypes
    from panopticnerf_amd import _lib
    ws = lambda n: int(_lib.load().pnr_mlp_wgrad_workspace_bytes(ctypes.byref(desc), int(n))) - 1024
    per_slab = ws(1)
    assert per_slab > 0 and ws(S) % per_slab == 0, (per_slab, ws(S))
    n_slabs = ws(S) // per_slab
    return (S if n_slabs == 1 else min(S, -(-S // (n_slabs - 1)))), n_slabs


# ------------------------------------------------------------------------------------------------------------ the check
def check_forward(rep, net, X, raw=None, pts=None, vd64=None, s0=0, regions=None, parts=None):
    """The forward half of the layer-local check over FEATURE-ordered regions, whoever produced them (the training forward's saved
    buffers through Buffers.feat, or the inference kernels' probe read-out of tests/_mlp_probe_bf16.py).
    X: region -> (S, width) float64 kernel values; raw: (S, channels) fp32 rows, or None.  pts (S, 3) fp32 sample points and vd64
    (S, 3) float64 unit view directions: where given, EX / ED are checked over the bands the weights see (identity columns of EX =
    bf16-RNE of pts bit for bit, bands inside the E_j of the header, ED with the 8 u direction term).  regions: the hidden regions
    to check (default: those of net.regions_fwd() that X holds); parts: the Linear names of raw_parts() to check (default: all).
    Every region is checked against float64 on the kernel's OWN input region(s), which X must hold."""
    if pts is not None:
        ex = 3 + 6 * net.Lx
        if not torch.equal(X["EX"][:, :3], pts.to(torch.bfloat16).double()):
            rep.fail("EX", "the xyz columns are not bf16 of the sample points (fp32 points differ from k_points?)")
        v, dl = embed_ref(pts.double(), 5)
        check_bf16(rep, "EX", X["EX"], v[:, :ex], dl[:, :ex], s0=s0)
    if vd64 is not None:
        ed = 3 + 6 * net.Ld
        v, dl = embed_ref(vd64, 2, dir_arg_err=8 * U)
        check_bf16(rep, "ED", X["ED"], v[:, :ed], dl[:, :ed], s0=s0)
    for nm in [r for r in net.regions_fwd() if r in X] if regions is None else regions:
        r, m, K = net.fwd(nm, X)
        check_bf16(rep, nm, X[nm], r, C_ACC * K * U * m, relu=nm != "F", s0=s0)
    if raw is not None:
        for name, c0, n, src in net.raw_parts():
            if parts is None or name in parts:
                r, m, K = net.lin(name, X[src])
                check_f32(rep, "raw[%s]" % name, raw[:, c0:c0 + n], r, m, K, key="fp32 raw")


def check_training(desc, params, pts, rays, raw, acts, dys=None, d_raw=None, grads=None, chunk=1 << 16, rep=None):
    """Every region of a training forward (raw, acts with gates), and if given of the data-gradient pass (dys) and of the
    weight gradients (grads), against the float64 layer-local reference.  pts (S, 3) fp32 sample points (bit-exact with the
    kernel's), rays (R, 8) fp32; raw / d_raw (ch, S) channel-major fp32.  Returns the Report; its ledger names every region
    of train_layout and every gradient tensor as 'checked' or 'unused: <why>'."""
    rep = rep or Report()
    net = Net(desc, params, acts.device)
    S = pts.shape[0]
    B = Buffers(desc, S, acts, dys)
    dev = acts.device
    an, gn, dn = B.an, B.gn, B.dn
    L = rep.ledger
    N = S // rays.shape[0]
    assert S == rays.shape[0] * N, "the kernels take S = R x N samples (a ragged count is R = 1, N = S)"
    vd64 = unit_dirs64(rays.to(dev)).repeat_interleave(N, 0)
    p64 = pts.to(dev).double()
    fwd_regions = net.regions_fwd()
    for nm in ("SH_sem", "SH_inst"):
        if nm not in fwd_regions:
            why = "unused: head_depth 1 (no hidden head layer)" if net.depth == 1 else "unused: no %s head" % nm[3:]
            L[nm] = L["gate_" + nm] = why
    bwd = dys is not None
    if bwd:
        for nm, c, why in (("dSEM", net.C, "no semantic head"), ("dINST", net.K, "no instance head")):
            if not c:
                L[nm] = "unused: " + why
        for nm, c in (("DY_sem0", net.C), ("DY_inst0", net.K)):
            if nm not in net.regions_bwd():
                L[nm] = "unused: head_depth 1 (the logit gradients feed the tap)" if net.depth == 1 else "unused: no head"
    # the feature-ordered bf16 tensors, whole S (bf16: small), chunks of them go float64
    Xb = {nm: B.feat(nm) for nm in ["EX", "ED"] + fwd_regions}
    Gb = {nm: B.gate(nm) for nm in fwd_regions if nm not in ("F",)}
    Yb = {}
    if bwd:
        Yb = {nm: B.feat(nm) for nm in ["dRGBS"] + (["dSEM"] if net.C else []) + (["dINST"] if net.K else []) + net.regions_bwd()}
    ex_slots, ed_slots = B.slots("EX"), B.slots("ED")
    for s0 in range(0, S, chunk):
        s1 = min(S, s0 + chunk)
        X = {k: v[s0:s1].double() for k, v in Xb.items()}
        # the feature-ordered half: visible embedding columns, every hidden region, every raw row
        check_forward(rep, net, X, raw[:, s0:s1].t(), pts[s0:s1].to(dev), vd64[s0:s1], s0=s0, regions=fwd_regions)
        # embeddings once more in slot order: pads and every band, also those the weights do not see
        v, dl = embed_slot_ref(p64[s0:s1], 5)
        xyz = ex_slots[s0:s1, [0, 1, 32]].double()
        if not torch.equal(xyz, pts[s0:s1].to(dev).to(torch.bfloat16).double()):
            rep.fail("EX", "the saved xyz slots are not bf16 of the sample points (fp32 points differ from k_points?)")
        check_bf16(rep, "EX", ex_slots[s0:s1], v, dl, s0=s0)
        v, dl = embed_slot_ref(vd64[s0:s1], 2, dir_arg_err=8 * U)
        check_bf16(rep, "ED", ed_slots[s0:s1], v, dl, s0=s0)
        for nm in fwd_regions:
            if nm != "F":
                g = Gb[nm][s0:s1]
                if not torch.equal(g, X[nm] > 0):
                    rep.fail("gate_" + nm, "%d gate bits differ from [X > 0]" % int((g != (X[nm] > 0)).sum()))
        if bwd:
            Y = {k: v[s0:s1].double() for k, v in Yb.items()}
            dr = d_raw[:, s0:s1].t()
            for nm, c0, n, w in (("dRGBS", 0, 4, 32), ("dSEM", 4, net.C, 64), ("dINST", 4 + net.C, net.K, 64)):
                if nm not in Y:
                    continue
                want = torch.zeros((s1 - s0, w), dtype=torch.float64, device=dev)
                want[:, :n] = dr[:, c0:c0 + n].to(torch.bfloat16).double()
                if not torch.equal(Y[nm], want):
                    rep.fail(nm, "stored d_raw block is not bf16-RNE of d_raw with zero padding channels (%d values differ)"
                             % int((Y[nm] != want).sum()))
            for nm in net.regions_bwd():
                r, m, K, gate = net.bwd(nm, Y)
                g = Gb[gate][s0:s1] if gate else None
                check_bf16(rep, nm, Y[nm], r, C_ACC * K * U * m, gate=g, s0=s0)
    for nm in ["EX", "ED"] + fwd_regions:
        L[nm] = "checked"
    for nm in fwd_regions:
        if nm != "F":
            L["gate_" + nm] = "checked"
    # acts padding rows: finite (the kernels' contract: the wgrad reads them unmasked against zero dY)
    Sp = pad_samples(S)
    if Sp > S:
        for nm in ["EX", "ED"] + fwd_regions:
            if not torch.isfinite(B.slots(nm, pad=True)[S:].float()).all():
                rep.fail(nm, "non-finite padding row")
    if bwd:
        for nm in Yb:
            L[nm] = "checked"
            if Sp > S and torch.count_nonzero(B.slots(nm, pad=True)[S:]):
                rep.fail(nm, "non-zero dY in the padding rows S..S_pad")
    if grads is not None:
        check_wgrad(rep, net, Xb, Yb, grads, S, chunk)
    return rep


def wgrad64(net, Xb, Yb, S, chunk=1 << 16):
    """name -> (dW64, |dY|^T |X|, db64, sum |dY|) over all S samples, float64 from the stored bf16 buffers"""
    acc = {}
    for s0 in range(0, S, chunk):
        s1 = min(S, s0 + chunk)
        X = {k: v[s0:s1].double() for k, v in Xb.items()}
        Y = {k: v[s0:s1].double() for k, v in Yb.items()}
        for name, (dy, x) in net.wgrad_terms(X, Y).items():
            t = (dy.t() @ x, dy.abs().t() @ x.abs(), dy.sum(0), dy.abs().sum(0))
            acc[name] = t if name not in acc else tuple(a + b for a, b in zip(acc[name], t))
    return acc


def check_wgrad(rep, net, Xb, Yb, grads, S, chunk=1 << 16):
    slab, n_slabs = wgrad_slabs(net.desc, S)
    K_eff = slab + n_slabs
    for name, (dw, mw, db, mb) in wgrad64(net, Xb, Yb, S, chunk).items():
        for suf, r, m in ((".weight", dw, mw), (".bias", db, mb)):
            k = grads.get(name + suf)
            if k is None:
                rep.fail(name + suf, "missing from the kernel's gradients")
                continue
            if tuple(k.shape) != tuple(r.shape):
                rep.fail(name + suf, "shape %s, expected %s" % (tuple(k.shape), tuple(r.shape)))
                continue
            check_f32(rep, name + suf, k.to(r.device), r, m, K_eff, key="fp32 d" + suf[1:])
            rep.ledger[name + suf] = "checked"
