"""Test support for the weight packers (test_pack_values.py, test_gpu_pack_device.py): the geometries, random and planted
parameters, the header of a packed image, and a restatement of what a packed image must hold that does not restate the fragment
layout.  Not part of the product package.

The restatement.  Every word of an image's data area is a copy of ONE parameter element (or zero padding).  Which one is read
off the packer itself: pack parameters whose values are their own element number (source_map; two packs, 14 bits of the number
each, as float32 bit patterns (digit + 1) << 16 that survive both the bf16 rounding and a verbatim copy), and the image is a
table word -> element.  expected_data() then fills that table with the values of any other parameter set under the layout
header's rule: fp32 images and bias fragments carry the float32 bits verbatim, bf16 weight fragments pnr_f32_to_bf16 of them --
restated here in numpy integer arithmetic (f32_to_bf16)."""
import ctypes

import numpy as np
import torch

from panopticnerf_amd import _lib, ops

# ------------------------------------------------------------------------------------------------------------ geometries
# (D, W, skip, n_sem, n_inst, head_tap, head_depth, xyz_L, dir_L): the order of test_gpu_mlp_sweep.GEOMS
GEOM_ID = "D%d_W%d_s%d_C%d_K%d_%s%d_L%d_%d"


def geometries():
    """one list, without repeats: the geometries of the two training sweeps, D = 16 with and without a skip, the head-width grid
    at a 256-wide network that has every plan and at a 128-wide one with shallow heads, both head depths and taps at both widths,
    and the short encodings"""
    from test_gpu_mlp_fp32_sweep import GEOMS as G32
    from test_gpu_mlp_sweep import GEOMS as G16
    out = list(G16) + [(D, W, s, C, K, tap, dep, Lx, Ld) for D, W, s, Lx, Ld, C, K, tap, dep in G32]
    out += [(16, 256, 14, 45, 32, "trunk", 2, 10, 4), (16, 256, -1, 45, 32, "trunk", 2, 10, 4),
            (16, 128, 14, 5, 3, "feature", 1, 10, 4), (16, 128, -1, 5, 3, "trunk", 2, 3, 1)]
    for C in (0, 1, 31, 32, 33, 64, 65, 96, 97, 200, 256):
        for K in (0, 1, 33, 256):
            out += [(8, 256, 4, C, K, "trunk", 2, 10, 4), (3, 128, 1, C, K, "feature", 1, 10, 4)]
    for W in (128, 256):
        for tap in ("trunk", "feature"):
            for dep in (1, 2):
                out.append((4, W, 1, 19, 8, tap, dep, 10, 4))
    for Lx in (0, 3, 10):
        for Ld in (0, 1, 4):
            out += [(3, 128, 1, 6, 4, "trunk", 2, Lx, Ld), (8, 256, 4, 45, 32, "trunk", 2, Lx, Ld)]
    seen, uniq = set(), []
    for g in out:
        if g not in seen:
            seen.add(g)
            uniq.append(g)
    return uniq


def make_desc(geom, precision="bf16", plan=0):
    D, W, skip, C, K, tap, dep, Lx, Ld = geom
    d = ops.make_desc(D, W, skip, Lx, Ld, C, K, W // 2, precision, tap, dep)
    d.plan = plan
    return d


def shapes(geom):
    """name -> shape of every parameter of the network, canonical NeRF names (panopticnerf_amd/network.py)"""
    D, W, skip, C, K, tap, dep, Lx, Ld = geom
    ex, ed, H = 3 + 6 * Lx, 3 + 6 * Ld, W // 2
    lin = {"pts_linears.0": (W, ex)}
    for i in range(1, D):
        lin["pts_linears.%d" % i] = (W, W + ex if i - 1 == skip else W)
    lin.update({"alpha_linear": (1, W), "feature_linear": (W, W), "views_linears.0": (H, W + ed), "rgb_linear": (3, H)})
    for head, n in (("semantic_linears", C), ("instance_linears", K)):
        if n and dep == 2:
            lin.update({head + ".0": (H, W), head + ".1": (n, H)})
        elif n:
            lin[head + ".0"] = (n, W)
    sh = {}
    for k, (o, i) in lin.items():
        sh[k + ".weight"], sh[k + ".bias"] = (o, i), (o,)
    return sh


def random_params(geom, seed=0):
    """float32 CPU tensors, every element drawn on its own: a fragment packed from the wrong place differs"""
    rng = np.random.default_rng(1000 + seed)
    return {k: torch.from_numpy(rng.uniform(-1.0, 1.0, s).astype(np.float32)) for k, s in shapes(geom).items()}


def images(geom):
    """[(label, desc, backward)]: every image the library packs for the geometry -- plan 0 always, plans 1 .. 4 where
    pnr_mlp_packed_bytes accepts them, fp32 at plan 0, the transposed image where pnr_mlp_bwd_packed_bytes is positive"""
    lib = _lib.load()
    out = [("bf16/plan0/fwd", make_desc(geom), 0)]
    for plan in (1, 2, 3, 4):
        d = make_desc(geom, plan=plan)
        if lib.pnr_mlp_packed_bytes(ctypes.byref(d)) > 0:
            out.append(("bf16/plan%d/fwd" % plan, d, 0))
    out.append(("fp32/plan0/fwd", make_desc(geom, "fp32"), 0))
    if lib.pnr_mlp_bwd_packed_bytes(ctypes.byref(out[0][1])) > 0:
        out.append(("bf16/plan0/bwd", make_desc(geom), 1))
    return out


def host_image(desc, params, backward=False):
    return (ops.pack_mlp_bwd if backward else ops.pack_mlp)(desc, params)


# ---------------------------------------------------------------------------------------------------------------- header
def header(img):
    """pnr_pack_header of an image (a CPU uint8 tensor): the fields as a dict, gap = the bytes between the chunk table and the
    data area, n_frags = fragments of the data area by the header's own arithmetic"""
    b = img[:128].numpy().tobytes()
    w = np.frombuffer(b, np.uint32, 6)
    h = dict(magic=int(w[0]), version=int(w[1]), n_chunks=int(w[2]), max_chunk_frags=int(w[3]), table_off=int(w[4]), data_off=int(w[5]),
             total_bytes=int(np.frombuffer(b, np.uint64, 1, 24)[0]))
    h["gap"] = (h["table_off"] + 8 * h["n_chunks"], h["data_off"])
    assert (h["total_bytes"] - h["data_off"]) % 1024 == 0
    h["n_frags"] = (h["total_bytes"] - h["data_off"]) // 1024
    return h


# --------------------------------------------------------------------------------------------------------------- values
def f32_to_bf16(u):
    """pnr_f32_to_bf16 of pnr_mlp_layout.h on float32 BIT PATTERNS (uint32 array -> uint16 array): round to nearest, ties to
    even, in integer arithmetic; a NaN keeps its sign and upper payload and gets the quiet bit, (u >> 16) | 0x40"""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def f32_to_bf16_truncating(u):
    """a WRONG restatement: drops the low half"""
    return (np.asarray(u, np.uint32) >> 16).astype(np.uint16)


def f32_to_bf16_half_up(u):
    """a WRONG restatement: ties away from zero (add half an ulp, truncate)"""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, (u + 0x8000) >> 16).astype(np.uint16)


NANS = [0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FC12345, 0x7F812345, 0xFF80FFFF]      # quiet, signalling, negative, with payload
PLANTED = np.array(NANS + [
    0x7F800000, 0xFF800000, 0x00000000, 0x80000000,      # +-Inf, +-0
    0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF,      # the smallest and the largest subnormal
    0x00010000, 0x00400000, 0x80400000,                  # subnormals that are bf16 subnormals exactly
    0x7F7FFFFF,                                          # FLT_MAX: rounds to bf16 Inf
    0x3F808000, 0x3F818000,                              # ties: down to the even 0x3F80, up to the even 0x3F82
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,      # their neighbours
], np.uint32)
SUBNORMALS = [0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x00010000, 0x00400000, 0x80400000]

# a network with a skip (the layer behind it is pts_linears.2) and a semantic head of three logit blocks; the transposed image
# exists only up to 64 logits, so its case has two blocks
PLANT_GEOM = (3, 128, 1, 70, 3, "trunk", 2, 10, 4)
PLANT_GEOM_BWD = (3, 128, 1, 40, 3, "trunk", 2, 10, 4)


def planted_params(geom, seed=0):
    """random_params with PLANTED written, as bit patterns, into weights and biases of a trunk layer, the gamma(x) columns of the
    layer behind the skip, the last logit block of the semantic head, alpha_linear and rgb_linear.  Returns (params, places):
    places = [(name, flat index, bits)]"""
    p = {k: v.clone() for k, v in random_params(geom, seed).items()}
    n, C = len(PLANTED), geom[3]
    ex = 3 + 6 * geom[7]
    assert n <= ex and geom[2] == 1 and C > 32
    last = C - 1 - (C - 1) % 32                          # first row of the last logit block
    bits = {k: v.numpy().view(np.uint32) for k, v in p.items()}      # views: writes go to the tensors
    places = []

    def plant(name, index, values):
        flat = bits[name].reshape(-1)
        for i, v in zip(index, values):
            flat[i] = v
            places.append((name, int(i), int(v)))

    W = geom[1]
    plant("pts_linears.1.weight", 5 * W + 7 + np.arange(n), PLANTED)                     # a row of a plain trunk layer
    plant("pts_linears.1.weight", (np.arange(n) * 5 + 1) * W + 64, PLANTED)              # and a column
    plant("pts_linears.1.bias", 3 + np.arange(n), PLANTED)
    plant("pts_linears.2.weight", 9 * (W + ex) + np.arange(n), PLANTED)                  # gamma(x) columns of the skip layer
    plant("pts_linears.2.weight", 100 * (W + ex) + ex - n + np.arange(n), PLANTED[::-1])
    plant("pts_linears.2.bias", W - n + np.arange(n), PLANTED)
    plant("semantic_linears.1.weight", (last + 2) * (W // 2) + 11 + np.arange(n), PLANTED)
    plant("semantic_linears.1.bias", last + np.arange(C - last), PLANTED)
    plant("alpha_linear.weight", 10 + np.arange(n), PLANTED)
    plant("alpha_linear.bias", [0], [0x7F800001])
    plant("rgb_linear.weight", (W // 2) + np.arange(n), PLANTED)                         # row 1
    plant("rgb_linear.bias", [0, 1, 2], [0x807FFFFF, 0xFFC00000, 0x3F808000])
    return p, places


# --------------------------------------------------------------------------------------------------- word -> element table
def _numbering(sh):
    """name -> (first element number, count); numbers start at 1 (0 = no element)"""
    base, o = {}, 1
    for k, s in sh.items():
        n = int(np.prod(s))
        base[k] = (o, n)
        o += n
    return base, o - 1


def source_map(geom, desc, backward=False):
    """For every word of the data area of the HOST image of (desc, backward) -- 32-bit words of an fp32 image, 16-bit words of a
    bf16 one -- the number of the parameter element it is a copy of, 0 where it is padding.  In a bf16 image a bias (kept as
    float32) has its number on the UPPER half-word and 0 on the lower."""
    sh = shapes(geom)
    base, total = _numbering(sh)
    assert total < 1 << 28
    digits = []
    for shift in (0, 14):
        p = {}
        for k, s in sh.items():
            ids = np.arange(base[k][0], base[k][0] + base[k][1], dtype=np.uint32)
            p[k] = torch.from_numpy(((((ids >> shift) & 0x3FFF) + 1) << 16).astype(np.uint32).view(np.float32).reshape(s))
        img = host_image(desc, p, backward)
        data = img[header(img)["data_off"]:].numpy()
        if desc.precision == _lib.PREC_BF16 or backward:
            digits.append(data.view(np.uint16).astype(np.int64))
        else:
            w = data.view(np.uint32)
            assert not (w & 0xFFFF).any()
            digits.append((w >> 16).astype(np.int64))
    lo, hi = digits
    assert ((lo == 0) == (hi == 0)).all()
    return np.where(lo > 0, (lo - 1) + ((hi - 1) << 14), 0)


def expected_data(geom, desc, params, backward=False, to_bf16=f32_to_bf16, smap=None):
    """the data area (uint8 array) that the rule of the module docstring gives for `params`"""
    sh = shapes(geom)
    base, total = _numbering(sh)
    flat = np.zeros(total + 1, np.uint32)
    is_bias = np.zeros(total + 1, bool)
    for k in sh:
        o, n = base[k]
        flat[o:o + n] = params[k].detach().cpu().contiguous().numpy().view(np.uint32).reshape(-1)
        is_bias[o:o + n] = k.endswith(".bias")
    m = source_map(geom, desc, backward) if smap is None else smap
    if not (desc.precision == _lib.PREC_BF16 or backward):
        return flat[m].view(np.uint8)
    out = np.where(is_bias[m], (flat[m] >> 16).astype(np.uint16), to_bf16(flat[m]))
    out[m == 0] = 0
    at = np.nonzero(is_bias[m])[0]
    assert (at % 2 == 1).all() and not m[at - 1].any()
    out[at - 1] = (flat[m[at]] & 0xFFFF).astype(np.uint16)
    return out.view(np.uint8)


def word_of(smap, geom, name, index):
    """positions in the table of source_map that hold element `index` (flat) of parameter `name`"""
    base, _ = _numbering(shapes(geom))
    return np.nonzero(smap == base[name][0] + index)[0]
