"""CPU tests of the field query (Network.query / ops.mlp_query / pnr_mlp_query): plan 4, the packed image k_mlp_pp_field consumes
(pnr_mlp_plan.h, pnr_mlp_pack.cpp), the C entry point's argument checks, and the Python surface's refusals.

Plan 4 = plan 3's chunks (the trunk with layer 0 as one chunk, the sigma block), then feature_linear where the heads read it, then
the head chunks of plan 0.  The kernel multiplies those fragments in plan 0's order, so what makes its sigma and logits the classic
pass's bits (tests/test_gpu_field_query.py) is checked here on the bytes: the trunk and sigma chunks ARE the plan-3 image's, every
head / feature chunk IS the plan-0 image's chunk of the same layer and blocks."""
import ctypes
import itertools
from types import SimpleNamespace as NS

import pytest
import torch

from _emulate import PackedImage
from oracle import torch_oracle as to
from panopticnerf_amd import _lib, make_network, ops

TRUNKS = {"8x256_skip4": (8, 256, [4]), "4x128_noskip": (4, 128, []), "3x128_skip1": (3, 128, [1])}
HEADS = [(0, 0), (45, 32), (45, 0), (0, 32), (96, 0)]
MATRIX = [(t, c, k, tap, depth) for t in TRUNKS for (c, k) in HEADS for tap in ("trunk", "feature") for depth in (2, 1)]


def _net(trunk, C, K, tap, depth, precision="bf16"):
    D, W, skips = TRUNKS[trunk]
    torch.manual_seed(D * 1000 + W + 7 * C + K)
    return make_network(NS(D=D, W=W, skips=skips, num_classes=C, num_instances=K, head_tap=tap, head_depth=depth,
                           precision=precision)).nerf_0


def _with_plan(desc, plan):
    d = _lib.MlpDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc), ctypes.sizeof(d))
    d.plan = plan
    return d


def _chunk_bytes(im, ci):
    off, nfrag = (int(v) for v in im.table[ci])
    return im.b[im.data_off + off * 1024: im.data_off + (off + nfrag) * 1024]


def _n_trunk_chunks(im, D, W, skip):
    """Chunks of the trunk at the head of a packed image (whatever its chunking of a layer)."""
    ci = 0
    for layer in range(D):
        nks = 4 if layer == 0 else (4 + W // 16 if layer - 1 == skip else W // 16)
        fb = 0
        while fb < W // 32:
            nfrag = int(im.table[ci, 1])
            assert (nfrag - 1) % nks == 0
            fb += (nfrag - 1) // nks
            ci += 1
        assert fb == W // 32
    return ci


# ---------------------------------------------------------------- 1. the premise (passes without the feature)
@pytest.mark.parametrize("tap,depth,emulate", list(itertools.product(("trunk", "feature"), (2, 1), (False, True))))
def test_sigma_and_logits_do_not_depend_on_the_view_direction(tap, depth, emulate):
    cfg = to.mlp_config(D=4, W=64, skips=(1,), n_sem=7, n_inst=5, head_W=32, head_tap=tap, head_depth=depth)
    p = to.init_params(cfg, seed=3)
    g = torch.Generator().manual_seed(1)
    pts = torch.rand(257, 3, generator=g) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(2, 257, 3, generator=g), dim=-1)
    a = to.mlp_forward(p, cfg, pts, d[0], emulate_bf16=emulate)
    b = to.mlp_forward(p, cfg, pts, d[1], emulate_bf16=emulate)
    assert torch.equal(a[:, 3:], b[:, 3:])
    assert not torch.equal(a[:, :3], b[:, :3])          # the colour does depend on it: the two directions are really different


# ---------------------------------------------------------------- 2. the packed image
@pytest.mark.parametrize("trunk,C,K,tap,depth", MATRIX)
def test_field_image_is_plan3_then_the_classic_head_chunks(trunk, C, K, tap, depth):
    net = _net(trunk, C, K, tap, depth)
    D, W, skip = net.D, net.W, net.skip
    sd = net.state_dict()
    desc = net.desc("bf16")
    img4, img3, img0 = (ops.pack_mlp(_with_plan(desc, p), sd) for p in (4, 3, 0))
    im4, im3, im0 = PackedImage(img4), PackedImage(img3), PackedImage(img0)
    assert int(im4.desc[9]) == 4
    assert int(_lib.load().pnr_mlp_packed_bytes(ctypes.byref(_with_plan(desc, 4)))) == img4.numel() < img0.numel()
    # trunk and sigma chunks: the plan-3 image's bytes, chunk for chunk
    nt = _n_trunk_chunks(im4, D, W, skip)
    assert nt == _n_trunk_chunks(im3, D, W, skip) and im3.n_chunks == nt + 1
    for ci in range(nt + 1):
        assert _chunk_bytes(im4, ci) == _chunk_bytes(im3, ci), ci
    # behind them: [feature_linear] and the heads -- plan 0's chunks (same layer, same blocks, same k-steps, same bias fragment)
    nt0 = _n_trunk_chunks(im0, D, W, skip)
    feat0, heads0 = nt0, nt0 + W // 64 + W // 128 + 1          # plan 0: trunk | feature (W/64 chunks) | views (W/128) | rgb + sigma | heads
    want = []
    if tap == "feature" and (C or K):
        want += [_chunk_bytes(im0, feat0 + i) for i in range(W // 64)]
    want += [_chunk_bytes(im0, ci) for ci in range(heads0, im0.n_chunks)]
    nfb = lambda n: (n + 31) // 32
    n_head_chunks = sum((W // 128 if depth == 2 else 0) + nfb(n) for n in (C, K) if n)
    assert im0.n_chunks - heads0 == n_head_chunks          # this test's own map of the classic image
    got = [_chunk_bytes(im4, ci) for ci in range(nt + 1, im4.n_chunks)]
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, i
    # the stream is sequential and dense: chunk offsets follow one another
    off = 0
    for ci in range(im4.n_chunks):
        assert int(im4.table[ci, 0]) == off
        off += int(im4.table[ci, 1])
    if not (C or K):        # a sigma-only network: the plan-3 image but for the descriptor's plan word
        b4, b3 = bytearray(img4.numpy().tobytes()), bytearray(img3.numpy().tobytes())
        assert len(b4) == len(b3)
        assert b4[32 + 36:32 + 40] == (4).to_bytes(4, "little") and b3[32 + 36:32 + 40] == (3).to_bytes(4, "little")
        b4[32 + 36:32 + 40] = b3[32 + 36:32 + 40]
        assert b4 == b3


def test_field_image_reads_no_view_branch_parameter():
    net = _net("8x256_skip4", 45, 32, "trunk", 2)
    sd = net.state_dict()
    d4 = _with_plan(net.desc("bf16"), 4)
    lean = {k: v for k, v in sd.items() if not k.startswith(("views_linears.", "rgb_linear.", "feature_linear."))}
    assert torch.equal(ops.pack_mlp(d4, lean), ops.pack_mlp(d4, sd))
    netf = _net("8x256_skip4", 45, 32, "feature", 2)
    d4f = _with_plan(netf.desc("bf16"), 4)
    leanf = {k: v for k, v in netf.state_dict().items() if not k.startswith(("views_linears.", "rgb_linear.", "feature_linear."))}
    with pytest.raises(RuntimeError, match="feature_linear"):
        ops.pack_mlp(d4f, leanf)
    with pytest.raises(RuntimeError, match="semantic head"):
        ops.pack_mlp(d4, {k: v for k, v in lean.items() if not k.startswith("semantic_linears.")})


# ---------------------------------------------------------------- 3. which geometries, and never by default
@pytest.mark.parametrize("trunk,C,K,tap,depth", MATRIX)
def test_field_plan_is_never_the_default(trunk, C, K, tap, depth):
    lib = _lib.load()
    d = _net(trunk, C, K, tap, depth).desc("bf16")
    for flags in (0, _lib.MLP_SOFTMAX):
        d.flags = flags
        assert int(lib.pnr_mlp_fused_plan(ctypes.byref(d))) in (0, 1, 2)
    d.flags = 0
    assert lib.pnr_mlp_query_supported(ctypes.byref(d)) == 1 and ops.field_query_supported(d)
    assert lib.pnr_mlp_query_supported(ctypes.byref(_with_plan(d, 4))) == 1          # the descriptor's own plan is ignored


def test_field_query_is_bf16_and_w128_or_w256_only():
    lib = _lib.load()
    d32 = _net("8x256_skip4", 45, 32, "trunk", 2).desc("fp32")
    assert lib.pnr_mlp_query_supported(ctypes.byref(d32)) == 0 and not ops.field_query_supported(d32)
    assert int(lib.pnr_mlp_packed_bytes(ctypes.byref(_with_plan(d32, 4)))) == -1
    for W in (64, 192, 512):
        d = ops.make_desc(D=4, W=W, skip=1, n_sem=5, n_inst=0)
        assert lib.pnr_mlp_query_supported(ctypes.byref(d)) == 0, W
        assert int(lib.pnr_mlp_packed_bytes(ctypes.byref(_with_plan(d, 4)))) < 0, W
    assert lib.pnr_mlp_query_supported(None) == 0
    assert lib.pnr_mlp_query_supported(ctypes.byref(ops.make_desc(n_sem=130, n_inst=0))) == 1      # heads wider than 128 logits
    bad = ops.make_desc()
    bad.flags = 0x2                  # not zero-initialised: no kernel is promised for it
    assert lib.pnr_mlp_query_supported(ctypes.byref(bad)) == 0


# ---------------------------------------------------------------- 4. the C entry point checks its arguments before any device work
def _query(lib, desc, packed=16, points=16, n=64, sigma=0, sem_label=0, inst_label=0, panoptic=0, is_thing=0, sem_logits=0,
           inst_logits=0, stride=0):
    v = ctypes.c_void_p
    return lib.pnr_mlp_query(ctypes.byref(desc) if desc is not None else None, v(packed), v(points), n, v(sigma), v(sem_label),
                             v(inst_label), v(panoptic), v(is_thing), v(sem_logits), v(inst_logits), stride, v(0))


def test_query_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    both = _with_plan(ops.make_desc(n_sem=45, n_inst=32), 4)
    sem_only = _with_plan(ops.make_desc(n_sem=45, n_inst=0), 4)
    inst_only = _with_plan(ops.make_desc(n_sem=0, n_inst=32), 4)
    none = _with_plan(ops.make_desc(), 4)
    P = 16                              # a non-null pointer that is never dereferenced: validation fails first
    cases = {
        "null descriptor": dict(desc=None, sigma=P),
        "null packed": dict(desc=both, packed=0, sigma=P),
        "null points": dict(desc=both, points=0, sigma=P),
        "negative n_points": dict(desc=both, n=-1, sigma=P),
        "n_points above the limit": dict(desc=both, n=(1 << 31) - 4096, sigma=P),
        "every output null": dict(desc=both),
        "sem_label without a semantic head": dict(desc=inst_only, sem_label=P),
        "sem_logits without a semantic head": dict(desc=none, sem_logits=P, stride=64),
        "panoptic without a semantic head": dict(desc=inst_only, panoptic=P),
        "inst_label without an instance head": dict(desc=sem_only, inst_label=P),
        "inst_logits without an instance head": dict(desc=sem_only, inst_logits=P, stride=64),
        "is_thing without a semantic head": dict(desc=inst_only, inst_label=P, is_thing=P),
        "logit_stride < n_points": dict(desc=both, sem_logits=P, stride=63),
        "not the field plan (0)": dict(desc=_with_plan(both, 0), sigma=P),
        "not the field plan (3)": dict(desc=_with_plan(both, 3), sigma=P),
        "fp32": dict(desc=_with_plan(ops.make_desc(n_sem=45, n_inst=32, precision="fp32"), 4), sigma=P),
        "unsupported width": dict(desc=_with_plan(ops.make_desc(D=4, W=64, skip=1), 4), sigma=P),
    }
    for what, kw in cases.items():
        assert _query(lib, **kw) == -1, what
        assert b"pnr_mlp_query" in lib.pnr_last_error(), (what, lib.pnr_last_error())
    # nothing to do is not an error (pointers may then be null), and is decided before any device work
    assert _query(lib, both, packed=0, points=0, n=0, sigma=P) == 0
    assert _query(lib, both, n=0, sem_label=P, inst_label=P, panoptic=P, is_thing=P, sem_logits=P, inst_logits=P, stride=0) == 0


def test_other_entry_points_refuse_a_field_image_by_name():
    lib = _lib.load()
    d4 = _with_plan(ops.make_desc(n_sem=45, n_inst=32), 4)
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    assert lib.pnr_mlp_forward(ctypes.byref(d4), one, one, one, 4, 8, one, 1, 32, null) == -1
    assert b"pnr_mlp_forward" in lib.pnr_last_error() and b"plan-4" in lib.pnr_last_error()
    assert lib.pnr_mlp_forward_train(ctypes.byref(d4), one, one, one, 4, 8, one, 1, 32, one, null) == -1
    assert b"plan-4" in lib.pnr_last_error()
    assert lib.pnr_mlp_forward_tiles(ctypes.byref(d4), one, one, one, 4, 64, one, null) == -1
    assert b"pnr_mlp_forward_composite" in lib.pnr_last_error() and b"plan-4" in lib.pnr_last_error()
    assert lib.pnr_mlp_forward_composite(ctypes.byref(d4), one, one, one, 4, 64, null, null, 0, null, one, null, null, null, null,
                                         null, null, one, null) == -1
    assert b"plan-4" in lib.pnr_last_error()
    assert lib.pnr_composite_combine(ctypes.byref(d4), one, one, 4, 64, null, null, 0, null, one, null, null, null, null, null, null,
                                     null) == -1
    assert b"pnr_composite_combine" in lib.pnr_last_error() and b"plan-4" in lib.pnr_last_error()
    assert int(lib.pnr_mlp_bwd_packed_bytes(ctypes.byref(d4))) < 0          # the backward is plan 0 only
    with pytest.raises(ValueError, match="plan-4"):
        ops.mlp_query(ops.make_desc(), None, None)


# ---------------------------------------------------------------- 5. the Python surface
def test_network_query_refuses_cpu_points_and_unknown_outputs():
    net = make_network(NS(N_samples=64, N_importance=64, num_classes=5, num_instances=3))
    pts = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        net.query(pts)
    with pytest.raises(ValueError, match="colour"):
        net.query(pts, want=("sigma", "colour"))
    with pytest.raises(ValueError, match="rgb"):
        net.query_grid((0, 0, 0), (1, 1, 1), 4, want="rgb")
    with pytest.raises(RuntimeError, match="GPU"):
        net.query_grid((0, 0, 0), (1, 1, 1), 4)                      # the parameters live on the CPU
    bare = make_network(NS(N_samples=64, N_importance=0))
    with pytest.raises(ValueError, match="nothing"):
        bare.query(pts, want=("labels",))
    d = net.nerf_0.desc("bf16")
    assert ops.query_keys(d, ("sigma", "labels")) == ["sigma", "sem_label", "inst_label"]
    assert ops.query_keys(d, ("logits", "panoptic")) == ["panoptic", "sem_logits", "inst_logits"]
    assert ops.query_keys(bare.nerf_0.desc("bf16"), ("sigma", "labels", "panoptic", "logits")) == ["sigma"]


def test_field_image_is_cached_and_invalidated_like_the_others():
    net = make_network(NS(N_samples=64, N_importance=64, num_classes=5, num_instances=3)).eval()
    d, img = net.packed(1, "cpu", fused="field")
    assert d.plan == 4 and net.packed(1, "cpu", fused="field")[1] is img          # served from the cache
    assert net.packed(1, "cpu")[0].plan == 0 and net.packed(1, "cpu", fused="sigma")[0].plan == 3
    with torch.no_grad():
        net.nerf_1.alpha_linear.bias.add_(1.0)                                     # bumps the tensor version
    img2 = net.packed(1, "cpu", fused="field")[1]
    assert img2 is not img and not torch.equal(img2, img)
    net.nerf_1.alpha_linear.bias.data.add_(1.0)                                    # invisible to versions ...
    assert net.packed(1, "cpu", fused="field")[1] is img2
    net.invalidate_packed()                                                        # ... hence the explicit call
    assert not torch.equal(net.packed(1, "cpu", fused="field")[1], img2)
    img3 = net.packed(1, "cpu", fused="field")[1]
    net.train()
    net.eval()                                                                     # every train <-> eval switch drops the images
    assert net.packed(1, "cpu", fused="field")[1] is not img3
