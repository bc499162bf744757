"""CPU tests of plan 3, the sigma-only image (pnr_mlp_plan.h, pnr_mlp_pack.cpp) that k_mlp_pp_sigma consumes, and of the
Renderer switch that uses it (cfg.coarse_outputs).  The image must hold the trunk exactly as the fused plans hold it, then one
32-row block whose row 3 is alpha_linear over h: the very fragments of the rgb / sigma chunk's h segment -- which is why the
sigma-only kernel reproduces the other plans' compositing weights bit for bit (tests/test_gpu_coarse_weights.py)."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from _emulate import PackedImage
from panopticnerf_amd import _lib, make_network, make_renderer, ops

GEOMS = {     # id: (D, W, skips, C, K, head_tap, head_depth)
    "8x256_45+32": (8, 256, [4], 45, 32, "trunk", 2),
    "8x256_0+0": (8, 256, [4], 0, 0, "trunk", 2),
    "8x256_96+0": (8, 256, [4], 96, 0, "trunk", 2),
    "8x256_tap_feature": (8, 256, [4], 45, 32, "feature", 2),
    "8x256_head_depth1": (8, 256, [4], 45, 32, "trunk", 1),
    "4x128_noskip": (4, 128, [], 0, 0, "trunk", 2),
    "2x128_skip_last": (2, 128, [0], 19, 8, "trunk", 2),       # the last trunk layer is the one behind the skip
}


def _net(geom):
    D, W, skips, C, K, tap, depth = GEOMS[geom]
    torch.manual_seed(D * 1000 + W + C + K)
    return make_network(NS(D=D, W=W, skips=skips, num_classes=C, num_instances=K, head_tap=tap, head_depth=depth)).nerf_0


def _with_plan(desc, plan):
    d = _lib.MlpDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc), ctypes.sizeof(d))
    d.plan = plan
    return d


def _plan_ok(desc, plan):
    return int(_lib.load().pnr_mlp_packed_bytes(ctypes.byref(_with_plan(desc, plan)))) > 0


def _trunk(im, D, W, skip):
    """The trunk of a packed image: ({(layer, first block, blocks): chunk bytes}, [(weight fragments, 128 bias bytes) per 32-row
    block, in layer order], number of trunk chunks)."""
    chunks, blocks, ci = {}, [], 0
    for layer in range(D):
        nks = 4 if layer == 0 else (4 + W // 16 if layer - 1 == skip else W // 16)      # gamma(x): 32 values / 8 per k-step
        fb = 0
        while fb < W // 32:
            off, nfrag = (int(v) for v in im.table[ci])
            nfb = (nfrag - 1) // nks
            assert nfb * nks + 1 == nfrag
            raw = im.b[im.data_off + off * 1024: im.data_off + (off + nfrag) * 1024]
            chunks[(layer, fb, nfb)] = raw
            bias = raw[(nfrag - 1) * 1024:]
            for b in range(nfb):
                blocks.append((raw[b * nks * 1024:(b + 1) * nks * 1024], bias[b * 128:(b + 1) * 128]))
            fb += nfb
            ci += 1
    return chunks, blocks, ci


def _sigma_fragments(alpha_w, W):
    """What the sigma chunk's k-step fragments must hold: lane l (row l & 31, half l >> 5), value j of k-step ks is h column
    pnr_seg_col(FEAT, hi, 8 ks + j) of alpha_linear in row 3, zero in every other row (bf16, round to nearest even)."""
    a = alpha_w.detach().reshape(-1).to(torch.bfloat16).float().numpy()
    out = np.zeros((W // 16, 64, 8), np.float32)
    for ks in range(W // 16):
        for hi in (0, 1):
            for j in range(8):
                v = ks * 8 + j
                r = v & 15
                col = (v >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi
                out[ks, 3 + 32 * hi, j] = a[col]
    return out


@pytest.mark.parametrize("geom", list(GEOMS))
def test_sigma_image_is_the_fused_trunk_and_the_sigma_row(geom):
    net = _net(geom)
    D, W, skip = net.D, net.W, net.skip
    sd = net.state_dict()
    desc = net.desc("bf16")
    img3 = ops.pack_mlp(_with_plan(desc, 3), sd)
    im3 = PackedImage(img3)
    assert int(im3.desc[9]) == 3
    chunks3, blocks3, n_trunk = _trunk(im3, D, W, skip)
    assert im3.n_chunks == n_trunk + 1                                  # trunk, then the one sigma chunk
    assert (0, 0, W // 32) in chunks3                                    # layer 0 as ONE chunk (plans 1 and 2)
    plans = [p for p in (0, 1, 2) if _plan_ok(desc, p)]
    assert 0 in plans
    for p in plans:
        img = ops.pack_mlp(_with_plan(desc, p), sd)
        assert img3.numel() < img.numel(), (p, img3.numel(), img.numel())
        im = PackedImage(img)
        chunks, blocks, n_trunk_p = _trunk(im, D, W, skip)
        assert len(blocks) == len(blocks3) == D * W // 32
        for b, (x, y) in enumerate(zip(blocks, blocks3)):                # every trunk weight fragment and bias row, whatever the chunking
            assert x == y, (p, b)
        same = set(chunks) & set(chunks3)
        assert all(chunks[k] == chunks3[k] for k in same), p
        if p == 1:      # plan 3 chunks the trunk exactly as plan 1 does: byte-identical chunk for chunk
            assert set(chunks) == set(chunks3)
        if p == 0:
            # the rgb / sigma chunk of the classic image: g segment (W/32 k-steps, zero in row 3), then h -- whose fragments ARE
            # the sigma chunk's, byte for byte
            A, _ = im.chunk(n_trunk_p + W // 64 + W // 128)              # behind the feature (W/64 chunks) and views (W/128) layers
            assert not A[:W // 32, 3].any() and not A[:W // 32, 35].any()
            A3, _ = im3.chunk(n_trunk)
            assert np.array_equal(A[W // 32:].view(np.uint32), A3.view(np.uint32))
    A3, bias3 = im3.chunk(n_trunk)
    assert A3.shape == (W // 16, 64, 8)
    np.testing.assert_array_equal(A3, _sigma_fragments(net.alpha_linear.weight, W))
    want_b = np.zeros(256, np.float32)
    want_b[3] = float(net.alpha_linear.bias.detach()[0])
    np.testing.assert_array_equal(bias3, want_b)


def test_sigma_image_needs_only_the_trunk_and_alpha_linear():
    net = _net("8x256_45+32")
    sd = net.state_dict()
    lean = {k: v for k, v in sd.items() if k.startswith(("pts_linears.", "alpha_linear."))}
    d3 = _with_plan(net.desc("bf16"), 3)
    assert torch.equal(ops.pack_mlp(d3, lean), ops.pack_mlp(d3, sd))
    with pytest.raises(RuntimeError, match="missing"):
        ops.pack_mlp(net.desc("bf16"), lean)                             # plan 0 reads every layer
    with pytest.raises(RuntimeError, match="alpha_linear"):
        ops.pack_mlp(d3, {k: v for k, v in lean.items() if not k.startswith("alpha_linear.")})


def test_sigma_plan_is_bf16_only_and_never_the_default():
    lib = _lib.load()
    for geom in GEOMS:
        net = _net(geom)
        d32 = _with_plan(net.desc("fp32"), 3)
        assert int(lib.pnr_mlp_packed_bytes(ctypes.byref(d32))) == -1          # PNR_EINVAL
        d = net.desc("bf16")
        assert _plan_ok(d, 3)
        for flags in (0, _lib.MLP_SOFTMAX):
            d.flags = flags
            assert int(lib.pnr_mlp_fused_plan(ctypes.byref(d))) in (0, 1, 2)
            assert ops.fused_plan(d, None) in (0, 1, 2)
        d.flags = 0
        assert ops.sigma_pass_supported(d, 64) and not ops.sigma_pass_supported(net.desc("fp32"), 64)
        assert not ops.sigma_pass_supported(d, 48) and not ops.sigma_pass_supported(d, 288)
    # a descriptor that is not zero-initialised is rejected as for every other plan
    d = _with_plan(ops.make_desc(), 3)
    d.flags = 0x2
    assert int(lib.pnr_mlp_packed_bytes(ctypes.byref(d))) < 0


def test_renderer_coarse_outputs_switch():
    cfg = NS(N_samples=64, N_importance=128, num_classes=5, num_instances=3)
    net = make_network(cfg)
    assert make_renderer(cfg, net).coarse_outputs == "all"
    assert make_renderer(NS(coarse_outputs="weights", **vars(cfg)), net).coarse_outputs == "weights"
    with pytest.raises(ValueError, match="coarse_outputs"):
        make_renderer(NS(coarse_outputs="sigma", **vars(cfg)), net)
    coarse_only = NS(N_samples=64, N_importance=0, num_classes=5, num_instances=3)
    assert make_renderer(coarse_only, make_network(coarse_only)).coarse_outputs == "all"
    with pytest.raises(ValueError, match="fine level"):
        make_renderer(NS(coarse_outputs="weights", **vars(coarse_only)), make_network(coarse_only))
