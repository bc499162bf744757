"""cfg.coarse_outputs = "weights" on an MI355X: an inference render evaluates the coarse level with the sigma-only kernel
(k_mlp_pp_sigma on the plan-3 image: the trunk and alpha_linear alone) and returns the coarse level only for what the fine level and
the bbox prior read of it.  Every value it does return must be the bits of the full render ("all"): the sigma-only kernel writes
the same Q and local weights as every other plan (the sigma row's fragments and their order are the rgb / sigma chunk's h
segment; its g segment adds exact zeros to row 3), so weights_0, depth_0, acc_0, fix_*_0, z_vals_1 and the whole fine level are
unchanged."""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

from _fused_io import labels, rays_z
from panopticnerf_amd import _lib, make_network, make_renderer, ops, synthetic

pytestmark = pytest.mark.gpu

DROPPED = {"rgb_0", "semantic_0", "instance_0"}
_NETS = {}


def _net(dev, C, K, tap="trunk", depth=2, D=8, W=256, skips=(4,)):
    key = (C, K, tap, depth, D, W, tuple(skips), str(dev))
    if key not in _NETS:
        torch.manual_seed(C * 7 + K + depth + D + W)
        net = make_network(NS(D=D, W=W, skips=list(skips), N_importance=128, num_classes=C, num_instances=K, head_tap=tap,
                              head_depth=depth)).to(dev).eval()
        synthetic.trained_like_(net, 0.05)
        _NETS[key] = net
    return _NETS[key]


def _sigma_images(net):
    return [k for k in net._packed if k[0] == "fwd" and k[-1] == 3]


def _batch(dev, R, C, K, with_box, step=127):
    rays = synthetic.camera_rays()[::step][:R].contiguous().to(dev)
    assert rays.shape[0] == R
    b = {"rays": rays[None]}
    if with_box:
        box, ids = synthetic.random_boxes(64, max(C, 1), max(K, 1))
        b.update(bbox=box.to(dev), bbox_ids=ids.to(dev))
    return b


def _check_equal(a, w):
    assert set(w) == set(a) - DROPPED and not DROPPED & set(w)
    for k in w:
        assert w[k].shape == a[k].shape and torch.equal(w[k], a[k]), k


@pytest.mark.parametrize("Nc,Nf", [(64, 128), (32, 96), (128, 128)])
@pytest.mark.parametrize("with_box", [False, True])
@pytest.mark.parametrize("act", ["logits", "softmax"])
@pytest.mark.parametrize("tap,depth", [("trunk", 2), ("feature", 2), ("trunk", 1)])
@pytest.mark.parametrize("heads", [(45, 32), (45, 0), (0, 0), (96, 0)])
def test_weights_mode_equals_the_full_render(dev, heads, tap, depth, act, with_box, Nc, Nf):
    C, K = heads
    net = _net(dev, C, K, tap, depth)
    base = dict(N_samples=Nc, N_importance=Nf, num_classes=C, num_instances=K, precision="bf16", semantic_activation=act)
    b = _batch(dev, 3001, C, K, with_box)
    net._packed.clear()
    with torch.no_grad():
        a = make_renderer(NS(coarse_outputs="all", **base), net).render(b)
        assert _sigma_images(net) == []
        w = make_renderer(NS(coarse_outputs="weights", **base), net).render(b)
        assert _sigma_images(net) != []                     # the sigma-only kernel ran: no fallback
    torch.cuda.synchronize()
    _check_equal(a, w)
    assert ("fix_semantic_0" in w) == bool(with_box and C) and ("fix_instance_0" in w) == bool(with_box and K)


def test_weights_mode_on_a_frame_of_several_chunks(dev):
    """Frame-sized outputs built from the first chunk's keys; the frame runs serially (the sigma-only launch takes no workgroup cap):
    no side stream is created, and the frame equals the full render -- which may overlap its levels -- bit for bit, twice."""
    C, K = 45, 32
    net = _net(dev, C, K)
    base = dict(N_samples=64, N_importance=128, num_classes=C, num_instances=K, precision="bf16", chunk_size=4096,
                keep_weights=True, overlap_levels=True)
    b = _batch(dev, 18000, C, K, True, step=29)
    with torch.no_grad():
        r_all = make_renderer(NS(coarse_outputs="all", **base), net)
        a = r_all.render(b)
        r_w = make_renderer(NS(coarse_outputs="weights", **base), net)
        assert r_w.frame_outputs and r_w._overlap_caps(dev, [(0, 1), (1, 2)], False, False, True, None, None) is None
        w = r_w.render(b)
        w2 = r_w.render(b)
        assert r_w._side_streams == {}
        e = r_w.render({"rays": b["rays"][:, :0], "bbox": b["bbox"], "bbox_ids": b["bbox_ids"]})
    torch.cuda.synchronize()
    _check_equal(a, w)
    _check_equal(a, w2)
    assert set(e) == set(w) and all(v.shape[1] == 0 for v in e.values())


def _tiles(desc, img, rays, z, rf):
    """pnr_mlp_forward_tiles into a 0xAB-filled workspace: (Q of every tile, quadruples (S, 4))"""
    lib = _lib.load()
    R, N = z.shape
    S = R * N
    nbytes = int(lib.pnr_mlp_forward_composite_workspace_bytes(ctypes.byref(desc), R, N, 0))
    pad = (S + 255) // 256 * 8
    if desc.plan == 3:
        assert nbytes == pad * rf * 4 + S * 16 + 256
    ws = torch.full((nbytes,), 0xAB, device=z.device, dtype=torch.uint8)
    _lib.check(lib.pnr_mlp_forward_tiles(ctypes.byref(desc), ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(rays.data_ptr()),
                                         ctypes.c_void_p(z.data_ptr()), R, N, ctypes.c_void_p(ws.data_ptr()),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pnr_mlp_forward_tiles")
    q = ws[:pad * rf * 4].view(torch.float32).reshape(pad, rf)[: (S + 31) // 32, 0]
    ps = ws[pad * rf * 4: pad * rf * 4 + S * 16].view(torch.float32).reshape(S, 4)
    return q.clone(), ps.clone()


@pytest.mark.parametrize("geom", ["8x256_45+32", "4x128", "2x128_skip_last"])
@pytest.mark.parametrize("N", [32, 64, 96, 128, 192, 256])
@pytest.mark.parametrize("R", [1, 7, 1001, 2051])
def test_sigma_records_equal_every_fused_plan(dev, geom, R, N):
    C, K, D, W, skips = {"8x256_45+32": (45, 32, 8, 256, (4,)), "4x128": (0, 0, 4, 128, ()),
                         "2x128_skip_last": (19, 8, 2, 128, (0,))}[geom]
    net = _net(dev, C, K, D=D, W=W, skips=skips)
    rays, z = rays_z(R * 1000 + N, R, N)
    rays, z = torch.from_numpy(rays).to(dev), torch.from_numpy(z).to(dev)
    d3, i3 = net.packed(0, dev, "bf16", fused="sigma")
    assert d3.plan == 3
    q3, ps3 = _tiles(d3, i3, rays, z, 4)
    plans = [0, 1, 2] if geom == "8x256_45+32" else [0]
    for p in plans:
        dp, ip = net.packed(0, dev, "bf16", fused=p)
        assert dp.plan == p
        qp, psp = _tiles(dp, ip, rays, z, (1 + C + K + 3) & ~3)
        assert torch.equal(q3.view(torch.int32), qp.view(torch.int32)), p
        assert torch.equal(ps3[:, 0].view(torch.int32), psp[:, 0].view(torch.int32)), p
    assert not ps3[:, 1:].any()                                 # r = g = b = 0: no rgb row in the image
    q3b, ps3b = _tiles(d3, i3, rays, z, 4)                      # a second launch leaves the same bits
    assert torch.equal(q3.view(torch.int32), q3b.view(torch.int32)) and torch.equal(ps3.view(torch.int32), ps3b.view(torch.int32))
    ds = ops.desc_for_mode(d3, 1)                               # PNR_MLP_SOFTMAX: accepted, nothing to act on
    q3s, ps3s = _tiles(ds, i3, rays, z, 4)
    assert torch.equal(q3.view(torch.int32), q3s.view(torch.int32)) and torch.equal(ps3.view(torch.int32), ps3s.view(torch.int32))
    # the maps of mlp_forward_weights are mlp_forward_composite's on the classic image, bit for bit (k_composite_combine<false>)
    ls = torch.from_numpy(labels(N, R, N, C)).to(dev) if C else None
    li = torch.from_numpy(labels(N + 1, R, N, K)).to(dev) if K else None
    d0, i0 = net.packed(0, dev, "bf16", fused=0)
    full = ops.mlp_forward_composite(d0, i0, rays, z, ls, li, False, True)
    wts = ops.mlp_forward_weights(d3, i3, rays, z, ls, li)
    assert set(wts) == set(full) - {"rgb", "semantic", "instance"}
    for k in wts:
        assert torch.equal(wts[k], full[k]), k


def test_fallbacks_give_the_reduced_keys_and_equal_maps(dev):
    C, K = 19, 8
    # fp32 parity mode: no fused pass, so the full coarse level runs and its three maps are dropped
    net = _net(dev, C, K)
    b = _batch(dev, 1500, C, K, True)
    base = dict(N_samples=64, N_importance=128, num_classes=C, num_instances=K, precision="fp32")
    net.precision = "fp32"
    net._packed.clear()
    try:
        with torch.no_grad():
            a = make_renderer(NS(coarse_outputs="all", **base), net).render(b)
            w = make_renderer(NS(coarse_outputs="weights", **base), net).render(b)
    finally:
        net.precision = "bf16"
    assert _sigma_images(net) == []
    _check_equal(a, w)
    # train-mode sigma noise (and perturbation) under no_grad, drawn inside the kernels: the same streams in both renderers
    torch.manual_seed(11)
    tnet = make_network(NS(N_importance=128, num_classes=C, num_instances=K)).to(dev)
    synthetic.trained_like_(tnet, 0.05)
    tnet.train()
    base = dict(N_samples=64, N_importance=128, num_classes=C, num_instances=K, precision="bf16", perturb=1.0, raw_noise_std=1.0,
                rng="device", rng_seed=1234)
    with torch.no_grad():
        a = make_renderer(NS(coarse_outputs="all", **base), tnet).render(b)
        w = make_renderer(NS(coarse_outputs="weights", **base), tnet).render(b)
    assert _sigma_images(tnet) == []
    _check_equal(a, w)
    # ... while under autograd the switch has no effect: every coarse map is there (the losses read them)
    g = make_renderer(NS(coarse_outputs="weights", **base), tnet).render(b)
    assert DROPPED <= set(g) and g["rgb_0"].requires_grad


def test_sigma_abi_errors(dev):
    lib = _lib.load()
    C, K = 19, 8
    net = _net(dev, C, K)
    d3, i3 = net.packed(0, dev, "bf16", fused="sigma")
    rays, z = rays_z(5, 64, 64)
    rays, z = torch.from_numpy(rays).to(dev), torch.from_numpy(z).to(dev)
    R, N = z.shape
    ws = torch.empty(int(lib.pnr_mlp_forward_composite_workspace_bytes(ctypes.byref(d3), R, N, 1)), device=dev, dtype=torch.uint8)
    f = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)     # noqa: E731
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())     # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    depth, acc, wts = f(R), f(R), f(R, N)
    for rgb, sem, inst in ((f(R, 3), None, None), (None, f(R, C), None), (None, None, f(R, K))):
        rc = lib.pnr_mlp_forward_composite(ctypes.byref(d3), p(i3), p(rays), p(z), R, N, None, None, 0, p(rgb), p(depth), p(acc),
                                           p(wts), p(sem), p(inst), None, None, p(ws), st)
        assert rc == -1 and "plan-3" in lib.pnr_last_error().decode()
        rc = lib.pnr_composite_combine(ctypes.byref(d3), p(ws), p(z), R, N, None, None, 0, p(rgb), p(depth), p(acc), p(wts), p(sem),
                                       p(inst), None, None, st)
        assert rc == -1 and "plan-3" in lib.pnr_last_error().decode()
    with pytest.raises(RuntimeError, match="plan=3"):
        ops.mlp_forward(d3, i3, rays, z)                          # the classic entry point takes plan 0 only
    with pytest.raises(RuntimeError):
        ops.mlp_forward_weights(d3, i3, rays, z[:, :48].contiguous())       # N = 48: not a multiple of 32
    assert int(lib.pnr_mlp_forward_composite_workspace_bytes(ctypes.byref(d3), R, 48, 1)) == -1
    with pytest.raises(ValueError, match="plan-3"):
        ops.mlp_forward_weights(*net.packed(0, dev, "bf16", fused=True), rays, z)
    torch.cuda.synchronize()


def test_sigma_image_packed_on_the_device(dev):
    torch.manual_seed(3)
    net = make_network(NS(N_importance=128, num_classes=45, num_instances=32)).to(dev)
    sd = dict(net.nerf_0.named_parameters())
    d3 = net.nerf_0.desc("bf16")
    d3.plan = 3
    host = lambda: ops.pack_mlp(d3, {k: v.detach().cpu() for k, v in sd.items()})       # noqa: E731
    img, ws = ops.pack_mlp_device(d3, sd)
    assert torch.equal(img.cpu(), host())
    with torch.no_grad():                                        # an optimiser step: the same tensors, new values
        net.nerf_0.alpha_linear.weight.mul_(-1.5)
        net.nerf_0.alpha_linear.bias.add_(0.25)
        net.nerf_0.pts_linears[3].weight.add_(0.01)
        net.nerf_0.pts_linears[0].bias.sub_(0.02)
    img2, ws2 = ops.pack_mlp_device(d3, sd, out=img, workspace=ws, repack=True)
    assert img2.data_ptr() == img.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(img2.cpu(), host())
    assert torch.equal(img2.cpu(), ops.pack_mlp_device(d3, sd)[0].cpu())
