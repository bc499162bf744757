"""GPU tests of the in-kernel RNG (include/pnr.h "in-kernel RNG", cfg.rng = "device"): the stream equals the numpy Philox
reference, every _rng kernel equals its explicit-tensor twin fed with rng_fill's tensors bit for bit, a whole training render /
backward equals the render fed with the materialised uniforms, the draws do not depend on the chunk plan, the state advances
once per render and restores, GraphedStep replays equal eager steps with perturbation and sigma noise on, and the draws have the
statistics they should."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _philox
from panopticnerf_amd import NetworkWrapper, make_network, make_renderer, ops, synthetic, train as pnr_train

pytestmark = pytest.mark.gpu


def _call(dev, seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


def _rays(dev, R, seed=0, near=0.5, far=40.0):
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 1, (R, 3)) + np.array([0, 1.5, 0])
    d = rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])
    r = np.concatenate([o, d, np.full((R, 1), near), np.full((R, 1), far)], 1).astype(np.float32)
    return torch.tensor(r, device=dev)


def _same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b), (what, (a.float() - b.float()).abs().max().item())


# ---------------------------------------------------------------------------------------------------------------- 1. stream
@pytest.mark.parametrize("seed,offset,tag,base", [(0, 0, 1, 0), (12345, 7, 2, 1000), (-1, 2**32 + 5, 3, 2**32 - 64),
                                                  (2**62 + 3, 2**40 + 1, 255, 77)])
def test_fill_equals_reference(dev, seed, offset, tag, base):
    R, N = 64, 40
    call = _call(dev, seed, offset)
    words = _philox.stream_words(seed, offset, tag, base, R, N)
    u = ops.rng_fill(call, tag, base, R, N)
    assert np.array_equal(u.cpu().numpy(), _philox.uniforms(words))
    n = ops.rng_fill(call, tag, base, R, N, normal=True, std=1.0).cpu().numpy().astype(np.float64)
    ref = _philox.normals64(words)
    assert (np.abs(n - ref) <= 2e-6 * np.maximum(1.0, np.abs(ref))).all(), np.abs(n - ref).max()
    n3 = ops.rng_fill(call, tag, base, R, N, normal=True, std=3.0).cpu().numpy()
    assert np.array_equal(n3, (n.astype(np.float32) * np.float32(3.0)))


def test_begin_copies_state_and_advances_it(dev):
    state = _call(dev, 99, 2**32 - 1)
    call = ops.rng_begin(state)
    assert call.tolist() == [99, 2**32 - 1] and state.tolist() == [99, 2**32]


# ---------------------------------------------------------------------------------------------------------------- 2. in-line = explicit
@pytest.mark.parametrize("lindisp", [False, True])
def test_stratified_rng_equals_explicit(dev, lindisp):
    R, N, base = 777, 64, 2**32 - 800
    rays = _rays(dev, R)
    call = _call(dev, 5, 3)
    t = ops.rng_fill(call, 1, base, R, N)
    _same(ops.stratified(rays, N, lindisp, ops.Draw(call, 1, base)), ops.stratified(rays, N, lindisp, t))
    # hull sampling through the separate kernels (restrict_rays + stratified)
    box, ids = synthetic.random_boxes(48, 7, 5, seed=3)
    hits = ops.bbox_hits(rays, box.to(dev), 8)
    rs = ops.restrict_rays(rays, hits[0], hits[2])
    _same(ops.stratified(rs, N, lindisp, ops.Draw(call, 1, base)), ops.stratified(rs, N, lindisp, t))


@pytest.mark.parametrize("hull", [False, True])
@pytest.mark.parametrize("N", [64, 100])
def test_ray_setup_rng_equals_explicit(dev, hull, N):
    R, base = 1000, 4096
    rays = _rays(dev, R, seed=1)
    box, ids = synthetic.random_boxes(48, 7, 5, seed=3)
    box, ids = box.to(dev), ids.to(dev)
    call = _call(dev, 11, 2**33)
    t = ops.rng_fill(call, 1, base, R, N)
    a = ops.ray_setup(rays, box, ids, N, 8, False, ops.Draw(call, 1, base), hull)
    b = ops.ray_setup(rays, box, ids, N, 8, False, t, hull)
    for x, y in zip(a[0], b[0]):
        _same(x, y, "hits")
    for x, y, w in zip(a[1:], b[1:], ("z", "label_sem", "label_inst")):
        _same(x, y, w)


def _weights(dev, R, Nc, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((R, Nc), generator=g) ** 4
    w[:, :: 7] *= 10
    return w.to(dev)


@pytest.mark.parametrize("Nc,Nf", [(64, 128), (64, 192), (128, 160)])        # (128, 160): the big instance
def test_sample_pdf_rng_equals_explicit(dev, Nc, Nf):
    R, base = 600, 123456
    rays = _rays(dev, R, seed=2)
    z = ops.stratified(rays, Nc)
    w = _weights(dev, R, Nc, Nc + Nf)
    call = _call(dev, 21, 1)
    u = ops.rng_fill(call, 2, base, R, Nf)
    a = ops.sample_pdf(z, w, Nf, ops.Draw(call, 2, base))
    b = ops.sample_pdf(z, w, Nf, u)
    for x, y, n in zip(a, b, ("z_fine", "z_samples", "inds")):
        _same(x, y, n)
    box, ids = synthetic.random_boxes(48, 7, 5, seed=4)
    box, ids = box.to(dev), ids.to(dev)
    hits = ops.bbox_hits(rays, box, 8)
    a = ops.sample_pdf_labels(z, w, Nf, hits, ids, ops.Draw(call, 2, base))
    b = ops.sample_pdf_labels(z, w, Nf, hits, ids, u)
    for x, y, n in zip(a, b, ("z_fine", "label_sem", "label_inst")):
        _same(x, y, n)


def _composite_inputs(dev, R, N, C, K, seed):
    g = torch.Generator().manual_seed(seed)
    rays = _rays(dev, R, seed=seed)
    z = ops.stratified(rays, N)
    raw = ops.alloc_raw(4 + C + K, R * N, dev)
    raw.copy_(torch.randn((4 + C + K, R * N), generator=g).to(dev))
    raw[3].copy_((torch.randn(R * N, generator=g) * 0.3 + 0.1).to(dev))
    ls = torch.randint(-1, C, (R, N), generator=g, dtype=torch.int32).to(dev)
    li = torch.randint(-1, K, (R, N), generator=g, dtype=torch.int32).to(dev)
    return rays, z, raw, ls, li


@pytest.mark.parametrize("N", [4, 8, 16, 36, 60, 64, 68, 132, 192, 256])
@pytest.mark.parametrize("sem_mode", [0, 1])
def test_composite_rng_equals_explicit(dev, N, sem_mode):
    R, C, K, base, std = 301, 45, 32, 9999, 1.0
    rays, z, raw, ls, li = _composite_inputs(dev, R, N, C, K, N + sem_mode)
    call = _call(dev, 3, 4)
    noise = ops.rng_fill(call, 4, base, R, N, normal=True, std=std)
    a = ops.composite(raw, z, rays, C, K, True, ops.Draw(call, 4, base, std), ls, li, sem_mode)
    b = ops.composite(raw, z, rays, C, K, True, noise, ls, li, sem_mode)
    assert a.keys() == b.keys()
    for k in a:
        _same(a[k], b[k], k)


@pytest.mark.parametrize("N", [4, 8, 16, 36, 60, 64, 68, 132, 192])
@pytest.mark.parametrize("sem_mode", [0, 1])
def test_composite_backward_rng_equals_explicit(dev, N, sem_mode):
    R, C, K, base, std = 257, 45, 32, 2**31, 0.7
    rays, z, raw, ls, li = _composite_inputs(dev, R, N, C, K, 7 * N + sem_mode)
    raw = raw.contiguous()                      # composite_backward takes dense channel rows (the training forward's layout)
    g = torch.Generator().manual_seed(N)
    grads = {"rgb": (R, 3), "depth": (R,), "acc": (R,), "semantic": (R, C), "instance": (R, K), "weights": (R, N),
             "fix_semantic": (R, C), "fix_instance": (R, K)}
    grads = {k: torch.randn(s, generator=g).to(dev) for k, s in grads.items()}
    ce = torch.tensor([0.01], device=dev)
    call = _call(dev, 8, 8)
    noise = ops.rng_fill(call, 3, base, R, N, normal=True, std=std)
    a = ops.composite_backward(raw, z, rays, C, K, grads, ops.Draw(call, 3, base, std), ls, li, ce, ce, sem_mode)
    b = ops.composite_backward(raw, z, rays, C, K, grads, noise, ls, li, ce, ce, sem_mode)
    _same(a, b, "d_raw")


# ---------------------------------------------------------------------------------------------------------------- 3. a training render
def _train_setup(dev, precision="bf16", R=1024, Nf=192, **kw):
    C, K = 45, 32
    cfg = NS(N_samples=64, N_importance=Nf, num_classes=C, num_instances=K, precision=precision, rng="device", rng_seed=4242,
             perturb=1.0, chunk_size=65536, **kw)
    torch.manual_seed(3)
    net = make_network(cfg)
    synthetic.trained_like_(net)
    net = net.to(dev).train()
    rays = synthetic.camera_rays()[:: 1408 * 376 // R][:R].contiguous()
    box, ids = synthetic.random_boxes(64, C, K, seed=5)
    batch = {"rays": rays[None].to(dev), "bbox": box.to(dev), "bbox_ids": ids.to(dev)}
    return cfg, net, batch


def _maps_and_grads(rend, net, batch):
    for p in net.parameters():
        p.grad = None
    out = rend.render(batch)
    loss = sum((v.float() ** 2).mean() for k, v in out.items() if v.dim() >= 2 and v.requires_grad)
    loss.backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in out.items()},
            {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, loss.detach())


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_training_render_equals_render_with_materialised_uniforms(dev, precision):
    cfg, net, batch = _train_setup(dev, precision)
    rend = make_renderer(cfg, net)
    R = batch["rays"].shape[1]
    call = rend.rng_state.clone()           # what the render's pnr_rng_begin will copy
    m_dev, g_dev, _ = _maps_and_grads(rend, net, batch)
    assert rend.rng_state.tolist() == [call[0].item(), call[1].item() + 1]
    explicit = dict(batch, t_rand=ops.rng_fill(call, 1, 0, R, cfg.N_samples)[None],
                    u=ops.rng_fill(call, 2, 0, R, cfg.N_importance)[None])
    m_exp, g_exp, _ = _maps_and_grads(rend, net, explicit)
    assert m_dev.keys() == m_exp.keys() and g_dev.keys() == g_exp.keys() and len(g_dev) > 0
    for k in m_dev:
        _same(m_dev[k], m_exp[k], k)
    for k in g_dev:
        _same(g_dev[k], g_exp[k], k)
    assert not torch.equal(m_dev["z_vals_0"], _maps_and_grads(make_renderer(NS(**dict(vars(cfg), perturb=0.0)), net), net, batch)[0]["z_vals_0"])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_level_train_device_noise_equals_tensor_noise(dev, precision):
    """sigma noise cannot be passed through the batch: train.level_train with a Draw against LevelFn fed rng_fill's tensor"""
    cfg, net, batch = _train_setup(dev, precision, raw_noise_std=1.0)
    rend = make_renderer(cfg, net)
    rays = batch["rays"][0].contiguous()
    box, ids = batch["bbox"], batch["bbox_ids"]
    R, N, base = rays.shape[0], 64, 12345
    hits, z, ls, li = ops.ray_setup(rays, box, ids, N, 8)
    call = _call(dev, 17, 2)
    res = []
    for noise in (ops.Draw(call, 3, base, 1.0), ops.rng_fill(call, 3, base, R, N, normal=True, std=1.0)):
        for p in net.parameters():
            p.grad = None
        out = pnr_train.level_train(rend, 0, rays, z, ls, li, noise)
        loss = sum((v ** 2).mean() for k, v in out.items() if v.dim() >= 1 and v.requires_grad) + out["ce3d_semantic"] + out["ce3d_instance"]
        loss.backward()
        res.append(({k: v.detach().clone() for k, v in out.items()}, {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
    (m0, g0), (m1, g1) = res
    assert m0.keys() == m1.keys() and g0.keys() == g1.keys() and len(g0) > 0
    for k in m0:
        _same(m0[k], m1[k], k)
    for k in g0:
        _same(g0[k], g1[k], k)


# ---------------------------------------------------------------------------------------------------------------- 4. chunk invariance
def test_training_draws_do_not_depend_on_the_chunk_plan(dev):
    """Same batch, same rng_state, chunk_size 1024 / 1536 / whole batch: every per-ray map of both levels bit for bit (the draws of
    a ray depend on its global index only).  Losses and weight gradients are sums over chunks in another order: they agree to
    1e-5 relative (loss) and 2e-3 relative in the norm of each gradient (bf16 dY, fp32 accumulation in another association)."""
    cfg, net, batch = _train_setup(dev, "bf16", R=4096, raw_noise_std=1.0)
    state0 = None
    runs = []
    for cs in (1024, 1536, 8192):
        rend = make_renderer(NS(**dict(vars(cfg), chunk_size=cs)), net)
        if state0 is None:
            state0 = rend.rng_state.clone()
        rend.rng_state.copy_(state0)
        runs.append(_maps_and_grads(rend, net, batch))
    m_ref, g_ref, l_ref = runs[-1]
    for m, g, l in runs[:-1]:
        for k, v in m_ref.items():
            if v.dim() >= 2:                  # per-ray maps (B, R, ...); the per-level ce3d scalars are chunk means
                _same(m[k], v, k)
        assert abs(l.item() - l_ref.item()) <= 1e-5 * abs(l_ref.item())
        for k in g_ref:
            assert ((g[k] - g_ref[k]).norm() / (g_ref[k].norm() + 1e-30)).item() < 2e-3, k
    # the torch path's draws DO depend on the chunk plan (what the device stream fixes)
    maps = []
    for cs in (1024, 8192):
        rend = make_renderer(NS(**dict(vars(cfg), chunk_size=cs, rng="torch")), net)
        torch.manual_seed(0)
        with torch.no_grad():
            maps.append(rend.render(batch)["z_vals_0"])
    assert not torch.equal(maps[0], maps[1])


# ---------------------------------------------------------------------------------------------------------------- 5. state
def test_state_advances_restores_and_ignores_torch_generator(dev):
    cfg, net, batch = _train_setup(dev, "bf16", R=1024, raw_noise_std=1.0)
    rend = make_renderer(cfg, net)
    s0 = rend.rng_state.clone()
    with torch.no_grad():
        gen0 = torch.cuda.get_rng_state(dev)
        cpu0 = torch.get_rng_state()
        a = rend.render(batch)
        assert torch.equal(torch.cuda.get_rng_state(dev), gen0) and torch.equal(torch.get_rng_state(), cpu0)
        assert rend.rng_state.tolist() == [s0[0].item(), s0[1].item() + 1]
        b = rend.render(batch)
        assert rend.rng_state.tolist() == [s0[0].item(), s0[1].item() + 2]
        assert not torch.equal(a["z_vals_0"], b["z_vals_0"]) and not torch.equal(a["z_vals_1"], b["z_vals_1"])
        rend.rng_state.copy_(s0)
        torch.manual_seed(987)                     # moves torch's generators: nothing of the device stream
        c = rend.render(batch)
    for k in a:
        _same(a[k], c[k], k)


# ---------------------------------------------------------------------------------------------------------------- 6. graphs
def test_graphed_step_with_device_rng_replays_equal_eager_steps(dev):
    C, K = 6, 4
    cfg = NS(N_samples=32, N_importance=32, num_classes=C, num_instances=K, precision="bf16", D=4, W=128, skips=[1],
             rng="device", rng_seed=31, perturb=1.0, raw_noise_std=1.0)
    torch.manual_seed(6)
    net_e = make_network(cfg).to(dev).train()
    net_g = copy.deepcopy(net_e)
    R = 256
    box, ids = synthetic.random_boxes(16, C, K, seed=2)
    g = torch.Generator().manual_seed(2)

    def batch(i):
        rays = synthetic.camera_rays()[i::2003][:R].contiguous()
        return {"rays": rays[None].to(dev), "bbox": box.to(dev), "bbox_ids": ids.to(dev),
                "rgb": torch.rand(1, R, 3, generator=g).to(dev), "depth": (torch.rand(1, R, generator=g) * 20 - 2).to(dev),
                "pseudo_label": torch.randint(-1, C, (1, R), generator=g).to(dev), "instance_label": torch.randint(-1, K, (1, R), generator=g).to(dev)}

    batches = [batch(i) for i in range(4)]
    wrap_e, wrap_g = NetworkWrapper(net_e, cfg), NetworkWrapper(net_g, cfg)
    opt_e = torch.optim.Adam(net_e.parameters(), lr=1e-3, capturable=True, fused=True)
    opt_g = torch.optim.Adam(net_g.parameters(), lr=1e-3, capturable=True, fused=True)
    s0 = wrap_g.renderer.rng_state.clone()
    step = pnr_train.GraphedStep(wrap_g, opt_g, batches[3])
    assert torch.equal(wrap_g.renderer.rng_state, s0)                  # construction draws nothing ...
    for a, b in zip(net_e.parameters(), net_g.parameters()):
        assert torch.equal(a, b)                                       # ... and trains nothing
    losses_g, z_g, losses_e, z_e = [], [], [], []
    for b in batches[:3]:
        ret, loss, _ = step(b)
        losses_g.append(loss.item())
        z_g.append(ret["z_vals_1"].clone())
    assert wrap_g.renderer.rng_state.tolist() == [s0[0].item(), s0[1].item() + 3]
    wrap_e.renderer.rng_state.copy_(s0)
    for b in batches[:3]:
        opt_e.zero_grad(set_to_none=False)
        ret, loss, _, _ = wrap_e(b)
        loss.backward()
        opt_e.step()
        losses_e.append(loss.item())
        z_e.append(ret["z_vals_1"].detach().clone())
    assert losses_g == losses_e, (losses_g, losses_e)
    for a, b in zip(z_g, z_e):
        _same(a, b, "z_vals_1")
    for (n, a), b in zip(net_e.named_parameters(), net_g.parameters()):
        assert torch.equal(a, b), n
    # two replays on the SAME batch draw different samples
    _, _, _ = step(batches[0])
    za = step.out[0]["z_vals_0"].clone()
    step(batches[0])
    assert not torch.equal(za, step.out[0]["z_vals_0"])


# ---------------------------------------------------------------------------------------------------------------- 7. statistics
def test_statistics(dev):
    n_r, n_s = 2**14, 2**8                      # 2^22 draws per stream, fixed seeds: deterministic
    n = n_r * n_s
    call = _call(dev, 2024, 1)
    u = ops.rng_fill(call, 1, 0, n_r, n_s).double()
    assert abs(u.mean().item() - 0.5) < 5 * (1 / 12) ** 0.5 / n ** 0.5
    assert abs(u.var().item() - 1 / 12) < 5 * (1 / 180) ** 0.5 / n ** 0.5
    srt = torch.sort(u.flatten())[0]
    ks = (torch.arange(1, n + 1, device=dev, dtype=torch.float64) / n - srt).abs().max().item()
    assert ks < 1.95 / n ** 0.5                  # KS 0.1 % critical value
    z = ops.rng_fill(call, 3, 0, n_r, n_s, normal=True).double()
    assert abs(z.mean().item()) < 5 / n ** 0.5 and abs(z.std().item() - 1) < 5 / (2 * n) ** 0.5
    # correlations between neighbouring rays, tags and offsets, and between the two words of a Box-Muller pair
    lim = 5 / n ** 0.5
    corr = lambda a, b: torch.corrcoef(torch.stack([a.flatten(), b.flatten()]))[0, 1].item()
    u_next_ray = ops.rng_fill(call, 1, 1, n_r, n_s).double()
    u_tag2 = ops.rng_fill(call, 2, 0, n_r, n_s).double()
    u_off2 = ops.rng_fill(_call(dev, 2024, 2), 1, 0, n_r, n_s).double()
    for other in (u_next_ray[:-1], u_tag2[:-1], u_off2[:-1]):
        assert abs(corr(u[:-1], other)) < lim
    assert abs(corr(u[1:], u_next_ray[:-1])) > 0.999999          # ray g + 1 from base 0 is ray g from base 1
    assert abs(corr(z[:, 0::2], z[:, 1::2])) < 5 / (n / 2) ** 0.5
    # stratified jitter fills each bin uniformly: the position inside the bin is the uniform
    R, N = 2**14, 64
    rays = torch.zeros((R, 8), device=dev)
    rays[:, 5] = 1.0
    rays[:, 6], rays[:, 7] = 2.0, 2.0 + (N - 1)        # bins of width 1 around the integers 2 .. 2 + N - 1
    zz = ops.stratified(rays, N, False, ops.Draw(call, 1, 0)).double()
    mids = torch.arange(N, device=dev, dtype=torch.float64) + 2.0
    lo = torch.cat([mids[:1], mids[1:] - 0.5]); hi = torch.cat([mids[:-1] + 0.5, mids[-1:]])
    frac = (zz - lo) / (hi - lo)
    assert ((frac > -1e-4) & (frac < 1 + 1e-4)).all()          # (lo / hi: the fp64 bin edges, the kernel's are fp32)
    inner = frac[:, 1:-1].clamp(0.0, 1.0 - 1e-9)
    assert abs(inner.mean().item() - 0.5) < 5 * (1 / 12) ** 0.5 / inner.numel() ** 0.5
    counts = torch.histc(inner.float(), bins=16, min=0.0, max=1.0).double()
    exp = inner.numel() / 16
    assert ((counts - exp) ** 2 / exp).sum().item() < 37.7          # chi^2, 15 dof, p = 0.001
    # fine samples against the coarse pdf: the fraction of samples in each bin is its pdf mass (chi^2)
    Nc, Nf, R = 64, 128, 2**13
    zc = (torch.arange(Nc, device=dev, dtype=torch.float32) + 1.0)[None].repeat(R, 1).contiguous()
    prof = torch.exp(-0.5 * ((torch.arange(Nc, dtype=torch.float32) - 30) / 6) ** 2) + 0.05
    w = prof[None].repeat(R, 1).to(dev).contiguous()
    _, zs, inds = ops.sample_pdf(zc, w, Nf, ops.Draw(call, 2, 0))
    nb = Nc - 1                                          # bins [mid_k, mid_k+1), k = 0 .. nb - 2 with pdf (w[k+1] + 1e-5) / total
    pdf = (prof[1:-1] + 1e-5) / (prof[1:-1] + 1e-5).sum()
    mids_c = 0.5 * (torch.arange(Nc - 1, dtype=torch.float64) + 1.0 + torch.arange(1, Nc, dtype=torch.float64) + 1.0)
    edges = mids_c.to(dev)
    k = torch.bucketize(zs.double().flatten(), edges, right=True) - 1
    k = k.clamp(0, nb - 2)
    counts = torch.bincount(k, minlength=nb - 1)[: nb - 1].double().cpu()
    expct = pdf.double() * zs.numel()
    keep = expct > 5
    chi2 = ((counts[keep] - expct[keep]) ** 2 / expct[keep]).sum().item()
    dof = int(keep.sum()) - 1
    assert chi2 < dof + 5 * (2 * dof) ** 0.5, (chi2, dof)
