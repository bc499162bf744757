"""Convex bounding primitives on an MI355X: k_convex_hits against the float32 restatement of the rule (tests/_convex_ref.py
hits32, pinned on the CPU by tests/test_convex_ref.py) BIT FOR BIT, the renderer and the training path fed primitives, and
cuboids through both producers of the hit lists."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _camera_ref as cr
import _convex_ref as cv
from panopticnerf_amd import ConvexSet, FrameSet, NetworkWrapper, Pinhole, extrude_polygon, make_network, make_renderer, ops, synthetic
from panopticnerf_amd import train as pnr_train

pytestmark = pytest.mark.gpu

R_MAX = 4099
RS = (1, 63, 64, 65, 257, R_MAX)
MHS = (1, 2, 8, 9, 33)


def N_(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))


# ------------------------------------------------------------------------------------------------ 1. the kernel against hits32
def _table(M, seed=0):
    """M primitives around the rays' origins with 1 .. 17 planes each, mixed in one table: the first (up to six) planes of a
    primitive are faces of an axis-aligned cuboid (exact normals: rays run exactly parallel to them; fewer than six leave it
    unbounded, so that many rays hit many primitives), the others are random unit normals at 0.5 .. 4 m from its centre."""
    rng = np.random.default_rng(seed)
    planes, offsets, ctrs = [], [0], []
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    for m in range(M):
        k = 1 + (m * 5) % 17
        c = np.round(rng.uniform([-30, -3, -40], [30, 3, 60]), 2)
        ctrs.append(c)
        n = np.concatenate([axes[rng.permutation(6)[:min(k, 6)]], rng.normal(size=(max(k - 6, 0), 3))], 0)
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        dd = n @ c + rng.uniform(0.5, 4.0, k)
        planes.append(np.concatenate([n, dd[:, None]], 1))
        offsets.append(offsets[-1] + k)
    planes = np.concatenate(planes, 0).astype(np.float32) if M else np.zeros((0, 4), np.float32)
    return planes, np.asarray(offsets, np.int32), np.asarray(ctrs).reshape(-1, 3)


@pytest.fixture(scope="module")
def rays_mix(dev):
    """R_MAX rays, the special ones first (every prefix holds some): d = 0, exactly axis-parallel directions, origins at the
    centres of primitives (inside them), near == far; then pinhole rays and fisheye rays of a sideways pose (d_cam.z < 0
    included, invalid pixels -- d = 0 -- kept) alternating."""
    rng = np.random.default_rng(11)
    ctr = np.concatenate([_table(M, M)[2] for M in (1, 3, 64)], 0)
    sp = []
    for i in range(96):
        o = ctr[i % len(ctr)] if i % 3 else np.array([0.0, 1.55, 0.0])
        d = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1), (0, -1, 0), (-0.0, 0.0, -0.0), (0.25, 0, -2), tuple(rng.normal(size=3))][i % 8]
        nf = (0.5, 60.0) if i % 5 else (3.0, 3.0)
        sp.append(np.concatenate([o, d, nf]))
    sp = np.asarray(sp, np.float32)
    n = (R_MAX - len(sp) + 1) // 2
    pin = synthetic.camera_rays(yaw=0.3, far=60.0)
    pin = pin[torch.as_tensor(rng.integers(0, pin.shape[0], n))].numpy()
    c2w = cr.POSES["sideways"]
    pix = torch.as_tensor(rng.integers(0, cr.FRAME * cr.FRAME, n).astype(np.int32)).to(dev)
    fish, valid = ops.gen_rays_fisheye(cr.KITTI_FISHEYE, c2w, cr.FRAME, cr.FRAME, 0.5, 60.0, pix=pix)
    fish, valid = N_(fish), N_(valid)
    back = (fish[:, 3:6].astype(np.float64) @ c2w[:, 2]) < 0.0
    assert back.mean() > 0.05 and (valid == 0).any() and not fish[valid == 0, 3:6].any()
    both = np.empty((2 * n, 8), np.float32)
    both[0::2], both[1::2] = pin, fish
    rays = np.concatenate([sp, both], 0)[:R_MAX]
    assert rays.shape == (R_MAX, 8)
    return np.ascontiguousarray(rays)


def _canaried(R, mh, dev):
    """caller-owned outputs inside larger buffers filled with a canary"""
    pad = 64
    bt = torch.full((R * mh * 2 + 2 * pad,), 777.0, device=dev)
    bb = torch.full((R * mh + 2 * pad,), 777, device=dev, dtype=torch.int32)
    bc = torch.full((R + 2 * pad,), 777, device=dev, dtype=torch.int32)
    out = (bt[pad:pad + R * mh * 2].view(R, mh, 2), bb[pad:pad + R * mh].view(R, mh), bc[pad:pad + R])

    def intact():
        return all(bool((b[:pad] == 777).all()) and bool((b[-pad:] == 777).all()) for b in (bt, bb, bc))
    return out, intact


@pytest.mark.parametrize("M", [0, 1, 3, 64, 300])
def test_kernel_equals_the_float32_rule_bit_for_bit(dev, rays_mix, M):
    planes, offsets, _ = _table(M, M)
    assert M < 64 or sorted(set(np.diff(offsets))) == list(range(1, 18))
    tmin, tmax, hit, _, _ = cv.hits32(rays_mix, planes, offsets)
    tp, to_ = torch.as_tensor(planes).to(dev), torch.as_tensor(offsets).to(dev)
    if M == 0:
        tp = torch.zeros((0, 4), device=dev)
    rays_d = torch.as_tensor(rays_mix).to(dev)
    cnt = hit.sum(1)
    if M >= 64:
        assert cnt.max() > (33 if M == 300 else 9) and cnt.min() < 33          # rays that overflow the lists, rays that do not
        assert (cnt[:96] > 0).any()                                           # ... the special rays among them
    for R in RS:
        rd = rays_d[:R].contiguous()
        for mh in MHS:
            want = cv.kept_lists(tmin[:R], tmax[:R], hit[:R], mh)
            out, intact = _canaried(R, mh, dev)
            got = ops.convex_hits(rd, tp, to_, mh, out=out)
            assert got[0] is out[0] and intact(), (R, mh)
            for name, g, w in zip(("hit_t", "hit_box", "hit_count"), got, want):
                assert np.array_equal(_bits(N_(g)), _bits(w)), (M, R, mh, name)
    # fresh outputs (no out=): the same lists
    got = ops.convex_hits(rays_d, tp, to_, 8)
    for g, w in zip(got, cv.kept_lists(tmin, tmax, hit, 8)):
        assert np.array_equal(_bits(N_(g)), _bits(w))


def test_primitives_without_planes_and_empty_inputs(dev, rays_mix):
    rays_d = torch.as_tensor(rays_mix[:300]).to(dev)
    planes, offsets, _ = _table(3, 3)
    # a primitive without planes in the middle of a table is the whole ray [near, far]
    off = np.array([0, offsets[1], offsets[1], offsets[2], offsets[3]], np.int32)
    a32 = cv.hits32(rays_mix[:300], planes, off)
    assert a32[2][:, 1].all() and not a32[2][:, 0].all()
    got = ops.convex_hits(rays_d, torch.as_tensor(planes).to(dev), torch.as_tensor(off).to(dev), 4)
    for g, w in zip(got, cv.kept_lists(*a32[:3], 4)):
        assert np.array_equal(_bits(N_(g)), _bits(w))
    # only such primitives: no plane at all
    got = ops.convex_hits(rays_d, torch.zeros((0, 4), device=dev), torch.zeros(3, dtype=torch.int32, device=dev), 2)
    assert N_(got[2]).tolist() == [2] * 300 and N_(got[1]).tolist() == [[0, 1]] * 300
    assert np.array_equal(N_(got[0]), np.repeat(rays_mix[:300, None, 6:8], 2, 1))
    # no rays
    e = ops.convex_hits(rays_d[:0], torch.as_tensor(planes).to(dev), torch.as_tensor(offsets).to(dev), 8)
    assert e[0].shape == (0, 8, 2) and e[1].shape == (0, 8) and e[2].shape == (0,)
    with pytest.raises(ValueError, match="max_hits"):
        ops.convex_hits(rays_d, torch.as_tensor(planes).to(dev), torch.as_tensor(offsets).to(dev), 0)
    with pytest.raises(ValueError, match=r"\(P, 4\)"):
        ops.convex_hits(rays_d, torch.zeros((6, 3), device=dev), torch.as_tensor(offsets).to(dev), 8)


def test_one_grid_stride_launch_equals_its_slices(dev):
    """1,600,001 rays on at most 256 CUs x 8 workgroups x 256 threads: at least three grid-stride trips, the last one ragged"""
    R = 1600001
    assert R > 3 * torch.cuda.get_device_properties(dev).multi_processor_count * 8 * 256
    g = torch.Generator(device=dev).manual_seed(5)
    rays = torch.empty((R, 8), device=dev)
    rays[:, 0:3] = torch.tensor([0.0, 1.55, 0.0], device=dev)
    rays[:, 3:6] = torch.randn((R, 3), device=dev, generator=g)
    rays[:, 6], rays[:, 7] = 0.5, 100.0
    planes, offsets, _ = _table(3, 3)
    tp, to_ = torch.as_tensor(planes).to(dev), torch.as_tensor(offsets).to(dev)
    whole = ops.convex_hits(rays, tp, to_, 2)
    assert int((whole[2] > 0).sum()) > R // 20
    for s, e in ((0, 1), (1, 524289), (524289, 1048576), (1048576, R)):
        part = ops.convex_hits(rays[s:e].contiguous(), tp, to_, 2)
        for w, p in zip(whole, part):
            assert _same(w[s:e], p), (s, e)


def test_captured_launch_replays_on_the_edited_table(dev, rays_mix):
    rays_d = torch.as_tensor(rays_mix[:2000]).to(dev)
    planes, offsets, _ = _table(64, 64)
    planes2 = _table(64, 65)[0]
    assert planes2.shape == planes.shape
    tp, to_ = torch.as_tensor(planes).to(dev), torch.as_tensor(offsets).to(dev)
    out = tuple(torch.empty_like(t) for t in ops.convex_hits(rays_d, tp, to_, 8))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.convex_hits(rays_d, tp, to_, 8, out=out)
    graph.replay()
    for a, b in zip(out, ops.convex_hits(rays_d, tp, to_, 8)):
        assert _same(a, b)
    first = [t.clone() for t in out]
    tp.copy_(torch.as_tensor(planes2))                       # the table edited in place
    graph.replay()
    for a, b in zip(out, ops.convex_hits(rays_d, tp, to_, 8)):
        assert _same(a, b)
    assert not _same(out[0], first[0])


# ------------------------------------------------------------------------------------------------ 2. the renderer
C5, K5 = 45, 32


@pytest.fixture(scope="module")
def scene(dev):
    cs = synthetic.primitive_scene(n_box=6, n_sem=C5, n_inst=K5, seed=2).to(dev)
    rays = synthetic.camera_rays()
    rays = rays[:: rays.shape[0] // 6144][:6144].contiguous().to(dev)
    torch.manual_seed(0)
    net = synthetic.trained_like_(make_network(synthetic.baseline_cfg(5, precision="bf16")).eval()).to(dev)
    return cs, rays, net


def _render(scene, **cfg):
    cs, rays, net = scene
    rend = make_renderer(synthetic.baseline_cfg(5, precision="bf16", **cfg), net)
    with torch.no_grad():
        out = rend.render({"rays": rays[None], **cs.batch()})
    return rend, out


def test_hull_sampling_is_the_separate_kernels_on_convex_hits(dev, scene):
    cs, rays, net = scene
    b = cs.batch()
    _, out = _render(scene, bbox_sampling="hull")
    hits = ops.convex_hits(rays, b["prim_planes"], b["prim_offsets"], 8)
    assert int((hits[2] > 0).sum()) > 1000 and int((hits[2] == 0).sum()) > 100
    want = ops.stratified(ops.restrict_rays(rays, hits[0], hits[2]), 64)
    assert _same(out["z_vals_0"][0], want)
    assert not _same(out["z_vals_0"][0], ops.stratified(rays, 64))


def test_fixed_fields_are_the_weights_summed_by_label(dev, scene):
    """fix_semantic / fix_instance of both levels against a scatter-sum of the returned weights by ops.sample_labels' labels of the
    returned z: another order of summation than the kernel's over weights that sum to at most 1 -- 1e-5 absolute."""
    cs, rays, net = scene
    b = cs.batch()
    _, out = _render(scene, bbox_sampling="none", keep_weights=True)
    hits = ops.convex_hits(rays, b["prim_planes"], b["prim_offsets"], 8)
    assert _same(out["z_vals_0"][0], ops.stratified(rays, 64))
    for lv in (0, 1):
        z, w = out[f"z_vals_{lv}"][0].contiguous(), out[f"weights_{lv}"][0]
        ls, li = ops.sample_labels(z, hits[0], hits[1], hits[2], b["prim_ids"])
        assert int((ls >= 0).sum()) > 1000
        for key, lab, n in (("fix_semantic", ls, C5), ("fix_instance", li, K5)):
            want = torch.zeros((z.shape[0], n + 1), device=dev).scatter_add_(1, torch.where(lab >= 0, lab, n).long(), w)[:, :n]
            err = float((out[f"{key}_{lv}"][0] - want).abs().max())
            print("%s_%d: max |kernel - scatter-sum| = %.3g, largest entry %.3g" % (key, lv, err, float(want.max())))
            assert float(want.max()) > 1e-3 and err <= 1e-5, (key, lv, err)


def test_one_chunk_equals_three_chunks_equals_the_overlapped_frame(dev, scene):
    _, one = _render(scene, chunk_size=65536)
    rend3, three = _render(scene, chunk_size=2048, overlap_levels=False)
    rendo, over = _render(scene, chunk_size=2048, overlap_levels=True)
    cs, rays, net = scene
    from panopticnerf_amd.renderer import chunk_plan
    plan = chunk_plan(rays.shape[0], 2048)
    assert len(plan) == 3
    assert rendo._overlap_caps(dev, plan, False, False, True, None, None) is not None          # the overlapped frame did run
    assert rend3._overlap_caps(dev, plan, False, False, True, None, None) is None
    assert sorted(one) == sorted(three) == sorted(over) and "fix_instance_1" in one
    for k in one:
        assert _same(one[k], three[k]), k
        assert _same(one[k], over[k]), k


def test_strict_hits_empty_batches_and_refusals(dev, scene):
    cs, rays, net = scene
    b = cs.batch()
    with pytest.raises(RuntimeError, match="max_hits = 1"):
        _render(scene, max_hits=1, strict_hits=True)
    _render(scene, max_hits=33, strict_hits=True)             # room for every primitive (and the route of lists longer than 8)
    rend = make_renderer(synthetic.baseline_cfg(5, precision="bf16"), net)
    with torch.no_grad():
        e = rend.render({"rays": rays[None, :0], **b})
        full = rend.render({"rays": rays[None, :64], **b})
    assert sorted(e) == sorted(full) and e["fix_semantic_1"].shape == (1, 0, C5) and e["z_vals_0"].shape == (1, 0, 64)
    box, ids = synthetic.random_boxes(4, C5, K5)
    with torch.no_grad():
        with pytest.raises(ValueError, match="ConvexSet.from_boxes"):
            rend.render({"rays": rays[None], "bbox": box.to(dev), "bbox_ids": ids.to(dev), **b})
        with pytest.raises(ValueError, match="prim_offsets"):
            rend.render({"rays": rays[None], "prim_planes": b["prim_planes"]})
        with pytest.raises(ValueError, match="prim_ids"):
            rend.render({"rays": rays[None], **dict(b, prim_ids=b["prim_ids"][:3])})


def test_render_view_with_primitives_is_zero_outside_the_lens(dev, scene):
    cs, rays, net = scene
    rend = make_renderer(synthetic.baseline_cfg(5, precision="bf16"), net)
    cam, c2w = synthetic.fisheye_camera(96 / 1400, yaw=0.0)
    with torch.no_grad():
        out = rend.render_view(cam, c2w, 0.5, 100.0, prims=cs)
        pix = cam.valid_pix(dev)
        want = rend.render({"rays": cam.rays(c2w, 0.5, 100.0, pix=pix, device=dev)[None], **cs.batch()})
    valid = out["valid"]
    assert 0.5 * 96 * 96 < int(valid.sum()) < 0.95 * 96 * 96
    for k in ("rgb_1", "fix_semantic_0", "fix_semantic_1", "fix_instance_1", "weights_1", "z_vals_1"):
        assert not out[k][~valid].any(), k
        assert _same(out[k][valid], want[k][0]), k
    assert float(out["fix_semantic_1"].sum()) > 0.1


# ------------------------------------------------------------------------------------------------ 3. training
def _kitti_pinhole():
    return Pinhole(synthetic.KITTI_F, synthetic.KITTI_F, synthetic.KITTI_CX, synthetic.KITTI_CY, synthetic.KITTI_W, synthetic.KITTI_H)


def _frames(dev, C, K, cs, seed=1):
    g = torch.Generator().manual_seed(4)
    fs = FrameSet(dev, capacity=4, seed=seed)
    pin = _kitti_pinhole()
    for yaw, org in ((0.0, (0.0, 1.55, 0.0)), (0.4, (1.0, 1.55, 2.0))):
        H, W = pin.height, pin.width
        fs.add(pin, cr.pose(yaw, 0.0, org), 0.5, 100.0, torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8),
               torch.rand(H, W, generator=g) * 60 - 5, torch.randint(-1, C, (H, W), generator=g), torch.randint(-1, K, (H, W), generator=g))
    fs.set_primitives(cs)
    return fs


TRAIN = dict(N_samples=32, N_importance=32, num_classes=6, num_instances=4, precision="bf16", D=4, W=128, skips=[1])


def test_frameset_primitives_feed_the_training_step(dev):
    C, K, R = 6, 4, 512
    cs = synthetic.primitive_scene(n_box=5, n_sem=C, n_inst=K, seed=3)
    fs = _frames(dev, C, K, cs)
    with pytest.raises(ValueError, match="from_boxes"):
        fs.set_boxes(*synthetic.random_boxes(4, C, K))
    fb = FrameSet(dev, capacity=2)
    fb.set_boxes(*synthetic.random_boxes(4, C, K))
    with pytest.raises(ValueError, match="from_boxes"):
        fb.set_primitives(cs)
    batch = fs.sample(R)
    assert batch["prim_planes"] is fs.prims["prim_planes"] and "bbox" not in batch
    assert sorted(k for k in fs.frame_batch(0) if k.startswith("prim_")) == ["prim_ids", "prim_offsets", "prim_planes"]
    # the same shapes again: in place; other shapes: new tensors
    fs.set_primitives(synthetic.primitive_scene(n_box=5, n_sem=C, n_inst=K, seed=4))
    assert batch["prim_planes"] is fs.prims["prim_planes"]
    assert torch.equal(batch["prim_planes"].cpu(), torch.as_tensor(synthetic.primitive_scene(n_box=5, n_sem=C, n_inst=K, seed=4).planes))
    fs.set_primitives(synthetic.primitive_scene(n_box=2, n_sem=C, n_inst=K, seed=4))
    assert batch["prim_planes"] is not fs.prims["prim_planes"] and batch["prim_planes"].shape[0] == 5 * 6 + 50
    fs.set_primitives(cs)
    batch = fs.sample(R)
    # one step on the set's batch == one step on the same rays and targets with explicit prim_* keys
    cfg = NS(**TRAIN)
    torch.manual_seed(6)
    net_a = make_network(cfg).to(dev).train()
    net_b = copy.deepcopy(net_a)
    explicit = {k: v.clone() for k, v in batch.items() if not k.startswith("prim_")}
    explicit.update(copy.deepcopy(cs).to(dev).batch())
    res = []
    for net, bt in ((net_a, batch), (net_b, explicit)):
        _, loss, stats, _ = NetworkWrapper(net, cfg)(bt)
        loss.backward()
        res.append((loss.item(), stats))
    assert res[0][0] == res[1][0] and np.isfinite(res[0][0])
    assert float(res[0][1]["ce3d_semantic_loss_0"]) > 0 and float(res[0][1]["fix_semantic_loss_1"]) > 0
    n = 0
    for (name, a), b in zip(net_a.named_parameters(), net_b.parameters()):
        assert (a.grad is None) == (b.grad is None), name
        if a.grad is not None:
            assert torch.equal(a.grad, b.grad), name
            n += int(a.grad.abs().sum() > 0)
    assert n > 10


def test_3d_cross_entropy_on_rays_that_meet_only_an_extruded_piece(dev):
    """the L-shaped ground slab alone: rays of the image's lower half meet nothing but its prisms, and the 3D CE terms are there"""
    C, K = 6, 4
    cs = extrude_polygon(synthetic.L_OUTLINE, 3.0, 3.5, [[1, 0, 0], [0, 0, 1], [0, 1, 0]], (0.0, 0.0, 0.0), (4, 2)).to(dev)
    rays = synthetic.camera_rays().reshape(synthetic.KITTI_H, synthetic.KITTI_W, 8)[250::9, ::37].reshape(-1, 8).contiguous().to(dev)
    b = cs.batch()
    hits = ops.convex_hits(rays, b["prim_planes"], b["prim_offsets"], 8)
    assert int((hits[2] > 0).sum()) > rays.shape[0] // 3
    cfg = NS(**TRAIN)
    torch.manual_seed(3)
    net = make_network(cfg).to(dev).train()
    g = torch.Generator().manual_seed(1)
    R = rays.shape[0]
    batch = {"rays": rays[None], "rgb": torch.rand((1, R, 3), generator=g).to(dev), "pseudo_label": torch.randint(0, C, (1, R), generator=g).int().to(dev),
             "instance_label": torch.randint(0, K, (1, R), generator=g).int().to(dev), **b}
    ret, loss, stats, _ = NetworkWrapper(net, cfg)(batch)
    loss.backward()
    for lv in (0, 1):
        for f in ("semantic", "instance"):
            v = float(stats[f"ce3d_{f}_loss_{lv}"])
            assert np.isfinite(v) and v > 0.1, (f, lv, v)             # the CE of untrained logits is about log(n)
        assert float(ret[f"ce3d_semantic_n_{lv}"]) > 100
        fix = ret[f"fix_semantic_{lv}"].detach()
        assert float(fix[..., 4].sum()) > 0 and not fix[..., :4].any()
    # ... and without the primitives they are not
    _, _, stats0, _ = NetworkWrapper(net, cfg)({k: v for k, v in batch.items() if not k.startswith("prim_")})
    assert "ce3d_semantic_loss_0" not in stats0


def test_graphed_step_on_a_frameset_with_primitives_equals_eager_steps(dev):
    C, K, R, STEPS = 6, 4, 512, 3
    cfg = NS(rng="device", rng_seed=31, perturb=1.0, raw_noise_std=1.0, **TRAIN)
    cs = synthetic.primitive_scene(n_box=5, n_sem=C, n_inst=K, seed=3)
    fs = _frames(dev, C, K, cs)
    torch.manual_seed(6)
    net_e = make_network(cfg).to(dev).train()
    net_g = copy.deepcopy(net_e)
    wraps = [NetworkWrapper(n, cfg) for n in (net_e, net_g)]
    opts = [torch.optim.Adam(n.parameters(), lr=1e-3, capturable=True, fused=True) for n in (net_e, net_g)]
    s0 = fs.rng_state.clone()
    step = pnr_train.GraphedStep(wraps[1], opts[1], frames=fs, n_rays=R)
    assert "prim_planes" in step.static
    losses_g = [step()[1].item() for _ in range(STEPS)]
    fs.rng_state.copy_(s0)
    losses_e = []
    for _ in range(STEPS):
        opts[0].zero_grad(set_to_none=False)
        _, loss, _, _ = wraps[0](fs.sample(R))
        loss.backward()
        opts[0].step()
        losses_e.append(loss.item())
    assert losses_g == losses_e and len(set(losses_g)) == STEPS, (losses_g, losses_e)
    for (name, a), b in zip(net_e.named_parameters(), net_g.parameters()):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ 4. cuboids both ways
def _box_bound(rays, box, hit_box, t, end):
    """Bound on |t32 - t64| of pnr_bbox_hits' slab test for the axis that binds (u = 2^-24, first order, as _convex_ref.t_bound):
      p = o - c: one rounding per component;  ol = (r0 p0 + r1 p1) + r2 p2: |ol^ - ol| <= 3u OL + u OL = 4u OL, OL = sum |r_i p_i|;
      num = +-e - ol^: |num^ - num| <= 4u OL + u (e + OL) = u (5 OL + e);   dl: |dl^ - dl| <= 3u DL, DL = sum |r_i d_i|;
      inv = 1 / dl^ rounded: relative error <= 3u DL / |dl| + u;   t = num^ * inv^ rounded:
      |t^ - t| <= u (5 OL + e) / |dl| + |t| (3u DL / |dl| + 2u) <= 5u (OL + e + |t| DL) / |dl|     (as |dl| <= DL),  times (1 + 16u).
    The axis: every axis whose own quotient lies within 1e-4 max(1, |t|) of t may be the one that binds in float32 (a ray
    through an edge): the largest of their bounds.  near / far binding: no error."""
    rays, box = rays.astype(np.float64), box.astype(np.float64)
    b = box[np.maximum(hit_box, 0)]                                   # (R,H,15)
    p = rays[:, None, 0:3] - b[..., 0:3]
    rot = b[..., 3:12].reshape(*b.shape[:2], 3, 3)
    e = b[..., 12:15]
    OL, DL = np.abs(rot * p[..., None, :]).sum(-1), np.abs(rot * rays[:, None, None, 3:6]).sum(-1)        # (R,H,3)
    ol, dl = (rot * p[..., None, :]).sum(-1), (rot * rays[:, None, None, 3:6]).sum(-1)
    with np.errstate(all="ignore"):
        t1, t2 = (-e - ol) / dl, (e - ol) / dl
        q = np.minimum(t1, t2) if end == 0 else np.maximum(t1, t2)
        bound = 5.0 * cv.U32 * (OL + e + np.abs(t)[..., None] * DL) / np.abs(dl) * (1.0 + 16.0 * cv.U32)
        near = np.abs(q - t[..., None]) <= 1e-4 * np.maximum(1.0, np.abs(t))[..., None]
    return np.where(near, bound, 0.0).max(-1)


def test_cuboids_through_both_producers(dev):
    """64 boxes as 384 planes through pnr_convex_hits and as boxes through pnr_bbox_hits, 20 000 rays: outside the rays float64
    excludes (tests/test_convex_ref.py's rule, at most 1 %) the same primitives and counts, every t within the SUM of the two
    derived bounds (different arithmetic: no bit equality)."""
    box, ids = synthetic.random_boxes(64)
    cs = ConvexSet.from_boxes(box, ids)
    rays = synthetic.camera_rays(origin=(0.3, -0.2, 0.1))
    rays = rays[:: rays.shape[0] // 20000][:20000].contiguous()
    r = rays.numpy()
    a64 = cv.hits64(r, cs.planes, cs.offsets)
    a32 = cv.hits32(r, cs.planes, cs.offsets)
    ex = cv.excluded(a64[0], a64[1], a64[2])
    assert ex.mean() <= 0.01
    keep = ~ex
    rd = rays.to(dev)
    b = cs.to(dev).batch()
    MH = 16
    gc = [N_(t) for t in ops.convex_hits(rd, b["prim_planes"], b["prim_offsets"], MH)]
    gb = [N_(t) for t in ops.bbox_hits(rd, box.to(dev), MH)]
    l64 = cv.kept_lists(*a64[:3], MH)
    assert gc[2].max() <= MH                 # no list is cut short
    assert np.array_equal(gc[2][keep], gb[2][keep]) and np.array_equal(gc[1][keep], gb[1][keep])
    assert np.array_equal(gc[1][keep], l64[1][keep]) and gc[2][keep].max() >= 3
    idx = np.maximum(l64[1], 0).astype(np.int64)
    pl = cs.planes.astype(np.float64)
    o, d = r[:, None, 0:3].astype(np.float64), r[:, None, 3:6].astype(np.float64)

    def quotient(p):
        q = pl[np.maximum(p, 0)]
        with np.errstate(all="ignore"):
            return (q[..., 3] - (q[..., :3] * o).sum(-1)) / (q[..., :3] * d).sum(-1)
    sel = keep[:, None] & (l64[1] >= 0)
    for end, (b32, b64) in enumerate(((a32[3], a64[3]), (a32[4], a64[4]))):
        t64 = l64[0][..., end]
        pa, pb = np.take_along_axis(b32, idx, 1), np.take_along_axis(b64, idx, 1)
        tol = np.maximum(cv.t_bound(r, cs.planes, pa, quotient(pa)), cv.t_bound(r, cs.planes, pb, quotient(pb)))
        tol = tol + _box_bound(r, box.numpy(), l64[1], t64, end)
        err = np.abs(gc[0][..., end].astype(np.float64) - gb[0][..., end].astype(np.float64))
        some = sel & (tol > 0)
        print("end %d: largest |t_convex - t_bbox| = %.3g, largest error / bound = %.3g" % (end, err[sel].max(), (err[some] / tol[some]).max()))
        assert (err[sel] <= tol[sel]).all(), (end, float((err[sel] - tol[sel]).max()))
