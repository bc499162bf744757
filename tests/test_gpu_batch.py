"""Training frames on an MI355X: pnr_sample_batch / data.FrameSet / the self-feeding train.GraphedStep.

The kernel must equal tests/_batch_ref.py (pinned on the CPU by tests/test_batch_ref.py) BIT FOR BIT in every output: the draw is
integer arithmetic on Philox words, the rays are the camera kernels' own arithmetic (pnr_camera_dev.h), rgb is one correctly
rounded division, the other targets are copies.  Training through a captured step that draws its own batches must equal eager
steps on FrameSet.sample() batches, and the parent-style GraphedStep fed those batches, in every parameter and Adam moment."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _batch_ref as br
import _camera_ref as cr
from panopticnerf_amd import FrameSet, NetworkWrapper, Pinhole, make_network, make_renderer, ops, synthetic
from panopticnerf_amd import train as pnr_train

pytestmark = pytest.mark.gpu

SEED = 77
KEYS = (("rays", "rays"), ("rgb", "rgb"), ("depth", "depth"), ("pseudo_label", "sem"), ("instance_label", "inst"), ("frame", "frame"),
        ("pix", "pix"))


def N_(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _kitti_pinhole():
    return Pinhole(synthetic.KITTI_F, synthetic.KITTI_F, synthetic.KITTI_CX, synthetic.KITTI_CY, synthetic.KITTI_W, synthetic.KITTI_H)


def _images(g, H, W, C=19, K=12):
    return {"rgb": torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8),
            "depth": torch.rand(H, W, generator=g) * 60 - 5,                                   # <= 0: no stereo depth there
            "pseudo_label": torch.randint(-1, C, (H, W), generator=g), "instance_label": torch.randint(-1, K, (H, W), generator=g)}


def _add(fs, ref, cam, c2w, near, far, imgs, mask=None):
    """the same frame into the FrameSet and into the reference's list"""
    fs.add(cam, c2w, near, far, imgs["rgb"], imgs.get("depth"), imgs.get("pseudo_label"), imgs.get("instance_label"))
    ref.append(br.ref_frame(cam.model, cam.intr if cam.model == "pinhole" else cam.cam, cam.width, cam.height, N_(torch.as_tensor(c2w)),
                            near, far, N_(imgs["rgb"]), *[None if imgs.get(k) is None else N_(imgs[k]) for k in
                                                         ("depth", "pseudo_label", "instance_label")], mask=mask))


@pytest.fixture(scope="module")
def mixed(dev):
    """pinhole 1408 x 376 (everything), fisheye 1400 x 1400 (depth, no labels), the same lens under a user mask (labels, no depth),
    pinhole at another pose (rgb alone)"""
    g = torch.Generator().manual_seed(3)
    fs, ref = FrameSet(dev, capacity=8, seed=SEED), []
    pin = _kitti_pinhole()
    _add(fs, ref, pin, cr.pose(0.2, 0.05, (1.0, 1.55, -3.0)), 0.5, 100.0, _images(g, pin.height, pin.width))
    fish, c2w = synthetic.fisheye_camera()
    im = _images(g, fish.height, fish.width)
    _add(fs, ref, fish, c2w, 0.25, 80.0, {"rgb": im["rgb"], "depth": im["depth"]})
    mask = torch.ones(fish.height, fish.width, dtype=torch.bool)
    mask[1000:, :] = False
    mask[200:400, 300:900] = False
    fish_m, c2w_m = synthetic.fisheye_camera(yaw=-1.3, origin=(2.0, 1.5, 7.0), mask=mask)
    im = _images(g, fish.height, fish.width)
    _add(fs, ref, fish_m, c2w_m, 0.5, 60.0, {k: im[k] for k in ("rgb", "pseudo_label", "instance_label")}, mask=N_(mask))
    _add(fs, ref, pin, cr.pose(-2.0, 0.0, (-4.0, 1.4, 12.0)), 1.0, 120.0, {"rgb": _images(g, pin.height, pin.width)["rgb"]})
    # the reference's drawable pixels are the cameras' (their equality pixel by pixel is tests/test_gpu_camera.py's subject)
    for fr, r in zip(fs.frames, ref):
        assert (fr["pix"] is None) == (r["valid_pix"] is None)
        if fr["pix"] is not None:
            assert np.array_equal(N_(fr["pix"]), r["valid_pix"])
    assert fs.n_pixels == br.cum_of(ref)[-1] and ref[2]["valid_pix"].size < ref[1]["valid_pix"].size < 1400 * 1400
    return fs, ref


def _state(fs, offset, seed=SEED):
    fs.rng_state.copy_(torch.tensor([seed, offset], dtype=torch.int64))


def _same_as_ref(batch, want, what):
    for k, n in KEYS:
        got = N_(batch[k]).reshape(want[n].shape)
        assert got.dtype == want[n].dtype, (what, k, got.dtype)
        bad = np.nonzero(_bits(got) != _bits(want[n]))[0]
        assert bad.size == 0, (what, k, bad[:5], got[bad[:1]], want[n][bad[:1]])


# ---------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("mode", ["pooled", "frame"])
@pytest.mark.parametrize("R", [1, 255, 4096, 4097, 70001])
def test_batch_equals_reference_bit_for_bit(dev, mixed, R, mode):
    fs, ref = mixed
    offs = (11, 12) if mode == "pooled" else (10, 11, 14, 16)          # mode "frame": these offsets pick frames 0, 3, 2, 1
    picked = set()
    for off in offs:
        _state(fs, off)
        batch = fs.sample(R, mode)
        want = br.sample(ref, SEED, off, R, 0 if mode == "pooled" else 1)
        _same_as_ref(batch, want, (R, mode, off))
        assert batch["rays"].shape == (1, R, 8) and batch["rgb"].shape == (1, R, 3) and batch["pseudo_label"].dtype == torch.int32
        picked |= set(want["frame"].tolist())
        assert fs.rng_state.tolist() == [SEED, off + 1]
    if mode == "frame" or R >= 255:
        assert picked == {0, 1, 2, 3}, picked


# ---------------------------------------------------------------------------------------------------- 2. against the cameras
@pytest.mark.parametrize("mode", ["pooled", "frame"])
def test_rays_are_the_cameras_rays_and_only_valid_pixels_are_drawn(dev, mixed, mode):
    fs, _ = mixed
    for off in (10, 14, 16):
        _state(fs, off)
        b = fs.sample(20000, mode)
        for f, fr in enumerate(fs.frames):
            rows = torch.nonzero(b["frame"] == f).reshape(-1)
            if rows.numel() == 0:
                continue
            pix = b["pix"][rows].contiguous()
            assert torch.equal(b["rays"][0][rows], fr["camera"].rays(fr["c2w"], fr["near"], fr["far"], pix))
            assert int(pix.min()) >= 0 and int(pix.max()) < fr["camera"].width * fr["camera"].height
            if fr["pix"] is not None:
                assert bool(torch.isin(pix, fr["pix"]).all())
            assert torch.equal(b["rgb"][0][rows].cpu(), fr["rgb"].reshape(-1, 3)[pix.long()].cpu().float() / 255.0)       # (IEEE division)
        assert int(b["frame"].min()) >= 0
        assert bool((b["rays"][0][:, 3:6].abs().sum(-1) > 0).all())          # no ray of a pixel that sees nothing


# ---------------------------------------------------------------------------------------------------- 3. ranks and offsets
@pytest.mark.parametrize("mode", ["pooled", "frame"])
def test_rank_batches_concatenate_and_successive_batches_differ(dev, mixed, mode):
    fs, ref = mixed
    R = 1000
    _state(fs, 21)
    whole = fs.sample(4 * R, mode)
    parts = []
    for rank in range(4):
        _state(fs, 21)
        parts.append(fs.sample(R, mode, rank=rank, world=4))
    for k, _ in KEYS:
        cat = torch.cat([p[k] for p in parts], 0 if k in ("frame", "pix") else 1)
        assert torch.equal(cat, whole[k]), k
    _state(fs, 30)
    a, b = fs.sample(R, mode), fs.sample(R, mode)
    assert not torch.equal(a["pix"], b["pix"])
    m = 0 if mode == "pooled" else 1
    _same_as_ref(a, br.sample(ref, SEED, 30, R, m), "first")
    _same_as_ref(b, br.sample(ref, SEED, 31, R, m), "second")
    # another seed: another stream
    _state(fs, 30, seed=SEED + 1)
    c = fs.sample(R, mode)
    assert not torch.equal(a["pix"], c["pix"])
    _same_as_ref(c, br.sample(ref, SEED + 1, 30, R, m), "seed")


# ---------------------------------------------------------------------------------------------------- 4. NULL outputs
def test_null_outputs_and_canaries(dev, mixed):
    fs, _ = mixed
    R, PAD = 777, 64
    call = torch.tensor([SEED, 40], dtype=torch.int64, device=dev)
    draw = ops.Draw(call, 16, 5)
    full = ops.sample_batch(fs.table, fs.cum, fs.n_frames, draw, R)
    names = [n for n, _, _ in ops.BATCH_OUTPUTS]
    assert sorted(full) == sorted(names)
    for want in [[n] for n in names] + [["rays", "pix"], ["rgb", "depth", "sem", "inst", "frame"], names]:
        bufs, out = {}, {}
        for n, tail, dt in ops.BATCH_OUTPUTS:
            if n not in want:
                continue
            width = int(np.prod(tail, dtype=np.int64))
            canary = -12345.0 if dt == torch.float32 else -12345
            bufs[n] = torch.full(((R + 2 * PAD) * width,), canary, dtype=dt, device=dev)
            out[n] = bufs[n][PAD * width:(PAD + R) * width].view((R,) + tail)
        res = ops.sample_batch(fs.table, fs.cum, fs.n_frames, draw, R, want=want, out=out)
        assert sorted(res) == sorted(want)
        for n in want:
            width = bufs[n].numel() // (R + 2 * PAD)
            assert res[n].data_ptr() == out[n].data_ptr() and torch.equal(res[n], full[n]), (want, n)
            assert bool((bufs[n][:PAD * width] == -12345).all()) and bool((bufs[n][(PAD + R) * width:] == -12345).all()), (want, n)
    with pytest.raises(ValueError, match="unknown output"):
        ops.sample_batch(fs.table, fs.cum, fs.n_frames, draw, R, want=["rays", "colour"])
    with pytest.raises(ValueError, match="out must be"):
        ops.sample_batch(fs.table, fs.cum, fs.n_frames, draw, R, out={"rays": torch.empty(R + 1, 8, device=dev)})
    with pytest.raises(RuntimeError, match="tag clash"):
        ops.sample_batch(fs.table, fs.cum, fs.n_frames, ops.Draw(call, 2), R)


# ---------------------------------------------------------------------------------------------------- 5. captured graphs
def _small_frame(g, W=40, H=24, pose=None, labels=True):
    cam = Pinhole(30.0, 31.0, 19.5, 11.5, W, H)
    im = _images(g, H, W, 6, 4)
    if not labels:
        im = {"rgb": im["rgb"], "depth": im["depth"]}
    return cam, (cr.pose(0.1) if pose is None else pose), im


def test_captured_sampler_replays_equal_eager_and_see_the_table_change(dev):
    g = torch.Generator().manual_seed(8)
    fs, ref = FrameSet(dev, capacity=4, seed=5), []
    R, K = 3000, 4
    # an empty set: zero rays, frame = pix = -1, labels -1
    static = fs.sample(R)
    assert not static["rays"].any() and not static["rgb"].any() and not static["depth"].any()
    for k in ("frame", "pix", "pseudo_label", "instance_label"):
        assert bool((static[k] == -1).all()), k
    e = fs.sample(R, "frame")
    assert not e["rays"].any() and bool((e["frame"] == -1).all())
    for i in range(2):
        cam, c2w, im = _small_frame(g, pose=cr.pose(0.4 * i, 0.0, (i, 1.0, 0.0)), labels=i == 0)
        _add(fs, ref, cam, c2w, 0.5, 30.0, im)
    s0 = fs.rng_state.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fs.sample(R, out=static)
    torch.cuda.synchronize()
    assert torch.equal(fs.rng_state, s0)                               # a capture runs nothing
    replays = []
    for _ in range(K):
        graph.replay()
        replays.append({k: static[k].clone() for k, _ in KEYS})
    assert fs.rng_state.tolist() == [5, int(s0[1]) + K]
    fs.rng_state.copy_(s0)
    for i in range(K):
        eager = fs.sample(R)
        for k, _ in KEYS:
            assert torch.equal(eager[k], replays[i][k]), (i, k)
        _same_as_ref(replays[i], br.sample(ref, 5, int(s0[1]) + i, R, 0), i)
    assert not torch.equal(replays[0]["pix"], replays[1]["pix"])
    # a frame added after the capture is drawn by later replays
    assert int(replays[-1]["frame"].max()) == 1
    cam, c2w, im = _small_frame(g, W=64, H=48, pose=cr.pose(-0.7, 0.1, (0.0, 2.0, 5.0)))
    _add(fs, ref, cam, c2w, 0.5, 30.0, im)
    off = int(fs.rng_state[1])
    graph.replay()
    assert int(static["frame"].max()) == 2 and int((static["frame"] == 2).sum()) > R // 4
    _same_as_ref(static, br.sample(ref, 5, off, R, 0), "after add")


def test_capacity_is_reached_through_add_and_boxes_update_in_place(dev):
    g = torch.Generator().manual_seed(12)
    fs = FrameSet(dev, capacity=2, seed=3)
    for i in range(2):
        cam, c2w, im = _small_frame(g, pose=cr.pose(0.2 * i))
        assert fs.add(cam, c2w, 0.5, 30.0, im["rgb"]) == i
    table, cum, nf = fs.table.clone(), fs.cum.clone(), fs.n_frames.clone()
    assert nf.tolist() == [2] and cum.tolist() == [0, 960, 1920]
    with pytest.raises(RuntimeError, match="full"):
        fs.add(cam, c2w, 0.5, 30.0, im["rgb"])
    assert len(fs) == 2 and fs.n_pixels == 1920
    assert torch.equal(fs.table, table) and torch.equal(fs.cum, cum) and torch.equal(fs.n_frames, nf)
    # set_boxes with the same number of boxes writes into the tensors earlier batches hold
    box, ids = synthetic.random_boxes(8, 6, 4, seed=1)
    fs.set_boxes(box, ids)
    batch = fs.sample(64)
    box2, ids2 = synthetic.random_boxes(8, 6, 4, seed=2)
    fs.set_boxes(box2, ids2)
    assert torch.equal(batch["bbox"].cpu(), box2) and torch.equal(batch["bbox_ids"].cpu(), ids2) and batch["bbox"] is fs.bbox
    fs.set_boxes(*synthetic.random_boxes(5, 6, 4, seed=2))                  # another count: new tensors, the old batch keeps its own
    assert batch["bbox"].shape == (8, 15) and fs.bbox.shape == (5, 15) and fs.sample(64)["bbox"] is fs.bbox


# ---------------------------------------------------------------------------------------------------- 6. the self-feeding step
def _training_set(dev, C, K, seed=1):
    g = torch.Generator().manual_seed(4)
    fs = FrameSet(dev, capacity=8, seed=seed)
    pin = _kitti_pinhole()
    im = _images(g, pin.height, pin.width, C, K)
    fs.add(pin, cr.pose(0.0, 0.0, (0.0, 1.55, 0.0)), 0.5, 100.0, im["rgb"], im["depth"], im["pseudo_label"], im["instance_label"])
    fish, c2w = synthetic.fisheye_camera(scale=200 / 1400)
    im = _images(g, fish.height, fish.width, C, K)
    fs.add(fish, c2w, 0.5, 100.0, im["rgb"], None, im["pseudo_label"], None)
    im = _images(g, pin.height, pin.width, C, K)
    fs.add(pin, cr.pose(0.6, 0.0, (3.0, 1.55, 4.0)), 0.5, 100.0, im["rgb"].float() / 255.0, im["depth"])
    box, ids = synthetic.random_boxes(16, C, K, seed=2)
    fs.set_boxes(box, ids)
    return fs


def _opt_state(opt):
    return [(k, v) for p in opt.param_groups[0]["params"] for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("mode", ["pooled", "frame"])
def test_self_feeding_graphed_step_equals_eager_and_parent_style_steps(dev, mode, split):
    C, K, R, STEPS = 6, 4, 512, 5
    cfg = NS(N_samples=32, N_importance=32, num_classes=C, num_instances=K, precision="bf16", D=4, W=128, skips=[1],
             rng="device", rng_seed=31, perturb=1.0, raw_noise_std=1.0)
    torch.manual_seed(6)
    net_e = make_network(cfg).to(dev).train()
    net_g, net_p = copy.deepcopy(net_e), copy.deepcopy(net_e)
    fs = _training_set(dev, C, K)
    wraps = [NetworkWrapper(n, cfg) for n in (net_e, net_g, net_p)]
    opts = [torch.optim.Adam(n.parameters(), lr=1e-3, capturable=True, fused=True) for n in (net_e, net_g, net_p)]
    fs.sample(R, mode)                                           # the state is not at its beginning
    s0 = fs.rng_state.clone()
    calls = []
    step = pnr_train.GraphedStep(wraps[1], opts[1], frames=fs, n_rays=R, mode=mode, reduce=(lambda: calls.append(1)) if split else None)
    # constructing it draws nothing and trains nothing
    assert torch.equal(fs.rng_state, s0) and torch.equal(wraps[1].renderer.rng_state, wraps[0].renderer.rng_state)
    for a, b in zip(net_e.parameters(), net_g.parameters()):
        assert torch.equal(a, b)
    for _, v in _opt_state(opts[1]):
        assert float(v.abs().sum()) == 0.0
    n_warm = len(calls)
    losses_g, drawn = [], []
    for _ in range(STEPS):
        _, loss, stats = step()
        losses_g.append(loss.item())
        drawn.append({k: step.static[k].clone() for k, _ in KEYS})
    assert fs.rng_state.tolist() == [int(s0[0]), int(s0[1]) + STEPS]
    assert len(calls) == n_warm + (STEPS if split else 0)
    with pytest.raises(ValueError, match="takes no batch"):
        step(drawn[0])
    # eager: wrapper(frames.sample(...)) from the same state
    fs.rng_state.copy_(s0)
    losses_e, batches = [], []
    for i in range(STEPS):
        batch = fs.sample(R, mode)
        for k, _ in KEYS:
            assert torch.equal(batch[k], drawn[i][k]), (i, k)              # the replay's batch IS the eager batch
        batches.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})
        opts[0].zero_grad(set_to_none=False)
        _, loss, _, _ = wraps[0](batch)
        loss.backward()
        opts[0].step()
        losses_e.append(loss.item())
    assert losses_g == losses_e, (losses_g, losses_e)
    assert len(set(losses_g)) == STEPS
    # the parent-style step fed those batches
    step_p = pnr_train.GraphedStep(wraps[2], opts[2], batches[-1])
    losses_p = [step_p(b)[1].item() for b in batches]
    assert losses_p == losses_e, (losses_p, losses_e)
    for (n, a), b, c in zip(net_e.named_parameters(), net_g.parameters(), net_p.parameters()):
        assert torch.equal(a, b), ("self-feeding != eager", n)
        assert torch.equal(a, c), ("parent-style != eager", n)
    for (k, a), (_, b), (_, c) in zip(_opt_state(opts[0]), _opt_state(opts[1]), _opt_state(opts[2])):
        assert torch.equal(a, b) and torch.equal(a, c), ("optimiser state", k)
    assert any(float(v.abs().sum()) > 0 for k, v in _opt_state(opts[1]) if k == "exp_avg")
    if mode == "frame":
        assert all(len(set(d["frame"].tolist())) == 1 for d in drawn)


# ---------------------------------------------------------------------------------------------------- 7. evaluation batches
def test_frame_batch_renders_as_render_view(dev):
    C, K = 6, 4
    cfg = NS(N_samples=32, N_importance=32, num_classes=C, num_instances=K, precision="bf16", D=4, W=128, skips=[1], chunk_size=4096)
    torch.manual_seed(2)
    net = synthetic.trained_like_(make_network(cfg)).to(dev).eval()
    rend = make_renderer(cfg, net)
    g = torch.Generator().manual_seed(9)
    fs = FrameSet(dev, capacity=4)
    mask = torch.ones(96, 96, dtype=torch.bool)
    mask[70:] = False
    fish, c2w = synthetic.fisheye_camera(scale=96 / 1400, mask=mask)
    im = _images(g, 96, 96, C, K)
    fs.add(fish, c2w, 0.5, 40.0, im["rgb"], im["depth"], im["pseudo_label"])
    cam, c2w_p, im_p = _small_frame(g, W=80, H=48)
    fs.add(cam, c2w_p, 0.5, 40.0, im_p["rgb"], None, None, im_p["instance_label"])
    box, ids = synthetic.random_boxes(16, C, K, seed=2)
    fs.set_boxes(box, ids)
    for i, (camera, pose, imgs) in enumerate(((fish, c2w, im), (cam, c2w_p, im_p))):
        b = fs.frame_batch(i)
        pix = camera.valid_pix(dev).long()
        P = pix.numel()
        assert b["rays"].shape == (1, P, 8) and torch.equal(b["pix"].long(), pix) and bool((b["frame"] == i).all())
        assert torch.equal(b["rgb"][0].cpu(), imgs["rgb"].reshape(-1, 3)[pix.cpu()].float() / 255.0)
        if i == 0:
            assert torch.equal(b["depth"][0], imgs["depth"].to(dev).reshape(-1)[pix]) and bool((b["instance_label"] == -1).all())
            assert torch.equal(b["pseudo_label"][0], imgs["pseudo_label"].to(dev).reshape(-1)[pix].int()) and P < 96 * 70
        else:
            assert not b["depth"].any() and bool((b["pseudo_label"] == -1).all()) and P == 80 * 48
        with torch.no_grad():
            out = rend.render(b)
            view = rend.render_view(camera, pose, 0.5, 40.0, fs.bbox, fs.bbox_ids)
        n = 0
        for k, v in out.items():
            if k in view and v.dim() >= 2 and v.shape[1] == P:
                assert torch.equal(v[0], view[k].reshape(camera.height * camera.width, *view[k].shape[2:])[pix]), (i, k)
                n += 1
        assert n >= 6, sorted(out)
