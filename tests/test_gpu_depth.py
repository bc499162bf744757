"""GPU tests of the depth front end (csrc/pnr_depth.hip; include/pnr.h "depth front end") against tests/_depth_ref.py: k_depth_filter's
output and support and k_depth_normals' normal, vertex and code are the restatement's bit patterns between canaries at the sizes
where a tile, a halo or an edge can go wrong; depth.view feeds fusion.track bit for bit; fusion.odometry equals the restated chain,
follows an edited depth image in a captured graph and closes the loop into set_pose and integrate; stereo -> filter -> normals end
to end.  tests/test_depth_ref.py pins the restatement on the CPU."""
import numpy as np
import pytest
import torch

import _depth_ref as dr
import _icp_ref as ir
from panopticnerf_amd.evaluate import Evaluator
from panopticnerf_amd import Equirect, Fisheye, FrameSet, Pinhole, camera, consistency, depth, fusion, ops, pointcloud, stereo, synthetic

pytestmark = pytest.mark.gpu

GUARD = 64
MODELS = ("pinhole", "fisheye", "equirect")
SIZES = [(1, 1), (7, 5), (64, 4), (65, 3), (70, 41), (300, 70)]     # one pixel; below a tile; a tile's width; one past it; ragged tiles; many
TRUTH = np.asarray(ir.TRUE_POSE, np.float32)
FAR = TRUTH.copy()
FAR[:, 3] += np.array([1203.7, 3817.3, 115.9], np.float32)           # KITTI-sized world coordinates
SOLVE_ARGS = dict(min_matches=64, max_rot=0.25, max_trans=0.5)
DIST_MAX = 0.25


class Guarded:
    """an output array filled with junk, with GUARD canary elements before and after it, in one allocation"""

    def __init__(self, shape, dtype, dev):
        self.n = int(np.prod(shape))
        self.canary, junk = (-7.25e30, 3.5e12) if dtype.is_floating_point else (0x65, 0x5A)
        self.buf = torch.full((self.n + 2 * GUARD,), self.canary, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(junk)
        self.junk = junk

    def intact(self):
        return bool((self.buf[:GUARD] == self.canary).all()) and bool((self.buf[GUARD + self.n:] == self.canary).all())

    def untouched(self):
        return bool((self.t == self.junk).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def w2c_of(c2w):
    return camera.invert_pose(torch.as_tensor(np.asarray(c2w, np.float32))).numpy()


def scene(w, h, seed):
    """a dirty depth image with slopes, a step, noise around the range gate, and edge values"""
    g = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = 2.0 + 0.5 * np.sin(i / 7.0) + 0.3 * np.cos(j / 5.0) + 0.04 * g.standard_normal((h, w))
    d[:, w // 2:] += 0.8
    return dr.dirty(d.astype(np.float32), seed) if w * h > 1 else d.astype(np.float32)


def cam_of(name, w, h):
    if name == "pinhole":
        f = 0.6 * max(w, h) + 5.0
        return Pinhole(f, f * 1.03, (w - 1) / 2.0, (h - 1) / 2.0, w, h)
    if name == "fisheye":
        g = 0.55 * max(w, h) + 3.0
        return Fisheye(ir._FISH[0], ir._FISH[1], ir._FISH[2], g, g * 1.01, (w - 1) / 2.0, (h - 1) / 2.0, w, h)
    return Equirect(w, h)


# ------------------------------------------------------------------------------------------------ the filter
def run_filter(dev, d, want_support=True, **args):
    h, w = d.shape
    out, sup = Guarded((h, w), torch.float32, dev), Guarded((h, w), torch.int16, dev)
    src = torch.as_tensor(d).to(dev)
    ops.depth_filter(src, out.t, support=sup.t if want_support else None, **args)
    torch.cuda.synchronize()
    assert out.intact() and sup.intact() and same(src.cpu().numpy(), d)
    if not want_support:
        assert sup.untouched()
    return out.t.cpu().numpy(), sup.t.cpu().numpy()


@pytest.mark.parametrize("w,h", SIZES)
def test_filter_bits_at_every_size_and_radius(dev, w, h):
    """radii 0, 1, 3 and 8 (a halo wider than the small images) on dirty depths: output and support are filter32's bits, between
    canaries; without `support` the output is the same and nothing else is written; two runs give the same bits"""
    d = scene(w, h, w + h)
    for radius in (0, 1, 3, 8):
        args = dict(radius=radius, sigma_space=1.5 if radius < 8 else 4.0, sigma_range=(0.01, 0.03), min_support=1 + radius)
        want, want_sup = dr.filter32(d, **args)
        got, got_sup = run_filter(dev, d, **args)
        assert same(got, want), "radius %d: %d of %d pixels differ" % (radius, (bits(got).view(np.uint32) != bits(want).view(np.uint32)).sum(), w * h)
        assert np.array_equal(got_sup, want_sup)
        alone, _ = run_filter(dev, d, want_support=False, **args)
        assert same(alone, got)
        if w * h >= 64 and radius:
            assert (want_sup > 1).any() and ((want == 0) & dr._valid(d)).any() == bool(((want_sup < 1 + radius) & dr._valid(d)).any())
    assert same(run_filter(dev, d, radius=3)[0], run_filter(dev, d, radius=3)[0])


def test_filter_module_call(dev):
    d = scene(70, 41, 3)
    src = torch.as_tensor(d).to(dev)
    out, sup = depth.filter(src, radius=2, min_support=3, support=True)
    want, want_sup = dr.filter32(d, radius=2, min_support=3)
    assert same(out.cpu().numpy(), want) and np.array_equal(sup.cpu().numpy(), want_sup) and sup.dtype == torch.int16
    assert torch.equal(depth.filter(src, radius=2, min_support=3).view(torch.int32), out.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the normals
def run_normals(dev, cam, c2w, d, want=("vertex", "code"), **args):
    h, w = cam.height, cam.width
    out = {"normal": Guarded((h, w, 3), torch.float32, dev), "vertex": Guarded((h, w, 3), torch.float32, dev), "code": Guarded((h, w), torch.uint8, dev)}
    ops.depth_normals(cam.model, cam.params, torch.as_tensor(np.asarray(c2w, np.float32)), w, h, torch.as_tensor(d).to(dev), out["normal"].t,
                      vertex=out["vertex"].t if "vertex" in want else None, code=out["code"].t if "code" in want else None, **args)
    torch.cuda.synchronize()
    assert all(g.intact() for g in out.values())
    for k in ("vertex", "code"):
        if k not in want:
            assert out[k].untouched(), "%s was written though it was not asked for" % k
    return {k: out[k].t.cpu().numpy().reshape(-1, 3) if k != "code" else out[k].t.cpu().numpy().reshape(-1) for k in ("normal",) + tuple(want)}


@pytest.mark.parametrize("pose_name", ["near", "far"])
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("w,h", SIZES)
def test_normals_bits_for_every_model_pose_and_size(dev, w, h, name, pose_name):
    """normal, vertex and code are normals32's bits for the three models x two poses (the far one at KITTI-sized coordinates) at
    every size, dirty depths mixed in.  A fisheye frame keeps a positive depth outside its lens (refused by its ray, not by its
    depth); a full panorama's first and last column have no neighbour across the seam"""
    cam = cam_of(name, w, h)
    c2w = TRUTH if pose_name == "near" else FAR
    d = ir.room_maps(cam, TRUTH)[0]
    if name == "fisheye":
        d[d == 0] = 2.0
    if w * h >= 64:
        d = dr.dirty(d, w)
    view = ir.model_of(cam, c2w)
    ref = dr.normals32(view, d)
    got = run_normals(dev, cam, c2w, d)
    for k in ("normal", "vertex", "code"):
        assert same(got[k], ref[k]), "%s: %d of %d values differ" % (k, (got[k] != ref[k]).sum(), ref[k].size)
    code = ref["code"].reshape(h, w)
    if w * h == 1:
        assert code[0, 0] == dr.NO_NEIGHBOUR
    if w >= 64 and h >= 41:
        assert (code == dr.OK).any() and (code == dr.NO_DEPTH).any()
    if name == "fisheye" and w >= 64 and h >= 41:
        assert code[0, 0] == dr.NO_DEPTH and code[-1, -1] == dr.NO_DEPTH and d[0, 0] > 0
    if name == "equirect" and w >= 7 and h >= 3:
        used = [u.reshape(h, w) for u in ref["used"]]                            # left, right, up, down
        assert not used[0][:, 0].any() and not used[1][:, -1].any()
        assert w < 64 or h < 41 or ((code[1:-1, 0] == dr.OK).any() and (code[1:-1, -1] == dr.OK).any())  # one-sided along x


def test_normals_optional_outputs_and_scalars(dev):
    """every optional output skipped in turn; other jump gates and min_cos, with GRAZING pixels"""
    cam = cam_of("fisheye", 70, 41)
    d = dr.dirty(ir.room_maps(cam, TRUTH)[0], 9)
    full = run_normals(dev, cam, TRUTH, d)
    for want in (("vertex",), ("code",), ()):
        got = run_normals(dev, cam, TRUTH, d, want=want)
        for k in got:
            assert same(got[k], full[k])
    for jump, min_cos in (((0.05, 0.02), 0.9), ((float("inf"), 0.0), 0.0), ((0.0, 0.0), 1.0)):
        ref = dr.normals32(ir.model_of(cam, TRUTH), d, jump, min_cos)
        got = run_normals(dev, cam, TRUTH, d, jump=jump, min_cos=min_cos)
        for k in ("normal", "vertex", "code"):
            assert same(got[k], ref[k]), (k, jump, min_cos)
    assert (dr.normals32(ir.model_of(cam, TRUTH), d, (0.05, 0.02), 0.9)["code"] == dr.GRAZING).any()


def test_normals_of_constructed_pixels(dev):
    """the constructed cases of test_depth_ref.py on the device: DEGENERATE by underflow, GRAZING on a ramp, s exactly 0"""
    cam = Pinhole(40.0, 40.0, 3.0, 2.0, 7, 5)
    view = ir.model_of(cam, np.eye(4, dtype=np.float32)[:3])
    eye = np.eye(4, dtype=np.float32)[:3]
    ramp = (2.0 + 0.6 * np.arange(7, dtype=np.float32))[None, :].repeat(5, 0)
    for d, jump, min_cos, code in ((np.full((5, 7), 1e-30, np.float32), (0.0, 0.05), 0.1, dr.DEGENERATE), (ramp, (float("inf"), 0.0), 0.5, dr.GRAZING)):
        ref = dr.normals32(view, d, jump, min_cos)
        got = run_normals(dev, cam, eye, d, jump=jump, min_cos=min_cos)
        assert (ref["code"] == code).all() and all(same(got[k], ref[k]) for k in got)
    cam0 = Pinhole(1e37, 1e10, 1.0, 1.0, 3, 3)
    d = np.full((3, 3), 2.5, np.float32)
    d[1, 0], d[1, 2] = 2.0, 3.0
    for min_cos, code in ((0.1, dr.GRAZING), (0.0, dr.OK)):
        ref = dr.normals32(ir.model_of(cam0, eye), d, (float("inf"), 0.0), min_cos)
        got = run_normals(dev, cam0, eye, d, jump=(float("inf"), 0.0), min_cos=min_cos)
        assert ref["s"][4] == 0.0 and ref["code"][4] == code and all(same(got[k], ref[k]) for k in got)


# ------------------------------------------------------------------------------------------------ depth.view into fusion.track
@pytest.mark.parametrize("ln,mn", [("pinhole", "pinhole"), ("fisheye", "equirect")])
def test_view_feeds_track_bit_for_bit(dev, ln, mn):
    """a model view made by depth.view of a depth image alone: fusion.track on it equals the restated track on normals32's normals in
    every history row and the final pose; the same view goes into consistency.reproject, pointcloud.lift and Evaluator.evaluate_depth"""
    lcam, mcam = ir.cameras()[ln], ir.cameras(0.75)[mn]
    dl = ir.room_maps(lcam, TRUTH)[0]
    dm = ir.room_maps(mcam, ir.MODEL_POSE)[0]
    c2w_m = torch.as_tensor(np.asarray(ir.MODEL_POSE, np.float32))
    view = depth.view(mcam, c2w_m, torch.as_tensor(dm).to(dev), vertex=True)
    assert view[0] is mcam and sorted(view[2]) == ["code", "depth", "normal", "valid", "vertex"]
    model = ir.model_of(mcam, ir.MODEL_POSE)
    ref = dr.normals32(model, dm)
    assert same(view[2]["normal"].cpu().numpy().reshape(-1, 3), ref["normal"]) and torch.equal(view[2]["valid"], view[2]["code"] == depth.OK)
    guess = ir.perturbed(TRUTH, *ir.GUESS).astype(np.float32)
    c2w, info = fusion.track(view, lcam, torch.as_tensor(dl).to(dev), torch.as_tensor(guess.reshape(3, 4)), iters=10, dist_max=DIST_MAX, **SOLVE_ARGS)
    torch.cuda.synchronize()
    grid = ir.blocks_for(lcam.width * lcam.height, cu_count(dev))
    pose, hist, out, _ = ir.track(ir.live_of(lcam), dl, guess, model, dm, ref["normal"], 10, DIST_MAX, grid=grid, w2c=w2c_of(ir.MODEL_POSE), **SOLVE_ARGS)
    assert same(info["history"].cpu().numpy(), hist) and same(c2w.cpu().numpy().reshape(12), pose)
    assert np.array_equal(info["code"].cpu().numpy().reshape(-1), out["code"]) and (hist[:, 4] == ir.OK).all()
    e = ir.pose_error(pose, TRUTH)
    print("%s -> %s with depth-derived normals: final error %.3g rad, %.3g" % ((ln, mn) + e))
    # the view as the other consumers take it
    match = consistency.reproject(view, view)
    have = view[2]["depth"] > 0
    own = torch.arange(mcam.width * mcam.height, device=dev, dtype=match.dtype).reshape(match.shape)
    assert float((match[have] == own[have]).float().mean()) > 0.95
    pts, pix = pointcloud.lift(view)
    vert = view[2]["vertex"].reshape(-1, 3)[pix.long()]
    assert pts.shape[0] == int((view[2]["code"] != depth.NO_DEPTH).sum()) and torch.equal(pts.view(torch.int32), vert.view(torch.int32))   # (lift's arithmetic is the rule's step 1)
    ev = Evaluator()
    ev.evaluate_depth(view[2], view[2]["depth"])


# ------------------------------------------------------------------------------------------------ fusion.odometry
@pytest.fixture(scope="module")
def sequence():
    cam = ir.cameras()["pinhole"]
    truths, depths = dr.room_sequence(cam, 6)
    return cam, truths, depths


def test_odometry_equals_the_restated_chain(dev, sequence):
    """six 64 x 48 room frames: the relative poses and the histories are the restated chain's bit for bit (every operation of the
    filter, the normals, the accumulate and the solve is pinned), the composed poses agree within 1e-6; a filter in front changes
    nothing about that; every status is ICP_OK"""
    cam, truths, depths = sequence
    grid = ir.blocks_for(cam.width * cam.height, cu_count(dev))
    eye_w2c = w2c_of(np.eye(4, dtype=np.float32)[:3])
    on_dev = [torch.as_tensor(d).to(dev) for d in depths]
    for filt, guess in ((None, "identity"), (dict(radius=2, min_support=3), "velocity")):
        poses, info = fusion.odometry(cam, on_dev, c2w0=torch.as_tensor(truths[0]), filter=filt, guess=guess, iters=6, dist_max=DIST_MAX, **SOLVE_ARGS)
        torch.cuda.synchronize()
        assert tuple(poses.shape) == (6, 3, 4) and poses.dtype == torch.float32 and poses.is_cuda
        assert tuple(info["relative"].shape) == (5, 3, 4) and tuple(info["history"].shape) == (5, 7, 5) and info["history"].dtype == torch.float64
        want, rel, hist = dr.odometry(cam, depths, c2w0=truths[0], filter=filt, guess=guess, iters=6, dist_max=DIST_MAX, grid=grid, w2c=eye_w2c, **SOLVE_ARGS)
        assert same(info["relative"].cpu().numpy(), rel), "the relative poses differ from the restated chain"
        assert same(info["history"].cpu().numpy(), hist)
        assert np.abs(poses.cpu().numpy().astype(np.float64) - want).max() <= 1e-6
        assert (hist[:, :, 4] == ir.OK).all()
        e = ir.pose_error(poses[5].cpu().numpy(), truths[5])
        print("odometry (filter %s, guess %s): drift after five steps %.3g rad, %.3g" % ((filt, guess) + e))
    # one (F, h, w) tensor, no c2w0: the first pose is the identity
    poses1, _ = fusion.odometry(cam, torch.stack(on_dev), iters=2, dist_max=DIST_MAX, **SOLVE_ARGS)
    assert torch.equal(poses1[0].cpu(), torch.eye(4)[:3])
    # a single frame: nothing to track
    poses0, info0 = fusion.odometry(cam, on_dev[:1], iters=2)
    assert tuple(poses0.shape) == (1, 3, 4) and tuple(info0["relative"].shape) == (0, 3, 4) and tuple(info0["history"].shape) == (0, 3, 5)


def test_a_failed_step_keeps_the_guess(dev, sequence):
    """a frame without depth in the middle: its two steps are ICP_TOO_FEW, their relative pose is the guess (identity), and the chain
    goes on"""
    cam, truths, depths = sequence
    on_dev = [torch.as_tensor(d).to(dev) for d in depths[:4]]
    on_dev[2] = torch.zeros_like(on_dev[2])
    poses, info = fusion.odometry(cam, on_dev, iters=3, dist_max=DIST_MAX, **SOLVE_ARGS)
    hist, rel = info["history"].cpu().numpy(), info["relative"].cpu()
    assert (hist[0, :, 4] == fusion.ICP_OK).all() and (hist[1:, :, 4] == fusion.ICP_TOO_FEW).all()
    assert torch.equal(rel[1], torch.eye(4)[:3]) and torch.equal(rel[2], torch.eye(4)[:3]) and not torch.equal(rel[0], torch.eye(4)[:3])
    assert torch.equal(poses[1], poses[2]) and torch.equal(poses[2], poses[3])


def test_odometry_in_a_graph_then_set_pose_and_integrate(dev, sequence):
    """the whole call captured: a replay after one depth image was edited equals the eager call on the edited images.  Then the
    poses close the loop: set_pose + integrate of those frames equals integrate of a set built with the same poses"""
    cam, truths, depths = sequence
    h, w = cam.height, cam.width
    imgs = [torch.as_tensor(d).to(dev) for d in depths]
    first = torch.as_tensor(truths[0]).to(dev)
    run = lambda: fusion.odometry(cam, imgs, c2w0=first, filter=dict(radius=1), iters=4, dist_max=DIST_MAX, **SOLVE_ARGS)
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        poses_g, info_g = run()
    graph.replay()
    torch.cuda.synchronize()
    before = poses_g.clone()
    other = ir.room_maps(cam, ir.perturbed(truths[3], (0.004, 0.003, -0.002), (0.01, -0.01, 0.005)).astype(np.float32))[0]
    imgs[3].copy_(torch.as_tensor(other).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    poses_e, info_e = run()
    torch.cuda.synchronize()
    assert not torch.equal(before, poses_g) and torch.equal(before[:3], poses_g[:3])
    assert torch.equal(poses_g.view(torch.int32), poses_e.view(torch.int32))
    assert torch.equal(info_g["relative"].view(torch.int32), info_e["relative"].view(torch.int32))
    assert torch.equal(info_g["history"].view(torch.int64), info_e["history"].view(torch.int64))
    # the loop
    host = poses_e.cpu()
    lo, hi = tuple(v - 0.3 for v in ir.ROOM[0]), tuple(v + 0.3 for v in ir.ROOM[1])
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8)
    tracked, built = FrameSet(dev, capacity=6), FrameSet(dev, capacity=6)
    for f in range(6):
        tracked.add(cam, torch.as_tensor(truths[0]), 0.1, 10.0, rgb, depth=imgs[f].cpu())          # placeholders for every pose
        built.add(cam, host[f], 0.1, 10.0, rgb, depth=imgs[f].cpu())
    tracked.w2c_table()
    for f in range(6):
        tracked.set_pose(f, host[f])
    vol_a, vol_b = fusion.Volume(lo, hi, 32, dev), fusion.Volume(lo, hi, 32, dev)
    fusion.integrate(vol_a, tracked, 0.45)
    fusion.integrate(vol_b, built, 0.45)
    torch.cuda.synchronize()
    assert torch.equal(vol_a.tsdf.view(torch.int32), vol_b.tsdf.view(torch.int32)) and torch.equal(vol_a.weight, vol_b.weight)
    assert float((vol_a.weight > 1).float().mean()) > 0.01


# ------------------------------------------------------------------------------------------------ end to end, refusals
def test_stereo_filter_normals_end_to_end(dev):
    """synthetic.stereo_pair -> stereo.depth_from_pair -> depth.filter(min_support) -> depth.normals equals the restatement on the
    matcher's own depth image; the share of valid pixels before and after the speckle rule"""
    left, right, _, _ = synthetic.stereo_pair(64, 128, seed=1)
    H, W = left.shape
    cam = Pinhole(120.0, 120.0, (W - 1) / 2.0, (H - 1) / 2.0, W, H)
    raw = stereo.depth_from_pair(left.to(dev), right.to(dev), cam, 0.6, max_disp=32)
    args = dict(radius=2, sigma_range=(0.0, 0.05), min_support=6)
    filt = depth.filter(raw, **args)
    eye = torch.eye(4)[:3]
    maps = depth.normals(cam, eye, filt, vertex=True)
    torch.cuda.synchronize()
    raw_h = raw.cpu().numpy()
    want = dr.filter32(raw_h, **args)[0]
    assert same(filt.cpu().numpy(), want)
    ref = dr.normals32(ir.model_of(cam, eye.numpy()), want)
    for k in ("normal", "vertex", "code"):
        assert same(maps[k].cpu().numpy().reshape(ref[k].shape), ref[k]), k
    assert maps["depth"] is filt
    print("stereo depth: %.1f %% of the pixels valid, %.1f %% after the filter with min_support %d, %.1f %% with a normal"
          % (100.0 * (raw_h > 0).mean(), 100.0 * (want > 0).mean(), args["min_support"], 100.0 * (ref["code"] == dr.OK).mean()))
    assert 0 < (want > 0).sum() <= (raw_h > 0).sum()


def test_transposed_views_are_refused_by_name(dev):
    """the kernels index the images flat: a transposed view of the right shape is refused in the caller's name, on real device tensors"""
    cam = ir.cameras()["pinhole"]
    h, w = cam.height, cam.width
    eye = torch.eye(4)[:3]
    bad, good = torch.ones((w, h), device=dev).t(), torch.ones((h, w), device=dev)
    with pytest.raises(ValueError, match="depth.filter: depth must be contiguous"):
        depth.filter(bad)
    with pytest.raises(ValueError, match="depth.normals: depth must be contiguous"):
        depth.normals(cam, eye, bad)
    with pytest.raises(ValueError, match="depth.view: depth must be contiguous"):
        depth.view(cam, eye, bad, filter=dict(radius=1))
    with pytest.raises(ValueError, match="fusion.odometry: frame 1: depth must be contiguous"):
        fusion.odometry(cam, [good, bad])
    with pytest.raises(ValueError, match="depth_filter: out: tensor must be contiguous"):
        ops.depth_filter(good, bad)
    with pytest.raises(ValueError, match="depth_filter: out must not be depth itself"):
        ops.depth_filter(good, good)
    with pytest.raises(ValueError, match="depth_normals: normal: tensor must be contiguous"):
        ops.depth_normals("pinhole", cam.params, eye, w, h, good, torch.zeros((h, 3, w), device=dev).transpose(1, 2))
    with pytest.raises(RuntimeError, match="depth_normals: normal: expected a GPU tensor"):
        ops.depth_normals("pinhole", cam.params, eye, w, h, good, torch.zeros((h, w, 3)))
