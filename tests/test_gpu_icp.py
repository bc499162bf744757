"""GPU tests of pose tracking (csrc/pnr_icp.hip; include/pnr.h "pose tracking") against tests/_icp_ref.py: k_icp_accumulate's code and
residual are accumulate32's bit patterns between canaries, its sums are exact in count and within the any-order bound of math.fsum
(and equal the restatement of the kernel's own order), k_icp_solve equals the Python-float solve bit for bit, fusion.track equals
the restated track, a captured graph follows an edited depth image, and raycast -> track -> set_pose -> integrate closes the loop.
tests/test_icp_ref.py pins the restatement on the CPU."""
import math

import numpy as np
import pytest
import torch

import _icp_ref as ir
from panopticnerf_amd import FrameSet, Pinhole, camera, fusion, ops, synthetic

pytestmark = pytest.mark.gpu

GUARD = 64
MODELS = ("pinhole", "fisheye", "equirect")
TRUTH = np.asarray(ir.TRUE_POSE, np.float32)
GUESS = ir.perturbed(TRUTH, *ir.GUESS).astype(np.float32)
FAR_GUESS = ir.perturbed(TRUTH, (0.0, 0.35, 0.05), (0.12, -0.05, 0.1)).astype(np.float32)      # 20 degrees: many pixels leave, many are too far
DIST_MAX = 0.25


class Guarded:
    """an output array filled with junk, with GUARD canary elements before and after it, in one allocation"""

    def __init__(self, shape, dtype, dev):
        self.n = int(np.prod(shape))
        self.canary, junk = (-7.25e30, 3.5e12) if dtype.is_floating_point else (0xA5, 0x5A)
        self.buf = torch.full((self.n + 2 * GUARD,), self.canary, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(junk)

    def intact(self):
        return bool((self.buf[:GUARD] == self.canary).all()) and bool((self.buf[GUARD + self.n:] == self.canary).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def w2c_of(c2w):
    """the world-to-camera ops.icp_accumulate hands the kernel: the package's own invert_pose of the float32 pose"""
    return camera.invert_pose(torch.as_tensor(np.asarray(c2w, np.float32))).numpy()


def dirty(dl, dm, nm, seed):
    """edge values into copies of the maps: depths 0 / negative / NaN / Inf on both sides, model normals 0 / NaN"""
    dl, dm, nm = dl.copy(), dm.copy(), nm.copy()
    g = np.random.default_rng(seed)
    for img in (dl, dm):
        flat = img.reshape(-1)
        k = min(flat.size // 8, 32)
        flat[g.choice(flat.size, k, replace=False)] = np.resize(np.array([0.0, -1.5, np.nan, np.inf], np.float32), k)
    nflat = nm.reshape(-1, 3)
    k = min(nflat.shape[0] // 16, 16)
    nflat[g.choice(nflat.shape[0], k, replace=False)] = 0.0
    nflat[g.choice(nflat.shape[0], k, replace=False), g.integers(0, 3, k)] = np.nan
    return dl, dm, nm


def run_accumulate(dev, lcam, dl, pose, mcam, c2w_m, dm, nm, want=("code", "residual")):
    """ops.icp_accumulate on uploaded maps: (outputs as numpy, the workspace as numpy float64, every canary intact)"""
    h, w = lcam.height, lcam.width
    out = {"code": Guarded((h, w), torch.uint8, dev), "residual": Guarded((h, w), torch.float32, dev)}
    n_ws = ops.icp_workspace(w * h, dev).numel()
    ws = Guarded((n_ws,), torch.float64, dev)
    pose_d = Guarded((12,), torch.float32, dev)
    pose_d.t.copy_(torch.as_tensor(np.asarray(pose, np.float32).reshape(12)))
    ops.icp_accumulate(lcam.model, lcam.params, w, h, torch.as_tensor(dl).to(dev), pose_d.t, mcam.model, mcam.params, torch.as_tensor(np.asarray(c2w_m, np.float32)),
                       mcam.width, mcam.height, torch.as_tensor(dm).to(dev), torch.as_tensor(nm).to(dev), DIST_MAX, ws.t,
                       code=out["code"].t if "code" in want else None, residual=out["residual"].t if "residual" in want else None)
    torch.cuda.synchronize()
    assert np.array_equal(bits(pose_d.t.cpu().numpy()), bits(np.asarray(pose, np.float32).reshape(12))), "accumulate changed the pose"
    ok = all(g.intact() for g in list(out.values()) + [ws, pose_d])
    for k in out:
        if k not in want:
            junk = out[k].t.reshape(-1)[0].item()
            assert bool((out[k].t == junk).all()), "%s was written though it was not asked for" % k
    return {k: out[k].t.cpu().numpy().reshape(-1) for k in want}, ws.t.cpu().numpy(), ok


def check_against(ref, got, ws, n_pix, dev):
    """code / residual bits, the exact count, every sum within count 2^-53 sum |term| of math.fsum, and the rows in the kernel's order"""
    for k in got:
        assert np.array_equal(bits(got[k]), bits(ref[k])), "%s: %d of %d pixels differ" % (k, (got[k] != ref[k]).sum(), n_pix)
    grid = int(ws[:1].view(np.int64)[0])
    assert grid == ir.blocks_for(n_pix, cu_count(dev))
    rows = ws[1:1 + grid * ir.ROW].reshape(grid, ir.ROW)
    counts = np.ascontiguousarray(rows[:, ir.SUMS]).view(np.int64)
    T, idx = ir.terms(ref)
    assert int(counts.sum()) == idx.size
    total = rows[:, :ir.SUMS].sum(0)
    for k in range(ir.SUMS):
        exact = math.fsum(T[:, k])
        bound = idx.size * 2.0 ** -53 * math.fsum(np.abs(T[:, k]))
        assert abs(total[k] - exact) <= bound, (k, total[k], exact, bound)
    want_rows, want_counts = ir.rows_device(ref, n_pix, grid)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(bits(rows[:, :ir.SUMS]), bits(want_rows)), "the rows are not the sums in the kernel's stated order"


# ------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (64, 4), (65, 3), (70, 41), (512, 300)])
def test_accumulate_bits_at_every_size(dev, w, h):
    """live pinhole images from one pixel to three stride trips of the capped grid (512 x 300 = 153600 pixels > 2 x 256 x 256)
    against a 48 x 36 model view of the room; edge depths and normals mixed in; two runs give the same bits"""
    f = 0.6 * max(w, h) + 5.0
    lcam = Pinhole(f, f * 1.03, (w - 1) / 2.0, (h - 1) / 2.0, w, h)
    mcam = ir.cameras(0.75)["pinhole"]
    dl, _ = ir.room_maps(lcam, TRUTH)
    dm, nm = ir.room_maps(mcam, ir.MODEL_POSE)
    if w * h >= 64:
        dl, dm, nm = dirty(dl, dm, nm, w)
    ref = ir.accumulate32(ir.live_of(lcam), dl, GUESS, ir.model_of(mcam, ir.MODEL_POSE), dm, nm, DIST_MAX, w2c=w2c_of(ir.MODEL_POSE))
    got, ws, intact = run_accumulate(dev, lcam, dl, GUESS, mcam, ir.MODEL_POSE, dm, nm)
    assert intact
    check_against(ref, got, ws, w * h, dev)
    if w * h > 1:
        assert (ref["code"] == ir.MATCH).any()
    if w * h >= 2 * 256 * 256:
        assert int(ws[:1].view(np.int64)[0]) * 256 * 2 < w * h
    got2, ws2, _ = run_accumulate(dev, lcam, dl, GUESS, mcam, ir.MODEL_POSE, dm, nm)
    grid = int(ws[:1].view(np.int64)[0])
    assert np.array_equal(bits(ws[:1 + grid * ir.ROW]), bits(ws2[:1 + grid * ir.ROW])) and all(np.array_equal(bits(got[k]), bits(got2[k])) for k in got)


@pytest.mark.parametrize("pose_name", ["near", "far"])
@pytest.mark.parametrize("mn", MODELS)
@pytest.mark.parametrize("ln", MODELS)
def test_accumulate_bits_for_every_pairing(dev, ln, mn, pose_name):
    """3 x 3 camera models x 2 poses, the model view smaller than the live frame.  A fisheye frame keeps a positive depth outside
    its lens on either side (the pixel is refused by its ray, not by its depth); an equirect live frame looks behind a pinhole model
    camera; a full-circle equirect model view has its seam in the middle of what the live frame sees"""
    lcam, mcam = ir.cameras()[ln], ir.cameras(0.75)[mn]
    pose = GUESS if pose_name == "near" else FAR_GUESS
    dl, _ = ir.room_maps(lcam, TRUTH)
    dm, nm = ir.room_maps(mcam, ir.MODEL_POSE)
    dl, dm, nm = dirty(dl, dm, nm, 3)
    if ln == "fisheye":
        dl[0, 0] = dl[-1, -1] = 2.0
    if mn == "fisheye":
        hole = dm == 0
        dm[hole], nm[hole] = 2.0, (0.0, 0.0, -1.0)
    ref = ir.accumulate32(ir.live_of(lcam), dl, pose, ir.model_of(mcam, ir.MODEL_POSE), dm, nm, DIST_MAX, w2c=w2c_of(ir.MODEL_POSE))
    got, ws, intact = run_accumulate(dev, lcam, dl, pose, mcam, ir.MODEL_POSE, dm, nm)
    assert intact
    check_against(ref, got, ws, lcam.width * lcam.height, dev)
    seen = set(np.unique(ref["code"]).tolist())
    assert ir.MATCH in seen and ir.NO_DEPTH in seen
    if ln == "fisheye":
        assert ref["code"][0] == ir.NO_DEPTH and ref["code"][-1] == ir.NO_DEPTH
    if ln == "equirect" and mn == "pinhole":
        assert ir.OUTSIDE in seen
    if ln == "equirect" and mn == "equirect":
        u = ref["uv"][ref["inside"], 0]
        assert (u < 1.0).any() and (u > mcam.width - 2.0).any()                  # matches on both sides of the seam


def test_accumulate_optional_outputs(dev):
    """every optional output skipped in turn: what is asked for and the sums do not depend on what else is written"""
    lcam, mcam = ir.cameras()["fisheye"], ir.cameras(0.75)["equirect"]
    dl, _ = ir.room_maps(lcam, TRUTH)
    dm, nm = ir.room_maps(mcam, ir.MODEL_POSE)
    full, ws_full, intact = run_accumulate(dev, lcam, dl, GUESS, mcam, ir.MODEL_POSE, dm, nm)
    assert intact
    used = 1 + int(ws_full[:1].view(np.int64)[0]) * ir.ROW
    for want in (("code",), ("residual",), ()):
        got, ws, intact = run_accumulate(dev, lcam, dl, GUESS, mcam, ir.MODEL_POSE, dm, nm, want=want)
        assert intact and np.array_equal(bits(ws[:used]), bits(ws_full[:used]))
        for k in want:
            assert np.array_equal(bits(got[k]), bits(full[k]))


# ------------------------------------------------------------------------------------------------ solve
def _room_rows(n_rows):
    """the room's exact terms split over n_rows hand-written rows"""
    lcam, mcam = ir.cameras()["pinhole"], ir.cameras()["pinhole"]
    dl, _ = ir.room_maps(lcam, TRUTH)
    dm, nm = ir.room_maps(mcam, ir.MODEL_POSE)
    out = ir.accumulate32(ir.live_of(lcam), dl, GUESS, ir.model_of(mcam, ir.MODEL_POSE), dm, nm, DIST_MAX)
    T, idx = ir.terms(out)
    parts = np.array_split(np.arange(idx.size), n_rows)
    return np.stack([T[p].sum(0) for p in parts]), np.array([p.size for p in parts], np.int64)


def _wall_rows():
    cam = Pinhole(32.0, 32.0, 7.5, 5.5, 16, 12)
    eye = np.eye(4, dtype=np.float32)[:3]
    flat = np.full(16 * 12, 5.0, np.float32)
    nm = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (16 * 12, 1))
    pose = eye.copy()
    pose[2, 3] = 0.0625
    out = ir.accumulate32(ir.live_of(cam), flat, pose, ir.model_of(cam, eye), flat, nm, DIST_MAX)
    T, idx = ir.terms(out)
    return T.sum(0)[None], np.array([idx.size], np.int64), pose


def run_solve(dev, rows, counts, pose, n_pix, stored=None, extra_rows=0, **args):
    n_ws = ops.icp_workspace(n_pix, dev).numel() + extra_rows * ir.ROW
    host = np.full(n_ws, 1e300)                                  # junk behind the rows: never read
    host[:1].view(np.int64)[0] = rows.shape[0] if stored is None else stored
    body = np.zeros((rows.shape[0], ir.ROW))
    body[:, :ir.SUMS] = rows
    body[:, ir.SUMS:].view(np.int64)[:, 0] = counts
    host[1:1 + body.size] = body.reshape(-1)
    pose_d, hist = Guarded((12,), torch.float32, dev), Guarded((5,), torch.float64, dev)
    pose_d.t.copy_(torch.as_tensor(np.asarray(pose, np.float32).reshape(12)))
    ops.icp_solve(torch.as_tensor(host).to(dev), n_pix, pose_d.t, hist.t, **args)
    torch.cuda.synchronize()
    assert pose_d.intact() and hist.intact()
    return pose_d.t.cpu().numpy(), hist.t.cpu().numpy()


SOLVE_CASES = {
    "ok": (dict(), ir.OK), "ok_one_row": (dict(), ir.OK), "too_few": (dict(min_matches=10 ** 6), ir.TOO_FEW),
    "degenerate": (dict(), ir.DEGENERATE), "rot_too_large": (dict(max_rot=1e-3), ir.STEP_TOO_LARGE),
    "trans_too_large": (dict(max_trans=1e-3), ir.STEP_TOO_LARGE), "no_update": (dict(update=False), ir.OK),
    "no_update_too_few": (dict(update=False, min_matches=10 ** 6), ir.TOO_FEW),
}


@pytest.mark.parametrize("case", sorted(SOLVE_CASES))
def test_solve_equals_the_restatement_bit_for_bit(dev, case):
    """hand-written partial rows reach every status; the pose and the history row are _icp_ref.solve's bits: every operation of
    the kernel is an IEEE double + - x / sqrt in the header's order"""
    args, status = SOLVE_CASES[case]
    if case == "degenerate":
        rows, counts, pose = _wall_rows()
    else:
        rows, counts = _room_rows(1 if case == "ok_one_row" else 5)
        pose = GUESS
    n_pix = 64 * 48
    got_pose, got_row = run_solve(dev, rows, counts, pose, n_pix, **args)
    tot, count = ir.combine(rows, counts)
    want_pose, want_row = ir.solve(tot, count, pose, **args)
    assert want_row[4] == status
    assert np.array_equal(bits(got_row), bits(np.array(want_row))), (got_row, want_row)
    assert np.array_equal(bits(got_pose), bits(want_pose))
    changed = not np.array_equal(bits(got_pose), bits(np.asarray(pose, np.float32).reshape(12)))
    assert changed == (status == ir.OK and args.get("update", True))


def test_solve_never_reads_past_the_workspace(dev):
    """slot 0 is device memory the kernel cannot trust: a stored row count beyond what n_pix allows is cut to that.  The stored count
    is two rows more than the workspace of n_pix holds, and the tensor is allocated those two rows larger, filled with junk that
    would change every sum: a lost clamp shows as a wrong result, never as a read outside the allocation"""
    rows, counts = _room_rows(3)
    n_pix = 2 * 256                                               # the workspace of 512 pixels holds 2 rows
    got_pose, got_row = run_solve(dev, rows[:2], counts[:2], GUESS, n_pix, stored=4, extra_rows=2)
    want_pose, want_row = ir.solve(*ir.combine(rows[:2], counts[:2]), GUESS)
    assert np.array_equal(bits(got_row), bits(np.array(want_row))) and np.array_equal(bits(got_pose), bits(want_pose))


def test_ops_refuse_non_contiguous_device_tensors(dev):
    """the kernels index the images flat: a transposed view of the right shape is refused by name, on real device tensors"""
    cam = ir.cameras()["pinhole"]
    h, w = cam.height, cam.width
    eye = torch.eye(4)[:3]
    good = dict(depth=torch.ones((h, w), device=dev), pose12=torch.zeros(12, device=dev), model_depth=torch.ones((h, w), device=dev),
                model_normal=torch.zeros((h, w, 3), device=dev), workspace=ops.icp_workspace(w * h, dev))
    call = lambda **kw: ops.icp_accumulate("pinhole", cam.params, w, h, kw["depth"], kw["pose12"], "pinhole", cam.params, eye, w, h, kw["model_depth"],
                                           kw["model_normal"], DIST_MAX, kw["workspace"], code=kw.get("code"), residual=kw.get("residual"))
    for name, bad in (("depth", torch.ones((w, h), device=dev).t()), ("model_depth", torch.ones((w, h), device=dev).t()),
                      ("model_normal", torch.zeros((h, 3, w), device=dev).transpose(1, 2)), ("pose12", torch.zeros(24, device=dev)[::2]),
                      ("code", torch.zeros((w, h), dtype=torch.uint8, device=dev).t()), ("residual", torch.zeros((w, h), device=dev).t())):
        with pytest.raises(ValueError, match="icp_accumulate: %s: tensor must be contiguous" % name):
            call(**dict(good, **{name: bad}))
    with pytest.raises(RuntimeError, match="icp_accumulate: model_depth: expected a GPU tensor"):
        call(**dict(good, model_depth=torch.ones((h, w))))
    hist = torch.zeros(10, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="icp_solve: history_row: tensor must be contiguous"):
        ops.icp_solve(good["workspace"], w * h, good["pose12"], hist[::2])
    with pytest.raises(ValueError, match=r"history_row must be \(5,\)"):
        ops.icp_solve(good["workspace"], w * h, good["pose12"], hist[:6])
    with pytest.raises(ValueError, match="fusion.track: depth must be contiguous"):
        fusion.track((cam, eye, {"depth": good["model_depth"], "normal": good["model_normal"]}), cam, torch.ones((w, h), device=dev).t(), eye)
    with pytest.raises(ValueError, match="fusion.track: max_rot must lie in"):
        fusion.track((cam, eye, {"depth": good["model_depth"], "normal": good["model_normal"]}), cam, good["depth"], eye, max_rot=0.75)


# ------------------------------------------------------------------------------------------------ fusion.track
def _track_scene(dev, ln="pinhole", mn="pinhole"):
    lcam, mcam = ir.cameras()[ln], ir.cameras(0.75)[mn]
    dl, _ = ir.room_maps(lcam, TRUTH)
    dm, nm = ir.room_maps(mcam, ir.MODEL_POSE)
    view = (mcam, torch.as_tensor(np.asarray(ir.MODEL_POSE, np.float32)), {"depth": torch.as_tensor(dm).to(dev), "normal": torch.as_tensor(nm).to(dev)})
    return lcam, mcam, dl, dm, nm, view


SOLVE_ARGS = dict(min_matches=64, max_rot=0.25, max_trans=0.5)


@pytest.mark.parametrize("ln,mn", [("pinhole", "pinhole"), ("fisheye", "equirect"), ("equirect", "fisheye")])
def test_track_equals_the_restatement(dev, ln, mn):
    """fusion.track on the room with analytic model maps, 10 iterations: history row 0 equals the restatement fed the same inputs
    (count, E, |omega|^2, |v|^2, status, bit for bit, the sums taken in the kernel's order), the final pose lies within the CPU
    test's bound of the truth (4 x the float64 restatement's own error + 1e-5) -- and, every operation being pinned, the whole
    history, the final pose and the maps equal the restated track"""
    lcam, mcam, dl, dm, nm, view = _track_scene(dev, ln, mn)
    c2w, info = fusion.track(view, lcam, torch.as_tensor(dl).to(dev), torch.as_tensor(GUESS.reshape(3, 4)), iters=10, dist_max=DIST_MAX, **SOLVE_ARGS)
    torch.cuda.synchronize()
    assert tuple(c2w.shape) == (3, 4) and c2w.dtype == torch.float32 and c2w.is_cuda
    assert tuple(info["history"].shape) == (11, 5) and info["history"].dtype == torch.float64
    grid = ir.blocks_for(lcam.width * lcam.height, cu_count(dev))
    live, model = ir.live_of(lcam), ir.model_of(mcam, ir.MODEL_POSE)
    pose, hist, out, _ = ir.track(live, dl, GUESS, model, dm, nm, 10, DIST_MAX, grid=grid, w2c=w2c_of(ir.MODEL_POSE), **SOLVE_ARGS)
    got_hist, got_pose = info["history"].cpu().numpy(), c2w.cpu().numpy().reshape(12)
    assert np.array_equal(bits(got_hist[0]), bits(hist[0])), (got_hist[0], hist[0])
    p64, _, _, _ = ir.track(live, dl, GUESS, model, dm, nm, 10, DIST_MAX, f=np.float64, w2c=w2c_of(ir.MODEL_POSE), **SOLVE_ARGS)
    e, e64 = ir.pose_error(got_pose, TRUTH), ir.pose_error(p64, TRUTH)
    print("%s -> %s: final error %s, the float64 restatement's %s" % (ln, mn, e, e64))
    assert e[0] <= 4.0 * e64[0] + 1e-5 and e[1] <= 4.0 * e64[1] + 1e-5
    assert np.array_equal(bits(got_hist), bits(hist))
    assert np.array_equal(bits(got_pose), bits(pose))
    assert np.array_equal(info["code"].cpu().numpy().reshape(-1), out["code"])
    assert np.array_equal(bits(info["residual"].cpu().numpy().reshape(-1)), bits(out["residual"]))
    assert torch.equal(info["valid"], info["code"] == fusion.MATCH)
    # maps=False: the same pose, no images; iters=0: the guess comes back with one history row
    c2w2, info2 = fusion.track(view, lcam, torch.as_tensor(dl).to(dev), torch.as_tensor(GUESS.reshape(3, 4)).to(dev), iters=10, dist_max=DIST_MAX, maps=False, **SOLVE_ARGS)
    assert torch.equal(c2w2, c2w) and sorted(info2) == ["history"]
    c2w0, info0 = fusion.track(view, lcam, torch.as_tensor(dl).to(dev), GUESS.reshape(3, 4), iters=0, dist_max=DIST_MAX, **SOLVE_ARGS)
    assert np.array_equal(bits(c2w0.cpu().numpy().reshape(12)), bits(GUESS.reshape(12))) and np.array_equal(bits(info0["history"].cpu().numpy()[0]), bits(hist[0] * [1, 1, 0, 0, 1]))


def test_track_in_a_graph_follows_the_depth_image(dev):
    """a captured track replayed after the depth image was edited equals the eager call on the edited image"""
    lcam, mcam, dl, dm, nm, view = _track_scene(dev)
    other = ir.perturbed(TRUTH, (0.01, 0.02, -0.01), (-0.03, 0.01, 0.02)).astype(np.float32)
    dl2, _ = ir.room_maps(lcam, other)
    depth = torch.as_tensor(dl).to(dev)
    guess = torch.as_tensor(GUESS.reshape(3, 4)).to(dev)
    run = lambda: fusion.track(view, lcam, depth, guess, iters=4, dist_max=DIST_MAX, **SOLVE_ARGS)
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c2w_g, info_g = run()
    graph.replay()
    torch.cuda.synchronize()
    first = c2w_g.clone()
    depth.copy_(torch.as_tensor(dl2).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    c2w_e, info_e = run()
    torch.cuda.synchronize()
    assert not torch.equal(first, c2w_g)
    assert torch.equal(c2w_g.view(torch.int32), c2w_e.view(torch.int32))
    assert torch.equal(info_g["history"].view(torch.int64), info_e["history"].view(torch.int64))
    assert torch.equal(info_g["code"], info_e["code"]) and torch.equal(info_g["residual"].view(torch.int32), info_e["residual"].view(torch.int32))
    assert torch.equal(guess.cpu(), torch.as_tensor(GUESS.reshape(3, 4)))


# ------------------------------------------------------------------------------------------------ the loop
def test_raycast_track_set_pose_integrate_loop(dev):
    """eight 64 x 48 pinhole frames of the room into a 48^3 lattice: integrate the first, then for every next frame raycast from the
    previous pose, track from it, set_pose, integrate.  Every tracked pose lies within 2 x the float64 restatement's error on the
    GPU's own ray-cast maps + 1/8 of the lattice cell's diagonal of the truth (an angle counted at an arm of one unit: no surface
    is nearer); integrate after set_pose equals integrate of a set built with the tracked poses"""
    cam = ir.cameras()["pinhole"]
    h, w = cam.height, cam.width
    lo, hi = tuple(v - 0.3 for v in ir.ROOM[0]), tuple(v + 0.3 for v in ir.ROOM[1])
    vol = fusion.Volume(lo, hi, 48, dev)
    diag = float(np.linalg.norm(np.asarray(vol.step, np.float64)))
    trunc = 0.45
    truths = [ir.perturbed(TRUTH, (0.004 * f, -0.012 * f, 0.002 * f), (0.025 * f, -0.01 * f, 0.02 * f)).astype(np.float32) for f in range(8)]
    depths = [ir.room_maps(cam, t)[0] for t in truths]
    frames = FrameSet(dev, capacity=8)
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8)
    for f in range(8):
        frames.add(cam, torch.as_tensor(truths[0]), 0.1, 10.0, rgb, depth=torch.as_tensor(depths[f]))     # every pose but the first is a placeholder
    frames.w2c_table()
    fusion.integrate(vol, frames, trunc, first=0, last=1)
    prev = torch.as_tensor(truths[0].reshape(3, 4))
    tracked = [prev.clone()]
    for f in range(1, 8):
        maps = fusion.raycast(vol, cam, prev, 0.1, 10.0, attributes=False)
        c2w, info = fusion.track((cam, prev, maps), cam, frames.frames[f]["depth"], prev, iters=10, dist_max=DIST_MAX, **SOLVE_ARGS)
        pose = c2w.cpu()
        hist = info["history"].cpu().numpy()
        assert np.all(hist[:, 4] == fusion.ICP_OK), hist
        dm, nm = maps["depth"].cpu().numpy(), maps["normal"].cpu().numpy()
        p64, _, _, _ = ir.track(ir.live_of(cam), depths[f], prev.numpy(), ir.model_of(cam, prev.numpy()), dm, nm, 10, DIST_MAX, f=np.float64,
                                w2c=w2c_of(prev.numpy()), **SOLVE_ARGS)
        e, e64 = ir.pose_error(pose.numpy(), truths[f]), ir.pose_error(p64, truths[f])
        print("frame %d: %d matches, error %s, the float64 restatement's %s, bound + %.4f" % (f, hist[-1, 0], e, e64, diag / 8))
        assert e[0] <= 2.0 * e64[0] + diag / 8 and e[1] <= 2.0 * e64[1] + diag / 8
        frames.set_pose(f, pose)
        assert torch.equal(frames.frames[f]["c2w"], pose) and torch.equal(frames.w2c_table()[f].cpu(), camera.invert_pose(pose).reshape(12))
        fusion.integrate(vol, frames, trunc, first=f, last=f + 1)
        prev = pose
        tracked.append(pose.clone())
    torch.cuda.synchronize()
    again = FrameSet(dev, capacity=8)
    for f in range(8):
        again.add(cam, tracked[f], 0.1, 10.0, rgb, depth=torch.as_tensor(depths[f]))
    vol2 = fusion.Volume(lo, hi, 48, dev)
    fusion.integrate(vol2, again, trunc)
    assert torch.equal(frames.table.cpu(), _same_images(again, frames).cpu())
    assert torch.equal(vol.tsdf.view(torch.int32), vol2.tsdf.view(torch.int32)) and torch.equal(vol.weight, vol2.weight)
    assert float((vol.weight > 1).float().mean()) > 0.01                       # the frames did overlap


def _same_images(built, tracked):
    """built's table with the image addresses of `tracked`: the records must agree in everything else, the poses included"""
    import ctypes
    from panopticnerf_amd import _lib
    rec = ctypes.sizeof(_lib.Frame)
    t, ref = built.table.cpu().clone(), tracked.table.cpu()
    for f in range(len(built)):
        for name in ("valid_pix", "rgb", "depth", "sem", "inst"):
            off = f * rec + getattr(_lib.Frame, name).offset
            t[off:off + 8] = ref[off:off + 8]
    return t
