"""CPU tests of pose tracking's boundary (include/pnr.h "pose tracking"): every PNR_EINVAL of the three entry points comes before
any launch, every refusal of ops.icp_accumulate / ops.icp_solve / fusion.track / FrameSet.set_pose by its message, the codes
against the header, and synthetic.room_depth's closed forms.  Nothing here touches a GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from panopticnerf_amd import Equirect, Fisheye, FrameSet, Pinhole, _lib, fusion, ops, synthetic

import _icp_ref as ir
from _fake_gpu import _FakeCuda, _fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(64)          # ONE: non-null, aligned, never dereferenced -- validation fails first
F4 = lambda *v: (ctypes.c_float * len(v))(*v)
PIN, EYE = F4(50.0, 50.0, 8.0, 6.0), F4(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def _header(name):
    src = open(os.path.join(ROOT, "include", "pnr.h")).read()
    m = re.search(r"#define\s+%s\s+(\S+)" % name, src)
    assert m, name
    return m.group(1)


def test_codes_and_constants_mirror_the_header():
    for name, value in ir.CODES.items():
        assert int(_header("PNR_ICP_" + name)) == value == getattr(ops, "ICP_" + name) == getattr(fusion, name)
    for name, value in ir.STATUS.items():
        assert int(_header("PNR_ICP_" + name)) == value == getattr(ops, "ICP_" + name) == getattr(fusion, "ICP_" + name)
    assert sorted(ir.CODES.values()) == list(range(6)) and sorted(ir.STATUS.values()) == list(range(4))
    assert int(_header("PNR_ICP_SUMS")) == ir.SUMS and int(_header("PNR_ICP_ROW")) == ir.ROW
    assert int(_header("PNR_ICP_MAX_BLOCKS")) == ir.MAX_BLOCKS and int(_header("PNR_ICP_SERIES_TERMS")) == ir.SERIES_TERMS
    assert float(_header("PNR_ICP_MAX_ROT").rstrip("f")) == ir.MAX_ROT == ops.ICP_MAX_ROT


def test_workspace_bytes():
    ws = _lib.load().pnr_icp_workspace_bytes
    assert ws(0) == -1 and ws(-5) == -1 and ws(2 ** 31) == -1
    assert ws(1) == (1 + ir.ROW) * 8 and ws(256) == (1 + ir.ROW) * 8 and ws(257) == (1 + 2 * ir.ROW) * 8
    assert ws(256 * ir.MAX_BLOCKS) == ws(2 ** 31 - 1) == (1 + ir.MAX_BLOCKS * ir.ROW) * 8
    for n in (1, 255, 256, 257, 70 * 41, 1408 * 376):
        assert ws(n) == (1 + ir.blocks_for(n) * ir.ROW) * 8


def _accumulate(**over):
    a = dict(model_l=0, cam_l=PIN, width_l=16, height_l=12, depth_l=ONE, pose12=ONE, model_m=0, cam_m=PIN, c2w_m=EYE, w2c_m=EYE, width_m=16,
             height_m=12, depth_m=ONE, normal_m=ONE, dist_max=0.25, workspace=ONE, code=NULL, residual=NULL, stream=NULL)
    a.update(over)
    lib = _lib.load()
    rc = lib.pnr_icp_accumulate(*a.values())
    return rc, lib.pnr_last_error()


@pytest.mark.parametrize("over,message", [
    (dict(model_l=2), b"unknown camera model"), (dict(model_m=7), b"unknown camera model"),
    (dict(cam_l=None), b"null camera"), (dict(cam_m=None), b"null camera"), (dict(c2w_m=None), b"null camera or model pose"),
    (dict(w2c_m=None), b"null camera or model pose"),
    (dict(width_l=0), b"bad size"), (dict(height_l=-1), b"bad size"), (dict(width_m=0), b"bad size"), (dict(height_m=0), b"bad size"),
    (dict(width_l=65536, height_l=32768), b"bad size"), (dict(width_m=65536, height_m=32768), b"bad size"),
    (dict(cam_l=F4(0.0, 50.0, 8.0, 6.0)), b"live: zero focal"), (dict(cam_m=F4(50.0, 0.0, 8.0, 6.0)), b"model: zero focal"),
    (dict(model_l=1, cam_l=F4(2.2, 0.0, 1.6, 0.0, 60.0, 8.0, 8.0)), b"live: zero focal length or gamma"),
    (dict(model_m=3, cam_m=F4(-1.0, 0.5, -0.5, 0.1)), b"model: equirect"),
    (dict(depth_l=NULL), b"null depth_l"), (dict(pose12=NULL), b"null depth_l, pose12"), (dict(depth_m=NULL), b"null"),
    (dict(normal_m=NULL), b"null"), (dict(workspace=NULL), b"null"),
    (dict(depth_l=ctypes.c_void_p(66)), b"4-byte aligned"), (dict(pose12=ctypes.c_void_p(65)), b"4-byte aligned"),
    (dict(depth_m=ctypes.c_void_p(67)), b"4-byte aligned"), (dict(normal_m=ctypes.c_void_p(66)), b"4-byte aligned"),
    (dict(residual=ctypes.c_void_p(66)), b"4-byte aligned"), (dict(workspace=ctypes.c_void_p(68)), b"8-byte aligned"),
    (dict(dist_max=0.0), b"dist_max"), (dict(dist_max=-1.0), b"dist_max"), (dict(dist_max=float("nan")), b"dist_max"),
    (dict(dist_max=float("inf")), b"dist_max"), (dict(dist_max=1e20), b"dist_max"),
])
def test_accumulate_einval_before_any_launch(over, message):
    rc, err = _accumulate(**over)
    assert rc == -1 and message in err, err


def _solve(**over):
    a = dict(workspace=ONE, n_pix=192, min_matches=6, max_rot=0.25, max_trans=0.5, update=1, pose12=ONE, history=ONE, stream=NULL)
    a.update(over)
    lib = _lib.load()
    rc = lib.pnr_icp_solve(*a.values())
    return rc, lib.pnr_last_error()


@pytest.mark.parametrize("over,message", [
    (dict(workspace=NULL), b"null workspace"), (dict(pose12=NULL), b"null workspace, pose12"), (dict(history=NULL), b"null"),
    (dict(workspace=ctypes.c_void_p(68)), b"8-byte aligned"), (dict(history=ctypes.c_void_p(68)), b"8-byte aligned"),
    (dict(pose12=ctypes.c_void_p(66)), b"pose12 4-byte"),
    (dict(n_pix=0), b"bad size"), (dict(n_pix=2 ** 31), b"bad size"), (dict(min_matches=0), b"min_matches"),
    (dict(max_rot=0.0), b"max_rot"), (dict(max_rot=0.5000001), b"max_rot"), (dict(max_rot=float("nan")), b"max_rot"),
    (dict(max_trans=0.0), b"max_trans"), (dict(max_trans=float("nan")), b"max_trans"),
])
def test_solve_einval_before_any_launch(over, message):
    rc, err = _solve(**over)
    assert rc == -1 and message in err, err


# ------------------------------------------------------------------------------------------------ the ops
def _acc_args(**over):
    a = dict(camera_model="pinhole", cam=(50.0, 50.0, 8.0, 6.0), width=16, height=12, depth=torch.zeros(12, 16), pose12=torch.zeros(12),
             model_camera_model="pinhole", model_cam=(50.0, 50.0, 8.0, 6.0), model_c2w=torch.eye(4)[:3], model_width=16, model_height=12,
             model_depth=torch.zeros(12, 16), model_normal=torch.zeros(12, 16, 3), dist_max=0.25,
             workspace=torch.zeros(1 + ir.ROW, dtype=torch.float64))
    a.update(over)
    return a


@pytest.mark.parametrize("over,exc,message", [
    (dict(camera_model="orthographic"), ValueError, "camera_model must be 'pinhole', 'fisheye' or 'equirect'"),
    (dict(model_camera_model=3), ValueError, "model_camera_model must be"),
    (dict(cam=(1.0, 2.0)), ValueError, "expected 4 values, got 2"),
    (dict(model_camera_model="fisheye"), ValueError, "expected 7 values, got 4"),
    (dict(model_c2w=torch.eye(3)), ValueError, "model_c2w: expected 12 values"),
    (dict(width=0), ValueError, "bad size of the live image"), (dict(model_height=0), ValueError, "bad size of the model image"),
    (dict(depth=None), ValueError, "depth must be a GPU tensor"), (dict(depth=torch.zeros(12, 16, dtype=torch.float64)), TypeError, "depth must be torch.float32"),
    (dict(depth=torch.zeros(16, 12)), ValueError, r"depth must be \(12, 16\)"),
    (dict(model_depth=torch.zeros(12, 15)), ValueError, r"model_depth must be \(12, 16\)"),
    (dict(model_normal=torch.zeros(12, 16)), ValueError, r"model_normal must be \(12, 16, 3\)"),
    (dict(model_normal=None), ValueError, "model_normal must be a GPU tensor"),
    (dict(code=torch.zeros(12, 16)), TypeError, "code must be torch.uint8"),
    (dict(residual=torch.zeros(12, 17)), ValueError, r"residual must be \(12, 16\)"),
    (dict(dist_max=0.0), ValueError, "dist_max must be positive"), (dict(dist_max=float("inf")), ValueError, "dist_max must be positive"),
    (dict(pose12=[0.0] * 12), ValueError, "pose12 must be a GPU tensor of 12 float32"),
    (dict(), RuntimeError, "pose12: expected a GPU tensor \\(the HIP path has no CPU fallback\\)"),
])
def test_icp_accumulate_refusals(over, exc, message):
    with pytest.raises(exc, match=message):
        ops.icp_accumulate(**_acc_args(**over))


def _solve_args(**over):
    a = dict(workspace=torch.zeros(1 + ir.ROW, dtype=torch.float64), n_pix=192, pose12=torch.zeros(12), history_row=torch.zeros(5, dtype=torch.float64))
    a.update(over)
    return a


@pytest.mark.parametrize("over,exc,message", [
    (dict(n_pix=0), ValueError, "n_pix must lie in"), (dict(min_matches=0), ValueError, "min_matches must be >= 1"),
    (dict(max_rot=0.6), ValueError, r"max_rot must lie in \(0, 0.5\]"), (dict(max_rot=0.0), ValueError, "max_rot must lie in"),
    (dict(max_trans=-1.0), ValueError, "max_trans must be positive"),
    (dict(pose12=None), ValueError, "pose12 must be a GPU tensor of 12 float32"),
    (dict(), RuntimeError, "pose12: expected a GPU tensor \\(the HIP path has no CPU fallback\\)"),
])
def test_icp_solve_refusals(over, exc, message):
    with pytest.raises(exc, match=message):
        ops.icp_solve(**_solve_args(**over))


def _fake_acc(**over):
    """icp_accumulate's arguments with every tensor saying it is on the GPU, so that the checks behind the device check are reached;
    every case must still be refused before the entry point is called"""
    a = _acc_args()
    for k, v in a.items():
        if isinstance(v, torch.Tensor) and k != "model_c2w":
            a[k] = _fake(v)
    a.update(over)
    return a


@pytest.mark.parametrize("over,exc,message", [
    (dict(depth=_fake(torch.zeros(16, 12).t())), ValueError, "icp_accumulate: depth: tensor must be contiguous"),
    (dict(model_depth=_fake(torch.zeros(16, 12).t())), ValueError, "icp_accumulate: model_depth: tensor must be contiguous"),
    (dict(model_normal=_fake(torch.zeros(12, 3, 16).transpose(1, 2))), ValueError, "icp_accumulate: model_normal: tensor must be contiguous"),
    (dict(code=_fake(torch.zeros(16, 12, dtype=torch.uint8).t())), ValueError, "icp_accumulate: code: tensor must be contiguous"),
    (dict(residual=_fake(torch.zeros(16, 12).t())), ValueError, "icp_accumulate: residual: tensor must be contiguous"),
    (dict(pose12=_fake(torch.zeros(24)[::2])), ValueError, "icp_accumulate: pose12: tensor must be contiguous"),
    (dict(workspace=_fake(torch.zeros(2 * (1 + ir.ROW), dtype=torch.float64)[::2])), ValueError, "icp_accumulate: workspace: tensor must be contiguous"),
    (dict(code=[0] * 192), ValueError, "code must be a GPU tensor, got list"),
    (dict(residual=np.zeros((12, 16), np.float32)), ValueError, "residual must be a GPU tensor, got ndarray"),
    (dict(model_depth=_fake(torch.zeros(12, 16), "cuda:1")), ValueError, "icp_accumulate: model_depth is on cuda:1, not on cpu"),
    (dict(residual=_fake(torch.zeros(12, 16), "cuda:1")), ValueError, "icp_accumulate: residual is on cuda:1, not on cpu"),
    (dict(depth=torch.zeros(12, 16)), RuntimeError, "icp_accumulate: depth: expected a GPU tensor"),
])
def test_icp_accumulate_refusals_behind_the_device_check(over, exc, message):
    """contiguity (the kernel indexes the images flat: a transposed view of the right shape is stopped only here), tensors on
    different devices, non-tensor optional outputs, and a CPU image among GPU ones"""
    with pytest.raises(exc, match=message):
        ops.icp_accumulate.__wrapped__(**_fake_acc(**over))          # (behind _on_device, which would ask the runtime for the current device)


def _fake_solve(**over):
    a = {k: _fake(v) if isinstance(v, torch.Tensor) else v for k, v in _solve_args().items()}
    a.update(over)
    return a


@pytest.mark.parametrize("over,exc,message", [
    (dict(history_row=None), ValueError, "history_row must be a GPU tensor of 5 float64, got NoneType"),
    (dict(history_row=_fake(torch.zeros(5))), TypeError, "icp_solve: history_row: expected torch.float64"),
    (dict(history_row=_fake(torch.zeros(6, dtype=torch.float64))), ValueError, r"history_row must be \(5,\), got \(6,\)"),
    (dict(history_row=_fake(torch.zeros(1, 5, dtype=torch.float64))), ValueError, r"history_row must be \(5,\), got \(1, 5\)"),
    (dict(history_row=_fake(torch.zeros(10, dtype=torch.float64)[::2])), ValueError, "icp_solve: history_row: tensor must be contiguous"),
    (dict(history_row=torch.zeros(5, dtype=torch.float64)), RuntimeError, "icp_solve: history_row: expected a GPU tensor"),
    (dict(pose12=_fake(torch.zeros(24)[::2])), ValueError, "icp_solve: pose12: tensor must be contiguous"),
    (dict(workspace=_fake(torch.zeros(2 * (1 + ir.ROW), dtype=torch.float64)[::2])), ValueError, "icp_solve: workspace: tensor must be contiguous"),
    (dict(workspace=_fake(torch.zeros(ir.ROW, dtype=torch.float64))), ValueError, "workspace must be a flat float64 tensor of at least 30 elements"),
    (dict(history_row=_fake(torch.zeros(5, dtype=torch.float64), "cuda:1")), ValueError, "icp_solve: history_row is on cuda:1, not on cpu"),
    (dict(pose12=_fake(torch.zeros(12), "cuda:1")), ValueError, "icp_solve: pose12 is on cuda:1, not on cpu"),
])
def test_icp_solve_refusals_behind_the_device_check(over, exc, message):
    with pytest.raises(exc, match=message):
        ops.icp_solve.__wrapped__(**_fake_solve(**over))


def test_icp_ops_check_the_gpu_side_arguments_by_name():
    """the two helpers behind the device check, called on their own (the ops' refusals that go through them are provoked above,
    and test_gpu_icp.py repeats contiguity on real device tensors)"""
    with pytest.raises(ValueError, match="pose12 must hold 12 values"):
        ops._icp_pose(_FakeCuda(torch.zeros(11)), "icp_solve")
    with pytest.raises(TypeError, match="pose12: expected torch.float32"):
        ops._icp_pose(_FakeCuda(torch.zeros(12, dtype=torch.float64)), "icp_solve")
    with pytest.raises(ValueError, match="workspace must be a flat float64 tensor of at least 59 elements"):
        ops._icp_workspace(_FakeCuda(torch.zeros(30, dtype=torch.float64)), 300, "icp_solve")
    with pytest.raises(TypeError, match="workspace: expected torch.float64"):
        ops._icp_workspace(_FakeCuda(torch.zeros(64)), 300, "icp_solve")
    with pytest.raises(ValueError, match="workspace must be a GPU tensor"):
        ops._icp_workspace(None, 300, "icp_solve")


# ------------------------------------------------------------------------------------------------ fusion.track, FrameSet.set_pose
def test_track_refusals():
    cam = Pinhole(50.0, 50.0, 8.0, 6.0, 16, 12)
    eye = torch.eye(4)[:3]
    maps = {"depth": torch.zeros(12, 16), "normal": torch.zeros(12, 16, 3)}
    depth = torch.zeros(12, 16)
    with pytest.raises(TypeError, match="model_view must be \\(camera, c2w, maps\\)"):
        fusion.track(None, cam, depth, eye)
    with pytest.raises(TypeError, match="the model view's camera must be"):
        fusion.track(("pinhole", eye, maps), cam, depth, eye)
    with pytest.raises(TypeError, match="camera must be a camera.Pinhole"):
        fusion.track((cam, eye, maps), (50.0, 50.0, 8.0, 6.0), depth, eye)
    with pytest.raises(ValueError, match="maps need 'depth'"):
        fusion.track((cam, eye, {"normal": maps["normal"]}), cam, depth, eye)
    with pytest.raises(ValueError, match="maps need 'normal' \\(fusion.raycast with normals=True\\)"):
        fusion.track((cam, eye, {"depth": maps["depth"]}), cam, depth, eye)
    with pytest.raises(ValueError, match="iters must be >= 0"):
        fusion.track((cam, eye, maps), cam, depth, eye, iters=-1)
    for kw, message in ((dict(dist_max=0.0), "dist_max must be positive"), (dict(dist_max=float("inf")), "dist_max must be positive"),
                        (dict(min_matches=0), "min_matches must be >= 1"), (dict(max_rot=0.6), r"max_rot must lie in \(0, 0.5\]"),
                        (dict(max_rot=float("nan")), "max_rot must lie in"), (dict(max_trans=0.0), "max_trans must be positive")):
        with pytest.raises(ValueError, match="fusion.track: " + message):          # before anything is allocated or launched
            fusion.track((cam, eye, maps), cam, _FakeCuda(depth), eye, **kw)
    with pytest.raises(ValueError, match="the model view's c2w must be a 3x4"):
        fusion.track((cam, torch.eye(3), maps), cam, depth, eye)
    with pytest.raises(TypeError, match="depth must be a GPU tensor"):
        fusion.track((cam, eye, maps), cam, depth.numpy(), eye)
    with pytest.raises(ValueError, match=r"depth must be a float32 tensor of shape \(12, 16\), got torch.float32 \(16, 12\)"):
        fusion.track((cam, eye, maps), cam, _FakeCuda(torch.zeros(16, 12)), eye)
    with pytest.raises(ValueError, match="depth must be contiguous"):
        fusion.track((cam, eye, maps), cam, _FakeCuda(torch.zeros(16, 12).t()), eye)
    with pytest.raises(ValueError, match=r"the model view's depth must be a float32 tensor of shape \(12, 16\), got torch.float64"):
        fusion.track((cam, eye, {"depth": maps["depth"].double(), "normal": maps["normal"]}), cam, _FakeCuda(depth), eye)
    with pytest.raises(ValueError, match=r"the model view's normal must be a float32 tensor of shape \(12, 16, 3\)"):
        fusion.track((cam, eye, {"depth": maps["depth"], "normal": torch.zeros(12, 16)}), cam, _FakeCuda(depth), eye)
    with pytest.raises(ValueError, match="the model view's depth is on cpu, depth on cuda:1"):
        fusion.track((cam, eye, maps), cam, _FakeCuda(depth, "cuda:1"), eye)
    with pytest.raises(RuntimeError, match="depth is not on the GPU \\(the HIP path has no CPU fallback\\)"):
        fusion.track((cam, eye, maps), cam, depth, eye)
    with pytest.raises(ValueError, match="c2w must be a 3x4 \\(or 4x4\\) matrix"):
        fusion.track((cam, eye, maps), cam, _FakeCuda(depth), torch.eye(3))


def test_set_pose_refusals():
    frames = FrameSet("cuda", capacity=2)
    with pytest.raises(IndexError, match="frame 0 of a set of 0"):
        frames.set_pose(0, torch.eye(4))
    frames.frames.append({"c2w": torch.eye(4)[:3].clone()})          # a host record alone: every refusal comes before the device
    with pytest.raises(IndexError, match="frame 1 of a set of 1"):
        frames.set_pose(1, torch.eye(4))
    with pytest.raises(IndexError, match="frame -1"):
        frames.set_pose(-1, torch.eye(4))
    with pytest.raises(TypeError, match="i must be a frame index"):
        frames.set_pose("first", torch.eye(4))
    with pytest.raises(ValueError, match="c2w must be a 3x4 \\(or 4x4\\) matrix"):
        frames.set_pose(0, torch.eye(3))
    bad = torch.eye(4)
    bad[0, 3] = float("nan")
    with pytest.raises(ValueError, match="c2w must be finite"):
        frames.set_pose(0, bad)
    with pytest.raises(TypeError, match="c2w must be host values"):
        frames.set_pose(0, _FakeCuda(torch.eye(4)))
    assert torch.equal(frames.frames[0]["c2w"], torch.eye(4)[:3])


# ------------------------------------------------------------------------------------------------ synthetic.room_depth
LO, HI = (-2.0, -1.5, -2.5), (2.5, 1.2, 3.0)


def test_room_depth_pinhole_closed_form():
    """an unturned pinhole at the origin sees the wall z = 3 at z-depth 3 wherever the ray does not meet a side wall first, and the
    side wall x = 2.5 at z-depth 2.5 / x_cam; normals point into the room"""
    cam = Pinhole(32.0, 32.0, 31.5, 23.5, 64, 48)
    d, n = synthetic.room_depth(cam, torch.eye(4), LO, HI, normals=True)
    assert d.dtype == torch.float32 and tuple(d.shape) == (48, 64) and tuple(n.shape) == (48, 64, 3)
    assert float(d[23, 31]) == 3.0 and n[23, 31].tolist() == [0.0, 0.0, -1.0]
    x = (63 - 31.5) / 32.0                                       # the last column of row 23: 3 x = 2.95 > 2.5, the side wall comes first
    assert float(d[23, 63]) == pytest.approx(2.5 / x, rel=1e-6) and n[23, 63].tolist() == [-1.0, 0.0, 0.0]
    y = (0 - 23.5) / 32.0                                        # the first row: the ceiling y = -1.5 at z-depth 1.5 / |y|
    assert float(d[0, 31]) == pytest.approx(1.5 / abs(y), rel=1e-6) and n[0, 31].tolist() == [0.0, 1.0, 0.0]
    # every point lies on the box
    j, i = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    X = torch.stack([(i - 31.5) / 32.0, (j - 23.5) / 32.0, torch.ones_like(i)], -1) * d[..., None]
    on = torch.minimum((X - torch.tensor(LO)).abs().min(-1).values, (X - torch.tensor(HI)).abs().min(-1).values)
    assert float(on.max()) < 1e-6 and bool(((X > torch.tensor(LO) - 1e-5) & (X < torch.tensor(HI) + 1e-5)).all())


def test_room_depth_range_cameras_and_poses():
    """a fisheye or equirect frame holds range: the point o + depth * (unit direction) lies on the box for a turned, displaced camera;
    pixels outside the fisheye lens hold 0"""
    c2w = np.asarray(ir.TRUE_POSE)
    for name, cam in ir.cameras().items():
        d, n = synthetic.room_depth(cam, c2w, LO, HI, normals=True)
        dirs, ok = synthetic.camera_directions(cam)
        assert bool((d[~ok] == 0).all()) and bool((d[ok] > 0).all()) and bool((n[~ok] == 0).all())
        assert (name == "fisheye") == bool((~ok).any())
        X = torch.as_tensor(c2w[:, 3]) + (dirs @ torch.as_tensor(c2w[:, :3]).T) * d.double()[..., None]
        on = torch.minimum((X - torch.tensor(LO).double()).abs().min(-1).values, (X - torch.tensor(HI).double()).abs().min(-1).values)
        assert float(on[ok].max()) < 2e-6, name
        if name != "pinhole":
            assert float((dirs[ok].norm(dim=-1) - 1).abs().max()) < 1e-12
        # the normal is the inward normal of the wall the point lies on
        along = (n.double() * (X - torch.where(n > 0, torch.tensor(LO), torch.tensor(HI)).double())).sum(-1)
        assert float(along[ok].abs().max()) < 2e-6
    # 4x4 poses are taken, the centre must lie inside, and the ray directions agree with the float32 restatements of the kernels
    assert torch.equal(synthetic.room_depth(Equirect(16, 8), torch.eye(4), LO, HI), synthetic.room_depth(Equirect(16, 8), torch.eye(4)[:3], LO, HI))
    with pytest.raises(ValueError, match="must lie strictly inside the box"):
        synthetic.room_depth(Equirect(16, 8), ir.cr.pose(0.0, 0.0, (5.0, 0.0, 0.0)), LO, HI)
    with pytest.raises(ValueError, match="c2w must be a 3x4"):
        synthetic.room_depth(Equirect(16, 8), torch.eye(3), LO, HI)
    for name, cam in ir.cameras().items():
        _, d32, ok32 = ir.pr._rays(np.float32, (cam.word, cam.params, ir.IDENTITY, cam.width, cam.height), np.arange(cam.width * cam.height))
        dirs, ok = synthetic.camera_directions(cam)
        both = ok.reshape(-1).numpy() & ok32
        assert np.abs(dirs.reshape(-1, 3).numpy()[both] - d32[both]).max() < 2e-4, name
