"""CPU tests of the ray-casting boundary: every refusal of pnr_tsdf_raycast, ops.tsdf_raycast and fusion.raycast happens before
any launch and names its argument; the defaults of step and max_steps; the code constants against the header."""
import ctypes

import numpy as np
import pytest
import torch

import _camera_ref as cr
import _raycast_ref as rr
from panopticnerf_amd import Equirect, Fisheye, Pinhole, _lib, fusion, ops

NULL = ctypes.c_void_p(0)
PTR = ctypes.c_void_p(4096)             # non-null and aligned, never dereferenced: validation fails first
INF = float("inf")
NAN = float("nan")
PIN = (50.0, 50.0, 8.0, 6.0)
POSE = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def refused(rc, *words):
    msg = _lib.load().pnr_last_error()
    return rc == -1 and all(w.encode() in msg for w in words)


def call(model=_lib.CAMERA_PINHOLE, cam=PIN, c2w=POSE, width=16, height=12, near=0.0, far=10.0, res=(4, 4, 4), lo=(0.0, 0.0, 0.0),
         step=(1.0, 1.0, 1.0), tsdf=PTR, weight=PTR, min_weight=1.0, dt=0.5, max_steps=10, depth=PTR, normal=NULL, src=NULL, code=PTR):
    arr = lambda v, n: None if v is None else (ctypes.c_float * n)(*v)
    return _lib.load().pnr_tsdf_raycast(model, arr(cam, 7 if cam is not None and len(cam) == 7 else 4), arr(c2w, 12), width, height, near, far,
                                        res[0], res[1], res[2], arr(lo, 3), arr(step, 3), tsdf, weight, min_weight, dt, max_steps, depth,
                                        normal, src, code, NULL)


# ---------------------------------------------------------------- the entry point
def test_entry_point_refuses_before_any_launch():
    who = "pnr_tsdf_raycast"
    assert refused(call(model=2), who, "unknown camera model 2") and refused(call(model=-1), who, "unknown camera model")
    assert refused(call(cam=None), who, "null camera or pose") and refused(call(c2w=None), who, "null camera or pose")
    assert refused(call(tsdf=NULL), who, "null tsdf or weight") and refused(call(weight=NULL), who, "null tsdf or weight")
    assert refused(call(depth=NULL), who, "null depth or code") and refused(call(code=NULL), who, "null depth or code")
    for name in ("tsdf", "weight", "depth", "normal", "src"):
        assert refused(call(**{name: ctypes.c_void_p(4098)}), who, "misaligned array"), name
    for w, h in ((0, 12), (16, 0), (-1, 12), (1 << 16, 1 << 15), (2 ** 31 - 1, 2)):
        assert refused(call(width=w, height=h), who, "bad image"), (w, h)
    # a camera the model's checks refuse
    assert refused(call(cam=(0.0, 50.0, 8.0, 6.0)), who, "zero focal length or gamma")
    assert refused(call(model=_lib.CAMERA_FISHEYE, cam=(2.2, 0.0, 1.6, 0.0, 80.0, 8.0, 6.0)), who, "zero focal length or gamma")
    assert refused(call(model=_lib.CAMERA_EQUIRECT, cam=(-1.0, 0.0, 0.5, -1.0 / 12)), who, "zero")
    assert refused(call(model=_lib.CAMERA_EQUIRECT, cam=(-1.0, 0.25, 0.5, -1.0 / 12)), who, "more than a full circle")
    assert refused(call(model=_lib.CAMERA_EQUIRECT, cam=(NAN, 2.0 / 16, 0.5, -1.0 / 12)), who, "non-finite equirect parameter")
    for res in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (-3, 4, 4), (1 << 16, 1 << 16, 2), (1290, 1290, 1291)):
        assert refused(call(res=res), who, "lattice", "every res >= 2"), res
    assert refused(call(lo=None), who, "null lo or step") and refused(call(step=None), who, "null lo or step")
    for axis in range(3):
        for bad in (NAN, INF, -INF):
            v = [0.5, 0.5, 0.5]
            v[axis] = bad
            assert refused(call(lo=v), who, "finite", "axis %d" % axis)
            assert refused(call(step=v), who, "finite", "axis %d" % axis)
        for zero in (0.0, -0.0):
            v = [0.5, 0.5, 0.5]
            v[axis] = zero
            assert refused(call(step=v), who, "step non-zero", "axis %d" % axis)
    for dt in (0.0, -0.5, NAN, INF, -INF):
        assert refused(call(dt=dt), who, "dt must be positive and finite"), dt
    for ms in (-1, -(2 ** 31)):
        assert refused(call(max_steps=ms), who, "max_steps"), ms
    for mw in (0.0, -1.0, NAN, -INF):
        assert refused(call(min_weight=mw), who, "min_weight must be positive"), mw
    for near, far in ((-0.5, 10.0), (NAN, 10.0), (1.0, 1.0), (2.0, 1.0), (0.0, NAN), (0.0, -INF)):
        assert refused(call(near=near, far=far), who, "0 <= near < far"), (near, far)


def test_constants_match_the_header():
    for name in ("HIT", "NO_RAY", "MISSED", "NO_SURFACE"):
        want = cr._header_constant("PNR_RAYCAST_" + name)
        assert getattr(fusion, name) == getattr(ops, "RAYCAST_" + name) == getattr(rr, name) == want, name
    assert (fusion.HIT, fusion.NO_RAY, fusion.MISSED, fusion.NO_SURFACE) == (0, 1, 2, 3)
    assert cr._header_constant("PNR_RAYCAST_TILE") ** 2 == 64 and cr._header_constant("PNR_RAYCAST_BLOCK") == 256


# ---------------------------------------------------------------- ops
def test_ops_refuse_by_name():
    t, w = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)
    depth, code = torch.zeros(12, 16), torch.zeros(12, 16, dtype=torch.uint8)
    lo, step = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)

    def go(model="pinhole", cam=PIN, c2w=POSE, width=16, height=12, near=0.0, far=10.0, lo=lo, step=step, tsdf=t, weight=w, depth=depth,
           code=code, **kw):
        return ops.tsdf_raycast(model, cam, c2w, width, height, near, far, lo, step, tsdf, weight, depth, code, **kw)

    with pytest.raises(RuntimeError, match="tsdf_raycast: tsdf.*no CPU fallback"):
        go()
    with pytest.raises(ValueError, match="camera_model must be 'pinhole', 'fisheye' or 'equirect'"):
        go(model="orthographic")
    with pytest.raises(ValueError, match="tsdf_raycast: model 'pinhole' cam: expected 4 values"):
        go(cam=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="tsdf_raycast: model 'fisheye' cam: expected 7 values"):
        go(model="fisheye")
    with pytest.raises(ValueError, match="tsdf_raycast: c2w: expected 12 values"):
        go(c2w=POSE[:9])
    for wh in ((0, 12), (16, -1), (1 << 16, 1 << 15)):
        with pytest.raises(ValueError, match="tsdf_raycast: bad image"):
            go(width=wh[0], height=wh[1])
    with pytest.raises(ValueError, match="tsdf must be a GPU tensor"):
        go(tsdf=np.zeros((3, 4, 5), np.float32))
    for bad in (torch.zeros(4, 5), torch.zeros(1, 4, 5), torch.zeros(3, 4, 1), torch.zeros(2, 3, 4, 5)):
        with pytest.raises(ValueError, match=r"tsdf must be \(res_z, res_y, res_x\) with every res >= 2"):
            go(tsdf=bad)
    with pytest.raises(ValueError, match="more than the limit"):
        go(tsdf=torch.zeros(1).expand(1291, 1290, 1290))
    with pytest.raises(TypeError, match="tsdf must be torch.float32"):
        go(tsdf=t.double())
    with pytest.raises(ValueError, match="weight must be a GPU tensor"):
        go(weight=None)
    with pytest.raises(ValueError, match=r"weight must be \(3, 4, 5\)"):
        go(weight=torch.zeros(3, 4, 6))
    with pytest.raises(TypeError, match="weight must be torch.float32"):
        go(weight=w.half())
    with pytest.raises(ValueError, match="depth must be a GPU tensor"):
        go(depth=None)
    with pytest.raises(ValueError, match=r"depth must be \(12, 16\)"):
        go(depth=torch.zeros(16, 12))
    with pytest.raises(TypeError, match="depth must be torch.float32"):
        go(depth=depth.double())
    with pytest.raises(ValueError, match="code must be a GPU tensor"):
        go(code=None)
    with pytest.raises(TypeError, match="code must be torch.uint8"):
        go(code=code.int())
    with pytest.raises(ValueError, match=r"code must be \(12, 16\)"):
        go(code=code.reshape(-1))
    with pytest.raises(ValueError, match=r"normal must be \(12, 16, 3\)"):
        go(normal=torch.zeros(12, 16))
    with pytest.raises(TypeError, match="normal must be torch.float32"):
        go(normal=torch.zeros(12, 16, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="src must be torch.int32"):
        go(src=torch.zeros(12, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"src must be \(12, 16\)"):
        go(src=torch.zeros(12, 17, dtype=torch.int32))
    with pytest.raises(ValueError, match="tsdf_raycast: lo"):
        go(lo=(0.0, 0.0))
    with pytest.raises(ValueError, match="lo must be finite"):
        go(lo=(0.0, NAN, 0.0))
    with pytest.raises(ValueError, match="step must be finite"):
        go(step=(1.0, 1.0, INF))
    with pytest.raises(ValueError, match="step must be non-zero"):
        go(step=(1.0, 0.0, 1.0))
    for near, far in ((-1.0, 10.0), (NAN, 10.0), (3.0, 3.0), (0.0, NAN)):
        with pytest.raises(ValueError, match="need 0 <= near < far"):
            go(near=near, far=far)
    for mw in (0.0, -2.0, NAN):
        with pytest.raises(ValueError, match="min_weight must be positive"):
            go(min_weight=mw)
    for dt in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="dt must be positive and finite"):
            go(dt=dt)
    with pytest.raises(ValueError, match="max_steps must be >= 0"):
        go(max_steps=-1)
    # (contiguity and the device are checked last, tensor by tensor: test_gpu_raycast.py)


# ---------------------------------------------------------------- fusion
def test_raycast_refuses_by_name():
    v = fusion.Volume((0, 0, 0), (1, 1, 1), 4, "cpu")
    cam = Pinhole(*PIN, 16, 12)
    pose = torch.tensor(POSE).reshape(3, 4)
    with pytest.raises(TypeError, match="fusion.raycast: volume must be a fusion.Volume"):
        fusion.raycast(v.tsdf, cam, pose, 0.0, 10.0)
    with pytest.raises(TypeError, match="fusion.raycast: camera must be a camera.Pinhole, camera.Fisheye or camera.Equirect"):
        fusion.raycast(v, PIN, pose, 0.0, 10.0)
    with pytest.raises(ValueError, match="ray casting needs every res >= 2"):
        fusion.raycast(fusion.Volume((0, 0, 0), (1, 1, 1), (4, 1, 4), "cpu"), cam, pose, 0.0, 10.0)
    for near, far in ((-1.0, 10.0), (2.0, 2.0), (NAN, 1.0)):
        with pytest.raises(ValueError, match="fusion.raycast: need 0 <= near < far"):
            fusion.raycast(v, cam, pose, near, far)
    for mw in (0.0, NAN):
        with pytest.raises(ValueError, match="fusion.raycast: min_weight must be positive"):
            fusion.raycast(v, cam, pose, 0.0, 10.0, min_weight=mw)
    for step in (0.0, -0.1, NAN, INF):
        with pytest.raises(ValueError, match="fusion.raycast: step must be positive and finite"):
            fusion.raycast(v, cam, pose, 0.0, 10.0, step=step)
    with pytest.raises(ValueError, match="fusion.raycast: max_steps must be >= 0"):
        fusion.raycast(v, cam, pose, 0.0, 10.0, max_steps=-2)
    for c in (cam, Fisheye(*cr.KITTI_FISHEYE, 16, 12), Equirect(16, 12)):
        with pytest.raises(RuntimeError, match="fusion.raycast: the volume is not on the GPU.*no CPU fallback"):
            fusion.raycast(v, c, pose, 0.0, 10.0)


def test_default_step_and_max_steps():
    v = fusion.Volume((-1, 0, 1), (1, 3, 2), (8, 5, 4), "cpu")         # steps 0.25, 0.6, 0.25
    dt = ops.raycast_default_dt(v.step)
    assert dt == float(np.float32(0.5) * np.abs(v.step).min()) == 0.125 and dt == float(rr.default_dt(v.step))
    ms = ops.raycast_default_max_steps(v.res, v.step, dt)
    diag = float(np.sqrt((7 * 0.25) ** 2 + (4 * float(v.step[1])) ** 2 + (3 * 0.25) ** 2))
    assert ms == int(diag / dt) + 2 == rr.default_max_steps(v.res, v.step, dt)
    assert ms * dt > diag                       # enough samples for the longest chord of the lattice
    assert ops.raycast_default_dt((-0.5, 0.25, 1.0)) == 0.125      # |step|: a box given hi < lo still marches forward
    assert ops.raycast_default_max_steps((2, 2, 2), (1.0, 1.0, 1.0), 1e-12) == 2 ** 31 - 1
