"""CPU tests of the depth front end's boundary (include/pnr.h "depth front end"): every PNR_EINVAL of the two entry points comes
before any launch, every refusal of ops.depth_filter / ops.depth_normals / depth.filter / depth.normals / depth.view /
fusion.odometry by its message, and the codes against the header.  Nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from panopticnerf_amd import Pinhole, _lib, depth, fusion, ops

import _depth_ref as dr
from _fake_gpu import _FakeCuda, _fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE, TWO = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(4096)      # non-null, aligned, never dereferenced
F4 = lambda *v: (ctypes.c_float * len(v))(*v)
PIN, EYE = F4(50.0, 50.0, 8.0, 6.0), F4(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
G = F4(1.0, 0.8, 0.4, 0.1, 0.05, 0.02, 0.01, 0.005, 0.001)
NAN, INF = float("nan"), float("inf")


def _header(name):
    src = open(os.path.join(ROOT, "include", "pnr.h")).read()
    m = re.search(r"#define\s+%s\s+(\S+)" % name, src)
    assert m, name
    return m.group(1)


def test_codes_and_constants_mirror_the_header():
    for name, value in dr.CODES.items():
        assert int(_header("PNR_NORMAL_" + name)) == value == getattr(ops, "NORMAL_" + name) == getattr(depth, name) == getattr(_lib, "NORMAL_" + name)
    assert sorted(dr.CODES.values()) == list(range(5))
    assert int(_header("PNR_DEPTH_MAX_RADIUS")) == dr.MAX_RADIUS == ops.DEPTH_MAX_RADIUS == depth.MAX_RADIUS == 8
    assert "pnr_depth_filter" in _lib.SIGNATURES and "pnr_depth_normals" in _lib.SIGNATURES
    import panopticnerf_amd
    assert panopticnerf_amd.depth is depth and "depth" in panopticnerf_amd.__all__


def test_spatial_weights_are_made_once_in_float64():
    """ops.depth_filter_params and the restatement make the same float32 weights: exp in float64, one rounding"""
    for radius, sigma in ((0, 1.5), (3, 1.5), (8, 4.0), (8, 0.9)):
        _, g, _, _, _ = ops.depth_filter_params("t", radius, sigma, (0.0, 0.03), 1)
        assert np.array_equal(np.array(g, np.float32), dr.spatial_weights(radius, sigma)) and g[0] == 1.0 and len(g) == radius + 1
    assert ops.depth_normals_params("t", (0.0, 0.05), 0.1) == (0.0, 0.05, 0.1 * 0.1)


# ------------------------------------------------------------------------------------------------ the entry points
def _filter(**over):
    a = dict(width=16, height=12, depth_in=ONE, radius=3, g=G, sigma_a=0.0, sigma_b=0.03, min_support=1, depth_out=TWO, support=NULL, stream=NULL)
    a.update(over)
    lib = _lib.load()
    rc = lib.pnr_depth_filter(*a.values())
    return rc, lib.pnr_last_error()


@pytest.mark.parametrize("over,message", [
    (dict(width=0), b"bad size"), (dict(height=-1), b"bad size"), (dict(width=65536, height=32768), b"bad size"),
    (dict(depth_in=NULL), b"null depth_in"), (dict(depth_out=NULL), b"null depth_in, depth_out"), (dict(g=None), b"null depth_in, depth_out or g"),
    (dict(depth_in=ctypes.c_void_p(66)), b"4-byte aligned"), (dict(depth_out=ctypes.c_void_p(4097)), b"4-byte aligned"),
    (dict(support=ctypes.c_void_p(65)), b"support 2-byte"),
    (dict(depth_out=ONE), b"depth_in and depth_out must differ"),
    (dict(radius=-1), b"radius must lie in 0 .. 8"), (dict(radius=9), b"radius must lie in 0 .. 8"),
    (dict(g=F4(1.0, 0.5, 0.0, 0.1)), b"g[2] must be positive and finite"), (dict(g=F4(1.0, -0.5, 0.2, 0.1)), b"g[1] must be positive"),
    (dict(g=F4(NAN, 0.5, 0.2, 0.1)), b"g[0] must be positive"), (dict(g=F4(1.0, 0.5, 0.2, INF)), b"g[3] must be positive and finite"),
    (dict(sigma_a=-1.0), b"sigma_a and sigma_b"), (dict(sigma_b=-0.5), b"sigma_a and sigma_b"), (dict(sigma_a=NAN), b"sigma_a and sigma_b"),
    (dict(sigma_b=INF), b"sigma_a and sigma_b"), (dict(sigma_a=0.0, sigma_b=0.0), b"not both 0"),
    (dict(min_support=0), b"min_support must be >= 1"), (dict(min_support=-3), b"min_support must be >= 1"),
])
def test_filter_einval_before_any_launch(over, message):
    rc, err = _filter(**over)
    assert rc == -1 and message in err, err


def test_filter_ignores_weights_beyond_the_radius():
    """g is read up to `radius` only: a zero behind it is no refusal (radius 1 with g[2] = 0 gets as far as the next check)"""
    rc, err = _filter(radius=1, g=F4(1.0, 0.5, 0.0), min_support=0)
    assert rc == -1 and b"min_support" in err


def _normals(**over):
    a = dict(model=0, cam=PIN, c2w=EYE, width=16, height=12, depth=ONE, jump_a=0.0, jump_b=0.05, mc2=0.01, normal=TWO, vertex=NULL, code=NULL,
             stream=NULL)
    a.update(over)
    lib = _lib.load()
    rc = lib.pnr_depth_normals(*a.values())
    return rc, lib.pnr_last_error()


@pytest.mark.parametrize("over,message", [
    (dict(model=2), b"unknown camera model"), (dict(model=-1), b"unknown camera model"),
    (dict(cam=None), b"null camera or pose"), (dict(c2w=None), b"null camera or pose"),
    (dict(width=0), b"bad size"), (dict(height=0), b"bad size"), (dict(width=65536, height=32768), b"bad size"),
    (dict(cam=F4(0.0, 50.0, 8.0, 6.0)), b"zero focal length or gamma"),
    (dict(model=1, cam=F4(2.2, 0.0, 1.6, 0.0, 60.0, 8.0, 8.0)), b"zero focal length or gamma"),
    (dict(model=3, cam=F4(-1.0, 0.5, -0.5, 0.1)), b"pnr_depth_normals: equirect"),
    (dict(depth=NULL), b"null depth or normal"), (dict(normal=NULL), b"null depth or normal"),
    (dict(depth=ctypes.c_void_p(66)), b"4-byte aligned"), (dict(normal=ctypes.c_void_p(4098)), b"4-byte aligned"),
    (dict(vertex=ctypes.c_void_p(65)), b"4-byte aligned"),
    (dict(jump_a=-1.0), b"jump_a and jump_b"), (dict(jump_b=-0.1), b"jump_a and jump_b"), (dict(jump_a=NAN), b"jump_a and jump_b"),
    (dict(jump_b=NAN), b"jump_a and jump_b"),
    (dict(mc2=-0.1), b"mc2"), (dict(mc2=1.5), b"mc2"), (dict(mc2=NAN), b"mc2"),
])
def test_normals_einval_before_any_launch(over, message):
    rc, err = _normals(**over)
    assert rc == -1 and message in err, err


# ------------------------------------------------------------------------------------------------ the ops
def _filter_args(**over):
    a = dict(depth=torch.zeros(12, 16), out=torch.zeros(12, 16))
    a.update(over)
    return a


@pytest.mark.parametrize("over,exc,message", [
    (dict(depth=None), ValueError, "depth_filter: depth must be a GPU tensor, got NoneType"),
    (dict(depth=torch.zeros(192)), ValueError, r"depth must be a \(height, width\) image, got \(192,\)"),
    (dict(depth=torch.zeros(0, 16), out=torch.zeros(0, 16)), ValueError, "bad image 16 x 0"),
    (dict(depth=torch.zeros(12, 16, dtype=torch.float64)), TypeError, "depth must be torch.float32"),
    (dict(out=None), ValueError, "out must be a GPU tensor"), (dict(out=torch.zeros(12, 17)), ValueError, r"out must be \(12, 16\)"),
    (dict(support=torch.zeros(12, 16, dtype=torch.int32)), TypeError, "support must be torch.int16"),
    (dict(support=torch.zeros(16, 12, dtype=torch.int16)), ValueError, r"support must be \(12, 16\)"),
    (dict(radius=9), ValueError, r"radius must lie in 0 .. 8 \(got 9\)"), (dict(radius=-1), ValueError, "radius must lie in"),
    (dict(sigma_space=0.0), ValueError, "sigma_space must be positive and finite"), (dict(sigma_space=INF), ValueError, "sigma_space must be positive"),
    (dict(radius=8, sigma_space=0.5), ValueError, "sigma_space 0.5 is too small for radius 8"),
    (dict(sigma_range=0.03), ValueError, r"sigma_range must be \(a, b\)"), (dict(sigma_range=(0.0, 0.0)), ValueError, "not both 0"),
    (dict(sigma_range=(-1.0, 0.03)), ValueError, "sigma_range must be non-negative"), (dict(sigma_range=(0.0, NAN)), ValueError, "sigma_range must be"),
    (dict(min_support=0), ValueError, r"min_support must be >= 1 \(got 0\)"),
    (dict(), RuntimeError, "depth_filter: depth: expected a GPU tensor \\(the HIP path has no CPU fallback\\)"),
])
def test_depth_filter_refusals(over, exc, message):
    with pytest.raises(exc, match=message):
        ops.depth_filter(**_filter_args(**over))


@pytest.mark.parametrize("over,exc,message", [
    (dict(depth=_fake(torch.zeros(16, 12).t())), ValueError, "depth_filter: depth: tensor must be contiguous"),
    (dict(out=_fake(torch.zeros(16, 12).t())), ValueError, "depth_filter: out: tensor must be contiguous"),
    (dict(support=_fake(torch.zeros(16, 12, dtype=torch.int16).t())), ValueError, "depth_filter: support: tensor must be contiguous"),
    (dict(out=_fake(torch.zeros(12, 16), "cuda:1")), ValueError, "depth_filter: out is on cuda:1, not on cpu"),
    (dict(support=_fake(torch.zeros(12, 16, dtype=torch.int16), "cuda:1")), ValueError, "depth_filter: support is on cuda:1, not on cpu"),
    (dict(out=torch.zeros(12, 16)), RuntimeError, "depth_filter: out: expected a GPU tensor"),
    (dict(support=np.zeros((12, 16), np.int16)), ValueError, "support must be a GPU tensor, got ndarray"),
    (dict(out="same"), ValueError, "out must not be depth itself"),
])
def test_depth_filter_refusals_behind_the_device_check(over, exc, message):
    a = {k: _fake(v) for k, v in _filter_args().items()}
    a.update(over)
    if isinstance(a["out"], str):
        a["out"] = a["depth"]
    with pytest.raises(exc, match=message):
        ops.depth_filter.__wrapped__(**a)


def _normals_args(**over):
    a = dict(camera_model="pinhole", cam=(50.0, 50.0, 8.0, 6.0), c2w=torch.eye(4)[:3], width=16, height=12, depth=torch.zeros(12, 16),
             normal=torch.zeros(12, 16, 3))
    a.update(over)
    return a


@pytest.mark.parametrize("over,exc,message", [
    (dict(camera_model="orthographic"), ValueError, "camera_model must be 'pinhole', 'fisheye' or 'equirect'"),
    (dict(cam=(1.0, 2.0)), ValueError, "expected 4 values, got 2"), (dict(camera_model="fisheye"), ValueError, "expected 7 values, got 4"),
    (dict(c2w=torch.eye(3)), ValueError, "depth_normals: c2w: expected 12 values"),
    (dict(width=0), ValueError, "bad image 0 x 12"),
    (dict(depth=None), ValueError, "depth must be a GPU tensor"), (dict(depth=torch.zeros(16, 12)), ValueError, r"depth must be \(12, 16\)"),
    (dict(depth=torch.zeros(12, 16, dtype=torch.float16)), TypeError, "depth must be torch.float32"),
    (dict(normal=torch.zeros(12, 16)), ValueError, r"normal must be \(12, 16, 3\)"), (dict(normal=None), ValueError, "normal must be a GPU tensor"),
    (dict(vertex=torch.zeros(12, 16, 4)), ValueError, r"vertex must be \(12, 16, 3\)"),
    (dict(code=torch.zeros(12, 16)), TypeError, "code must be torch.uint8"),
    (dict(jump=0.05), ValueError, r"jump must be \(a, b\)"), (dict(jump=(-0.1, 0.0)), ValueError, "jump must be non-negative"),
    (dict(jump=(0.0, NAN)), ValueError, "jump must be non-negative"),
    (dict(min_cos=-0.1), ValueError, r"min_cos must lie in \[0, 1\]"), (dict(min_cos=1.5), ValueError, "min_cos must lie in"),
    (dict(min_cos=NAN), ValueError, "min_cos must lie in"),
    (dict(), RuntimeError, "depth_normals: depth: expected a GPU tensor \\(the HIP path has no CPU fallback\\)"),
])
def test_depth_normals_refusals(over, exc, message):
    with pytest.raises(exc, match=message):
        ops.depth_normals(**_normals_args(**over))


@pytest.mark.parametrize("over,exc,message", [
    (dict(depth=_fake(torch.zeros(16, 12).t())), ValueError, "depth_normals: depth: tensor must be contiguous"),
    (dict(normal=_fake(torch.zeros(12, 3, 16).transpose(1, 2))), ValueError, "depth_normals: normal: tensor must be contiguous"),
    (dict(vertex=_fake(torch.zeros(12, 3, 16).transpose(1, 2))), ValueError, "depth_normals: vertex: tensor must be contiguous"),
    (dict(code=_fake(torch.zeros(16, 12, dtype=torch.uint8).t())), ValueError, "depth_normals: code: tensor must be contiguous"),
    (dict(vertex=_fake(torch.zeros(12, 16, 3), "cuda:1")), ValueError, "depth_normals: vertex is on cuda:1, not on cpu"),
    (dict(normal=torch.zeros(12, 16, 3)), RuntimeError, "depth_normals: normal: expected a GPU tensor"),
    (dict(code=[0] * 192), ValueError, "code must be a GPU tensor, got list"),
])
def test_depth_normals_refusals_behind_the_device_check(over, exc, message):
    a = _normals_args()
    a.update(depth=_fake(a["depth"]), normal=_fake(a["normal"]))
    a.update(over)
    with pytest.raises(exc, match=message):
        ops.depth_normals.__wrapped__(**a)


# ------------------------------------------------------------------------------------------------ depth.*, fusion.odometry
CAM = Pinhole(50.0, 50.0, 8.0, 6.0, 16, 12)


def test_depth_module_refusals():
    eye, img = torch.eye(4)[:3], torch.zeros(12, 16)
    for kw, message in ((dict(radius=9), "depth.filter: radius must lie in"), (dict(sigma_space=-1.0), "depth.filter: sigma_space must be positive"),
                        (dict(sigma_range=(0.0, 0.0)), "depth.filter: sigma_range must be"), (dict(min_support=0), "depth.filter: min_support must be >= 1")):
        with pytest.raises(ValueError, match=message):                           # before anything is allocated or launched
            depth.filter(_FakeCuda(img), **kw)
    with pytest.raises(TypeError, match="depth.filter: depth must be a GPU tensor, got ndarray"):
        depth.filter(img.numpy())
    with pytest.raises(ValueError, match=r"depth.filter: depth must be a float32 tensor of shape \(height, width\), got torch.float64"):
        depth.filter(img.double())
    with pytest.raises(ValueError, match=r"depth.filter: depth must be a float32 tensor of shape \(height, width\), got torch.float32 \(192,\)"):
        depth.filter(img.reshape(-1))
    with pytest.raises(RuntimeError, match="depth.filter: depth is not on the GPU \\(the HIP path has no CPU fallback\\)"):
        depth.filter(img)
    with pytest.raises(ValueError, match="depth.filter: depth must be contiguous"):
        depth.filter(_FakeCuda(torch.zeros(16, 12).t()))

    with pytest.raises(TypeError, match="depth.normals: camera must be a camera.Pinhole"):
        depth.normals("pinhole", eye, img)
    with pytest.raises(ValueError, match="depth.normals: c2w must be a 3x4"):
        depth.normals(CAM, torch.eye(3), img)
    with pytest.raises(TypeError, match="depth.normals: c2w must be host values"):
        depth.normals(CAM, _FakeCuda(eye), img)
    for kw, message in ((dict(jump=(-1.0, 0.0)), "depth.normals: jump must be non-negative"), (dict(min_cos=2.0), "depth.normals: min_cos must lie in"),
                        (dict(jump=3), r"depth.normals: jump must be \(a, b\)")):
        with pytest.raises(ValueError, match=message):
            depth.normals(CAM, eye, _FakeCuda(img), **kw)
    with pytest.raises(ValueError, match=r"depth.normals: depth must be a float32 tensor of shape \(12, 16\), got torch.float32 \(16, 12\)"):
        depth.normals(CAM, eye, _FakeCuda(torch.zeros(16, 12)))
    with pytest.raises(ValueError, match="depth.normals: depth must be contiguous"):
        depth.normals(CAM, eye, _FakeCuda(torch.zeros(16, 12).t()))
    with pytest.raises(RuntimeError, match="depth.normals: depth is not on the GPU"):
        depth.normals(CAM, eye, img)

    with pytest.raises(ValueError, match="depth.view: unknown argument 'near'"):
        depth.view(CAM, eye, img, near=0.1)
    with pytest.raises(TypeError, match="depth.view: filter must be None or a dict"):
        depth.view(CAM, eye, img, filter=3)
    with pytest.raises(ValueError, match="depth.view: unknown filter argument 'support'"):
        depth.view(CAM, eye, img, filter=dict(support=True))
    with pytest.raises(ValueError, match="depth.view: radius must lie in"):
        depth.view(CAM, eye, _FakeCuda(img), filter=dict(radius=12))
    with pytest.raises(ValueError, match="depth.view: min_cos must lie in"):
        depth.view(CAM, eye, _FakeCuda(img), min_cos=-1.0)
    with pytest.raises(TypeError, match="depth.view: camera must be"):
        depth.view(None, eye, img)
    with pytest.raises(ValueError, match="depth.view: depth must be contiguous"):
        depth.view(CAM, eye, _FakeCuda(torch.zeros(16, 12).t()))
    with pytest.raises(RuntimeError, match="depth.view: depth is not on the GPU"):
        depth.view(CAM, eye, img)


def test_odometry_refusals():
    img = torch.zeros(12, 16)
    with pytest.raises(TypeError, match="fusion.odometry: camera must be"):
        fusion.odometry("pinhole", [img])
    with pytest.raises(ValueError, match="fusion.odometry: guess must be 'identity' or 'velocity', not 'zero'"):
        fusion.odometry(CAM, [img], guess="zero")
    with pytest.raises(ValueError, match="fusion.odometry: unknown argument 'maps'"):
        fusion.odometry(CAM, [img], maps=True)
    with pytest.raises(ValueError, match="fusion.odometry: depths is empty"):
        fusion.odometry(CAM, [])
    with pytest.raises(TypeError, match="fusion.odometry: depths must be a sequence"):
        fusion.odometry(CAM, 3)
    with pytest.raises(ValueError, match=r"fusion.odometry: depths must be a sequence of \(height, width\) images or one \(F, height, width\) tensor, got \(12, 16\)"):
        fusion.odometry(CAM, img)
    for kw, message in ((dict(iters=-1), "iters must be >= 0"), (dict(dist_max=0.0), "dist_max must be positive"), (dict(min_matches=0), "min_matches must be >= 1"),
                        (dict(max_rot=0.6), r"max_rot must lie in \(0, 0.5\]"), (dict(max_trans=0.0), "max_trans must be positive")):
        with pytest.raises(ValueError, match="fusion.odometry: " + message):
            fusion.odometry(CAM, [_FakeCuda(img)], **kw)
    with pytest.raises(TypeError, match="fusion.odometry: frame 1: depth must be a GPU tensor, got ndarray"):
        fusion.odometry(CAM, [_FakeCuda(img), img.numpy()])
    with pytest.raises(ValueError, match=r"fusion.odometry: frame 0: depth must be a float32 tensor of shape \(12, 16\)"):
        fusion.odometry(CAM, [_FakeCuda(torch.zeros(16, 12))])
    with pytest.raises(ValueError, match="fusion.odometry: frame 1: depth must be contiguous"):
        fusion.odometry(CAM, [_FakeCuda(img), _FakeCuda(torch.zeros(16, 12).t())])
    with pytest.raises(RuntimeError, match="fusion.odometry: frame 0: depth is not on the GPU"):
        fusion.odometry(CAM, [img])
    with pytest.raises(ValueError, match="fusion.odometry: frame 1 is on cuda:1, frame 0 on cpu"):
        fusion.odometry(CAM, [_FakeCuda(img), _FakeCuda(img, "cuda:1")])
    with pytest.raises(ValueError, match="fusion.odometry: c2w0 must be a 3x4"):
        fusion.odometry(CAM, [_FakeCuda(img)], c2w0=torch.eye(3))
    with pytest.raises(ValueError, match="fusion.odometry: radius must lie in"):
        fusion.odometry(CAM, [_FakeCuda(img)], filter=dict(radius=20))


def test_compose_is_the_rigid_product_without_a_matmul():
    a = torch.as_tensor(np.asarray(dr.ir.TRUE_POSE, np.float64))
    b = torch.as_tensor(np.asarray(dr.ir.MODEL_POSE, np.float64))
    got = fusion._compose(a, b).numpy()
    A, B = np.vstack([a.numpy(), [0, 0, 0, 1]]), np.vstack([b.numpy(), [0, 0, 0, 1]])
    assert np.abs(got - (A @ B)[:3]).max() < 1e-15 and np.array_equal(got, dr.compose(a.numpy(), b.numpy()))
