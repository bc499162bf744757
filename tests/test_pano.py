"""CPU tests of the panoramic camera's boundary: every refusal of camera.Equirect, ops.gen_rays_equirect,
ops.project_points("equirect"), FrameSet.add and the C entry points that take model word 3 (pnr_gen_rays_equirect,
pnr_project_points, pnr_reproject) -- all rejected before any launch, so none needs a GPU --, the parameters Equirect derives
from degrees, and the unassigned word 2."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import _pano_ref as pr
from panopticnerf_amd import Equirect, Pinhole, _lib, camera, ops, synthetic
from panopticnerf_amd.data import FrameSet

EYE = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
F = lambda *v: (ctypes.c_float * len(v))(*v)
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)       # ONE: non-null, never dereferenced (validation fails first)
FULL = F(-1.0, 2.0 / 64, -0.5, 1.0 / 32)


def test_model_word_matches_the_header_and_leaves_2_unassigned():
    hdr = open(pr.ROOT + "/include/pnr.h").read()
    words = {n: int(v) for n, v in re.findall(r"#define\s+PNR_CAMERA_(\w+)\s+(-?\d+)", hdr)}
    assert words == {"PINHOLE": 0, "FISHEYE": 1, "EQUIRECT": 3}
    assert (_lib.CAMERA_PINHOLE, _lib.CAMERA_FISHEYE, _lib.CAMERA_EQUIRECT) == (0, 1, 3) and pr.EQUIRECT == 3


def test_equirect_parameters_from_degrees():
    cam = Equirect(64, 32)
    assert cam.model == "equirect" and (cam.width, cam.height) == (64, 32)
    assert cam.cam == (-1.0, 2.0 / 64, -0.5, 1.0 / 32) == pr.equirect_cam(64, 32)
    # float64 on the host, rounded to float32 once
    cam = Equirect(37, 19, lon=(150.0, 260.0), lat=(40.0, -75.0))
    want = (150 / 180, 110 / 180 / 37, -40 / 180, 115 / 180 / 19)
    assert cam.cam == tuple(float(np.float32(v)) for v in want) == pr.equirect_cam(37, 19, (150.0, 260.0), (40.0, -75.0))
    # mirrored and upside down are allowed
    assert Equirect(8, 4, lon=(180.0, -180.0), lat=(-90.0, 90.0)).cam == (1.0, -0.25, 0.5, -0.25)
    cam, c2w = synthetic.equirect_camera(64 / 1408)
    assert (cam.width, cam.height) == (64, 32) and cam.cam[0] == -1.0 and tuple(c2w.shape) == (3, 4)
    assert c2w[:, 3].tolist() == synthetic.fisheye_camera(0.1)[1][:, 3].tolist()
    assert synthetic.equirect_camera()[0].width == 1408 and synthetic.equirect_camera()[0].height == 704


@pytest.mark.parametrize("kw,word", [
    (dict(lon=(math.nan, 180.0)), "non-finite"), (dict(lat=(90.0, math.inf)), "non-finite"),
    (dict(lon=(10.0, 10.0)), "zero span"), (dict(lat=(0.0, 0.0)), "zero span"),
    (dict(lon=(-180.0, 180.5)), "above 360"), (dict(lon=(100.0, -261.0)), "above 360"),
    (dict(lat=(90.5, -90.0)), "outside"), (dict(lat=(10.0, -91.0)), "outside"),
    (dict(lon=(-181.0, 0.0)), "left edge"), (dict(lon=(200.0, 300.0)), "left edge"),
])
def test_equirect_refuses(kw, word):
    with pytest.raises(ValueError, match=word):
        Equirect(64, 32, **kw)


def test_equirect_refuses_bad_sizes_and_cpu_devices():
    with pytest.raises(ValueError, match="width and height"):
        Equirect(0, 32)
    cam = Equirect(64, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.rays(EYE, 0.5, 50.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.rays(EYE, 0.5, 50.0, pix=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.valid_pix("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam.project(torch.zeros(5, 3), EYE)
    with pytest.raises(ValueError, match="3x4"):
        cam.rays(EYE[:9], 0.5, 50.0)


def test_ops_refuse_bad_arguments():
    full = (-1.0, 2.0 / 64, -0.5, 1.0 / 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gen_rays_equirect(full, EYE, 64, 32, 0.5, 50.0, device="cpu")
    with pytest.raises(ValueError, match="cam: expected 4 values"):
        ops.gen_rays_equirect(full + (0.0,), EYE, 64, 32, 0.5, 50.0)
    with pytest.raises(ValueError, match="c2w: expected 12 values"):
        ops.gen_rays_equirect(full, EYE[:8], 64, 32, 0.5, 50.0)
    # what the entry point refuses is refused before any device memory is touched (so: also here, without a GPU)
    for cam, word in (((-1.0, 0.0, -0.5, 1 / 32), "zero equirect step"), ((-1.0, 2 / 64, -0.5, 0.0), "zero equirect step"),
                      ((math.nan, 2 / 64, -0.5, 1 / 32), "non-finite"), ((-1.0, 2 / 64, -0.5, math.inf), "non-finite"),
                      ((-1.5, 2 / 64, -0.5, 1 / 32), "lon0"), ((-1.0, 2.2 / 64, -0.5, 1 / 32), "full circle"),
                      ((-1.0, 2 / 64, -0.6, 1 / 32), "pitch range"), ((-1.0, 2 / 64, -0.5, 1.2 / 32), "pitch range")):
        with pytest.raises(RuntimeError, match=word):
            ops.gen_rays_equirect(cam, EYE, 64, 32, 0.5, 50.0, device="cuda")
    with pytest.raises(RuntimeError, match="bad size"):
        ops.gen_rays_equirect(full, EYE, 0, 32, 0.5, 50.0, device="cuda")
    with pytest.raises(ValueError, match="'pinhole', 'fisheye' or 'equirect'"):
        ops.project_points("panorama", full, EYE, 64, 32, torch.zeros(5, 3))
    with pytest.raises(ValueError, match="cam: expected 4 values"):
        ops.project_points("equirect", full + (0.0, 0.0, 0.0), EYE, 64, 32, torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.project_points("equirect", full, EYE, 64, 32, torch.zeros(5, 3))
    # _camera_words knows the three cameras and nothing else
    assert ops._camera_words(Equirect(64, 32), "x")[0::2] == (3, 64) and list(ops._camera_words(Equirect(64, 32), "x")[1]) == list(full)
    with pytest.raises(ValueError, match="camera.Pinhole or camera.Fisheye"):
        ops._camera_words(object(), "reproject: src")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reproject(Equirect(64, 32), EYE, torch.ones(32, 64), Pinhole(40.0, 41.0, 31.5, 23.5, 64, 48), EYE)
    with pytest.raises(ValueError, match=r"depth_src: expected a \(32, 64\) image"):
        ops.reproject(Equirect(64, 32), EYE, torch.ones(48, 64), Pinhole(40.0, 41.0, 31.5, 23.5, 64, 48), EYE)


def test_frameset_takes_an_equirect_and_still_refuses_strangers():
    class Stranger:
        model, width, height = "cubemap", 8, 8
    fs = FrameSet("cuda", capacity=2)
    with pytest.raises(TypeError, match="camera.Pinhole or camera.Fisheye"):
        fs.add(Stranger(), np.eye(3, 4), 0.5, 50.0, torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"rgb must be \(32, 64, 3\)"):
        fs.add(Equirect(64, 32), np.eye(3, 4), 0.5, 50.0, torch.zeros(8, 8, 3, dtype=torch.uint8))


def _rejected(lib, rc, word):
    assert rc == -1
    assert word in lib.pnr_last_error(), lib.pnr_last_error()


BAD_CAMERAS = [(F(-1.0, 0.0, -0.5, 1 / 32), b"zero"), (F(-1.0, 2 / 64, -0.5, 0.0), b"zero"),
               (F(math.nan, 2 / 64, -0.5, 1 / 32), b"non-finite"), (F(-1.0, math.inf, -0.5, 1 / 32), b"non-finite"),
               (F(-1.0, 2 / 64, -math.inf, 1 / 32), b"non-finite"), (F(-1.0, 2 / 64, -0.5, math.nan), b"non-finite"),
               (F(1.01, 2 / 64, -0.5, 1 / 32), b"lon0"), (F(-1.01, 2 / 64, -0.5, 1 / 32), b"lon0"),
               (F(-1.0, 2.01 / 64, -0.5, 1 / 32), b"more than a full circle"), (F(1.0, -2.01 / 64, -0.5, 1 / 32), b"more than a full circle"),
               (F(-1.0, 2 / 64, -0.51, 1 / 32), b"pitch range"), (F(-1.0, 2 / 64, -0.5, 1.01 / 32), b"pitch range"),
               (F(-1.0, 2 / 64, 0.5, -1.01 / 32), b"pitch range"), (F(-1.0, 2 / 64, 0.2, 0.5 / 32), b"pitch range")]


def test_pnr_gen_rays_equirect_rejects_before_any_launch():
    lib = _lib.load()

    def call(cam=FULL, c2w=F(*EYE), w=64, h=32, pix=NULL, n=64 * 32, rays=ONE):
        return lib.pnr_gen_rays_equirect(cam, c2w, w, h, 0.5, 50.0, pix, n, rays, NULL)

    _rejected(lib, call(cam=None), b"null camera")
    _rejected(lib, call(c2w=None), b"null camera")
    for kw in (dict(w=0), dict(h=0), dict(n=-1)):
        _rejected(lib, call(**kw), b"bad size")
    for cam, word in BAD_CAMERAS:
        _rejected(lib, call(cam=cam), word)
        _rejected(lib, call(cam=cam, n=0), word)                 # the camera is checked even when there is nothing to do
    _rejected(lib, call(n=100), b"without pixel indices")
    _rejected(lib, call(rays=NULL), b"16-byte aligned")
    _rejected(lib, call(rays=ctypes.c_void_p(24)), b"16-byte aligned")
    assert call(n=0, pix=ONE, rays=NULL) == 0                     # an empty pixel list is fine
    # full ranges whose float32 step carries the far edge a rounding past its limit are NOT refused
    for w, h in ((37, 19), (1408, 704), (4096, 2048), (1400, 700), (3, 7)):
        cam = F(*pr.equirect_cam(w, h))
        assert lib.pnr_gen_rays_equirect(cam, F(*EYE), w, h, 0.5, 50.0, ONE, 0, NULL, NULL) == 0, (w, h, lib.pnr_last_error())


def test_pnr_project_points_word_3_and_unknown_words():
    lib = _lib.load()

    def call(model=3, cam=FULL, w2c=F(*EYE), w=64, h=32, pts=ONE, n=10, uv=ONE):
        return lib.pnr_project_points(model, cam, w2c, w, h, pts, n, uv, ONE, ONE, NULL)

    for word in (2, -1, 4, 5):
        _rejected(lib, call(model=word), b"unknown camera model")
    _rejected(lib, call(cam=None), b"null camera")
    _rejected(lib, call(w=0), b"bad size")
    for cam, word in BAD_CAMERAS:
        _rejected(lib, call(cam=cam), word)
    _rejected(lib, call(pts=NULL), b"null points")
    _rejected(lib, call(uv=ctypes.c_void_p(20)), b"8-byte aligned")
    assert call(n=0) == 0


def test_pnr_reproject_word_3_and_unknown_words():
    lib = _lib.load()
    pin = F(40.0, 41.0, 31.5, 23.5)

    def call(ms=3, cs=FULL, ws=64, hs=32, n=64 * 32, mt=3, ct=FULL, wt=64, ht=32, ds=ONE):
        return lib.pnr_reproject(ms, cs, F(*EYE), ws, hs, NULL, n, ds, mt, ct, F(*EYE), wt, ht, ONE, 0.0, 0.02, NULL, NULL, 0, ONE, ONE, NULL,
                                 ONE, NULL)

    _rejected(lib, call(ms=2), b"unknown camera model")
    _rejected(lib, call(mt=-1), b"unknown camera model")
    _rejected(lib, call(mt=5), b"unknown camera model")
    _rejected(lib, call(cs=F(-1.0, 0.0, -0.5, 1 / 32)), b"zero focal length or gamma")
    _rejected(lib, call(ct=F(-1.0, 2 / 64, -0.5, 0.0)), b"zero focal length or gamma")
    for cam, word in BAD_CAMERAS[2:]:
        _rejected(lib, call(cs=cam), word)
        assert b"pnr_reproject: src:" in lib.pnr_last_error()
        _rejected(lib, call(ms=0, cs=pin, ws=64, hs=48, n=64 * 48, ct=cam), word)
        assert b"pnr_reproject: tgt:" in lib.pnr_last_error()
    _rejected(lib, call(n=100), b"without pixel indices")
    _rejected(lib, call(ds=NULL), b"null source depth")
