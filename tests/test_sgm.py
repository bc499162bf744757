"""CPU tests of the stereo-matching boundary (include/pnr.h "stereo matching"): every refusal of the four ops and of
panopticnerf_amd.stereo by name, and every PNR_EINVAL of the five entry points, returned before anything is launched (no GPU
here: a launch would fail differently).  The arithmetic is tested in test_sgm_ref.py (CPU) and test_gpu_sgm.py (GPU)."""
import ctypes
import itertools

import pytest
import torch

from panopticnerf_amd import Equirect, Fisheye, Pinhole, _lib, ops, stereo, synthetic

PTR = ctypes.c_void_p(0x10000)          # a non-null, 32-byte aligned address that is never touched
NULL = ctypes.c_void_p(0)


def _einval(rc, *words):
    assert rc == -1
    msg = _lib.load().pnr_last_error().decode()
    for w in words:
        assert w in msg, msg


# ---------------------------------------------------------------- the entry points
def test_census_einval():
    lib = _lib.load()
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 65536)):
        _einval(lib.pnr_census(PTR, w, h, PTR, None), "pnr_census", "size")
    _einval(lib.pnr_census(NULL, 4, 4, PTR, None), "pnr_census", "null")
    _einval(lib.pnr_census(PTR, 4, 4, NULL, None), "pnr_census", "null")


def test_aggregate_einval():
    lib = _lib.load()
    ok = dict(w=8, h=4, d=16, p1=10, p2=120, paths=8)

    def call(cl=PTR, cr=PTR, S=PTR, **kw):
        a = dict(ok, **kw)
        return lib.pnr_sgm_aggregate(cl, cr, a["w"], a["h"], a["d"], a["p1"], a["p2"], a["paths"], S, NULL, None)

    for d in (0, 8, 24, 100, 272, 512, -16):
        _einval(call(d=d), "pnr_sgm_aggregate", "max_disp")
    _einval(call(p1=121), "pnr_sgm_aggregate", "p1 <= p2")
    _einval(call(p1=10, p2=9), "pnr_sgm_aggregate", "p1 <= p2")
    _einval(call(p2=193), "pnr_sgm_aggregate", "192")
    _einval(call(p1=0), "pnr_sgm_aggregate", "0 < p1")
    for paths in (6, 0, 5, 16):
        _einval(call(paths=paths), "pnr_sgm_aggregate", "paths")
    for w, h in ((0, 4), (4, 0), (-3, 4), (4, -3), (65536, 65536)):
        _einval(call(w=w, h=h), "pnr_sgm_aggregate", "size")
    for k in ("cl", "cr", "S"):
        _einval(call(**{k: NULL}), "pnr_sgm_aggregate", "null")
    _einval(call(S=ctypes.c_void_p(0x10010)), "pnr_sgm_aggregate", "aligned")
    _einval(call(cl=ctypes.c_void_p(0x10004)), "pnr_sgm_aggregate", "aligned")


def test_select_einval():
    lib = _lib.load()

    def call(S=PTR, w=8, h=4, d=16, uniq=5, lr=1, d16=PTR, dr=PTR):
        return lib.pnr_sgm_select(S, w, h, d, uniq, lr, d16, dr, None)

    for d in (0, 24, 272):
        _einval(call(d=d), "pnr_sgm_select", "max_disp")
    for u in (-1, 100):
        _einval(call(uniq=u), "pnr_sgm_select", "uniqueness")
    _einval(call(lr=-2), "pnr_sgm_select", "lr_tol")
    _einval(call(dr=NULL, lr=0), "pnr_sgm_select", "disp_right")
    _einval(call(dr=NULL, lr=3), "pnr_sgm_select", "disp_right")
    _einval(call(S=NULL), "pnr_sgm_select", "null")
    _einval(call(d16=NULL), "pnr_sgm_select", "null")
    for w, h in ((0, 4), (4, 0), (-1, -1)):
        _einval(call(w=w, h=h), "pnr_sgm_select", "size")
    _einval(call(S=ctypes.c_void_p(0x10002)), "pnr_sgm_select", "aligned")


def test_depth_einval():
    lib = _lib.load()
    inf = float("inf")
    _einval(lib.pnr_disparity_depth(PTR, -1, 1.0, 1e-3, inf, PTR, None), "pnr_disparity_depth", "size")
    for fb in (0.0, -1.0, inf, float("nan")):
        _einval(lib.pnr_disparity_depth(PTR, 4, fb, 1e-3, inf, PTR, None), "pnr_disparity_depth", "fb")
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (1.0, float("nan"))):
        _einval(lib.pnr_disparity_depth(PTR, 4, 1.0, lo, hi, PTR, None), "pnr_disparity_depth", "range")
    _einval(lib.pnr_disparity_depth(NULL, 4, 1.0, 1e-3, inf, PTR, None), "pnr_disparity_depth", "null")
    _einval(lib.pnr_disparity_depth(PTR, 4, 1.0, 1e-3, inf, NULL, None), "pnr_disparity_depth", "null")
    assert lib.pnr_disparity_depth(NULL, 0, 1.0, 1e-3, inf, NULL, None) == 0          # nothing to do: PNR_OK, nothing launched


def test_workspace_bytes():
    lib = _lib.load()
    f = lib.pnr_sgm_workspace_bytes
    for bad in ((0, 4, 16, 8), (4, 0, 16, 8), (4, 4, 24, 8), (4, 4, 272, 8), (4, 4, 16, 6), (65536, 65536, 16, 8)):
        assert f(*bad) == -1
        assert "pnr_sgm_workspace_bytes" in lib.pnr_last_error().decode()
    axes = ((1, 64, 1408), (1, 33, 376), (16, 64, 128, 256), (4, 8))
    size = {k: f(*k) for k in itertools.product(*axes)}
    assert all(v >= 0 for v in size.values())
    for k, v in size.items():           # monotone (never decreasing) in each argument
        for i, axis in enumerate(axes):
            for bigger in axis:
                if bigger > k[i]:
                    assert size[k[:i] + (bigger,) + k[i + 1:]] >= v


# ---------------------------------------------------------------- the ops
def _raises(exc, words, fn, *a, **kw):
    with pytest.raises(exc) as e:
        fn(*a, **kw)
    for w in ([words] if isinstance(words, str) else words):
        assert w in str(e.value), str(e.value)


U8 = torch.zeros((6, 20), dtype=torch.uint8)
I64 = torch.zeros((6, 20), dtype=torch.int64)
VOL = torch.zeros((6, 20, 16), dtype=torch.int16)
D16 = torch.zeros((6, 20), dtype=torch.int16)


def test_census_refusals():
    _raises(ValueError, "census: img", ops.census, [[1, 2]])
    _raises(TypeError, ["census: img", "uint8"], ops.census, U8.float())
    _raises(ValueError, "census: img", ops.census, torch.zeros((2, 3, 3), dtype=torch.uint8))
    _raises(ValueError, "census: img", ops.census, torch.zeros((0, 3), dtype=torch.uint8))
    _raises(TypeError, "census: out", ops.census, U8, out=U8)
    _raises(ValueError, "census: out", ops.census, U8, out=torch.zeros((6, 21), dtype=torch.int64))
    _raises(RuntimeError, ["census: img", "GPU"], ops.census, U8)


def test_aggregate_refusals():
    _raises(ValueError, "sgm_aggregate: census_l", ops.sgm_aggregate, None, I64)
    _raises(TypeError, "sgm_aggregate: census_l", ops.sgm_aggregate, U8, I64)
    _raises(TypeError, "sgm_aggregate: census_r", ops.sgm_aggregate, I64, I64.int())
    _raises(ValueError, "sgm_aggregate: census_r", ops.sgm_aggregate, I64, I64[:, :19])
    _raises(ValueError, "sgm_aggregate: census_l", ops.sgm_aggregate, I64[0], I64[0])
    for d in (0, 8, 24, 272, -16):
        _raises(ValueError, ["sgm_aggregate", "max_disp"], ops.sgm_aggregate, I64, I64, d)
    _raises(ValueError, ["sgm_aggregate", "p1"], ops.sgm_aggregate, I64, I64, 16, 121, 120)
    _raises(ValueError, ["sgm_aggregate", "p2"], ops.sgm_aggregate, I64, I64, 16, 10, 193)
    _raises(ValueError, ["sgm_aggregate", "p1"], ops.sgm_aggregate, I64, I64, 16, 0, 120)
    _raises(ValueError, ["sgm_aggregate", "paths"], ops.sgm_aggregate, I64, I64, 16, paths=6)
    _raises(TypeError, "sgm_aggregate: out", ops.sgm_aggregate, I64, I64, 16, out=VOL.int())
    _raises(ValueError, "sgm_aggregate: out", ops.sgm_aggregate, I64, I64, 32, out=VOL)
    _raises(RuntimeError, ["sgm_aggregate: census_l", "GPU"], ops.sgm_aggregate, I64, I64, 16)


def test_select_refusals():
    _raises(ValueError, "sgm_select: S", ops.sgm_select, "S")
    _raises(TypeError, "sgm_select: S", ops.sgm_select, VOL.int())
    _raises(ValueError, "sgm_select: S", ops.sgm_select, D16)
    _raises(ValueError, ["sgm_select", "max_disp"], ops.sgm_select, torch.zeros((6, 20, 24), dtype=torch.int16))
    for u in (-1, 100):
        _raises(ValueError, ["sgm_select", "uniqueness"], ops.sgm_select, VOL, u)
    _raises(ValueError, ["sgm_select", "lr_tol"], ops.sgm_select, VOL, 5, -2)
    _raises(TypeError, "sgm_select: out", ops.sgm_select, VOL, out=D16.int())
    _raises(ValueError, "sgm_select: disp_right", ops.sgm_select, VOL, disp_right=D16[:5])
    _raises(RuntimeError, ["sgm_select: S", "GPU"], ops.sgm_select, VOL)


def test_depth_refusals():
    _raises(ValueError, "disparity_depth: d16", ops.disparity_depth, 3, 1.0)
    _raises(TypeError, "disparity_depth: d16", ops.disparity_depth, D16.float(), 1.0)
    for fb in (0.0, -2.0, float("inf"), float("nan")):
        _raises(ValueError, ["disparity_depth", "fb"], ops.disparity_depth, D16, fb)
    for r in ((0.0, 1.0), (2.0, 1.0), (1.0,), 5.0, (float("nan"), 1.0)):
        _raises(ValueError, ["disparity_depth", "d_range"], ops.disparity_depth, D16, 1.0, r)
    _raises(TypeError, "disparity_depth: out", ops.disparity_depth, D16, 1.0, out=D16)
    _raises(ValueError, "disparity_depth: out", ops.disparity_depth, D16, 1.0, out=torch.zeros((6, 21)))
    _raises(RuntimeError, ["disparity_depth: d16", "GPU"], ops.disparity_depth, D16, 1.0)


# ---------------------------------------------------------------- the module
def test_to_gray():
    rgb = torch.tensor([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 30]]], dtype=torch.uint8)
    want = [(77 * r + 150 * g + 29 * b + 128) >> 8 for r, g, b in rgb[0].tolist()]
    assert want[:2] == [0, 255]
    got = stereo.to_gray(rgb)
    assert got.dtype == torch.uint8 and got.shape == (1, 6) and got[0].tolist() == want
    every = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(stereo.to_gray(torch.stack([every, every, every], -1)[None])[0], every)      # a gray image stays what it is
    for bad in (rgb.float(), rgb[0], rgb[..., :2], [[1, 2, 3]]):
        _raises(ValueError, "stereo.to_gray", stereo.to_gray, bad)


def test_stereo_refusals():
    pin = Pinhole(500.0, 500.0, 10.0, 3.0, 20, 6)
    _raises(ValueError, "stereo.sgm: left", stereo.sgm, None, U8)
    _raises(TypeError, "stereo.sgm: right", stereo.sgm, U8, U8.float())
    _raises(ValueError, "stereo.sgm: left", stereo.sgm, U8[0], U8)
    _raises(ValueError, "stereo.sgm", stereo.sgm, U8, U8[:, :19])
    _raises(RuntimeError, "GPU", stereo.sgm, U8, U8, max_disp=16)
    _raises(RuntimeError, "GPU", stereo.sgm, torch.zeros((6, 20, 3), dtype=torch.uint8), U8, max_disp=16)        # through to_gray
    fish, _ = synthetic.fisheye_camera(scale=0.02)
    for cam, name in ((fish, "Fisheye"), (Equirect(20, 10), "Equirect"), (None, "NoneType")):
        _raises(TypeError, ["stereo.depth", "Pinhole", name], stereo.depth, D16, cam, 0.6)
        _raises(TypeError, ["stereo.depth", "Pinhole", name], stereo.depth_from_pair, U8, U8, cam, 0.6)
    assert isinstance(fish, Fisheye)
    for b in (0.0, -0.6, float("inf"), float("nan")):
        _raises(ValueError, ["stereo.depth", "baseline"], stereo.depth, D16, pin, b)
    _raises(ValueError, "stereo.depth", stereo.depth, D16, Pinhole(500.0, 500.0, 10.0, 3.0, 21, 6), 0.6)
    _raises(ValueError, ["disparity_depth", "d_range"], stereo.depth, D16, pin, 0.6, (0.0, 5.0))
    _raises(RuntimeError, "GPU", stereo.depth, {"d16": D16}, pin, 0.6)
    _raises(ValueError, ["stereo.sgm", "max_disp"], stereo.depth_from_pair, U8, U8, pin, 0.6, max_disp=20)
    for kw, word in ((dict(max_disp=272), "max_disp"), (dict(p1=20, p2=10), "p1"), (dict(p2=200), "p2"), (dict(paths=6), "paths"),
                     (dict(uniqueness=100), "uniqueness"), (dict(lr_tol=-2), "lr_tol")):
        _raises(ValueError, ["stereo.sgm", word], stereo.sgm, U8, U8, **kw)
    assert "stereo" in __import__("panopticnerf_amd").__all__
