"""CPU tests of the cross-view reprojection boundary: every ValueError / RuntimeError of ops.reproject, consistency.* and
Evaluator.evaluate_pair, pnr_reproject's PNR_EINVALs (rejected before any launch, so they need no GPU), camera.invert_pose
against tests/_camera_ref.py, consistency.warp against numpy indexing, and Evaluator.summarize() with and without pairs."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _camera_ref as cr
from panopticnerf_amd import Fisheye, Pinhole, _lib, camera, consistency, ops
from panopticnerf_amd.evaluate import Evaluator

PIN = Pinhole(40.0, 41.0, 31.5, 23.5, 64, 48)
FISH = Fisheye(2.2134, 0.016798, 1.6548, 91.6, 91.6, 48.66, 47.9, 96, 96)
EYE = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_invert_pose_is_the_float64_inverse_rounded_once():
    for c2w in list(cr.POSES.values()) + [cr.pose(0.05, -0.03, (0.3, 1.5, 0.4))]:
        want = cr.invert_pose(c2w)
        for given in (c2w, torch.as_tensor(c2w), np.concatenate([c2w, [[0.0, 0.0, 0.0, 1.0]]], 0), c2w.reshape(-1).tolist()):
            got = camera.invert_pose(given)
            assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4) and got.device.type == "cpu"
            # one rounding of the float64 result: within half a float32 ulp of it (float64 summation order aside)
            half_ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) / 2
            assert (np.abs(got.double().numpy() - want) <= half_ulp * (1 + 1e-6)).all()
        # a rigid pose: w2c c2w = identity
        full = np.concatenate([got.double().numpy(), [[0, 0, 0, 1.0]]], 0) @ np.concatenate([c2w, [[0, 0, 0, 1.0]]], 0)
        assert np.abs(full - np.eye(4)).max() < 1e-5
    with pytest.raises(ValueError, match="3x4"):
        camera.invert_pose(np.zeros((3, 3)))


def test_ops_reproject_refuses_bad_arguments():
    d = torch.ones(48, 64)
    df = torch.ones(96, 96)
    lab = torch.zeros(48, 64, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reproject(PIN, EYE, d, PIN, EYE)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reproject(FISH, EYE, df, PIN, EYE, depth_tgt=d, want=("match", "uv", "stats"))
    with pytest.raises(ValueError, match="depth_src is required"):
        ops.reproject(PIN, EYE, None, PIN, EYE)
    with pytest.raises(ValueError, match=r"depth_src: expected a \(48, 64\) image"):
        ops.reproject(PIN, EYE, df, PIN, EYE)
    with pytest.raises(ValueError, match=r"depth_tgt: expected a \(96, 96\) image"):
        ops.reproject(PIN, EYE, d, FISH, EYE, depth_tgt=d)
    with pytest.raises(ValueError, match="camera.Pinhole or camera.Fisheye"):
        ops.reproject("pinhole", EYE, d, PIN, EYE)
    with pytest.raises(ValueError, match="camera.Pinhole or camera.Fisheye"):
        ops.reproject(PIN, EYE, d, None, EYE)
    with pytest.raises(ValueError, match="c2w_src: expected 12 values"):
        ops.reproject(PIN, EYE[:9], d, PIN, EYE)
    with pytest.raises(ValueError, match="w2c_tgt: expected 12 values"):
        ops.reproject(PIN, EYE, d, PIN, EYE + [0.0, 0.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="unknown output"):
        ops.reproject(PIN, EYE, d, PIN, EYE, want=("match", "depth"))
    with pytest.raises(ValueError, match="come together"):
        ops.reproject(PIN, EYE, d, PIN, EYE, label_src=lab, n_classes=4)
    with pytest.raises(ValueError, match="come together"):
        ops.reproject(PIN, EYE, d, PIN, EYE, label_tgt=lab, n_classes=4)
    with pytest.raises(ValueError, match="agree needs"):
        ops.reproject(PIN, EYE, d, PIN, EYE, want=("agree",))
    with pytest.raises(ValueError, match="agree needs"):
        ops.reproject(PIN, EYE, d, PIN, EYE, agree=torch.zeros(4, 4, dtype=torch.int64))
    for n in (0, -1, 8193):
        with pytest.raises(ValueError, match="n_classes must be in 1 .. 8192"):
            ops.reproject(PIN, EYE, d, PIN, EYE, label_src=lab, label_tgt=lab, n_classes=n)
    for tol in ((-1e-3, 0.02), (0.0, -0.02), (math.inf, 0.0), (0.0, math.nan)):
        with pytest.raises(ValueError, match="finite and >= 0"):
            ops.reproject(PIN, EYE, d, PIN, EYE, tol=tol)
    with pytest.raises(ValueError, match=r"label_src: expected a \(48, 64\) image"):
        ops.reproject(PIN, EYE, d, PIN, EYE, label_src=lab[:40], label_tgt=lab, n_classes=4)
    with pytest.raises(ValueError, match="1-D tensor"):
        ops.reproject(PIN, EYE, d, PIN, EYE, pix=torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reproject(PIN, EYE, d, PIN, EYE, pix=torch.zeros(4, dtype=torch.int32))


def test_pnr_reproject_rejects_before_any_launch():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)       # `one`: non-null, never dereferenced (validation fails first)
    F = lambda *v: (ctypes.c_float * len(v))(*v)
    pin, fish, pose = F(40.0, 41.0, 31.5, 23.5), F(2.2, 0.01, 1.6, 91.0, 91.0, 48.0, 47.0), F(*EYE)

    def call(ms=0, cs=pin, c2w=pose, ws=64, hs=48, pix=null, n=64 * 48, ds=one, mt=1, ct=fish, w2c=pose, wt=96, ht=96, dt=one, ta=0.0, tr=0.02,
             ls=null, lt=null, nc=0, match=one, uv=one, agree=null, stats=one):
        return lib.pnr_reproject(ms, cs, c2w, ws, hs, pix, n, ds, mt, ct, w2c, wt, ht, dt, ta, tr, ls, lt, nc, match, uv, agree, stats, null)

    def rejected(word, **kw):
        assert call(**kw) == -1, kw
        assert word in lib.pnr_last_error(), (kw, lib.pnr_last_error())

    rejected(b"unknown camera model", ms=2)
    rejected(b"unknown camera model", mt=-1)
    for k in ("cs", "c2w", "ct", "w2c"):
        rejected(b"null camera or pose", **{k: None})
    rejected(b"null source depth", ds=null)
    rejected(b"zero focal length or gamma", cs=F(0.0, 41.0, 31.5, 23.5))
    rejected(b"zero focal length or gamma", cs=F(40.0, 0.0, 31.5, 23.5))
    rejected(b"zero focal length or gamma", ct=F(2.2, 0.01, 1.6, 0.0, 91.0, 48.0, 47.0))
    rejected(b"zero focal length or gamma", ms=1, cs=F(2.2, 0.01, 1.6, 91.0, 0.0, 48.0, 47.0), n=64 * 48)
    for kw in (dict(ws=0), dict(hs=-1), dict(wt=0), dict(ht=0), dict(n=-1), dict(ws=65536, hs=32768, pix=one), dict(wt=46341, ht=46341)):
        rejected(b"bad size", **kw)
    rejected(b"without pixel indices", n=100)
    rejected(b"come together", ls=one, nc=4)
    rejected(b"come together", lt=one, nc=4)
    rejected(b"agree needs label images", agree=one, nc=4)
    for nc in (0, -3, 8193):
        rejected(b"n_classes must be in 1 .. 8192", ls=one, lt=one, nc=nc, agree=one)
    for kw in (dict(ta=-1.0), dict(tr=-0.5), dict(ta=math.inf), dict(tr=math.nan)):
        rejected(b"tolerances", **kw)
    rejected(b"8-byte aligned", uv=ctypes.c_void_p(20))
    # an empty pixel list is a no-op, before the pointer checks
    assert call(n=0, pix=null, ds=null, match=null, uv=null, stats=null) == 0
    assert call(n=0, ms=5) == -1                                   # ... but not before the model check


def _maps(cam, **extra):
    m = {"depth_1": torch.ones(cam.height, cam.width), "semantic_1": torch.zeros(cam.height, cam.width, 4),
         "valid": torch.ones(cam.height, cam.width, dtype=torch.bool)}
    m.update(extra)
    return m


def test_consistency_refuses_bad_views():
    c2w = torch.as_tensor(EYE).reshape(3, 4)
    good = (PIN, c2w, _maps(PIN))
    for bad in (None, (PIN, c2w), (PIN, c2w, _maps(PIN), 1)):
        with pytest.raises(ValueError, match=r"must be \(camera, c2w, maps\)"):
            consistency.reproject(bad, good)
        with pytest.raises(ValueError, match=r"view_b must be \(camera, c2w, maps\)"):
            consistency.reproject(good, bad)
    with pytest.raises(ValueError, match="must be a dict"):
        consistency.reproject((PIN, c2w, torch.ones(48, 64)), good)
    with pytest.raises(ValueError, match="hold no depth image"):
        consistency.reproject((PIN, c2w, {"rgb_1": torch.ones(48, 64, 3)}), good)
    with pytest.raises(ValueError, match="hold no 'depth_7'"):
        consistency.reproject(good, good, depth="depth_7")
    with pytest.raises(ValueError, match="must be a GPU tensor"):
        consistency.reproject((PIN, c2w, {"depth": np.ones((48, 64))}), good)
    with pytest.raises(ValueError, match=r"depth image of view_b is \(48, 64\), its camera \(96, 96\)"):
        consistency.reproject(good, (FISH, c2w, _maps(PIN)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consistency.reproject(good, (FISH, c2w, _maps(FISH)))
    with pytest.raises(ValueError, match="finite and >= 0"):
        consistency.reproject(good, good, tol=(0.0, -1.0))
    assert consistency.depth_key({"depth_0": 0, "depth_1": 1}) == "depth_1" and consistency.depth_key({"depth_0": 0}) == "depth_0"
    assert consistency.depth_key({"depth": 0, "x": 1}) == "depth"
    assert (consistency.NOTHING, consistency.LEFT_VIEW, consistency.UNKNOWN, consistency.OCCLUDED) == (-1, -2, -3, -4)


def test_warp_equals_numpy_indexing():
    g = np.random.default_rng(0)
    match = g.integers(-4, 96 * 96, (48, 64)).astype(np.int32)
    for img in (g.normal(size=(96, 96)).astype(np.float32), g.integers(0, 45, (96, 96)).astype(np.int32), g.normal(size=(96, 96, 3)).astype(np.float32)):
        for fill in (0, -1):
            got = consistency.warp(torch.as_tensor(img), torch.as_tensor(match), fill).numpy()
            flat = img.reshape(96 * 96, *img.shape[2:])
            want = np.where((match >= 0).reshape(48, 64, *([1] * (img.ndim - 2))), flat[np.maximum(match, 0)], np.asarray(fill, img.dtype))
            assert got.dtype == img.dtype and np.array_equal(got, want)
    flat_match = torch.as_tensor(match.reshape(-1)[:100])
    assert tuple(consistency.warp(torch.as_tensor(img), flat_match).shape) == (100, 3)
    with pytest.raises(ValueError, match="image_b must be"):
        consistency.warp(torch.zeros(5), torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="image_b must be"):
        consistency.warp(img, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="match must be"):
        consistency.warp(torch.zeros(4, 4), torch.zeros(5))


def test_evaluate_pair_refuses_bad_arguments():
    c2w = torch.as_tensor(EYE).reshape(3, 4)
    ev = Evaluator(n_classes=4)
    out = _maps(PIN)
    with pytest.raises(ValueError, match="no classes"):
        Evaluator().evaluate_pair(out, (PIN, c2w), out, (PIN, c2w))
    with pytest.raises(ValueError, match="view_a must be the dict"):
        ev.evaluate_pair(None, (PIN, c2w), out, (PIN, c2w))
    with pytest.raises(ValueError, match="view_b holds no semantic map"):
        ev.evaluate_pair(out, (PIN, c2w), {"depth_1": out["depth_1"]}, (PIN, c2w))
    for bad in (PIN, (PIN,), (PIN, c2w, out, 0)):
        with pytest.raises(ValueError, match=r"view_a must be \(camera, c2w\) or \(camera, c2w, maps\)"):
            ev.evaluate_pair(out, bad, out, (PIN, c2w))
    with pytest.raises(ValueError, match="hold no 'depth_1'"):
        ev.evaluate_pair({"semantic_1": out["semantic_1"]}, (PIN, c2w), out, (PIN, c2w))
    with pytest.raises(ValueError, match="hold no depth image"):
        ev.evaluate_pair(out, (PIN, c2w, {"rgb": 0}), out, (PIN, c2w))
    with pytest.raises(ValueError, match=r"depth image of view_b is \(48, 64\), its camera \(96, 96\)"):
        ev.evaluate_pair(out, (PIN, c2w), out, (FISH, c2w))
    with pytest.raises(ValueError, match=r"semantic map of view_a is \(48, 64, 4\), expected \(48, 64, 5\)"):
        Evaluator(n_classes=5).evaluate_pair(out, (PIN, c2w), out, (PIN, c2w))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.evaluate_pair(out, (PIN, c2w), out, (PIN, c2w))
    assert ev.mc_agree is None and ev.mc_stats is None and ev.summarize() == {}


def test_summarize_without_pairs_is_unchanged_and_with_pairs_gains_three_keys():
    ev = Evaluator(n_classes=3)
    assert ev.summarize() == {}
    ev.conf = torch.tensor([[5, 1, 0], [0, 2, 0], [0, 0, 0]])
    ev.mse = [torch.tensor(0.01), torch.tensor(0.04)]
    ev.pq = torch.tensor([[0.8, 1.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]], dtype=torch.float64)
    out = ev.summarize()
    assert set(out) == {"psnr", "mse", "iou", "miou", "pixel_acc", "pq_per_class", "pq", "sq", "rq"}
    assert ev.summarize() == {}
    # pairs seen: mc = trace / sum, per class = diagonal / row sum (NaN for a class no source pixel had), the five counts
    ev.mc_agree = torch.tensor([[6, 2, 0], [1, 3, 0], [0, 0, 0]])
    ev.mc_stats = torch.tensor([12, 1, 2, 3, 4])
    ev.conf = torch.tensor([[5, 1, 0], [0, 2, 0], [0, 0, 0]])
    out = ev.summarize()
    assert set(out) == {"iou", "miou", "pixel_acc", "mc", "mc_per_class", "mc_stats"}
    assert out["mc"] == 9 / 12 and out["mc_stats"] == [12, 1, 2, 3, 4]
    assert out["mc_per_class"][:2] == [6 / 8, 3 / 4] and math.isnan(out["mc_per_class"][2])
    assert ev.mc_agree is None and ev.mc_stats is None and ev.summarize() == {}         # the reset covers the new accumulators
    ev.mc_agree, ev.mc_stats = torch.zeros(3, 3, dtype=torch.int64), torch.tensor([0, 5, 0, 0, 0])
    out = ev.summarize()
    assert math.isnan(out["mc"]) and all(math.isnan(v) for v in out["mc_per_class"]) and out["mc_stats"] == [0, 5, 0, 0, 0]
