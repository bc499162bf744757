"""Fisheye cameras on an MI355X: k_gen_rays_fisheye / k_project_points against tests/_camera_ref.py, the existing stage
kernels on rays no pinhole can make, Renderer.render_view, and a convention check that ties the two camera models together.

Bounds (all measured on the CPU, whole 1400 x 1400 frames, recorded in tests/_camera_ref.py "measured figures" and
re-measured by tests/test_camera_ref.py; the kernels must equal the float32 restatements BIT FOR BIT, so the 2 x margin only
guards against a different pixel set):
  max |d32 - d64| per direction component: kitti 9.04e-5, strong 1.35e-4 (both at the rim, where sqrt(disc) is near 0),
      xi1 2.83e-7, xi0 1.94e-7;
  pixels with |disc64| < 1e-4, where validity may differ from float64 and which are left out: kitti 259 (0.013 % of the
      frame), strong 332 (0.017 %), xi1 and xi0 none -- capped at 0.05 %; measured: validity differs at no pixel;
  all-float32 round trip project(o + t d) - pixel: 3.7e-4 .. 4.9e-4 px for the poses near the origin, and for the pose 42 m
      from it 1.96e-2 / 1.47e-3 / 3.7e-4 px at t = 0.5 / 7 / 90 (the float32 rounding of o + t d).
"""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _camera_ref as cr
from oracle import c_oracle as co
from oracle import torch_oracle as to
from panopticnerf_amd import Equirect, Fisheye, FrameSet, Pinhole, make_network, make_renderer, ops, synthetic

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import config_case  # noqa: E402

pytestmark = pytest.mark.gpu

W = H = cr.FRAME
_REF64 = {}


def N_(t):
    return t.detach().cpu().numpy()


def _ref64(name):
    """camera-space unproject64 of the whole frame, once per parameter set"""
    if name not in _REF64:
        _REF64[name] = cr.unproject64(cr.PARAM_SETS[name], W, H)
    return _REF64[name]


def _check_invalid_rays(rays, valid, c2w):
    bad = valid == 0
    assert np.isfinite(rays).all()
    assert (rays[bad, 3:] == 0.0).all() and (rays[:, :3] == np.asarray(c2w, dtype=np.float32).reshape(3, 4)[:, 3]).all()


# ------------------------------------------------------------------------------------------- 1 + 2: ray generation
@pytest.mark.parametrize("pname", list(cr.POSES))
@pytest.mark.parametrize("name", list(cr.PARAM_SETS))
def test_gen_rays_fisheye_whole_frame_bit_for_bit_and_against_float64(dev, name, pname):
    """1,960,000 rays on at most 256 CUs x 8 workgroups x 256 threads: every thread takes 3 or 4 rays (grid-stride)."""
    cam, c2w = cr.PARAM_SETS[name], cr.POSES[pname]
    rays, valid = ops.gen_rays_fisheye(cam, c2w, W, H, 0.5, 100.0, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert W * H >= 3 * cus * 8 * 256
    rays, valid = N_(rays), N_(valid)
    want, wvalid = cr.unproject32(cam, c2w, W, H, 0.5, 100.0)
    assert np.array_equal(valid, wvalid)
    assert np.array_equal(rays.view(np.uint32), want.view(np.uint32))
    _check_invalid_rays(rays, valid, c2w)
    # against float64
    d64, ok64, disc = _ref64(name)
    d64 = d64 @ c2w[:, :3].T
    near_rim = np.abs(disc) < cr.NEAR_RIM_DISC
    share = near_rim.mean()
    flips = (ok64 != (valid != 0))
    print("%s / %s: %d pixels near the rim left out of the validity check (%.4f %% of the frame), validity differs at %d"
          % (name, pname, int(near_rim.sum()), 100.0 * share, int(flips.sum())))
    assert share <= cr.NEAR_RIM_CAP
    assert not (flips & ~near_rim).any()
    both = ok64 & (valid != 0)
    err = np.abs(rays[both, 3:6] - d64[both]).max()
    print("%s / %s: max |d - d64| = %.3e (CPU figure %.3e, bound 2 x)" % (name, pname, err, cr.F32_VS_F64[name]))
    assert err <= 2.0 * cr.F32_VS_F64[name]
    assert np.abs(np.sqrt((rays[both, 3:6].astype(np.float64) ** 2).sum(-1)) - 1.0).max() < 1e-6       # unit length: 4 ulp of float32


@pytest.mark.parametrize("name", list(cr.PARAM_SETS))
def test_gen_rays_fisheye_pixel_subsets_bit_for_bit(dev, name):
    cam = cr.PARAM_SETS[name]
    _, _, disc = _ref64(name)
    rng = np.random.default_rng(11)
    rim = np.flatnonzero(np.abs(disc) < 1e-3)
    parts = [np.array([0, W * H - 1, W - 1, W * (H - 1)]), rng.integers(0, W * H, 5000), np.full(70, 123456), np.arange(700 * W, 700 * W + 300)]
    if rim.size:
        parts.append(rim)               # every pixel near the rim, both sides of it
    pix = np.concatenate(parts)
    pix = pix[rng.permutation(pix.size)].astype(np.int32)               # unsorted, repeated
    for pname, c2w in cr.POSES.items():
        for want_valid in (True, False):
            rays, valid = ops.gen_rays_fisheye(cam, c2w, W, H, 0.25, 80.0, pix=torch.as_tensor(pix).to(dev), want_valid=want_valid)
            want, wvalid = cr.unproject32(cam, c2w, W, H, 0.25, 80.0, pix=pix)
            assert np.array_equal(N_(rays).view(np.uint32), want.view(np.uint32))
            if want_valid:
                assert np.array_equal(N_(valid), wvalid)
                _check_invalid_rays(N_(rays), N_(valid), c2w)
            else:
                assert valid is None
    if rim.size:
        assert 0 < wvalid[np.isin(pix, rim)].mean() < 1               # the rim set holds valid and invalid pixels
    r0, v0 = ops.gen_rays_fisheye(cam, cr.POSES["identity"], W, H, 0.5, 100.0, pix=torch.zeros(0, dtype=torch.int32, device=dev))
    assert r0.shape == (0, 8) and v0.shape == (0,)
    one = ops.gen_rays_fisheye(cam, cr.POSES["identity"], W, H, 0.5, 100.0, pix=torch.tensor([5], dtype=torch.int32, device=dev))[0]
    assert np.array_equal(N_(one), cr.unproject32(cam, cr.POSES["identity"], W, H, 0.5, 100.0, pix=[5])[0])


# ------------------------------------------------------------------------------------------- 3: projection
def _points(seed, P, c2w):
    """points all around a camera at c2w: every direction, ranges 0.05 .. 200, the camera centre itself, far and huge ones"""
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (P, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    p = c2w[:, 3] + d * np.exp(rng.uniform(np.log(0.05), np.log(200.0), (P, 1)))
    p[:4] = c2w[:, 3]                                   # |p_cam| = 0
    p[4:8] = c2w[:, 3] + c2w[:, :3] @ np.array([0.0, 0.0, -3.0])      # straight behind
    p[8:12] = [1e30, -1e30, 1e30]
    p[12:16] = c2w[:, 3] + c2w[:, :3] @ np.array([1e-30, 0.0, 0.0])
    return p.astype(np.float32)


@pytest.mark.parametrize("pname", list(cr.POSES))
def test_project_points_bit_for_bit(dev, pname):
    c2w = cr.POSES[pname]
    w2c = cr.invert_pose(c2w).astype(np.float32)
    pts = _points(5, 300001, c2w)
    cams = [("pinhole", (552.554261, 552.554261, 682.049453, 238.769549), 1408, 376)] + [("fisheye", cr.PARAM_SETS[n], W, H) for n in cr.PARAM_SETS]
    for model, cam, w, h in cams:
        uv, rng, valid = ops.project_points(model, cam, w2c, w, h, torch.as_tensor(pts).to(dev))
        wuv, wrng, wvalid = cr.project32(cr.PINHOLE if model == "pinhole" else cr.FISHEYE, cam, w2c, w, h, pts)
        uv, rng, valid = N_(uv), N_(rng), N_(valid)
        assert np.isfinite(uv).all() and not np.isnan(rng).any()
        assert np.array_equal(valid, wvalid)
        assert np.array_equal(uv.view(np.uint32), wuv.view(np.uint32)) and np.array_equal(rng.view(np.uint32), wrng.view(np.uint32))
        assert 0.02 < valid.mean() < 0.98
        # valid means what it says: in the domain (float64) and inside the image, up to points within 1e-3 px of a border
        uv64, _, ok64 = cr.project64(cr.PINHOLE if model == "pinhole" else cr.FISHEYE, cam, cr.invert_pose(c2w), w, h, pts.astype(np.float64))
        differ = ok64 != (valid != 0)
        print("%s %s: %.1f %% valid, validity differs from float64 at %d of %d points" % (model, pname, 100 * valid.mean(), int(differ.sum()), len(pts)))
        assert differ.mean() < 1e-3
    e = ops.project_points("fisheye", cr.KITTI_FISHEYE, w2c, W, H, torch.zeros((0, 3), device=dev))
    assert e[0].shape == (0, 2) and e[1].shape == (0,) and e[2].shape == (0,)


@pytest.mark.parametrize("name", list(cr.PARAM_SETS))
def test_round_trip_on_the_gpu_returns_the_pixel(dev, name):
    cam = Fisheye(*cr.PARAM_SETS[name], W, H)
    i, j = cr.pixel_grid(W, H)
    for pname, c2w in cr.POSES.items():
        rays, valid = ops.gen_rays_fisheye(cam.cam, c2w, W, H, 0.5, 100.0, device=dev)
        ok = N_(valid) != 0
        for t in (0.5, 7.0, 90.0):
            pts = ops.points(rays, torch.full((W * H, 1), t, device=dev)).reshape(-1, 3)        # o + d * t (pnr_points)
            uv, rng, pv = cam.project(pts, cr.invert_pose(c2w))
            uv, rng, pv = N_(uv), N_(rng), N_(pv)
            assert pv[ok].all()
            e = np.maximum(np.abs(uv[ok, 0] - i[ok]), np.abs(uv[ok, 1] - j[ok])).max()
            print("%s / %s t = %4.1f: round trip max %.3e px (CPU figure %.3e, bound 2 x)" % (name, pname, t, e, cr.ROUND_TRIP32_PX[(pname, t)]))
            assert e <= 2.0 * cr.ROUND_TRIP32_PX[(pname, t)]
            assert np.abs(rng[ok] - t).max() <= 1e-5 * max(t, 50.0)          # |o + t d - o|: ulp(|o|) = 3.8e-6 at the far pose


def test_pinhole_projection_inverts_gen_rays(dev):
    pin = Pinhole(552.554261, 552.554261, 682.049453, 238.769549, 1408, 376)
    c2w = cr.POSES["sideways"]
    rays = pin.rays(c2w, 0.5, 100.0, device=dev)
    i, j = cr.pixel_grid(1408, 376)
    for t in (0.5, 7.0, 90.0):
        pts = ops.points(rays, torch.full((rays.shape[0], 1), t, device=dev)).reshape(-1, 3)
        uv, rng, ok = pin.project(pts, cr.invert_pose(c2w))
        uv = N_(uv)
        assert N_(ok).all()
        # (i - cx)/fx and back: two roundings of a value below 1408 px -> a few ulp(1024) = 1.2e-4 px
        assert max(np.abs(uv[:, 0] - i).max(), np.abs(uv[:, 1] - j).max()) < 1e-3
        d = N_(rays[:, 3:6]).astype(np.float64)
        assert np.abs(N_(rng) - t * np.sqrt((d * d).sum(-1))).max() < 1e-4 * t          # range, not z-depth: t |d|


# ------------------------------------------------------------------------------------------- 4: the stage kernels
def _boxes_around(seed, M, origin):
    """oriented boxes on every side of `origin` (beside and behind a camera standing there): (M, 15), ids (M, 2)"""
    g = np.random.default_rng(seed)
    ang = g.uniform(0, 2 * np.pi, M)
    dist = g.uniform(4.0, 40.0, M)
    ctr = np.stack([origin[0] + dist * np.cos(ang), origin[1] + g.uniform(-3, 3, M), origin[2] + dist * np.sin(ang)], -1)
    yaw = g.uniform(0, np.pi, M)
    c, s, z0, o1 = np.cos(yaw), np.sin(yaw), np.zeros(M), np.ones(M)
    rot = np.stack([c, z0, s, z0, o1, z0, -s, z0, c], -1)
    ext = g.uniform(1.0, 5.0, (M, 3))
    ids = np.stack([g.integers(0, 45, M), g.integers(0, 32, M)], -1).astype(np.int32)
    return np.concatenate([ctr, rot, ext], -1).astype(np.float32), ids


@pytest.mark.parametrize("pname", ["sideways", "oblique"])
def test_stage_kernels_on_rays_no_pinhole_can_make(dev, pname):
    """ray_setup / bbox_hits / sample_labels / stratified / points on fisheye rays, d_cam.z < 0 included, against the C oracle."""
    c2w = cr.POSES[pname]
    rng = np.random.default_rng(3)
    pix = torch.as_tensor(rng.integers(0, W * H, 6000).astype(np.int32)).to(dev)
    rays, valid = ops.gen_rays_fisheye(cr.KITTI_FISHEYE, c2w, W, H, 0.5, 60.0, pix=pix)
    rays = rays[valid != 0].contiguous()
    r = N_(rays)
    back = (r[:, 3:6].astype(np.float64) @ c2w[:, 2]) < 0.0                     # d_cam.z < 0
    assert back.mean() > 0.05
    box, ids = _boxes_around(7, 48, c2w[:, 3])
    tb, ti = torch.as_tensor(box).to(dev), torch.as_tensor(ids).to(dev)
    for mh in (4, 8):
        a = ops.bbox_hits(rays, tb, mh)
        b = co.bbox_hits(r, box, mh)
        for x, y in zip(a, b):
            assert np.array_equal(N_(x), y)
    print("%s: %d rays, %d with d_cam.z < 0, of which %d hit a box" % (pname, len(r), int(back.sum()), int((b[2][back] > 0).sum())))
    assert (b[2][back] > 0).mean() > 0.05 and (b[2][~back] > 0).mean() > 0.05
    for N, lindisp in ((64, False), (32, True)):
        tr = rng.random((len(r), N)).astype(np.float32)
        for t in (None, tr):
            z = ops.stratified(rays, N, lindisp, None if t is None else torch.as_tensor(t).to(dev))
            zo = co.stratified(r, N, lindisp, t)
            assert np.array_equal(N_(z), zo)
            assert np.array_equal(N_(ops.points(rays, z)), co.points(r, zo))
            ls, li = ops.sample_labels(z, *a, ti)
            lso, lio = co.sample_labels(zo, *b, ids)
            assert np.array_equal(N_(ls), lso) and np.array_equal(N_(li), lio)
            hits, z2, ls2, li2 = ops.ray_setup(rays, tb, ti, N, 8, lindisp, None if t is None else torch.as_tensor(t).to(dev))
            for x, y in zip(hits, b):
                assert np.array_equal(N_(x), y)
            assert np.array_equal(N_(z2), zo) and np.array_equal(N_(ls2), lso) and np.array_equal(N_(li2), lio)
        assert (lso[back] >= 0).any()


# ------------------------------------------------------------------------------------------- 5: render_view
def _renderer(dev, prec, **extra):
    c, oc, params, _, box, ids = config_case(5)
    cfg = synthetic.baseline_cfg(5, precision=prec, **extra)
    net = make_network(cfg).eval()
    net.nerf_0.load_state_dict(params["coarse"])
    net.nerf_1.load_state_dict(params["fine"])
    return c, oc, params, box, ids, make_renderer(cfg, net.to(dev))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_render_view_fisheye(dev, prec):
    c, oc, params, box, ids, rend = _renderer(dev, prec)
    box, ids = synthetic.random_boxes(32, 45, 32)
    cam, c2w = synthetic.fisheye_camera(96 / 1400)
    bx, bi = box.to(dev), ids.to(dev)
    with torch.no_grad():
        out = rend.render_view(cam, c2w, 0.5, 100.0, bbox=bx, bbox_ids=bi)
        pix = cam.valid_pix(dev)
        assert pix.dtype == torch.int32 and 0.8 * 96 * 96 < pix.numel() < 0.9 * 96 * 96 and bool((pix[1:] > pix[:-1]).all())
        ref = rend.render({"rays": cam.rays(c2w, 0.5, 100.0, pix=pix), "bbox": bx, "bbox_ids": bi})
        assert cam.valid_pix(dev) is pix and cam.valid_pix("cuda:%d" % dev.index) is pix          # cached: the same tensor object
        again = rend.render_view(cam, c2w, 0.5, 100.0, bbox=bx, bbox_ids=bi)
    assert set(out) == set(ref) | {"valid"}
    assert out["valid"].dtype == torch.bool and out["valid"].shape == (96, 96) and int(out["valid"].sum()) == pix.numel()
    vmask = out["valid"].reshape(-1)
    assert torch.equal(torch.nonzero(vmask).reshape(-1), pix.long())
    for k, v in ref.items():
        img = out[k]
        assert img.shape[:2] == (96, 96) and img.shape[2:] == v.shape[1:] and img.dtype == v.dtype, k
        flat = img.reshape(96 * 96, *v.shape[1:])
        assert torch.equal(flat[pix.long()], v), k
        assert not flat[~vmask].any(), k
        assert torch.equal(again[k], img), k
    assert bool((out["fix_semantic_1"].reshape(96 * 96, -1)[pix.long()].sum(-1) > 0).any())              # the boxes are seen
    # a frame of several chunks equals the one-chunk frame
    _, _, _, _, _, small = _renderer(dev, prec, chunk_size=2048)
    with torch.no_grad():
        chunked = small.render_view(cam, c2w, 0.5, 100.0, bbox=bx, bbox_ids=bi)
    for k in out:
        assert torch.equal(chunked[k], out[k]), k
    # a user mask removes exactly its pixels
    mask = np.ones((96, 96), bool)
    mask[60:, :] = False
    mask[10, 20] = False
    mcam, _ = synthetic.fisheye_camera(96 / 1400, mask=mask)
    with torch.no_grad():
        mout = rend.render_view(mcam, c2w, 0.5, 100.0, bbox=bx, bbox_ids=bi)
    keep = torch.as_tensor(mask).to(dev)
    assert torch.equal(mout["valid"], out["valid"] & keep) and int(mout["valid"].sum()) == mcam.valid_pix(dev).numel() < pix.numel()
    for k in ("rgb_1", "depth_1", "semantic_1", "z_vals_1"):
        kk = keep.reshape(96, 96, *([1] * (out[k].dim() - 2)))
        assert torch.equal(mout[k], out[k] * kk), k
    # under autograd it raises by name
    for p in rend.net.parameters():
        p.requires_grad_(True)
    with pytest.raises(RuntimeError, match="render_view is inference only"):
        rend.render_view(cam, c2w, 0.5, 100.0)
    # against the oracle on identical stage inputs: the method and the bounds of test_gpu_configs.py::test_render_baseline_configs
    with torch.no_grad():
        zc = cam.rays(c2w, 0.5, 100.0, pix=pix)[:, 3:6] @ c2w[:, 2].to(dev)               # d_cam.z of every valid ray
        sel = torch.cat([pix[:: pix.numel() // 16][:16], pix[torch.argsort(zc)[:8]]]).contiguous()      # 16 across the frame + the 8 that look back farthest
        rays = cam.rays(c2w, 0.5, 100.0, pix=sel)
        o24 = rend.render({"rays": rays[None], "bbox": bx, "bbox_ids": bi})
    rays = rays.cpu()
    assert int(((rays[:, 3:6].double() @ c2w[:, 2].double()) < 0).sum()) >= 8
    hits = co.bbox_hits(rays.numpy(), box.numpy(), 8)
    for lv in (0, 1):
        z = o24[f"z_vals_{lv}"][0].cpu()
        raw = to.run_network(params["coarse" if lv == 0 else "fine"], oc, rays, z, emulate_bf16=(prec == "bf16"))
        ls, li = (torch.tensor(a) for a in co.sample_labels(z.numpy(), *hits, ids.numpy()))
        want = to.raw2outputs(raw, z, rays[:, 3:6], 45, 32, None, ls, li)
        ok = torch.ones(24, dtype=torch.bool) if prec == "fp32" else raw[:, -1, 3].abs() > 2e-2
        print("fisheye %s level %d: %d of 24 rays excluded (|sigma_last| <= 2e-2)" % (prec, lv, 24 - int(ok.sum())))
        assert ok.sum() >= 20
        tol = 1e-4 if prec == "fp32" else 1e-2
        for k in ("rgb", "acc", "weights", "semantic", "instance", "fix_semantic", "fix_instance"):
            err = (o24[f"{k}_{lv}"][0].cpu() - want[k])[ok].abs().max().item()
            print("    %s_%d: %.3e" % (k, lv, err))
            assert err < tol, (prec, k, lv, err)
        derr = (o24[f"depth_{lv}"][0].cpu() - want["depth"])[ok].abs().max().item()
        assert derr < tol * 100.0, (prec, "depth", lv, derr)


def test_render_view_pinhole_equals_the_plain_render(dev):
    _, _, _, box, ids, rend = _renderer(dev, "bf16", chunk_size=4096)
    pin = Pinhole(40.0, 41.0, 63.5, 35.5, 128, 72)
    c2w = torch.as_tensor(cr.POSES["sideways"], dtype=torch.float32)
    bx, bi = box.to(dev), ids.to(dev)
    with torch.no_grad():
        out = rend.render_view(pin, c2w, 0.5, 100.0, bbox=bx, bbox_ids=bi)
        ref = rend.render({"rays": pin.rays(c2w, 0.5, 100.0, device=dev), "bbox": bx, "bbox_ids": bi})
    assert bool(out["valid"].all()) and set(out) == set(ref) | {"valid"}
    assert torch.equal(pin.rays(c2w, 0.5, 100.0, pix=pin.valid_pix(dev)), pin.rays(c2w, 0.5, 100.0, device=dev))
    for k, v in ref.items():
        assert torch.equal(out[k], v.reshape(72, 128, *v.shape[1:])), k


# ------------------------------------------------------------------------------------------- 6: one convention for both cameras
def _cross_camera_figures(raysF, depthF, semF, depthP, semP, c2w, project):
    """fisheye pixels whose ray falls inside the pinhole image: the point o + range d projected into the pinhole image, its
    z-depth (range times d_cam.z) against the pinhole depth at the nearest pixel, and the semantic argmax of the two."""
    pts = raysF[:, :3] + raysF[:, 3:6] * depthF[:, None]
    uv, rng, ok = project(pts)
    ok = ok != 0
    u = np.floor(uv[ok, 0] + 0.5).astype(np.int64)
    v = np.floor(uv[ok, 1] + 0.5).astype(np.int64)
    zc = raysF[ok, 3:6].astype(np.float64) @ np.asarray(c2w, dtype=np.float64)[:, 2]
    zdepth = rng[ok] * zc
    rel = np.abs(zdepth - depthP[v, u]) / depthP[v, u]
    agree = (semF[ok].argmax(-1) == semP[v, u].argmax(-1)).mean()
    return int(ok.sum()), float(rel.mean()), float(agree)


def test_fisheye_and_pinhole_share_axes_signs_and_depth_convention(dev):
    """A pinhole and a fisheye camera at ONE pose, fp32, the synthetic field of synthetic.trained_like_.
    (a) Geometry: the point o + t d of a fisheye ray, projected into the pinhole image, lands on a pixel whose OWN pinhole ray
    points the same way: the angle between the two is at most that of half a pixel diagonal, atan(0.71 / f) -- nearest-pixel
    rounding and nothing else.  A flipped or swapped axis in either model misses this by tens of degrees.
    (b) Maps: depth (fisheye range converted to z-depth with d_cam.z) and the semantic argmax against the pinhole render at
    the nearest pixel.  This checks the depth convention, not precision: the bound is what torch_oracle.render_rays gives for
    the same comparison on the same rays, times 2.  Measured with the oracle on the CPU for this scene: mean relative depth
    difference 3.98e-2 (the two cameras sample a ray at different positions: 64 samples over 30 m of fog with a 3 m mean free
    path), argmax agreement 0.9973 over 1,102 fisheye pixels; range taken for z-depth gives 1.32e-1.  The field is too uniform
    for a flipped axis to show in (b) (measured: 3.7e-2 .. 4.0e-2 with x or y flipped) -- that is what (a) is for."""
    cfg = NS(D=4, W=128, skips=[2], N_samples=32, N_importance=32, num_classes=19, num_instances=0, precision="fp32")
    torch.manual_seed(3)
    net = make_network(cfg).eval()
    synthetic.trained_like_(net, 0.3)
    rend = make_renderer(cfg, net.to(dev))
    fish, c2w = synthetic.fisheye_camera(96 / 1400, yaw=0.3, origin=(0.5, 1.55, -1.0))
    pin = Pinhole(40.0, 40.0, 31.5, 23.5, 64, 48)
    w2c = cr.invert_pose(c2w.numpy())
    with torch.no_grad():
        outF = rend.render_view(fish, c2w, 0.5, 30.0)
        outP = rend.render_view(pin, c2w, 0.5, 30.0)
        pix = fish.valid_pix(dev)
        raysF = fish.rays(c2w, 0.5, 30.0, pix=pix)
        raysP = pin.rays(c2w, 0.5, 30.0, device=dev)
    # (a)
    rF, rP = N_(raysF), N_(raysP).reshape(48, 64, 8)
    for t in (0.5, 7.0):
        uv, _, ok = (N_(x) for x in pin.project(ops.points(raysF, torch.full((rF.shape[0], 1), t, device=dev)).reshape(-1, 3), w2c))
        u, v = np.floor(uv[ok, 0] + 0.5).astype(np.int64), np.floor(uv[ok, 1] + 0.5).astype(np.int64)
        dp = rP[v, u, 3:6].astype(np.float64)
        cosang = (dp * rF[ok, 3:6]).sum(-1) / np.linalg.norm(dp, axis=-1)
        worst = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))).max()
        print("cross-camera geometry t = %.1f: %d fisheye rays inside the pinhole image, worst angle %.3f deg (half a pixel diagonal: %.3f)"
              % (t, int(ok.sum()), worst, np.degrees(np.arctan(0.5 * np.sqrt(2.0) / 40.0))))
        assert ok.sum() > 1000 and worst <= np.degrees(np.arctan(0.5 * np.sqrt(2.0) / 40.0)) * 1.001
    # (b)
    gpu_project = lambda pts: tuple(N_(x) for x in pin.project(torch.as_tensor(pts).to(dev), w2c))
    idx = N_(pix).astype(np.int64)
    got = _cross_camera_figures(rF, N_(outF["depth_1"]).reshape(-1)[idx], N_(outF["semantic_1"]).reshape(96 * 96, -1)[idx],
                                N_(outP["depth_1"]), N_(outP["semantic_1"]), c2w.numpy(), gpu_project)
    # the same comparison by the oracle, on the same rays
    params = {"coarse": {k: v.detach().cpu() for k, v in net.nerf_0.state_dict().items()},
              "fine": {k: v.detach().cpu() for k, v in net.nerf_1.state_dict().items()}}
    oc = to.mlp_config(D=4, W=128, skips=(2,), n_sem=19, n_inst=0)
    with torch.no_grad():
        oF = to.render_rays(params, oc, raysF.cpu(), 32, 32)
        oP = to.render_rays(params, oc, raysP.cpu(), 32, 32)
    cpu_project = lambda pts: cr.project32(cr.PINHOLE, pin.intr, w2c, 64, 48, pts)
    want = _cross_camera_figures(rF, oF["depth_1"].numpy(), oF["semantic_1"].numpy(), oP["depth_1"].numpy().reshape(48, 64),
                                 oP["semantic_1"].numpy().reshape(48, 64, -1), c2w.numpy(), cpu_project)
    print("cross-camera maps: GPU %d pixels, mean relative depth difference %.3e, argmax agreement %.4f; oracle %d, %.3e, %.4f" % (got + want))
    assert got[0] > 1000 and want[0] > 1000
    assert got[1] <= 2.0 * want[1]
    assert 1.0 - got[2] <= 2.0 * (1.0 - want[2])


# ------------------------------------------------------------------------------------------- 7: stream capture
def test_camera_ops_replay_from_a_captured_graph(dev):
    cam, c2w = cr.KITTI_FISHEYE, cr.POSES["oblique"]
    w2c = cr.invert_pose(c2w)
    g0 = torch.Generator().manual_seed(2)
    pix_a = torch.randint(0, W * H, (50000,), generator=g0, dtype=torch.int32).to(dev)
    pix_b = torch.randint(0, W * H, (50000,), generator=g0, dtype=torch.int32).to(dev)
    static_pix = pix_a.clone()

    def chain(p):
        rays, valid = ops.gen_rays_fisheye(cam, c2w, W, H, 0.5, 100.0, pix=p)
        pts = ops.points(rays, rays[:, 7:8].contiguous()).reshape(-1, 3)              # o + far * d, on the same stream
        return (rays, valid) + ops.project_points("fisheye", cam, w2c, W, H, pts)

    chain(static_pix)                                     # warm call: module loading is not capturable
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        static_out = chain(static_pix)
    static_pix.copy_(pix_b)
    g.replay()
    torch.cuda.synchronize()
    got = [v.clone() for v in static_out]
    ref = chain(pix_b)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], chain(pix_a)[0])


# ------------------------------------------------------------------------------------------- every caller of pnr_camera_ray
def _rotation(axis, angle):
    """a general rotation (Rodrigues, float64)"""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


_SMALL = {   # 13 x 7: odd, no multiple of the wave size; the fisheye's rim (xi > 1: r^2 = 1/(xi^2 - 1) = 0.26) leaves the corners dark
    "pinhole": lambda: Pinhole(11.0, 10.5, 6.2, 3.1, 13, 7),
    "fisheye": lambda: Fisheye(2.2, 0.01, 0.001, 8.0, 7.5, 6.2, 3.1, 13, 7),
    "equirect": lambda: Equirect(13, 7, lon=(-100.0, 140.0), lat=(60.0, -50.0)),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("model", list(_SMALL))
def test_every_ray_maker_writes_the_rays_of_camera_rays_bit_for_bit(dev, model):
    """The whole frame of Camera.rays against the pixel list, k_sample_batch and the rays k_reproject lifts: bitwise only."""
    from panopticnerf_amd import camera as camera_mod
    cam = _SMALL[model]()
    n = cam.width * cam.height
    c2w = torch.tensor(np.concatenate([_rotation((1.0, 2.0, 3.0), 0.7), [[0.4], [-1.3], [2.1]]], 1), dtype=torch.float32)
    full = cam.rays(c2w, 0.5, 20.0, device=dev)
    assert tuple(full.shape) == (n, 8)
    lens = torch.zeros(n, dtype=torch.bool, device=dev)
    lens[cam.valid_pix(dev).long()] = True
    assert bool(lens.all()) == (model != "fisheye") and bool(lens.any())
    # 1: the pixel list
    listed = cam.rays(c2w, 0.5, 20.0, pix=torch.arange(n, dtype=torch.int32, device=dev))
    assert torch.equal(_bits(listed), _bits(full))
    # 2: a one-frame FrameSet
    frames = FrameSet(dev, capacity=1)
    frames.add(cam, c2w, 0.5, 20.0, torch.zeros((cam.height, cam.width, 3), dtype=torch.uint8))
    batch = frames.sample(512)
    pix = batch["pix"].long()
    assert bool(lens[pix].all()) and pix.unique().numel() > n // 4
    assert torch.equal(_bits(batch["rays"][0]), _bits(full[pix]))
    # 3: reproject with depth 1 lifts o + d; the target is the same camera, moved and turned
    c2w_t = torch.tensor(np.concatenate([_rotation((0.0, 1.0, 0.2), 0.5) @ _rotation((1.0, 2.0, 3.0), 0.7), [[0.5], [-1.2], [2.0]]], 1),
                         dtype=torch.float32)
    w2c_t = camera_mod.invert_pose(c2w_t)
    res = ops.reproject(cam, c2w, torch.ones((cam.height, cam.width), device=dev), cam, w2c_t, want=("match", "uv"))
    uv, _, valid = cam.project(full[:, :3] + full[:, 3:6], w2c_t)
    match = res["match"]
    assert torch.equal(match[~lens], torch.full_like(match[~lens], -1)) and not bool(res["uv"][~lens].any())
    assert torch.equal(_bits(res["uv"][lens]), _bits(uv[lens]))
    assert torch.equal(match[lens] >= 0, valid[lens]) and torch.equal(match[lens] == -2, ~valid[lens])
    assert bool(valid[lens].any()) and not bool(valid[lens].all())          # both codes occur
