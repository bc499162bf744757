"""CPU tests of the camera feature: the float64 reference of the fisheye model is pinned (round trip, closed-form answers,
corrupted variants must fail) BEFORE tests/test_gpu_camera.py uses it; the float32 restatement is measured against it (the
figures the GPU bounds are taken from, tests/_camera_ref.py "measured figures"); and everything of the feature that needs no
GPU: Fisheye.__init__'s refusal, the CPU-tensor refusals, the new PNR_REQUIREs through the raw library."""
import ctypes

import numpy as np
import pytest
import torch

import _camera_ref as cr
from panopticnerf_amd import Fisheye, Pinhole, _lib, ops, synthetic

W = H = cr.FRAME


def _round_trip64(cam, variant=None):
    d, valid, _ = cr.unproject64(cam, W, H, variant=variant)
    i, j = cr.pixel_grid(W, H)
    uv, _, pv = cr.project64(cr.FISHEYE, cam, None, W, H, d[valid])
    return np.maximum(np.abs(uv[:, 0] - i[valid]), np.abs(uv[:, 1] - j[valid])), pv, d[valid]


@pytest.mark.parametrize("name", list(cr.PARAM_SETS))
def test_reference_round_trip_and_unit_length(name):
    err, pv, d = _round_trip64(cr.PARAM_SETS[name])
    print("%s: project64(unproject64(pixel)) max %.2e px over %d valid pixels (%.1f %% of the frame)"
          % (name, err.max(), err.size, 100.0 * err.size / (W * H)))
    assert err.max() < 1e-9
    assert pv.all()                               # every valid pixel's direction projects into the domain and the image
    assert np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max() < 1e-12


def test_reference_known_answers():
    xi, k1, k2, g1, g2, u0, v0 = cr.KITTI_FISHEYE
    # the share of the frame that sees anything, and how far off the axis it sees (the issue's figures)
    d, valid, disc = cr.unproject64(cr.KITTI_FISHEYE, W, H)
    assert abs(valid.mean() - 0.868) < 1e-3
    assert abs(np.degrees(np.arccos(d[valid, 2].min())) - 116.8) < 0.1
    # the principal point looks along the axis
    cam = (xi, k1, k2, g1, g2, 700.0, 650.0)
    d0, v0ok, _ = cr.unproject64(cam, W, H, pix=[650 * W + 700])
    assert v0ok[0] and np.abs(d0[0] - [0.0, 0.0, 1.0]).max() < 1e-15
    # k = 0: a direction at angle theta off the axis lands at radius gamma sin(theta) / (cos(theta) + xi), also behind the camera
    cam = (xi, 0.0, 0.0, 1000.0, 1000.0, 0.0, 0.0)
    for th in (0.1, 0.7, 1.5, 1.9):
        for phi in (0.0, 0.9):
            p = 3.0 * np.array([[np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)]])
            uv, rng, _ = cr.project64(cr.FISHEYE, cam, None, 10 ** 6, 10 ** 6, p)
            assert abs(np.hypot(*uv[0]) - 1000.0 * np.sin(th) / (np.cos(th) + xi)) < 1e-9 and abs(rng[0] - 3.0) < 1e-12
            assert abs(np.arctan2(uv[0, 1], uv[0, 0]) - phi) < 1e-12
    # xi = 0, k = 0: the normalised pinhole direction, and the pinhole projection
    i, j = cr.pixel_grid(W, H)
    dx, vx, _ = cr.unproject64(cr.XI0_FISHEYE, W, H)
    pin = np.stack([(i - 700.0) / 900.0, (j - 690.0) / 905.0, np.ones(i.shape)], -1)
    assert vx.all() and np.abs(dx - pin / np.linalg.norm(pin, axis=-1, keepdims=True)).max() < 1e-15
    uvp, _, okp = cr.project64(cr.PINHOLE, (900.0, 905.0, 700.0, 690.0), None, W, H, pin * 7.0)
    assert okp.all() and np.abs(uvp - np.stack([i, j], -1)).max() < 1e-9
    # the rim is where r2 = 1 / (xi^2 - 1): disc = 0 there, the ray is tangent (z = -1/xi) and still unit length
    r2 = 1.0 / (xi * xi - 1.0)
    assert abs(1.0 + (1.0 - xi * xi) * r2) < 1e-15
    lam = xi / (r2 + 1.0)
    assert abs(lam - xi + 1.0 / xi) < 1e-15 and abs(lam * lam * r2 + (lam - xi) ** 2 - 1.0) < 1e-15
    near = np.abs(disc) < 1e-3
    assert near.any() and np.abs(d[near & valid, 2] + 1.0 / xi).max() < np.sqrt(1e-3)      # z + 1/xi = sqrt(disc) / (r2 + 1) <= sqrt(disc)
    # a direction behind the rim is outside the projection's domain although z + xi > 0 (it would fold back into the image)
    uv, _, ok = cr.project64(cr.FISHEYE, cr.KITTI_FISHEYE, None, 10 ** 6, 10 ** 6, [[0.6, 0.0, -0.8], [0.9, 0.0, -0.43]])
    assert not ok[0] and ok[1]


@pytest.mark.parametrize("variant", ["sign", "distort", "gamma_swap"])
def test_reference_checks_fail_on_corrupted_models(variant):
    """The round trip that pins the reference is not vacuous: three plausible mistakes miss it by pixels, not by 1e-9."""
    err, pv, d = _round_trip64(cr.KITTI_FISHEYE, variant)
    print("%s: round trip max %.3g px, %d of %d directions leave the domain or the image" % (variant, err.max(), int((~pv).sum()), pv.size))
    assert err.max() > 0.1
    if variant == "sign":
        assert np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max() > 0.1


def _subset(cam):
    """every 5th pixel of every 5th row, and every pixel within |disc64| < 1e-3 of the rim"""
    _, _, disc = cr.unproject64(cam, W, H)
    i, j = cr.pixel_grid(W, H)
    return np.flatnonzero(((i % 5 == 0) & (j % 5 == 0)) | (np.abs(disc) < 1e-3))


@pytest.mark.parametrize("name", list(cr.PARAM_SETS))
def test_float32_restatement_against_float64(name):
    """The figures tests/test_gpu_camera.py takes its bounds from (printed; none may exceed what _camera_ref.py records)."""
    cam = cr.PARAM_SETS[name]
    _, v64, disc = cr.unproject64(cam, W, H)
    share = float((np.abs(disc) < cr.NEAR_RIM_DISC).mean())
    print("%s: %d pixels (%.4f %% of the frame) have |disc64| < 1e-4" % (name, int(round(share * W * H)), 100.0 * share))
    assert share <= cr.NEAR_RIM_SHARE[name] + 1e-12 and share <= cr.NEAR_RIM_CAP
    pix = _subset(cam)
    i, j = cr.pixel_grid(W, H, pix)
    for pname, c2w in cr.POSES.items():
        d64, ok64, dsc = cr.unproject64(cam, W, H, pix=pix, c2w=c2w)
        rays, ok32 = cr.unproject32(cam, c2w, W, H, 0.5, 100.0, pix=pix)
        assert np.isfinite(rays).all()
        flip = ok64 != (ok32 != 0)
        assert not (flip & (np.abs(dsc) >= cr.NEAR_RIM_DISC)).any()
        both = ok64 & (ok32 != 0)
        err = np.abs(rays[both, 3:6] - d64[both]).max()
        print("%s / %s: max |d32 - d64| = %.3e over %d pixels, validity differs at %d" % (name, pname, err, int(both.sum()), int(flip.sum())))
        assert err <= cr.F32_VS_F64[name]
        w2c = cr.invert_pose(c2w)
        for t in (0.5, 7.0, 90.0):
            pts = rays[:, :3] + rays[:, 3:6] * np.float32(t)
            uv, rng, pv = cr.project32(cr.FISHEYE, cam, w2c, W, H, pts)
            ok = ok32 != 0
            e = np.maximum(np.abs(uv[ok, 0] - i[ok]), np.abs(uv[ok, 1] - j[ok])).max()
            print("    t = %4.1f: float32 round trip max %.3e px" % (t, e))
            assert pv[ok].all() and e <= cr.ROUND_TRIP32_PX[(pname, t)]


def test_newton_step_count_leaves_margin():
    """float32 Newton does not reach a bitwise fixed point at every pixel (last-ulp cycles), so the count is judged by the
    distance to float64: at its floor from 4 steps on for both KITTI-360-shaped sets; the kernel runs twice that."""
    assert cr.NEWTON_STEPS == 8
    for name in ("kitti", "strong"):
        cam = cr.PARAM_SETS[name]
        pix = _subset(cam)
        d64, ok64, _ = cr.unproject64(cam, W, H, pix=pix)
        errs = {}
        for steps in (2, 4, 8, 16):
            rays, ok32 = cr.unproject32(cam, cr.POSES["identity"], W, H, 0.5, 100.0, pix=pix, steps=steps)
            both = ok64 & (ok32 != 0)
            errs[steps] = np.abs(rays[both, 3:6] - d64[both]).max()
        print(name, {k: "%.3e" % v for k, v in errs.items()})
        assert errs[2] > 10 * errs[8] and errs[4] <= 2 * errs[8] and errs[16] <= 2 * errs[8] and errs[8] <= 2 * errs[16]


def test_fisheye_refuses_a_polynomial_that_is_not_increasing_up_to_the_rim():
    Fisheye(*cr.KITTI_FISHEYE, W, H)
    Fisheye(*cr.STRONG_FISHEYE, W, H)
    Fisheye(*cr.XI1_FISHEYE, W, H)
    Fisheye(*cr.XI0_FISHEYE, W, H)
    Fisheye(2.2134, -0.5, 0.0, 1336.3, 1335.8, 716.94, 705.76, W, H)          # negative k1, but increasing up to the rim r = 0.51
    with pytest.raises(ValueError, match="not strictly increasing"):
        Fisheye(1.2, -0.9, 0.0, 1336.3, 1335.8, 716.94, 705.76, W, H)         # rim r = 1.51: derivative 1 - 2.7 r^2 < 0 from r = 0.61
    with pytest.raises(ValueError, match="not strictly increasing"):
        Fisheye(2.2134, 3.0, -12.0, 1336.3, 1335.8, 716.94, 705.76, W, H)
    with pytest.raises(ValueError, match="not strictly increasing|never reaches"):
        Fisheye(0.5, -0.9, 0.0, 700.0, 700.0, 700.0, 700.0, W, H)             # no rim (xi < 1): judged up to the image corner
    with pytest.raises(ValueError, match="gamma"):
        Fisheye(2.2, 0.0, 0.0, 0.0, 1335.8, 716.94, 705.76, W, H)
    with pytest.raises(ValueError, match="mask"):
        Fisheye(*cr.KITTI_FISHEYE, W, H, mask=np.ones((3, 3), bool))
    cam, c2w = synthetic.fisheye_camera()
    assert cam.cam == cr.KITTI_FISHEYE and (cam.width, cam.height) == (W, H) and tuple(c2w.shape) == (3, 4)
    small, _ = synthetic.fisheye_camera(96 / 1400)
    assert (small.width, small.height) == (96, 96)


def test_camera_ops_refuse_cpu_tensors_and_devices():
    eye = torch.eye(4)[:3]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gen_rays_fisheye(cr.KITTI_FISHEYE, eye, W, H, 0.5, 100.0, pix=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gen_rays_fisheye(cr.KITTI_FISHEYE, eye, W, H, 0.5, 100.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.project_points("fisheye", cr.KITTI_FISHEYE, eye, W, H, torch.zeros(4, 3))
    with pytest.raises(ValueError, match="model"):
        ops.project_points("equirect", cr.KITTI_FISHEYE, eye, W, H, torch.zeros(4, 3))
    for cam in (Fisheye(*cr.KITTI_FISHEYE, W, H), Pinhole(552.55, 552.55, 682.05, 238.77, 1408, 376)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cam.rays(eye, 0.5, 100.0, device="cpu")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cam.rays(eye, 0.5, 100.0, pix=torch.zeros(4, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cam.valid_pix("cpu")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cam.project(torch.zeros(4, 3), eye)


def test_camera_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(20)     # never dereferenced: validation fails first
    cam = (ctypes.c_float * 7)(*cr.KITTI_FISHEYE)
    c2w = (ctypes.c_float * 12)()
    err = lambda: lib.pnr_last_error()
    assert lib.pnr_gen_rays_fisheye(None, c2w, 8, 8, 0.5, 10.0, null, 64, one, null, null) == -1 and b"null camera" in err()
    assert lib.pnr_gen_rays_fisheye(cam, None, 8, 8, 0.5, 10.0, null, 64, one, null, null) == -1 and b"null camera" in err()
    assert lib.pnr_gen_rays_fisheye(cam, c2w, 0, 8, 0.5, 10.0, null, 64, one, null, null) == -1 and b"bad size" in err()
    assert lib.pnr_gen_rays_fisheye(cam, c2w, 8, 8, 0.5, 10.0, null, 63, one, null, null) == -1 and b"width*height" in err()
    assert lib.pnr_gen_rays_fisheye(cam, c2w, 8, 8, 0.5, 10.0, null, 64, odd, null, null) == -1 and b"16-byte" in err()
    assert lib.pnr_gen_rays_fisheye(cam, c2w, 8, 8, 0.5, 10.0, null, 64, null, null, null) == -1 and b"16-byte" in err()
    for k in (3, 4):
        bad = (ctypes.c_float * 7)(*cr.KITTI_FISHEYE)
        bad[k] = 0.0
        assert lib.pnr_gen_rays_fisheye(bad, c2w, 8, 8, 0.5, 10.0, null, 64, one, null, null) == -1 and b"zero gamma" in err()
    assert lib.pnr_gen_rays_fisheye(cam, c2w, 8, 8, 0.5, 10.0, null, 0, null, null, null) == 0            # empty input: a no-op
    intr = (ctypes.c_float * 4)(500.0, 500.0, 4.0, 4.0)
    assert lib.pnr_project_points(2, cam, c2w, 8, 8, one, 4, one, one, one, null) == -1 and b"unknown camera model 2" in err()
    assert lib.pnr_project_points(-1, cam, c2w, 8, 8, one, 4, one, one, one, null) == -1 and b"unknown camera model" in err()
    assert lib.pnr_project_points(1, None, c2w, 8, 8, one, 4, one, one, one, null) == -1 and b"null camera" in err()
    assert lib.pnr_project_points(0, intr, None, 8, 8, one, 4, one, one, one, null) == -1 and b"null camera" in err()
    assert lib.pnr_project_points(0, intr, c2w, 8, 0, one, 4, one, one, one, null) == -1 and b"bad size" in err()
    assert lib.pnr_project_points(0, intr, c2w, 8, 8, null, 4, one, one, one, null) == -1 and b"null points" in err()
    assert lib.pnr_project_points(1, cam, c2w, 8, 8, one, 4, odd, one, one, null) == -1 and b"8-byte" in err()
    assert lib.pnr_project_points(1, cam, c2w, 8, 8, null, 0, null, null, null, null) == 0                # n = 0: a no-op
