"""Pins tests/_pano_ref.py, the CPU references of the panoramic camera (include/pnr.h "cameras", PNR_CAMERA_EQUIRECT), before
anything on the GPU is measured against them: values the float32 rule must hit exactly, closed forms that both precisions
must give and that each corrupted variant of the model misses, then float32 against float64 as conditions.

Conditions (u = 2^-24; none is taken from what the float32 rule gives), with the values measured here beside them:
    sincospi32, atan2pi32 against float64                    <= 2 u each        measured sin 1.50 u, cos 1.48 u, atan2pi 1.10 u
        (2 u is what _pano_ref's error chain assumes.  The sine: P(t) near pi carries half an ulp of its last addition (2 u),
        the rounding of the coefficient pi (up to 1.5 u) and the inner terms (0.5 u), about 4 u, times |r| <= 1/4, plus the
        half ulp of a result below 1: 1.5 u.  The cosine: half an ulp of a result in [0.7, 1], the last product's quarter
        and the inner sum's 8 u times t <= 1/16: 1.3 u.  The arctangent: a result of at most 1 half-turn assembled from a
        quotient good to 1.5 ulp times at most 1/8 and two subtractions from exact constants: below 1.5 u.)
    each component of d against the float64 direction of the float32-rounded angles, two rotations   <= 4 u     measured 3.50 u
    | |d| - 1 |                                                                                         <= 4 u     measured 3.37 u
    pixel -> ray -> point at t in {0.5, 7.3, 100} -> projection, identity pose, in pixels             <= 1e-3    measured 1.22e-4
    whole-frame reprojection float32 against float64: excluded share of the pixels with depth           <= 1 %     measured
        equirect -> equirect 0.235 %,  equirect -> pinhole 0.029 %,  fisheye -> equirect 0.481 %
        (55 / 5 / 96 pixels differ, all inside the excluded set)
"""
import math

import numpy as np
import pytest

import _camera_ref as cr
import _pano_ref as pr
import _warp_ref as wr

f32 = lambda a: np.asarray(a, np.float32)
U = pr.U32
EYE = np.eye(3, 4)
SQ = math.sqrt(0.5)


# ------------------------------------------------------------------------------------------------ exact values
def test_sincospi_is_exact_at_every_multiple_of_half():
    x = np.arange(-16, 17) * 0.5
    s, c = pr.sincospi32(x)
    k = np.arange(-16, 17)
    assert np.array_equal(s, [0.0, 1.0, 0.0, -1.0] * 8 + [0.0]) and np.array_equal(s, np.round(np.sin(math.pi * x)))
    assert np.array_equal(c, np.round(np.cos(math.pi * x)))
    assert s.dtype == c.dtype == np.float32 and k.size == 33
    # ties to even in the reduction: x = 0.25 and 0.75 (2x = 0.5, 1.5) reduce to r = +-1/4 from k = 0 and k = 2
    s, c = pr.sincospi32([0.25, 0.75, -0.25])
    assert np.abs(s - f32([SQ, SQ, -SQ])).max() <= 2 * U and np.abs(c - f32([SQ, -SQ, SQ])).max() <= 2 * U


def test_atan2pi_on_the_axes_the_diagonals_and_at_zero():
    a = pr.atan2pi32
    assert a(0.0, 1.0) == 0.0 and a(1.0, 0.0) == 0.5 and a(-1.0, 0.0) == -0.5 and a(0.0, -1.0) == 1.0
    assert a(0.0, 3e-30) == 0.0 and a(7e20, 0.0) == 0.5
    for y, x, want in ((1, 1, 0.25), (1, -1, 0.75), (-1, 1, -0.25), (-1, -1, -0.75), (3.5, 3.5, 0.25)):
        got = a(float(y), float(x))
        assert abs(float(got) - want) <= float(np.spacing(np.float32(abs(want)))), (y, x, got)
    assert a(0.0, 0.0) == 0.0 and a(-0.0, 0.0) == 0.0 and a(0.0, -0.0) == 0.0 and a(-0.0, -0.0) == 0.0
    # -0 counts as +0: no sign flip, no reflection
    assert a(-0.0, 1.0) == 0.0 and a(-0.0, -1.0) == 1.0 and a(1.0, -0.0) == 0.5
    assert a(0.0, 1.0).dtype == np.float32


def test_sincospi_and_atan2pi_against_float64():
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.uniform(-3.0, 3.0, 2000000), np.linspace(-0.25, 0.25, 200001)]).astype(np.float32)
    s, c = pr.sincospi32(x)
    es = np.abs(s - np.sin(math.pi * x.astype(np.float64))).max() / U
    ec = np.abs(c - np.cos(math.pi * x.astype(np.float64))).max() / U
    ang = rs.uniform(-math.pi, math.pi, 2000000)
    rad = np.exp(rs.uniform(-20, 20, ang.size))
    y, xx = f32(rad * np.sin(ang)), f32(rad * np.cos(ang))
    ea = np.abs(pr.atan2pi32(y, xx) - np.arctan2(y.astype(np.float64), xx.astype(np.float64)) / math.pi).max() / U
    print("sincospi32: sin %.2f u, cos %.2f u; atan2pi32: %.2f u" % (es, ec, ea))
    assert max(es, ec) * U <= pr.SINCOS_BOUND and ea * U <= pr.ATAN_BOUND
    assert pr.SINCOS_BOUND == 2 * U and pr.ATAN_BOUND == 2 * U


# ------------------------------------------------------------------------------------------------ closed forms
def closed_form_failures(variant=None):
    """Names of the closed-form checks that the float64 model, run with `variant`, does NOT pass."""
    bad = []

    def check(name, ok):
        if not bool(ok):
            bad.append(name)

    un = lambda cam, w, h, **kw: pr.unproject64(cam, w, h, variant=variant, **kw)
    pj = lambda cam, w, h, pts: pr.project64(cam, None, w, h, pts, variant=variant)
    # (1) 2 x 1 over lon (-90, 90): the two pixel centres are 45 degrees either side of +z, on the horizon
    cam = pr.equirect_cam(2, 1, lon=(-90.0, 90.0))
    check("two_columns", np.abs(un(cam, 2, 1) - [[-SQ, 0.0, SQ], [SQ, 0.0, SQ]]).max() < 1e-7)
    # (2) 1 x 2 full sphere: row 0 looks 45 degrees UP (y is down: d.y < 0), row 1 45 degrees down
    cam = pr.equirect_cam(1, 2)
    check("two_rows", np.abs(un(cam, 1, 2) - [[0.0, -SQ, SQ], [0.0, SQ, SQ]]).max() < 1e-7)
    # (3) poles and axes of a full 8 x 4 sphere: straight up is the top edge v = -0.5 (valid), straight down the bottom edge
    # v = 3.5 (outside); +z is the image centre; +x a quarter turn to the right
    cam = pr.equirect_cam(8, 4)
    uv, rng, ok = pj(cam, 8, 4, [[0, -2.0, 0], [0, 2.0, 0], [0, 0, 3.0], [5.0, 0, 0], [0, 0, 0]])
    check("poles", abs(uv[0, 1] + 0.5) < 1e-9 and ok[0] and abs(uv[1, 1] - 3.5) < 1e-9 and not ok[1])
    check("axes", np.abs(uv[2] - [3.5, 1.5]).max() < 1e-9 and np.abs(uv[3] - [5.5, 1.5]).max() < 1e-9 and ok[2] and ok[3])
    check("centre", not ok[4] and np.array_equal(uv[4], [0, 0]) and np.allclose(rng[:4], [2, 2, 3, 5]))
    # (4) the seam, both directions.  -z seen with x = +0 has longitude +1 half-turn = the right edge: one period back, onto
    # the left edge u = -0.5 of pixel 0 (valid).  A camera whose left edge is +90 degrees runs to 450: the direction -x
    # (longitude -90 = 270) lies half way, one period forward.
    uv, _, ok = pj(cam, 8, 4, [[0.0, 0, -1.0], [-1e-9, 0, -1.0], [1e-9, 0, -1.0]])
    check("seam_back", abs(uv[0, 0] + 0.5) < 1e-9 and ok[0] and abs(uv[1, 0] + 0.5) < 1e-6 and abs(uv[2, 0] - 7.5) < 1e-6 and ok[1] and ok[2])
    cam90 = pr.equirect_cam(8, 4, lon=(90.0, 450.0))
    uv, _, ok = pj(cam90, 8, 4, [[-1.0, 0, 0], [1.0, 0, -1e-12]])
    check("seam_forward", abs(uv[0, 0] - 3.5) < 1e-6 and ok[0] and abs(uv[1, 0] + 0.5) < 1e-6)
    # (5) a partial range across +-180: 170 .. 190 degrees, 20 columns of one degree; -175 degrees = 185 is column 14.5 + 0.5
    camp = pr.equirect_cam(20, 10, lon=(170.0, 190.0), lat=(5.0, -5.0))
    a = math.radians(-175.0)
    uv, _, ok = pj(camp, 20, 10, [[math.sin(a), 0, math.cos(a)], [0, 0, 1.0]])
    check("partial_range", np.abs(uv[0] - [14.5, 4.5]).max() < 1e-4 and ok[0] and not ok[1])
    # (6) the mirrored range (dlon < 0) and the round trip pixel -> direction -> pixel on every camera above
    camm = pr.equirect_cam(20, 10, lon=(-170.0, -190.0), lat=(5.0, -5.0))
    uv, _, ok = pj(camm, 20, 10, [[math.sin(a), 0, math.cos(a)]])
    check("mirrored", np.abs(uv[0] - [4.5, 4.5]).max() < 1e-4 and ok[0])
    for name, c, w, h in (("full", cam, 8, 4), ("from90", cam90, 8, 4), ("partial", camp, 20, 10), ("mirror", camm, 20, 10)):
        i, j = cr.pixel_grid(w, h)
        uv, _, ok = pj(c, w, h, 4.0 * un(c, w, h))
        check("round_trip_" + name, ok.all() and np.abs(uv - np.stack([i, j], -1)).max() < 1e-4)
    return bad


def test_closed_forms():
    assert closed_form_failures() == []


@pytest.mark.parametrize("variant", pr.VARIANTS)
def test_corrupted_variants_fail_the_closed_forms(variant):
    bad = closed_form_failures(variant)
    print(variant, "fails", bad)
    assert bad, variant
    assert len(pr.VARIANTS) >= 4


def test_float32_restatement_gives_the_closed_forms():
    """the same answers from unproject32 / project32, to float32 accuracy; the exact ones exactly"""
    cam = pr.equirect_cam(2, 1, lon=(-90.0, 90.0))
    assert np.abs(pr.unproject32(cam, EYE, 2, 1, 0.5, 9.0)[:, 3:6] - [[-SQ, 0.0, SQ], [SQ, 0.0, SQ]]).max() <= 4 * U
    assert np.array_equal(pr.unproject32(cam, cr.pose(0.0, 0.0, (1, 2, 3)), 2, 1, 0.5, 9.0)[:, [0, 1, 2, 6, 7]], [[1, 2, 3, 0.5, 9.0]] * 2)
    cam = pr.equirect_cam(8, 4)
    pts = f32([[0, -2.0, 0], [0, 2.0, 0], [0, 0, 3.0], [5.0, 0, 0], [0, 0, 0], [0.0, 0, -1.0], [-0.0, 0, -1.0],
               [np.nan, 0, 1], [np.inf, 0, 1], [3e38, 3e38, 3e38]])
    uv, rng, ok = pr.project32(cam, EYE, 8, 4, pts)
    assert np.array_equal(uv[:7], [[3.5, -0.5], [3.5, 3.5], [3.5, 1.5], [5.5, 1.5], [0, 0], [-0.5, 1.5], [-0.5, 1.5]])
    assert ok.tolist() == [1, 0, 1, 1, 0, 1, 1, 0, 0, 0]
    assert np.array_equal(uv[7:], np.zeros((3, 2))) and np.isnan(rng[7]) and np.isnan(rng[8]) and np.isinf(rng[9])        # (0 * inf in the pose product)
    uv64, _, ok64 = pr.project64(cam, EYE, 8, 4, pts[:7])
    assert np.abs(uv - 0)[:7].shape == uv64.shape and np.abs(uv[:7] - uv64).max() < 1e-5 and np.array_equal(ok[:7] != 0, ok64)


# ------------------------------------------------------------------------------------------------ float32 against float64
CAMERAS = {"4096x2048": (4096, 2048, pr.equirect_cam(4096, 2048)), "1408x704": (1408, 704, pr.equirect_cam(1408, 704)),
           "37x19 partial": (37, 19, pr.equirect_cam(37, 19, lon=(150.0, 260.0), lat=(40.0, -75.0)))}
ROTATIONS = {"identity": cr.pose(0.0), "yaw_pitch": cr.pose(-2.2, 0.35)}


def _subset(w, h):
    """the whole frame when small; otherwise every 7th pixel (7 is coprime to both widths) and the whole border"""
    if w * h <= 1 << 20:
        return None
    i, j = cr.pixel_grid(w, h)
    p = np.arange(w * h)
    return p[(p % 7 == 0) | (i < 2) | (i >= w - 2) | (j < 2) | (j >= h - 2)]


@pytest.mark.parametrize("name", list(CAMERAS))
def test_directions_and_round_trip_float32_against_float64(name):
    """The conditions of the module docstring.  Directions under both rotations.  The round trip under the identity pose: there
    p0 / p2 = (cp sl) / (cp cl) carries relative errors only, so longitude comes back to a few u at every latitude.  Under a
    general rotation the three-term sums of R d leave an absolute error of a few u in each component, which near a pole, where
    the horizontal part of d is h = cos(latitude) ~ 1e-3, is a longitude error of u / h: a property of float32 unit vectors,
    not of this rule, so no pixel bound is set there (the reprojection test below bounds it per pixel instead)."""
    w, h, cam = CAMERAS[name]
    pix = _subset(w, h)
    i, j = cr.pixel_grid(w, h, pix)
    worst_d = worst_n = worst_rt = 0.0
    for pose, c2w in ROTATIONS.items():
        rays = pr.unproject32(cam, c2w, w, h, 0.5, 100.0, pix)
        d = rays[:, 3:6].astype(np.float64)
        d64 = pr.unproject64(cam, w, h, pix, c2w=f32(c2w), rounded=True)
        worst_d = max(worst_d, np.abs(d - d64).max())
        worst_n = max(worst_n, np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max())
        # the angles themselves, unrounded, agree with the float32 ones to the rounding of lon0 + (i + 0.5) dlon
        assert np.abs(d64 - pr.unproject64(cam, w, h, pix, c2w=f32(c2w))).max() < 3 * math.pi * 4 * U
        if pose != "identity":
            continue
        for t in (0.5, 7.3, 100.0):
            X = rays[:, 0:3] + np.float32(t) * rays[:, 3:6]
            uv, rng, ok = pr.project32(cam, EYE, w, h, X)
            assert ok.all()
            worst_rt = max(worst_rt, np.abs(uv - np.stack([i, j], -1)).max())
            assert np.abs(rng / np.float32(t) - 1.0).max() < 8 * U
    print("%s: max |d32 - d64| = %.2f u, | |d| - 1 | = %.2f u, round trip %.2e px" % (name, worst_d / U, worst_n / U, worst_rt))
    assert worst_d <= 4 * U and worst_n <= 4 * U and worst_rt <= 1e-3


PIN = (552.554261, 552.554261, 682.049453, 238.769549)
POSE_A = cr.pose(0.0, 0.0, (0.0, 1.55, 0.0))
POSE_B = cr.pose(0.05, -0.03, (0.3, 1.5, 0.4))            # 0.5 m and 3.3 degrees from A
SPHERE = ((1.0, 0.0, 3.0), 15.0)
MAX_EXCLUDED = 0.01


def frame_pair(kind_s, kind_t):
    """as test_warp_ref.frame_pair, with the panorama as a third benchmark shape (1408 x 704, full sphere)"""
    mk = {"pinhole": (pr.PINHOLE, f32(PIN), 1408, 376), "fisheye": (pr.FISHEYE, f32(cr.KITTI_FISHEYE), 1400, 1400),
          "equirect": (pr.EQUIRECT, f32(pr.equirect_cam(1408, 704)), 1408, 704)}
    depth = lambda m, c, pose, w, h: (pr.sphere_depth(c, pose, w, h, *SPHERE) if m == pr.EQUIRECT
                                      else wr.sphere_depth(m, c, pose, w, h, *SPHERE))
    ms, cs, ws, hs = mk[kind_s]
    mt, ct, wt, ht = mk[kind_t]
    ca, cb = f32(POSE_A), f32(POSE_B)
    ds = depth(ms, cs, ca, ws, hs)
    dt = depth(mt, ct, cb, wt, ht).reshape(-1)
    i, j = cr.pixel_grid(wt, ht)
    dt = (dt * (1.0 + 0.03 * np.sin(i / 97.0) * np.cos(j / 61.0))).astype(np.float32)
    return (ms, cs, ca, ws, hs), ds, (mt, ct, f32(cr.invert_pose(cb.astype(np.float64))), wt, ht), dt


@pytest.mark.parametrize("kind_s,kind_t", [("equirect", "equirect"), ("equirect", "pinhole"), ("fisheye", "equirect")])
def test_reprojection_float32_against_float64_on_whole_frames(kind_s, kind_t):
    src, ds, tgt, dt = frame_pair(kind_s, kind_t)
    tol = (0.0, 0.02)
    a = pr.reproject32(src, ds, tgt, dt, tol)
    b = pr.reproject64(src, ds, tgt, dt, tol)
    ex, du = pr.excluded(b, src, ds, tgt, tol)
    have = b["have"]
    share = ex.sum() / have.sum()
    differ = a["match"] != b["match"]
    print("%s -> %s: %d pixels with depth, %.3f %% excluded, %d differ (%d outside the excluded set); codes %s"
          % (kind_s, kind_t, have.sum(), 100 * share, differ.sum(), (differ & ~ex).sum(), a["stats"].tolist()))
    assert share <= MAX_EXCLUDED
    assert not (differ & ~ex).any()
    # not vacuous: matched and occluded pixels occur in numbers; a panoramic target is never left, a pinhole target is
    assert (a["stats"][[0, 4]] > 1000).all() and (a["stats"][2] > 1000) == (kind_t == "pinhole")
    if kind_t != "pinhole":
        assert a["stats"][2] == 0 and (kind_s == "fisheye") == (a["stats"][1] > 1000)


def test_reproject_restatement_equals_warp_ref_without_a_panorama():
    """steps 2-8 restated: on the two older models the restatement is _warp_ref's, bit for bit"""
    cam_p, cam_f = (40.0, 41.0, 31.5, 23.5), tuple(cr.KITTI_FISHEYE[:3]) + (91.6, 91.6, 48.66, 47.9)
    c2w, w2c = f32(cr.pose(0.2, 0.05, (0.0, 1.5, 0.0))), f32(cr.invert_pose(cr.pose(0.25, 0.0, (0.3, 1.5, 0.1))))
    ds = wr.sphere_depth(wr.FISHEYE, cam_f, c2w, 96, 96, (0, 1.5, 0), 9.0)
    dt = np.full(64 * 48, 9.0, np.float32)
    ls, lt = (np.arange(96 * 96) % 5).astype(np.int32), (np.arange(64 * 48) % 5).astype(np.int32)
    for fn_a, fn_b in ((pr.reproject32, wr.reproject32), (pr.reproject64, wr.reproject64)):
        a = fn_a((wr.FISHEYE, f32(cam_f), c2w, 96, 96), ds, (wr.PINHOLE, f32(cam_p), w2c, 64, 48), dt, label_src=ls, label_tgt=lt, n_classes=5)
        b = fn_b((wr.FISHEYE, f32(cam_f), c2w, 96, 96), ds, (wr.PINHOLE, f32(cam_p), w2c, 64, 48), dt, label_src=ls, label_tgt=lt, n_classes=5)
        for k in ("match", "uv", "stats", "agree"):
            assert np.array_equal(a[k], b[k]), k
