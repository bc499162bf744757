"""Pins tests/_splat_ref.py, the CPU references of point splatting and the depth metrics (include/pnr.h "point splatting"),
before anything on the GPU is measured against them: closed-form answers that splat32 must give and that each corrupted
variant of the rule must miss; the cross-kernel property against the (already pinned) reprojection reference; float32 against
float64 per point on whole clouds at the benchmark shapes; closed forms of the metrics and their corrupted variants.

float32 against float64: per POINT (not per winner) the pixel and the clip decision of points32 and splat64 must agree
outside an excluded set, the points whose float64 u + 0.5 / v + 0.5 lies within the projection's float32 error bound of an
integer or whose depth lies within its bound of near / far.  The bound is derived from the roundings of the projection chain
(_warp_ref.E), never from the difference of the two evaluations.  Condition: at most 1 % of the points excluded, per view.
Measured here (20 160-point scans, sensor and camera inside a 30 m sphere with a ground plane):
    pinhole 1408 x 376    0.010 % excluded,  0 points differ
    fisheye 1400 x 1400   0.089 % excluded,  1 point differs, inside the excluded set
    equirect 1408 x 704   0.144 % excluded,  1 point differs, inside the excluded set
"""
import numpy as np
import pytest

import _camera_ref as cr
import _pano_ref as pr
import _splat_ref as sr
from panopticnerf_amd import synthetic

f32 = lambda a: np.asarray(a, np.float32)
EYE = f32(cr.pose(0.0))
PIN_SMALL = f32((40.0, 41.0, 31.5, 23.5))
W1, H1 = 64, 48
FISH_SMALL = f32(tuple(v * s for v, s in zip(cr.KITTI_FISHEYE, (1, 1, 1, 96 / 1400, 96 / 1400, 0, 0)))[:5] + (48.66, 47.9))
W2 = H2 = 96
EQ_SMALL = f32(pr.equirect_cam(16, 8))


def _w2c(c2w):
    return f32(cr.invert_pose(f32(c2w).astype(np.float64)))


def closed_form_failures(variant=None):
    """Names of the closed-form checks that splat32, run with `variant`, does NOT pass."""
    bad = []

    def check(name, ok):
        if not ok:
            bad.append(name)

    def run(model, cam, w, h, pts, **kw):
        return sr.splat32(model, cam, EYE, w, h, f32(pts), variant=variant, **kw)

    def cells(z):
        return {int(q): int(v) for q, v in zip(np.flatnonzero(z != sr.EMPTY), z[z != sr.EMPTY])}

    # (1) one point on the optical axis: u = cx = 31.5 rounds UP to column 32, v = cy = 23.5 to row 24; depth z = 5
    z, st = run(sr.PINHOLE, PIN_SMALL, W1, H1, [[0, 0, 5]])
    check("axis", cells(z) == {24 * W1 + 32: sr.key(5.0, 0)} and st.tolist() == [1, 0, 0])
    # ... and one off it: pinhole depth is z = 4, not the range 5; u = 40 * 0.75 + 31.5 = 61.5 -> column 62
    z, st = run(sr.PINHOLE, PIN_SMALL, W1, H1, [[3, 0, 4]])
    check("z_depth", cells(z) == {24 * W1 + 62: sr.key(4.0, 0)})
    # ... while fisheye and equirect depth is the range
    for model, cam, w, h in ((sr.FISHEYE, FISH_SMALL, W2, H2), (sr.EQUIRECT, EQ_SMALL, 16, 8)):
        d, _ = sr.resolve(run(model, cam, w, h, [[3, 0, 4]])[0])
        check("range_%d" % model, (d > 0).sum() == 1 and d.max() == np.float32(5.0))
    # (2) two points on one pixel at different depths: the nearer wins whichever order they come in
    for order in ((5.0, 3.0), (3.0, 5.0)):
        z, st = run(sr.PINHOLE, PIN_SMALL, W1, H1, [[0, 0, order[0]], [0, 0, order[1]]])
        check("nearest_%g" % order[0], cells(z) == {24 * W1 + 32: sr.key(3.0, order.index(3.0))} and st.tolist() == [2, 0, 0])
    # (3) equal depth: the lower index wins
    z, _ = run(sr.PINHOLE, PIN_SMALL, W1, H1, [[0, 0, 5]] * 3, index_base=7)
    check("tie", cells(z) == {24 * W1 + 32: sr.key(5.0, 7)})
    # (4) behind a pinhole, at the camera centre (any model), NaN / Inf coordinates: the point leaves the view
    z, st = run(sr.PINHOLE, PIN_SMALL, W1, H1, [[0, 0, -5], [0, 0, 0], [np.nan, 0, 5], [0, np.inf, 5], [0, 0, np.inf], [-np.inf, 0, 1]])
    check("left_pinhole", not cells(z) and st.tolist() == [0, 6, 0])
    for model, cam, w, h in ((sr.FISHEYE, FISH_SMALL, W2, H2), (sr.EQUIRECT, EQ_SMALL, 16, 8)):
        z, st = run(model, cam, w, h, [[0, 0, 0], [np.nan, 0, 5], [0, np.inf, 5]])
        check("left_%d" % model, not cells(z) and st.tolist() == [0, 3, 0])
    # ... the image border: u = width - 0.5 - eps is column width - 1, u = width - 0.5 is outside; likewise -0.5 and below
    unit = f32((1.0, 1.0, 0.0, 0.0))                        # u = x / z, v = y / z exactly at z = 1
    below = np.nextafter(np.float32(W1 - 0.5), np.float32(0))
    z, st = run(sr.PINHOLE, unit, W1, H1, [[below, 0, 1], [W1 - 0.5, 0, 1], [-0.5, 0, 1], [np.nextafter(np.float32(-0.5), np.float32(-1)), 0, 1],
                                           [0, np.nextafter(np.float32(H1 - 0.5), np.float32(0)), 1], [0, H1 - 0.5, 1]])
    check("border", cells(z) == {W1 - 1: sr.key(1.0, 0), 0: sr.key(1.0, 2), (H1 - 1) * W1: sr.key(1.0, 4)} and st.tolist() == [3, 3, 0])
    # (5) near / far: both ends belong to the range
    up, down = float(np.nextafter(np.float32(5), np.float32(9))), float(np.nextafter(np.float32(5), np.float32(0)))
    for near, far, lands in ((5.0, 9.0, 1), (0.0, 5.0, 1), (5.0, 5.0, 1), (up, 9.0, 0), (0.0, down, 0), (0.0, np.inf, 1)):
        z, st = run(sr.PINHOLE, PIN_SMALL, W1, H1, [[0, 0, 5]], near=near, far=far)
        check("clip_%g_%g" % (near, far), len(cells(z)) == lands and st.tolist() == [lands, 0, 1 - lands])
    # (6) the footprint at a corner is clipped, not wrapped
    for radius, side in ((0, 1), (1, 2), (2, 3)):
        z, _ = run(sr.PINHOLE, unit, W1, H1, [[0, 0, 1]], radius=radius)
        want = {y * W1 + x: sr.key(1.0, 0) for y in range(side) for x in range(side)}
        check("corner_r%d" % radius, cells(z) == want)
        z, _ = run(sr.PINHOLE, unit, W1, H1, [[W1 - 1, H1 - 1, 1]], radius=radius)
        want = {y * W1 + x: sr.key(1.0, 0) for y in range(H1 - side, H1) for x in range(W1 - side, W1)}
        check("far_corner_r%d" % radius, cells(z) == want)
    # ... at the seam of a full-circle panorama too: a point just inside column 0 does not reach column 15
    for radius in (1, 2):
        z, _ = run(sr.EQUIRECT, EQ_SMALL, 16, 8, [[-0.05, 0, -5]], radius=radius)
        got = cells(z)
        want = {y * 16 + x for y in range(4 - radius, 4 + radius + 1) for x in range(0, radius + 1)}
        check("seam_r%d" % radius, set(got) == want and len(set(got.values())) == 1)
    # (7) two chunks with index_base equal the single call, in either order
    g = np.random.default_rng(3)
    pts = f32(g.normal(size=(600, 3)) * (4, 3, 2) + (0, 0, 6))
    pts[::7] = pts[3]                                       # ties
    one, st1 = run(sr.PINHOLE, PIN_SMALL, W1, H1, pts, radius=1, near=3.0, far=9.0)
    if variant not in ("farthest", "tie_high"):
        a, sa = run(sr.PINHOLE, PIN_SMALL, W1, H1, pts[:250], radius=1, near=3.0, far=9.0)
        ab, sb = run(sr.PINHOLE, PIN_SMALL, W1, H1, pts[250:], radius=1, near=3.0, far=9.0, index_base=250, zbuf=a)
        b, _ = run(sr.PINHOLE, PIN_SMALL, W1, H1, pts[250:], radius=1, near=3.0, far=9.0, index_base=250)
        ba, _ = run(sr.PINHOLE, PIN_SMALL, W1, H1, pts[:250], radius=1, near=3.0, far=9.0, zbuf=b)
        check("chunks", np.array_equal(one, ab) and np.array_equal(one, ba) and np.array_equal(st1, sa + sb) and st1.min() > 0)
    # ... and against a per-point loop over Python integers
    landed, _, iu, iv, e = sr.points32((sr.PINHOLE, PIN_SMALL, EYE, W1, H1), pts, 3.0, 9.0)
    want = {}
    for i in np.flatnonzero(landed):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                x, y = int(iu[i]) + dx, int(iv[i]) + dy
                if 0 <= x < W1 and 0 <= y < H1:
                    want[y * W1 + x] = min(want.get(y * W1 + x, 2 ** 64 - 1), sr.key(e[i], i))
    check("loop", cells(one) == want)
    return bad


def test_closed_forms():
    assert closed_form_failures() == []


@pytest.mark.parametrize("variant,misses", [("farthest", "nearest_5"), ("tie_high", "tie"), ("trunc", "axis"), ("range_pinhole", "z_depth")])
def test_corrupted_variants_fail_the_closed_forms(variant, misses):
    assert misses in closed_form_failures(variant)


def test_resolve_unpacks_both_words():
    z = np.array([sr.EMPTY, sr.key(2.5, 7), sr.key(np.inf, 2 ** 31 - 2), sr.key(1e-40, 0)], np.uint64)
    d, i = sr.resolve(z)
    assert d.tolist() == [0.0, 2.5, np.inf, float(np.float32(1e-40))] and i.tolist() == [-1, 7, 2 ** 31 - 2, 0]
    d2, i2 = sr.resolve(z.view(np.int64).reshape(2, 2))
    assert d2.shape == (2, 2) and np.array_equal(d2.reshape(-1), d) and np.array_equal(i2.reshape(-1), i)
    # the empty word is no key: its high word is a NaN pattern
    assert np.isnan(np.uint32(0xFFFFFFFF).view(np.float32))


# ------------------------------------------------------------------------------------------------ against reprojection
CENTRE, RADIUS = (0.5, 1.0, 2.0), 15.0
POSE_A, POSE_B = cr.pose(0.10, -0.05, (0.2, 1.5, 0.3)), cr.pose(0.15, -0.02, (0.7, 1.45, 0.4))


def _sphere(model, cam, c2w, w, h):
    if model == sr.EQUIRECT:
        return pr.sphere_depth(cam, c2w, w, h, CENTRE, RADIUS)
    import _warp_ref as wr
    return wr.sphere_depth(model, cam, c2w, w, h, CENTRE, RADIUS)


SMALL = {sr.PINHOLE: (PIN_SMALL, W1, H1), sr.FISHEYE: (FISH_SMALL, W2, H2), sr.EQUIRECT: (f32(pr.equirect_cam(64, 32)), 64, 32)}


def lift32(src, depth):
    """(points (m, 3) float32, pix (m)) of the source pixels that have depth: reprojection steps 1-3"""
    w, h = src[3], src[4]
    pc = np.arange(w * h, dtype=np.int64)
    o, d, ok = pr._rays(np.float32, src, pc)
    t = f32(depth).reshape(-1)
    with np.errstate(all="ignore"):
        have = ok & (t > 0) & (np.abs(t) <= sr.FMAX)
    X = np.stack([o[k] + t[have] * d[have, k] for k in range(3)], -1).astype(np.float32)
    return X, pc[have]


def cross_property_failures(ms, mt, variant=None, radius=0):
    cam_s, ws, hs = SMALL[ms]
    cam_t, wt, ht = SMALL[mt]
    src = (ms, cam_s, f32(POSE_A), ws, hs)
    tgt = (mt, cam_t, _w2c(POSE_B), wt, ht)
    depth = _sphere(ms, cam_s, f32(POSE_A), ws, hs)
    depth.reshape(-1)[::97] = 0.0
    rp = pr.reproject32(src, depth, tgt, None)
    X, pix = lift32(src, depth)
    zbuf, stats = sr.splat32(mt, cam_t, tgt[2], wt, ht, X, radius=radius, variant=variant)
    bad = []
    assert np.array_equal(np.flatnonzero(rp["have"]), pix)
    match, e = rp["match"][pix], rp["e"][pix]
    if not (stats[0] == (match >= 0).sum() and stats[1] == (match == -2).sum() and stats[2] == 0 and stats[0] > 100):
        bad.append("stats")
    # every source pixel that lands is beaten or met at its own pixel
    r = np.flatnonzero(match >= 0)
    keys = np.array([sr.key(e[k], k) for k in r], np.uint64)
    if not (zbuf[match[r]] <= keys).all():
        bad.append("not_beaten")
    # every filled cell's winner is a source pixel that reprojection sends there, at that depth
    d, idx = sr.resolve(zbuf)
    q = np.flatnonzero(idx >= 0)
    if radius == 0 and not (np.array_equal(match[idx[q]], q) and np.array_equal(d[q], e[idx[q]])):
        bad.append("winner")
    if radius == 0 and set(q) != set(match[r]):
        bad.append("cells")
    return bad


@pytest.mark.parametrize("ms,mt", [(sr.PINHOLE, sr.FISHEYE), (sr.FISHEYE, sr.EQUIRECT), (sr.EQUIRECT, sr.PINHOLE), (sr.PINHOLE, sr.PINHOLE),
                                   (sr.PINHOLE, sr.EQUIRECT)])
def test_lift_and_splat_agrees_with_reprojection(ms, mt):
    assert cross_property_failures(ms, mt) == []
    assert cross_property_failures(ms, mt, radius=1) == []


@pytest.mark.parametrize("variant,ms,mt", [("farthest", sr.PINHOLE, sr.EQUIRECT), ("trunc", sr.EQUIRECT, sr.PINHOLE),
                                           ("range_pinhole", sr.EQUIRECT, sr.PINHOLE)])
def test_corrupted_variants_fail_the_cross_property(variant, ms, mt):
    # "farthest" needs a pairing in which source pixels share a target pixel (a narrow view into a coarse panorama).  The tie
    # rule cannot show here: no two lifted pixels share a pixel AND a bit-equal depth -- the closed form 'tie' covers it.
    assert cross_property_failures(ms, mt) == []
    assert cross_property_failures(ms, mt, variant) != []


# ------------------------------------------------------------------------------------------------ float32 against float64
BENCH = {"pinhole": (sr.PINHOLE, f32((synthetic.KITTI_F, synthetic.KITTI_F, synthetic.KITTI_CX, synthetic.KITTI_CY)), synthetic.KITTI_W, synthetic.KITTI_H),
         "fisheye": (sr.FISHEYE, f32(cr.KITTI_FISHEYE), 1400, 1400),
         "equirect": (sr.EQUIRECT, f32(pr.equirect_cam(1408, 704)), 1408, 704)}
EXCLUDED_CAP = 0.01


@pytest.mark.parametrize("name", list(BENCH))
def test_float32_agrees_with_float64_per_point(name):
    model, cam, w, h = BENCH[name]
    pts, _ = synthetic.lidar_scan(origin=(0.3, 1.2, -0.4), sphere=((0.0, 1.55, 10.0), 30.0), ground_y=3.0, n_azimuth=360, n_elevation=56)
    pts = pts.numpy()
    assert pts.shape[0] == 20160
    c2w = f32(cr.pose(np.pi / 2, 0.0, (0.0, 1.55, 0.0)) if model == sr.FISHEYE else cr.pose(0.05, -0.03, (0.0, 1.55, 0.0)))
    view = (model, cam, _w2c(c2w), w, h)
    near, far = 4.0, 35.0
    landed, left, iu, iv, e = sr.points32(view, pts, near, far)
    ref = sr.splat64(view, pts, near, far)
    du, dv, de = sr.project_bound(view, pts)
    ex = sr.near_decision(ref, view, near, far, du, dv, de)
    share = ex.mean()
    differ = (landed != ref["landed"]) | (left != ~ref["inside"]) | (~left & ((iu != ref["iu"]) | (iv != ref["iv"])))
    print("%s: %.3f %% of %d points excluded, %d differ, %d of them outside the excluded set; %d land"
          % (name, 100 * share, ex.size, differ.sum(), (differ & ~ex).sum(), landed.sum()))
    assert landed.sum() > 1000 and (~left & ~landed).sum() > 100          # the cloud exercises the image and the clip
    assert share <= EXCLUDED_CAP
    assert not (differ & ~ex).any()
    # the depth itself: within its bound wherever both land
    both = landed & ref["landed"] & np.isfinite(de)
    assert (np.abs(e[both].astype(np.float64) - ref["e"][both]) <= de[both] * 1.0625).all()


# ------------------------------------------------------------------------------------------------ depth metrics
def metric_closed_form_failures(variant=None):
    bad = []

    def check(name, ok):
        if not ok:
            bad.append(name)

    m = lambda *a, **k: sr.metrics32_64(*a, variant=variant, **k)
    g = f32(np.linspace(0.5, 60.0, 200))
    # pred == gt: every sum is 0 and every delta is n
    s, c, b = m(g, g)
    check("equal", (s == 0).all() and c.tolist() == [200, 200, 200, 200, 0] and (b >= 0).all() and b.max() < 1e-9)
    # pred = 1.25 gt sits exactly ON the strict threshold (gt a power of two: the product and both quotients are exact)
    g2 = f32([1.0, 2.0, 4.0, 8.0])
    s, c, _ = m(f32(1.25) * g2, g2)
    check("strict", c.tolist() == [4, 0, 4, 4, 0])
    s, c, _ = m(g2, f32(1.5625) * g2)                       # ... symmetric in pred and gt, second threshold
    check("strict2", c.tolist() == [4, 0, 0, 4, 0])
    check("sums", np.allclose(s, [0.5625 * 15, 0.5625 ** 2 * 85, 4 * 0.5625 / 1.5625, 0.5625 ** 2 / 1.5625 * 15, 4 * np.log(1.5625) ** 2], rtol=1e-12))
    # a missing prediction (0, negative, NaN, Inf) counts as missing and nothing else
    p = g2.copy()
    p[0], p[1] = 0.0, np.nan
    s, c, _ = m(p, g2)
    check("missing", c.tolist() == [2, 2, 2, 2, 2] and (s == 0).all())
    s, c, _ = m(f32([-1.0, np.inf, 3.0, 8.0]), g2)
    check("missing2", c.tolist() == [2, 1, 2, 2, 2] and s[0] == 1.0)
    # gt outside the range, not finite, or masked off: the pixel does not count at all
    s, c, _ = m(g2, f32([1.0, 2.0, 90.0, 1e-4]), d_range=(1e-3, 80.0))
    check("range", c.tolist() == [2, 2, 2, 2, 0])
    s, c, _ = m(g2, f32([np.nan, np.inf, 0.0, 8.0]))
    check("gt_finite", c.tolist() == [1, 1, 1, 1, 0])
    s, c, _ = m(g2, g2, d_range=(2.0, 4.0))
    check("range_ends", c.tolist() == [2, 2, 2, 2, 0])
    s, c, _ = m(f32([0.0, 3.0, 4.0, 8.0]), g2, mask=np.array([0, 1, 0, 2], np.uint8))
    check("mask", c.tolist() == [2, 1, 2, 2, 0] and s[0] == 1.0)
    return bad


def test_metric_closed_forms():
    assert metric_closed_form_failures() == []


@pytest.mark.parametrize("variant,misses", [("le", "strict"), ("missing_in_sums", "missing")])
def test_corrupted_metric_variants_fail(variant, misses):
    assert misses in metric_closed_form_failures(variant)


def test_metric_bound_covers_another_summation_order_and_float128():
    g = np.random.default_rng(5)
    gt = f32(g.uniform(0.5, 70.0, 5000))
    pred = f32(gt * g.uniform(0.7, 1.4, 5000))
    s, c, b = sr.metrics32_64(pred, gt)
    p, q = pred.astype(np.longdouble), gt.astype(np.longdouble)
    d = p - q
    exact = [np.abs(d).sum(), (d * d).sum(), (np.abs(d) / q).sum(), (d * d / q).sum(), ((np.log(p) - np.log(q)) ** 2).sum()]
    assert all(abs(float(x) - y) <= bb for x, y, bb in zip(exact, s, b))
    assert (b / s < 1e-11).all()                           # a bound that says something: a dozen digits
    assert sr.summary(s, c)["depth_n"] == 5000 and abs(sr.summary(s, c)["depth_rmse"] - float(np.sqrt(exact[1] / 5000))) < 1e-12
