"""CPU tests of the depth front end's restatements (tests/_depth_ref.py; the rule is include/pnr.h "depth front end"): the two
float32 forms agree bit for bit, the rule's properties hold on constructed images, every corrupted variant fails a named check,
float32 against float64 outside a derived excluded set, and -- on the room of _icp_ref -- what normals made of a depth image are
worth to fusion.track and to a frame-to-frame odometry chain.  Nothing here touches a GPU."""
import numpy as np
import pytest

import _depth_ref as dr
import _icp_ref as ir

MODELS = ("pinhole", "fisheye", "equirect")
SOLVE_ARGS = dict(min_matches=64, max_rot=0.25, max_trans=0.5)
EYE = np.eye(4, dtype=np.float32)[:3]
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def pinhole(w, h, f=40.0):
    from panopticnerf_amd import Pinhole
    return Pinhole(f, f, (w - 1) / 2.0, (h - 1) / 2.0, w, h)


def patch(w=24, h=20, seed=2):
    """a small dirty crop of the room with noise: every pixel's window differs"""
    d = ir.room_maps(ir.cameras()["pinhole"], ir.TRUE_POSE)[0][:h, :w]
    return dr.dirty(dr.noisy(d, seed, rel=0.01), seed)


# ------------------------------------------------------------------------------------------------ the float32 forms
@pytest.mark.parametrize("radius,min_support", [(0, 1), (1, 2), (3, 1), (3, 6), (8, 1)])
def test_filter_loops_equal_the_vectorised_form(radius, min_support):
    d = patch()
    args = dict(radius=radius, sigma_space=1.5 if radius < 8 else 4.0, sigma_range=(0.01, 0.03), min_support=min_support)
    a, b = dr.filter_loops(d, **args), dr.filter32(d, **args)
    assert same(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (b[0][~dr._valid(d)] == 0).all() and (b[1][~dr._valid(d)] == 0).all()          # holes are not filled
    assert np.isfinite(b[0]).all() and b[1].max() <= (2 * radius + 1) ** 2 and (b[1][dr._valid(d)] >= 1).all()


@pytest.mark.parametrize("pose", ["identity", "turned"])
@pytest.mark.parametrize("name", MODELS)
def test_normals_loops_equal_the_vectorised_form(name, pose):
    cam = ir.cameras()[name]
    c2w = EYE if pose == "identity" else np.asarray(ir.TRUE_POSE, np.float32)
    d = dr.dirty(ir.room_maps(cam, ir.TRUE_POSE)[0], 5)
    view = ir.model_of(cam, c2w)
    a, b = dr.normals_loops(view, d), dr.normals32(view, d)
    for k in ("normal", "vertex", "code"):
        assert same(a[k], b[k]), k
    assert (b["code"] == dr.OK).sum() > 0.4 * d.size and (b["code"] == dr.NO_DEPTH).any() and (b["code"] == dr.NO_NEIGHBOUR).any()
    ok = b["code"] == dr.OK
    assert np.abs(np.linalg.norm(b["normal"][ok].astype(np.float64), axis=1) - 1).max() < 1e-6 and (b["normal"][~ok] == 0).all()
    assert (b["vertex"][b["code"] == dr.NO_DEPTH] == 0).all()
    # the normal faces the camera: (vertex - origin) . n < 0
    v = b["vertex"].astype(np.float64) - np.asarray(c2w, np.float64)[:, 3]
    assert ((v[ok] * b["normal"][ok]).sum(-1) < 0).all()


# ------------------------------------------------------------------------------------------------ the filter's properties
def test_a_constant_image_is_a_fixed_point():
    """a power of two bit for bit (every product w c is exact, so acc = c ws); any other constant within the rounding of the 2 n
    additions and n products of n = (2 r + 1)^2 positive terms, the product and the quotient: (3 n + 2) 2^-24 relative"""
    for r in (0, 1, 3, 8):
        out, sup = dr.filter32(np.full((19, 23), 4.0, np.float32), radius=r, sigma_space=2.0)
        assert same(out, np.full((19, 23), 4.0, np.float32))
        assert sup[9, 11] == (2 * min(r, 9) + 1) ** 2 and sup[0, 0] == (min(r, 18) + 1) * (min(r, 22) + 1)
        out, _ = dr.filter32(np.full((19, 23), 3.3, np.float32), radius=r, sigma_space=2.0)
        n = (2 * r + 1) ** 2
        assert np.abs(out.astype(np.float64) / float(np.float32(3.3)) - 1).max() <= (3 * n + 2) * 2.0 ** -24


def test_a_lone_pixel_is_removed_by_min_support():
    d = np.zeros((9, 9), np.float32)
    d[4, 4] = 2.5
    d[0, :] = 3.0                                        # a row with support of its own
    keep, sup = dr.filter32(d, radius=3, min_support=1)
    drop, sup2 = dr.filter32(d, radius=3, min_support=2)
    assert same(keep[4, 4], np.float32(2.5)) and drop[4, 4] == 0 and sup[4, 4] == 1 and sup2[4, 4] == 1
    assert (drop[0] > 0).all() and (drop[1:] == 0).all()
    # a speckle among good pixels: outside every neighbour's sigma, so it neither survives nor leaks
    d = np.full((9, 9), 2.0, np.float32)
    d[4, 4] = 3.5
    out, _ = dr.filter32(d, radius=2, min_support=2)
    assert out[4, 4] == 0 and same(np.delete(out.reshape(-1), 40), np.full(80, 2.0, np.float32))


def test_a_step_larger_than_sigma_is_not_blurred():
    """2 | 4 with sigma = 0.03 c: no pixel of one side is used by the other, and the pixels keep their bits (powers of two: the
    window's mean of equal values is exact)"""
    d = np.full((12, 16), 2.0, np.float32)
    d[:, 8:] = 4.0
    out, sup = dr.filter32(d, radius=3)
    assert same(out, d)
    assert sup[6, 7] == 7 * 4 and sup[6, 8] == 7 * 4 and sup[6, 3] == 7 * 7
    blurred, _ = dr.filter32(d, radius=3, sigma_range=(3.0, 0.0))                # a sigma wider than the step does blur
    assert 2.0 < blurred[6, 7] < blurred[6, 8] < 4.0
    # exactly one sigma away: u = 0, not used (the gate is u > 0)
    d = np.full((1, 2), 2.0, np.float32)
    d[0, 1] = 3.0
    out, sup = dr.filter32(d, radius=1, sigma_range=(1.0, 0.0))
    assert same(out, d) and sup.tolist() == [[1, 1]]


# ------------------------------------------------------------------------------------------------ the normals' properties
def test_a_fronto_parallel_wall_gives_the_exact_axis_normal():
    cam = pinhole(9, 7)
    out = dr.normals32(ir.model_of(cam, EYE), np.full((7, 9), 2.0, np.float32))
    assert (out["code"] == dr.OK).all()
    assert np.array_equal(out["normal"], np.tile(np.array([0.0, 0.0, -1.0], np.float32), (63, 1)))      # (the flip leaves -0 beside the -1)
    assert same(out["vertex"][:, 2], np.full(63, 2.0, np.float32))
    turned = np.array([[0, 0, 1, 5], [0, 1, 0, 6], [-1, 0, 0, 7]], np.float32)             # the camera looks along world +x
    out = dr.normals32(ir.model_of(cam, turned), np.full((7, 9), 2.0, np.float32))
    assert np.array_equal(out["normal"], np.tile(np.array([-1.0, 0.0, 0.0], np.float32), (63, 1))) and same(out["vertex"][:, 0], np.full(63, 7.0, np.float32))


def test_every_code_is_reached_by_a_constructed_pixel():
    cam = pinhole(7, 5)
    view = ir.model_of(cam, EYE)
    d = np.full((5, 7), 2.0, np.float32)
    d[0, 0] = 0.0                                        # NO_DEPTH
    d[2, 3] = 2.5                                        # beyond the jump gate of all four neighbours: NO_NEIGHBOUR
    d[4, 5], d[4, 4], d[4, 6], d[3, 5] = np.nan, 2.0, 2.0, 2.0
    out = dr.normals32(view, d)
    code = out["code"].reshape(5, 7)
    assert code[0, 0] == dr.NO_DEPTH and code[4, 5] == dr.NO_DEPTH and code[2, 3] == dr.NO_NEIGHBOUR
    assert code[2, 2] == dr.OK and code[0, 1] == dr.OK                          # one-sided differences next to the hole and the jump
    assert code[4, 4] == dr.OK and code[4, 6] == dr.NO_NEIGHBOUR                # the corner has no usable neighbour along x
    # one axis alone without a neighbour is enough
    one = dr.normals32(ir.model_of(pinhole(5, 1), EYE), np.full((1, 5), 2.0, np.float32))
    assert (one["code"] == dr.NO_NEIGHBOUR).all()
    # DEGENERATE: depths so small that every product of two differences underflows to 0
    tiny = dr.normals32(view, np.full((5, 7), 1e-30, np.float32))
    assert (tiny["code"] == dr.DEGENERATE).all() and (tiny["normal"] == 0).all() and (tiny["vertex"][:, 2] > 0).all()
    # GRAZING: a ramp seen at a cosine below min_cos, with the jump gate open
    ramp = (2.0 + 0.6 * np.arange(7, dtype=np.float32))[None, :].repeat(5, 0)
    steep = dr.normals32(view, ramp, jump=(INF, 0.0), min_cos=0.5)["code"].reshape(5, 7)
    loose = dr.normals32(view, ramp, jump=(INF, 0.0), min_cos=0.0)["code"].reshape(5, 7)
    assert (steep == dr.GRAZING).all() and (loose == dr.OK).all()
    a = dr.normals_loops(view, d)
    assert same(a["code"], out["code"]) and same(a["normal"], out["normal"])
    assert same(dr.normals_loops(view, np.full((5, 7), 1e-30, np.float32))["code"], tiny["code"])
    assert same(dr.normals_loops(view, ramp, jump=(INF, 0.0), min_cos=0.5)["code"], steep.reshape(-1))


def test_a_pixel_whose_s_is_exactly_zero():
    """geometrically a surface through two pixels never contains the ray between them, so s = 0 needs arithmetic: at the principal
    point v = (0, 0, t) and s = c_z t; with fx = 1e37 the product Dx_x Dy_y = c_z underflows to 0 while c_x = -(t_r - t_l) Dy_y does
    not.  s = 0 is GRAZING for any min_cos > 0 (0 < (mc2 cc) vv), and with min_cos = 0 it is OK and NOT negated (the flip is s > 0)"""
    from panopticnerf_amd import Pinhole
    cam = Pinhole(1e37, 1e10, 1.0, 1.0, 3, 3)
    view = ir.model_of(cam, EYE)
    d = np.full((3, 3), 2.5, np.float32)
    d[1, 0], d[1, 2] = 2.0, 3.0
    for fn in (dr.normals32, dr.normals_loops):
        graz = fn(view, d, jump=(INF, 0.0), min_cos=0.1)
        flat = fn(view, d, jump=(INF, 0.0), min_cos=0.0)
        assert graz["code"][4] == dr.GRAZING and (graz["normal"][4] == 0).all()
        assert flat["code"][4] == dr.OK and flat["normal"][4].tolist() == [-1.0, 0.0, 0.0]
    assert dr.normals32(view, d, jump=(INF, 0.0), min_cos=0.0)["s"][4] == 0.0


# ------------------------------------------------------------------------------------------------ the corrupted variants
def test_every_variant_fails_its_check():
    """order: the bits of a noisy patch;  gate: a neighbour exactly one sigma away;  support: the lone pixel at min_support = 1;
    sign: the wall's normal faces away;  world: the bits at KITTI-sized coordinates (and not at the origin);  onesided: the bits of
    the room (and never where only one side is usable)"""
    d = patch()
    args = dict(radius=3, sigma_range=(0.01, 0.03))
    assert not same(dr.filter32(d, variant="order", **args)[0], dr.filter32(d, **args)[0])
    assert same(dr.filter_loops(d, variant="order", **args)[0], dr.filter32(d, variant="order", **args)[0])
    edge = np.array([[2.0, 3.0]], np.float32)
    assert same(dr.filter32(edge, radius=1, sigma_range=(1.0, 0.0))[0], edge)
    assert not same(dr.filter32(edge, radius=1, sigma_range=(1.0, 0.0), variant="gate")[1], dr.filter32(edge, radius=1, sigma_range=(1.0, 0.0))[1])
    lone = np.zeros((5, 5), np.float32)
    lone[2, 2] = 2.0
    assert dr.filter32(lone, min_support=1)[0][2, 2] == 2.0 and dr.filter32(lone, min_support=1, variant="support")[0][2, 2] == 0.0
    for v in dr.FILTER_VARIANTS:
        a, b = dr.filter_loops(d, variant=v, min_support=3, **args), dr.filter32(d, variant=v, min_support=3, **args)
        assert same(a[0], b[0]) and np.array_equal(a[1], b[1]), v
    cam = pinhole(9, 7)
    wall = np.full((7, 9), 2.0, np.float32)
    assert (dr.normals32(ir.model_of(cam, EYE), wall, variant="sign")["normal"][:, 2] == 1.0).all()
    room_cam = ir.cameras()["pinhole"]
    rd = ir.room_maps(room_cam, ir.TRUE_POSE)[0]
    far = np.asarray(ir.TRUE_POSE, np.float32).copy()
    far[:, 3] += np.array([1203.7, 3817.3, 115.9], np.float32)
    near_v, far_v = ir.model_of(room_cam, ir.TRUE_POSE), ir.model_of(room_cam, far)
    assert same(dr.normals32(near_v, rd)["normal"], dr.normals32(far_v, rd)["normal"])                   # v does not see the origin
    assert not same(dr.normals32(far_v, rd, variant="world")["normal"], dr.normals32(far_v, rd)["normal"])
    ang = dr.angles(dr.normals32(far_v, rd, variant="world")["normal"], dr.normals32(far_v, rd)["normal"], dr.normals32(far_v, rd)["code"] == dr.OK)
    print("differences of vertex at %s: up to %.2f degrees off" % (far[:, 3].tolist(), ang.max()))
    assert ang.max() > 0.01                   # (an ulp of 3817 is 2.4e-4 against differences of about 0.1: some 0.1 degrees; v's own error is 1e-5)
    assert not same(dr.normals32(near_v, rd, variant="onesided")["normal"], dr.normals32(near_v, rd)["normal"])
    for v in dr.NORMALS_VARIANTS:
        a, b = dr.normals_loops(far_v, rd, variant=v), dr.normals32(far_v, rd, variant=v)
        assert same(a["normal"], b["normal"]) and same(a["code"], b["code"]), v


# ------------------------------------------------------------------------------------------------ float32 against float64
@pytest.mark.parametrize("name", MODELS)
def test_float32_codes_equal_float64_outside_the_excluded_set(name):
    """the codes agree wherever no deciding value lies within its first-order float32 error bound of its threshold; that set is at
    most 1 % of the pixels on these inputs (measured: 0 .. 0.3 %), and the normals of the pixels both call OK agree within 0.1 degree"""
    cam = ir.cameras()[name]
    for c2w, jump, min_cos in ((ir.TRUE_POSE, (0.0, 0.05), 0.1), (EYE, (0.02, 0.0), 0.3)):
        d = dr.dirty(ir.room_maps(cam, ir.TRUE_POSE)[0], 7)
        view = ir.model_of(cam, c2w)
        a, b = dr.normals32(view, d, jump, min_cos), dr.normals64(view, d, jump, min_cos)
        ex = dr.excluded(b, view, d, jump, min_cos)
        print("%s: %d of %d pixels excluded, %d codes differ" % (name, ex.sum(), ex.size, (a["code"] != b["code"]).sum()))
        assert ex.sum() <= 0.01 * ex.size
        assert np.array_equal(a["code"][~ex], b["code"][~ex])
        ok = (a["code"] == dr.OK) & (b["code"] == dr.OK)
        assert dr.angles(a["normal"], b["normal"], ok).max() < 0.1
        # the float32 ray lies within 2e-4 of the float64 one (the bound test_room_depth_range_cameras_and_poses holds the restated rays to)
        assert (np.abs(a["vertex"].astype(np.float64) - b["vertex"]).max(-1) <= 2e-4 * np.where(b["have"], d.reshape(-1), 0) + 1e-6).all()


def test_filter_float32_against_float64():
    """where both count the same pixels the float32 mean lies within (3 n + 2) 2^-24 of the float64 one (positive terms); the counts
    differ on no more than 1 % of the pixels of a noisy patch (a neighbour within one rounding of one sigma away)"""
    d = patch(48, 40, 3)
    a, b = dr.filter32(d, radius=3, sigma_range=(0.0, 0.03)), dr.filter64(d, radius=3, sigma_range=(0.0, 0.03))
    differ = a[1] != b[1]
    print("filter: %d of %d supports differ" % (differ.sum(), differ.size))
    assert differ.sum() <= 0.01 * differ.size
    m = ~differ & (b[0] > 0)
    assert np.abs(a[0][m].astype(np.float64) / b[0][m] - 1).max() <= (3 * 49 + 2) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the room
GUESS = ir.perturbed(np.asarray(ir.TRUE_POSE, np.float32), *ir.GUESS).astype(np.float32)


@pytest.mark.parametrize("name", MODELS)
def test_track_with_depth_derived_normals_on_the_room(name):
    """the model view's normals made of its depth image in place of the analytic ones: the share of pixels that get one, their angle to
    the analytic normal, and fusion.track restated with either.  Every status is ICP_OK, and the float32 track ends within 4 x the
    float64 restatement's own error + 1e-5 of the truth (the form of test_track_converges_on_the_room).
    Measured at these model views' 48 pixels across: a normal on 76 / 72 / 49 % of the valid pixels (pinhole / fisheye / equirect; 92 / 83 /
    57 % at 64 across), median angle 0, 9 - 12 % beyond 5 degrees
    (the creases between walls: depth is continuous there, so no jump gate sees them)"""
    cam, mcam = ir.cameras()[name], ir.cameras(0.75)[name]
    dl, _ = ir.room_maps(cam, ir.TRUE_POSE)
    dm, nm = ir.room_maps(mcam, ir.MODEL_POSE)
    model = ir.model_of(mcam, ir.MODEL_POSE)
    derived = dr.normals32(model, dm)
    ok = derived["code"] == dr.OK
    ang = dr.angles(derived["normal"], nm, ok)
    print("%s: a normal on %.1f %% of the valid pixels; angle to the analytic normal: median %.3g, mean %.3g, max %.3g degrees, %.1f %% beyond 5"
          % (name, 100.0 * ok.sum() / (dm > 0).sum(), np.median(ang), ang.mean(), ang.max(), 100.0 * (ang > 5).mean()))
    assert ok.sum() > 0.4 * (dm > 0).sum() and np.median(ang) < 0.01
    live = ir.live_of(cam)
    truth = np.asarray(ir.TRUE_POSE, np.float32)
    for label, normal in (("depth-derived", derived["normal"]), ("analytic", nm)):
        p32, h32, _, _ = ir.track(live, dl, GUESS, model, dm, normal, 10, 0.25, **SOLVE_ARGS)
        n64 = dr.normals64(model, dm)["normal"] if label == "depth-derived" else nm
        p64, h64, _, _ = ir.track(live, dl, GUESS, model, dm, n64, 10, 0.25, f=np.float64, **SOLVE_ARGS)
        e, e64 = ir.pose_error(p32, truth), ir.pose_error(p64, truth)
        print("  %s normals: final error %.3g rad, %.3g; the float64 restatement's %.3g rad, %.3g" % ((label,) + e + e64))
        assert (h32[:, 4] == ir.OK).all() and (h64[:, 4] == ir.OK).all()
        assert e[0] <= 4.0 * e64[0] + 1e-5 and e[1] <= 4.0 * e64[1] + 1e-5


@pytest.mark.parametrize("name", ["pinhole", "fisheye"])
def test_an_odometry_chain_of_five_steps(name):
    """six frames 1.4 degrees and 6.5 cm apart, frame to frame from guess identity, no volume: every status ICP_OK, and the float32
    chain's drift stays within 4 x the float64 restatement's + 1e-5"""
    cam = ir.cameras()[name]
    truths, depths = dr.room_sequence(cam, 6)
    poses, rel, hist = dr.odometry(cam, depths, c2w0=truths[0], iters=10, dist_max=0.25, **SOLVE_ARGS)
    poses64, rel64, hist64 = dr.odometry(cam, depths, c2w0=truths[0], iters=10, dist_max=0.25, f=np.float64, **SOLVE_ARGS)
    assert poses.shape == (6, 3, 4) and rel.shape == (5, 3, 4) and hist.shape == (5, 11, 5)
    assert (hist[:, :, 4] == ir.OK).all() and (hist64[:, :, 4] == ir.OK).all()
    for k in range(1, 6):
        e, e64 = ir.pose_error(poses[k], truths[k]), ir.pose_error(poses64[k], truths[k])
        print("%s frame %d: drift %.3g rad, %.3g; the float64 restatement's %.3g rad, %.3g" % ((name, k) + e + e64))
        assert e[0] <= 4.0 * e64[0] + 1e-5 and e[1] <= 4.0 * e64[1] + 1e-5
    # the velocity guess starts every step from the previous relative pose and ends no worse
    vel, _, hv = dr.odometry(cam, depths, c2w0=truths[0], guess="velocity", iters=10, dist_max=0.25, **SOLVE_ARGS)
    assert (hv[:, :, 4] == ir.OK).all()
    ev, e = ir.pose_error(vel[5], truths[5]), ir.pose_error(poses[5], truths[5])
    assert ev[0] <= 2.0 * e[0] + 1e-4 and ev[1] <= 2.0 * e[1] + 1e-4
    assert hv[1, 0, 1] < hist[1, 0, 1]                                           # the second step starts at a smaller residual


def test_the_filter_helps_the_normals_of_a_noisy_frame():
    """0.5 % multiplicative noise on the pinhole frame: the median angle to the analytic normal before and after a radius-3 filter
    (measured about 9 -> 4 degrees); no figure is fixed in advance: the filter must not make them worse"""
    cam = ir.cameras()["pinhole"]
    d, n = ir.room_maps(cam, ir.TRUE_POSE)
    view = ir.model_of(cam, ir.TRUE_POSE)
    noisy = dr.noisy(d, 11, rel=0.005)
    raw = dr.normals32(view, noisy)
    filt = dr.normals32(view, dr.filter32(noisy, radius=3)[0])
    a, b = dr.angles(raw["normal"], n, raw["code"] == dr.OK), dr.angles(filt["normal"], n, filt["code"] == dr.OK)
    print("median normal error: %.2f degrees raw, %.2f after the radius-3 filter" % (np.median(a), np.median(b)))
    assert np.median(b) < np.median(a)
