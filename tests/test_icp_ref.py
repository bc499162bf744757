"""CPU tests of the pose-tracking rule (include/pnr.h "pose tracking") as tests/_icp_ref.py restates it: the two float32 forms agree
bit for bit, closed forms worked by hand, deliberately wrong variants fail named checks, float32 against float64 outside a
derived excluded set, and convergence on the analytic room.  No GPU: tests/test_gpu_icp.py pins the kernels against these."""
import math

import numpy as np
import pytest

import _camera_ref as cr
import _icp_ref as ir

MODELS = ("pinhole", "fisheye", "equirect")
CAMS = ir.cameras()
TRUTH = np.asarray(ir.TRUE_POSE, np.float32)
GUESS = ir.perturbed(TRUTH, *ir.GUESS).astype(np.float32)
_scene = {}


def scene(ln, mn):
    """(live, live depth, model, model depth, model normal) of the room for a pairing of camera models; made once, never changed"""
    if (ln, mn) not in _scene:
        dl, _ = ir.room_maps(CAMS[ln], TRUTH)
        dm, nm = ir.room_maps(CAMS[mn], ir.MODEL_POSE)
        for a in (dl, dm, nm):
            a.setflags(write=False)
        _scene[ln, mn] = (ir.live_of(CAMS[ln]), dl, ir.model_of(CAMS[mn], ir.MODEL_POSE), dm, nm)
    return _scene[ln, mn]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------ the two float32 forms
@pytest.mark.parametrize("mn", MODELS)
@pytest.mark.parametrize("ln", MODELS)
def test_loops_equal_vectorised_bit_for_bit(ln, mn):
    live, dl, model, dm, nm = scene(ln, mn)
    dl, dm, nm = dl.copy(), dm.copy(), nm.copy()
    g = np.random.default_rng(7)
    for img, values in ((dl, (0.0, -1.0, np.nan, np.inf)), (dm, (0.0, -2.0, np.nan, np.inf))):
        flat = img.reshape(-1)
        flat[g.choice(flat.size, 40, replace=False)] = np.resize(np.array(values, np.float32), 40)
    nflat = nm.reshape(-1, 3)
    nflat[g.choice(nflat.shape[0], 20, replace=False)] = 0.0
    nflat[g.choice(nflat.shape[0], 20, replace=False), 1] = np.nan
    a = ir.accumulate32(live, dl, GUESS, model, dm, nm, 0.25)
    b = ir.accumulate_loops(live, dl, GUESS, model, dm, nm, 0.25)
    for k in ("code", "residual", "J"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["mq"], b["mq"])
    assert (a["code"] == ir.MATCH).sum() > 100


# ------------------------------------------------------------------------------------------------ closed forms by hand
WALL_Z, WALL_OFFSET = 5.0, 0.0625
_PIN = (ir.PINHOLE, (32.0, 32.0, 7.5, 5.5), 16, 12)          # focal lengths and centre exact in float32; no pixel on an axis but row 5.5


def _wall(variant=None, offset=WALL_OFFSET):
    """one wall z = WALL_Z seen head-on by the same pinhole on both sides; the live pose is `offset` too far along the normal"""
    eye = np.asarray(cr.pose(0.0), np.float32)
    model = (_PIN[0], _PIN[1], eye, _PIN[2], _PIN[3])
    n_pix = _PIN[2] * _PIN[3]
    dm = np.full(n_pix, WALL_Z, np.float32)
    nm = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (n_pix, 1))
    dl = np.full(n_pix, WALL_Z, np.float32)
    pose = eye.copy()
    pose[2, 3] = offset                                          # p_z = WALL_Z + offset: the live points lie behind the wall
    return ir.accumulate32(_PIN, dl, pose, model, dm, nm, 0.25, variant=variant if variant in ir.ACC_VARIANTS else None), pose, (model, dl, dm, nm)


def check_wall(variant=None):
    """every r is the offset (m lies `offset` in front of p along n = -z: r = n . (m - p) = +offset); the translation block of A is
    count n n^T; g's translation part is count offset n"""
    out, _, _ = _wall(variant)
    match = out["code"] == ir.MATCH
    T, idx = ir.terms(out)
    tot = T.sum(0)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = tot[:21]
    n = np.array([0.0, 0.0, -1.0])
    return bool(match.all() and np.all(out["residual"] == np.float32(WALL_OFFSET)) and np.array_equal(A[3:, 3:], match.sum() * np.outer(n, n))
                and np.array_equal(tot[24:27], match.sum() * WALL_OFFSET * n) and tot[27] == match.sum() * WALL_OFFSET ** 2)


def check_linearisation(variant=None):
    """r(pose moved by the twist x) = r - J x to first order, with the pairs held: the Jacobian, the sign of r, the centre of the
    twist and the side R_delta multiplies on must all fit each other.  In float64 on the room, at a turned pose."""
    live, dl, model, dm, nm = scene("pinhole", "fisheye")
    acc = variant if variant in ir.ACC_VARIANTS else None
    a = ir.accumulate64(live, dl, GUESS, model, dm, nm, 0.25, variant=acc)
    k = a["code"] == ir.MATCH
    x = np.array([2e-4, -3e-4, 1e-4, 3e-4, 1e-4, -2e-4])
    moved = ir.apply_twist(GUESS, list(x), variant if variant in ir.SOLVE_VARIANTS else None).astype(np.float64).reshape(3, 4)
    old = np.asarray(GUESS, np.float64).reshape(3, 4)
    p_cam = (a["p"][k] - old[:, 3]) @ old[:, :3]                  # R^T (p - T)
    p_new = p_cam @ moved[:, :3].T + moved[:, 3]
    r_new = np.einsum("ij,ij->i", a["n"][k], a["m"][k] - p_new) * (-1.0 if variant == "sign" else 1.0)
    predicted = a["residual"][k] - a["J"][k] @ x
    # second order in |x| ~ 5e-4 on arms of a few units: below 1e-6; the float32 store of the moved pose: 3 x 2^-24 x 4 units
    return bool(np.abs(r_new - predicted).max() < 3e-6)


def check_facing_zero(variant=None):
    """a pixel whose facing product is exactly 0 is BACK_FACING: n = +y and qv_y = 0 on the row j = cy of an unturned pinhole"""
    cam = (ir.PINHOLE, (32.0, 32.0, 7.5, 5.0), 16, 12)
    eye = np.asarray(cr.pose(0.0), np.float32)
    n_pix = 16 * 12
    nm = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (n_pix, 1))
    flat = np.full(n_pix, WALL_Z, np.float32)
    out = ir.accumulate32(cam, flat, eye, (cam[0], cam[1], eye, 16, 12), flat, nm, 0.25, variant=variant if variant in ir.ACC_VARIANTS else None)
    code = out["code"].reshape(12, 16)
    return bool(np.all(code[5] == ir.BACK_FACING) and np.all(code[:5] == ir.MATCH) and np.all(code[6:] == ir.BACK_FACING))


def check_nearest(variant=None):
    """the model is looked up at the NEAREST pixel: a live point that projects to u = 3.75 reads model column 4, not 3"""
    live = (ir.PINHOLE, (32.0, 32.0, 7.5, 5.5), 16, 12)
    mcam = (ir.PINHOLE, (24.0, 32.0, 7.5, 5.5), 16, 12)          # u_m = 0.75 (i - 7.5) + 7.5: i = 2.5 + ... live column 2 -> 3.375, 3 -> 4.125
    eye = np.asarray(cr.pose(0.0), np.float32)
    flat = np.full(16 * 12, WALL_Z, np.float32)
    nm = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (16 * 12, 1))
    out = ir.accumulate32(live, flat, eye, (mcam[0], mcam[1], eye, 16, 12), flat, nm, 0.25, variant=variant if variant in ir.ACC_VARIANTS else None)
    u = 0.75 * (np.arange(16) - 7.5) + 7.5
    want = np.minimum(np.floor(u + 0.5), 15).astype(np.int64)
    assert np.any(want != np.floor(u).astype(np.int64))
    return bool(np.array_equal(out["mq"].reshape(12, 16) % 16, np.tile(want, (12, 1))))


CHECKS = {"wall": check_wall, "linearisation": check_linearisation, "facing_zero": check_facing_zero, "nearest": check_nearest}
FAILS = {"sign": "wall", "cross": "linearisation", "origin": "linearisation", "gt": "facing_zero", "floor": "nearest", "right": "linearisation"}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_closed_forms_hold(name):
    assert CHECKS[name]()


@pytest.mark.parametrize("variant", ir.VARIANTS)
def test_every_variant_fails_its_check(variant):
    assert not CHECKS[FAILS[variant]](variant), "the check %r does not notice the wrong rule %r" % (FAILS[variant], variant)


def test_every_code_is_produced_by_a_constructed_pixel():
    """one 4 x 1 strip in front of a head-on wall, one pixel per code: a hole in the live depth, a live point that leaves the small
    model image, a hole in the model, a model normal of 0, a model point far behind, a normal that faces away, and a match"""
    live = (ir.PINHOLE, (32.0, 32.0, 3.5, 0.0), 8, 1)
    eye = np.asarray(cr.pose(0.0), np.float32)
    model = (ir.PINHOLE, (32.0, 32.0, 3.5, 0.0), eye, 7, 1)       # one column narrower: live column 7 leaves it
    dl = np.full(8, WALL_Z, np.float32)
    dm = np.full(7, WALL_Z, np.float32)
    nm = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (7, 1))
    dl[0] = 0.0                     # NO_DEPTH
    dm[1] = 0.0                     # NO_MODEL: a hole
    nm[2] = 0.0                     # NO_MODEL: no normal
    dm[3] = WALL_Z + 1.0            # TOO_FAR
    nm[4] = (0.0, 0.0, 1.0)         # BACK_FACING
    nm[5, 0] = np.nan               # NO_MODEL: a NaN component
    out = ir.accumulate32(live, dl, eye, model, dm, nm, 0.25)
    want = [ir.NO_DEPTH, ir.NO_MODEL, ir.NO_MODEL, ir.TOO_FAR, ir.BACK_FACING, ir.NO_MODEL, ir.MATCH, ir.OUTSIDE]
    assert out["code"].tolist() == want
    assert set(want) == set(ir.CODES.values())
    assert np.array_equal(out["code"], ir.accumulate_loops(live, dl, eye, model, dm, nm, 0.25)["code"])
    assert np.all(out["residual"] == 0) and np.all(out["J"][np.array(want) != ir.MATCH] == 0)
    # a point BEHIND a pinhole model camera is outside its domain; a fisheye live pixel outside the lens has no depth to lift
    back = np.asarray(cr.pose(math.pi), np.float32)
    assert np.all(ir.accumulate32(live, dl, back, model, dm, nm, 0.25)["code"][1:] == ir.OUTSIDE)
    fl, fdl, fm, fdm, fnm = scene("fisheye", "fisheye")
    o = ir.accumulate32(fl, np.ones_like(fdl), GUESS, fm, fdm, fnm, 0.25)
    assert o["code"][0] == ir.NO_DEPTH and fdl.reshape(-1)[0] == 0


# ------------------------------------------------------------------------------------------------ the solve
def _sums(ln="pinhole", mn="pinhole", pose=GUESS, keep=None):
    live, dl, model, dm, nm = scene(ln, mn)
    out = ir.accumulate32(live, dl, pose, model, dm, nm, 0.25)
    T, idx = ir.terms(out)
    if keep is not None:
        T = T[keep(out, idx)]
    return [math.fsum(T[:, k]) for k in range(ir.SUMS)], T.shape[0]


def test_a_single_plane_is_degenerate_and_the_room_is_not():
    """the pivot threshold 2^-30 of a pivot's own diagonal entry separates them cleanly: the room's smallest pivot ratio is above
    1e-3, a single wall's falls to 0 or to rounding noise (below 1e-12) whether it is seen head-on or obliquely"""
    tot, count = _sums()
    pose, row = ir.solve(tot, count, GUESS)
    assert row[4] == ir.OK and not np.array_equal(pose, GUESS.reshape(12))
    out, wall_pose, _ = _wall()
    T, idx = ir.terms(out)
    pose, row = ir.solve([math.fsum(T[:, k]) for k in range(ir.SUMS)], idx.size, wall_pose)
    assert row[4] == ir.DEGENERATE and row[2] == 0 and row[3] == 0 and np.array_equal(bits(pose), bits(wall_pose.reshape(12)))
    # one wall of the room alone, seen obliquely (the pose is turned by 14 degrees): the matches whose normal is -z
    tot, count = _sums(keep=lambda out, idx: out["J"][idx, 5] == -1.0)
    assert count > 100
    pose, row = ir.solve(tot, count, GUESS)
    assert row[4] == ir.DEGENERATE and np.array_equal(bits(pose), bits(GUESS.reshape(12)))
    # a plane in general position, n = (0.36, 0.48, -0.8) through (0, 0, 5): no entry of A is an exact zero
    n = np.array([0.36, 0.48, -0.8])
    i, j = np.meshgrid(np.arange(_PIN[2]), np.arange(_PIN[3]))
    dirs = np.stack([(i - _PIN[1][2]) / _PIN[1][0], (j - _PIN[1][3]) / _PIN[1][1], np.ones(i.shape)], -1)
    depth = (-4.0 / (dirs @ n)).astype(np.float32).reshape(-1)
    eye = np.asarray(cr.pose(0.0), np.float32)
    out = ir.accumulate32(_PIN, depth, eye, (_PIN[0], _PIN[1], eye, _PIN[2], _PIN[3]), depth, np.tile(n.astype(np.float32), (depth.size, 1)), 0.25)
    T, idx = ir.terms(out)
    assert idx.size == depth.size
    tilted = [math.fsum(T[:, k]) for k in range(ir.SUMS)]
    pose, row = ir.solve(tilted, idx.size, eye)
    assert row[4] == ir.DEGENERATE and np.array_equal(bits(pose), bits(eye.reshape(12)))
    ratios = [min(_pivot_ratios(s)) for s in (_sums()[0], tot, tilted)]
    print("smallest pivot / its diagonal entry: the room %.3g, one wall of it %.3g, a tilted plane %.3g; the threshold %.3g" % (*ratios, ir.PIVOT))
    assert ratios[0] > 1e-3 and abs(ratios[1]) < 1e-12 and abs(ratios[2]) < 1e-12


def _pivot_ratios(tot):
    """every pivot of the factorisation over its own diagonal entry of A, up to the first that is not positive (0 / 0 counts 0)"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = tot[:21]
    A = A + np.triu(A, 1).T
    L = np.zeros((6, 6))
    ratios = []
    for j in range(6):
        s = A[j, j] - (L[j, :j] ** 2).sum()
        ratios.append(s / A[j, j] if A[j, j] > 0 else 0.0)
        if not s > 0:
            break
        L[j, j] = math.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return ratios


def test_too_few_and_step_too_large_leave_the_pose_untouched():
    tot, count = _sums()
    pose, row = ir.solve(tot, count, GUESS, min_matches=count + 1)
    assert row == [float(count), tot[27], 0.0, 0.0, float(ir.TOO_FEW)] and np.array_equal(bits(pose), bits(GUESS.reshape(12)))
    pose, row = ir.solve(tot, count, GUESS, min_matches=count)
    assert row[4] == ir.OK
    pose, row = ir.solve(tot, count, GUESS, max_rot=1e-3)
    assert row[4] == ir.STEP_TOO_LARGE and row[2] > 1e-6 and np.array_equal(bits(pose), bits(GUESS.reshape(12)))
    pose, row = ir.solve(tot, count, GUESS, max_trans=1e-3)
    assert row[4] == ir.STEP_TOO_LARGE and row[3] > 1e-6 and np.array_equal(bits(pose), bits(GUESS.reshape(12)))
    pose, row = ir.solve(tot, count, GUESS, update=False)
    assert row == [float(count), tot[27], 0.0, 0.0, float(ir.OK)] and np.array_equal(bits(pose), bits(GUESS.reshape(12)))
    nan = list(tot)
    nan[21] = float("nan")
    pose, row = ir.solve(nan, count, GUESS)
    assert row[4] == ir.STEP_TOO_LARGE and np.array_equal(bits(pose), bits(GUESS.reshape(12)))


@pytest.mark.parametrize("theta", [0.0, 1e-8, 0.1, 0.5])
def test_series_against_math(theta):
    """8 terms: the first dropped terms at the cap theta = 0.5 are 0.25^8 / 17! = 2^-64.4 and 0.25^8 / 18! = 2^-68.5, below 2^-60;
    against math.sin / math.cos the difference is the roundings of the Horner form (a few 2^-53)"""
    a, b = ir.series(theta * theta)
    if theta == 0.0:
        assert a == 1.0 and b == 0.5
        return
    assert abs(a - math.sin(theta) / theta) <= 4 * 2.0 ** -53
    # 1 - cos cancels for small theta: 2 sin^2(theta / 2) / theta^2 is the same function without the cancellation
    assert abs(b - 2.0 * math.sin(theta / 2) ** 2 / theta ** 2) <= 4 * 2.0 ** -53
    if theta >= 0.1:
        assert abs(b - (1.0 - math.cos(theta)) / theta ** 2) <= 2.0 ** -53 / theta ** 2 + 4 * 2.0 ** -53


def test_series_truncation_at_the_cap_is_below_2_to_minus_60():
    s = ir.MAX_ROT ** 2
    assert s ** ir.SERIES_TERMS / math.factorial(2 * ir.SERIES_TERMS + 1) < 2.0 ** -60
    assert s ** ir.SERIES_TERMS / math.factorial(2 * ir.SERIES_TERMS + 2) < 2.0 ** -60
    assert s ** (ir.SERIES_TERMS - 1) / math.factorial(2 * ir.SERIES_TERMS) > 2.0 ** -60          # ... and 7 terms would not do for b
    a8, b8 = ir.series(s)
    a12, b12 = ir.series(s, 12)
    assert abs(a8 - a12) <= 2.0 ** -53 and abs(b8 - b12) <= 2.0 ** -53                             # (only roundings are left)


def test_the_update_is_a_rotation_about_the_camera_centre():
    x = [0.3, -0.2, 0.25, 0.01, -0.02, 0.03]
    new = ir.apply_twist(GUESS, x).astype(np.float64).reshape(3, 4)
    old = np.asarray(GUESS, np.float64).reshape(3, 4)
    Rd = new[:, :3] @ old[:, :3].T
    want = ir.perturbed(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), x[:3], (0, 0, 0))[:, :3]
    assert np.abs(Rd - want).max() < 4e-7                          # float32 storage of R and R'
    assert np.abs(new[:, 3] - (old[:, 3] + np.array(x[3:]))).max() < 2e-7


# ------------------------------------------------------------------------------------------------ float32 against float64
@pytest.mark.parametrize("mn", MODELS)
@pytest.mark.parametrize("ln", MODELS)
def test_float32_codes_equal_float64_outside_the_excluded_set(ln, mn):
    live, dl, model, dm, nm = scene(ln, mn)
    a = ir.accumulate32(live, dl, GUESS, model, dm, nm, 0.25)
    c = ir.accumulate64(live, dl, GUESS, model, dm, nm, 0.25)
    ex = ir.excluded(c, live, dl, GUESS, model, dm, nm)
    differ = a["code"] != c["code"]
    print("%s -> %s: %d pixels, %d excluded (%.2f %%), %d differ, %d of them outside the excluded set"
          % (ln, mn, ex.size, ex.sum(), 100.0 * ex.mean(), differ.sum(), (differ & ~ex).sum()))
    assert ex.mean() <= 0.01
    assert not np.any(differ & ~ex)
    both = (a["code"] == ir.MATCH) & (c["code"] == ir.MATCH) & ~ex
    # the residual is a difference of points a few units from the origin: a few float32 ulps of them
    assert np.abs(a["residual"][both] - c["residual"][both]).max() < 64 * ir.U32 * 4.0


# ------------------------------------------------------------------------------------------------ convergence
ITERS = 10


@pytest.mark.parametrize("ln,mn", [("pinhole", "pinhole"), ("fisheye", "equirect"), ("equirect", "fisheye")])
def test_track_converges_on_the_room(ln, mn):
    """From GUESS (1.6 degrees and 4.4 cm off) on room_depth frames with analytic model maps the pose error falls over each of the
    first two iterations (Gauss-Newton on planes: the third already sits on the floor), and after ITERS = 10 it lies below 4 x the
    float64 restatement's own final error + 1e-5 (rotation in radians and translation in world units alike).  Measured, float64 /
    float32 final (rotation, translation), from a start of (2.77e-2, 4.39e-2):
        pinhole -> pinhole    (5.32e-4, 1.142e-3) / (5.34e-4, 1.142e-3)
        fisheye -> equirect   (1.576e-3, 4.233e-3) / (1.569e-3, 4.233e-3)
        equirect -> fisheye   (6.52e-4, 5.55e-4) / (6.72e-4, 5.55e-4)
    The floor is not rounding: at a wall's edge a live point is paired with the neighbouring wall's model pixel (the images are
    64 pixels wide), and those pairs pull the same way in both precisions."""
    live, dl, model, dm, nm = scene(ln, mn)
    start = ir.pose_error(GUESS, TRUTH)
    p32, h32, _, poses32 = ir.track(live, dl, GUESS, model, dm, nm, ITERS, 0.25)
    p64, h64, _, _ = ir.track(live, dl, GUESS, model, dm, nm, ITERS, 0.25, f=np.float64)
    e32, e64 = ir.pose_error(p32, TRUTH), ir.pose_error(p64, TRUTH)
    errs = [start] + [ir.pose_error(p, TRUTH) for p in poses32]
    print("%s -> %s: start %s, float64 final %s, float32 final %s" % (ln, mn, start, e64, e32))
    print("   per iteration:", ["(%.2e, %.2e)" % e for e in errs])
    assert np.all(h32[:, 4] == ir.OK)
    for k in range(2):
        assert errs[k + 1][0] < errs[k][0] and errs[k + 1][1] < errs[k][1], (k, errs[k], errs[k + 1])
    assert e32[0] <= 4.0 * e64[0] + 1e-5 and e32[1] <= 4.0 * e64[1] + 1e-5
    assert e32[0] < 0.1 * start[0] and e32[1] < 0.1 * start[1]
    assert h32[-1, 1] < 0.5 * h32[0, 1]                             # E falls with it (what is left: the pairs across a wall's edge)
