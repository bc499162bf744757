"""The per-ray preamble on the CPU (COVERAGE.md rows a3, a4, a8): the float64 references of tests/_setup_ref.py against closed
forms worked by hand and against five corrupted variants of the rule; the C oracle (oracle/pnr_oracle.c, the float32 restatement
the kernels are held to bit for bit in tests/test_gpu_setup_sweep.py) against those references inside the bounds derived in
_setup_ref.py's docstring; and every PNR_EINVAL of the preamble's entry points, returned before anything is launched."""
import ctypes

import numpy as np
import pytest

import _mlp32_ref as m32
import _setup_ref as sr
from oracle import c_oracle as co
from panopticnerf_amd import _lib, synthetic

INF = np.inf
EYE = np.eye(3, dtype=np.float32).reshape(-1)
S2 = np.float32(np.sqrt(0.5))


def ray(o, d, near=0.0, far=100.0):
    return np.array([list(o) + list(d) + [near, far]], np.float32)


def boxes(*rows):
    """rows of (centre, rotation rows (9), half extents)"""
    return np.array([list(c) + list(rot) + list(e) for c, rot, e in rows], np.float32).reshape(-1, 15)


UNIT = boxes(((0, 0, 5), EYE, (1, 1, 1)))                                                   # [-1, 1]^2 x [4, 6] on the optical axis
ROT45 = boxes(((0, 0, 0), (S2, 0, S2, 0, 1, 0, -S2, 0, S2), (1, 1, 1)))                     # turned 45 degrees about y
COLUMN = boxes(*(((0, 0, zc), EYE, (1, 1, 1)) for zc in (50, 10, 40, 20, 30, 45)))         # test_bbox_hits_keep_nearest_and_report_overflow
COLUMN_RAY = ray((0.5, 0.5, 0), (0, 0, 1), 0.1, 80)


def rule64(rays, box, max_hits, variant=None):
    return sr.kept_lists(*sr.bbox_hits64(rays, box), max_hits, variant)


def rule32(rays, box, max_hits, variant=None):
    return sr.kept_lists(*sr.bbox_hits32(rays, box), max_hits, variant)


def rule_c(rays, box, max_hits, variant=None):
    return co.bbox_hits(rays, box, max_hits)


def first(rule, r, box, mh=1):
    t, b, c = rule(r, box, mh)
    return float(t[0, 0, 0]), float(t[0, 0, 1]), int(c[0])


def closed_forms(hits=rule64, strat=sr.stratified64, labels=sr.labels_loops, hull=sr.restrict64, embed=sr.embed64, variant=None):
    """every closed form of the issue, each worked by hand; AssertionError on the first that fails"""
    v = dict(variant=variant) if variant else {}
    # the unit box on the optical axis: in at z = 4, out at z = 6; d of length 2 halves the depths
    assert first(hits, ray((0, 0, 0), (0, 0, 1)), UNIT) == (4.0, 6.0, 1)
    assert first(hits, ray((0.5, -0.25, 0), (0, 0, 2)), UNIT) == (2.0, 3.0, 1)
    assert first(hits, ray((0, 0, 0), (0, 0, -1)), UNIT)[2] == 0                       # behind the camera
    assert first(hits, ray((0, 0, 0), (0, 0, 1), 0.0, 3.5), UNIT)[2] == 0              # far in front of the box
    assert first(hits, ray((0, 0, 0), (0, 0, 1), 4.5, 5.0), UNIT) == (4.5, 5.0, 1)     # [near, far] inside the box
    # turned 45 degrees: along world z the box is a diamond of half diagonal sqrt(2) -- to float64 rounding of S2
    t = first(hits, ray((0, 0, -4), (0, 0, 1)), ROT45)
    assert abs(t[0] - (4 - np.sqrt(2))) < 4e-6 and abs(t[1] - (4 + np.sqrt(2))) < 4e-6 and t[2] == 1
    t = first(hits, ray((1.0, 0, -4), (0, 0, 1)), ROT45)                               # off axis by 1: chord sqrt(2) - 1 each way
    assert abs(t[0] - (4 - (np.sqrt(2) - 1))) < 4e-6 and abs(t[1] - (4 + (np.sqrt(2) - 1))) < 4e-6
    assert first(hits, ray((1.5, 0, -4), (0, 0, 1)), ROT45)[2] == 0                    # past the corner at sqrt(2)
    # starting inside: t_in = near
    assert first(hits, ray((0, 0, 5), (0, 0, 1), 0.25), UNIT) == (0.25, 1.0, 1)
    assert first(hits, ray((0, 0, 5), (0, 0.5, 0), 0.25), UNIT) == (0.25, 2.0, 1)
    # along a face (dl = 0 on x and y): inside the slab hits, outside misses, exactly on the face misses (include/pnr.h)
    assert first(hits, ray((0.5, 0.5, 0), (0, 0, 1)), UNIT) == (4.0, 6.0, 1)
    assert first(hits, ray((1.5, 0.5, 0), (0, 0, 1)), UNIT)[2] == 0
    assert first(hits, ray((1.0, 0.0, 0), (0, 0, 1)), UNIT)[2] == 0
    assert first(hits, ray((-1.0, 0.0, 0), (0, 0, 1)), UNIT)[2] == 0
    # through an edge: t_in == t_out is a hit
    assert first(hits, ray((-2, 0, 5), (1, 0, 1)), UNIT) == (1.0, 1.0, 1)
    # the 6-box column: nearest first, the farthest dropped, the true count reported
    for mh in (1, 3, 6, 8):
        t, b, c = hits(COLUMN_RAY, COLUMN, mh, **v)
        assert int(c[0]) == 6 and list(b[0][: min(mh, 6)]) == [1, 3, 4, 2, 5, 0][: min(mh, 6)] and (b[0][6:] == -1).all()
        assert list(t[0, : min(mh, 6), 0]) == [9.0, 19.0, 29.0, 39.0, 44.0, 49.0][: min(mh, 6)]
    # depths
    r2 = np.concatenate([ray((0, 0, 0), (0, 0, 1), 0.5, 128.0), ray((0, 0, 0), (0, 0, 1), 2.0, 6.0)])
    for N in (2, 3, 50, 64, 129):
        for lindisp in (False, True):
            z = strat(r2, N, lindisp, **v)
            assert (z[:, 0] == r2[:, 6]).all() and (z[:, -1] == r2[:, 7]).all(), (N, lindisp)
    assert list(strat(r2, 5)[1]) == [2.0, 3.0, 4.0, 5.0, 6.0]
    assert np.allclose(strat(r2, 3, True)[1], [2.0, 3.0, 6.0], rtol=1e-6, atol=0)                              # 1 / z linear: 1/2, 1/3, 1/6
    assert list(strat(r2, 1)[:, 0]) == [0.5, 2.0] and list(strat(r2, 1, True)[:, 0]) == [0.5, 2.0]       # N = 1: near
    assert list(strat(r2, 1, False, np.full((2, 1), 0.75))[:, 0]) == [0.5, 2.0]        # one bin of width 0
    z = strat(r2, 5, False, np.full((2, 5), 0.5))[1]                                   # bins [2, 2.5] [2.5, 3.5] ... [5.5, 6]
    assert list(z) == [2.25, 3.0, 4.0, 5.0, 5.75]
    rng = np.random.default_rng(0)
    for lindisp in (False, True):
        tr = rng.random((2, 9))
        z0, z = strat(r2, 9, lindisp), strat(r2, 9, lindisp, tr)
        mids = 0.5 * (z0[:, 1:] + z0[:, :-1])
        slack = 4e-7 * np.abs(z)            # float32: lo + w t may round one ulp past the bin's end
        assert (z >= np.concatenate([z0[:, :1], mids], 1) - slack).all() and (z <= np.concatenate([mids, z0[:, -1:]], 1) + slack).all()
    # labels: the containing interval with the smallest t_in, ends included, ties to the earlier entry
    ht = np.array([[[2, 4], [3, 8], [3, 5], [9.5, 9.75]]], np.float32)
    hb, ids = np.array([[5, 1, 0, 2]], np.int32), np.array([[10, 20], [11, 21], [12, 22], [13, 23], [14, 24], [15, 25]], np.int32)
    z = np.array([[1.0, 2.0, 3.0, 4.0, 4.5, 8.0, 9.0, 9.625]], np.float32)
    ls, li = labels(z, ht, hb, np.array([3], np.int32), ids, **v)
    assert list(ls[0]) == [-1, 15, 15, 15, 11, 11, -1, -1] and list(li[0]) == [-1, 25, 25, 25, 21, 21, -1, -1]
    ls, _ = labels(z, ht, hb, np.array([7], np.int32), ids)                            # an overflowing count uses max_hits entries
    assert list(ls[0]) == [-1, 15, 15, 15, 11, 11, -1, 12]
    ls, _ = labels(z, ht, hb, np.array([1], np.int32), ids)
    assert list(ls[0]) == [-1, 15, 15, 15, -1, -1, -1, -1]
    # the hull: [min t_in, max t_out] over the kept entries; no hit: unchanged
    r3 = np.concatenate([ray((0, 0, 0), (0, 0, 1), 0.5, 100.0)] * 3)
    ht3 = np.array([[[2, 4], [3, 8], [3, 5]], [[2, 4], [3, 8], [3, 5]], [[0, 0], [0, 0], [0, 0]]], np.float32)
    out = hull(r3, ht3, np.array([3, 1, 0], np.int32), **v)
    assert [tuple(x) for x in out[:, 6:8]] == [(2.0, 8.0), (2.0, 4.0), (0.5, 100.0)] and (out[:, :6] == r3[:, :6]).all()
    assert tuple(hull(r3[:1], ht3[:1], np.array([9], np.int32))[0, 6:8]) == (2.0, 8.0)
    # the embedder at x = 0 and x = pi / 2 (float32): sin columns first
    e = embed(np.array([[0.0, 0.0, 0.0]], np.float32), 2, **v)
    assert list(e[0]) == [0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    x = np.array([[np.pi / 2, 0.0, -np.pi / 2]], np.float32)
    e = embed(x, 2)
    assert e.shape == (1, 15) and list(e[0, :3]) == list(x[0])
    assert np.allclose(e[0, 3:], [1, 0, -1, 0, 1, 0, 0, 0, 0, -1, 1, -1], atol=2e-7)
    assert embed(x, 0).shape == (1, 3)


def test_closed_forms():
    closed_forms()
    closed_forms(hits=rule32)
    closed_forms(hits=rule_c, strat=lambda r, N, lindisp=False, t=None: co.stratified(r, N, lindisp, t),
                 labels=lambda z, ht, hb, hc, ids: co.sample_labels(z, ht, hb, hc, ids),
                 hull=lambda r, ht, hc: co.restrict_rays(r, ht, hc), embed=lambda x, L: co.embed(x, L))
    closed_forms(labels=sr.labels_vec, hull=sr.hull_loops)


@pytest.mark.parametrize("which, variant", [("hits", "first"), ("labels", "strict"), ("hull", "hull0"), ("strat", "onesided"),
                                            ("embed", "swapcs")])
def test_corrupted_rules_fail_the_closed_forms(which, variant):
    """each variant corrupts one function of _setup_ref.py (`which`); the others ignore it"""
    with pytest.raises(AssertionError):
        closed_forms(variant=variant)


def test_min_max_rule():
    """include/pnr.h "a8: min / max": NaN loses, -0 below +0, in the reference and in the C oracle (through the hull)"""
    nz, pz, nan = np.float32(-0.0), np.float32(0.0), np.float32(np.nan)
    for a, b in ((nz, pz), (pz, nz)):
        assert np.signbit(sr.fmin(a, b)) and not np.signbit(sr.fmax(a, b))
    assert sr.fmin(nan, 1.0) == 1.0 and sr.fmin(1.0, nan) == 1.0 and sr.fmax(nan, -1.0) == -1.0 and np.isnan(sr.fmax(nan, nan))
    r = ray((0, 0, 0), (0, 0, 1), 0.5, 9.0)
    for t0, t1 in ((nz, pz), (pz, nz)):
        ht = np.array([[[t0, t0], [t1, t1]]], np.float32)
        for out in (co.restrict_rays(r, ht, np.array([2], np.int32)), sr.hull_loops(r, ht, np.array([2], np.int32))):
            assert out[0, 6] == 0 and np.signbit(out[0, 6]) and out[0, 7] == 0 and not np.signbit(out[0, 7])
    # a zero-extent box through the origin of a ray with near = 0: t1 = -0, t2 = +0 on every axis -> t_in = max(+0, -0) = +0
    z = boxes(((0, 0, 0), EYE, (0, 0, 0)))
    r = ray((0, 0, 0), (1, 1, 1), 0.0, 9.0)
    for t in (co.bbox_hits(r, z, 1), rule32(r, z, 1)):
        assert t[2][0] == 1 and t[0][0, 0, 0] == 0 and not np.signbit(t[0][0, 0, 0]) and not np.signbit(t[0][0, 0, 1])
    r = ray((0, 0, 0), (1, 1, 1), -1.0, 9.0)                                           # near below: t_in = min(-0, +0) = -0
    for t in (co.bbox_hits(r, z, 1), rule32(r, z, 1)):
        assert t[2][0] == 1 and np.signbit(t[0][0, 0, 0]) and t[0][0, 0, 0] == 0 and not np.signbit(t[0][0, 0, 1])


# ------------------------------------------------------------------------------------------------- the C oracle against float64
def scene_rays(n=20000):
    rays = synthetic.camera_rays(origin=(0.3, -0.2, 0.1))
    rays = rays[:: rays.shape[0] // n][:n].numpy()
    assert rays.shape[0] == n
    return rays


TABLES = ((12, 1, 1.0), (40, 1, 1.0), (64, 1, 1.0), (64, 5, 4.0))      # (boxes, seed, scale of the extents) of synthetic.random_boxes


def test_unsafe_rays_flag_what_float32_may_decide_otherwise():
    """a grazing ray, a duplicated box (tied t_in with a non-zero bound) and a ray along a box axis are unsafe; a plain hit, a
    plain miss and a box entered at `near` (bound 0) are not; a tie behind the cut of the list does not count"""
    far_box = boxes(((0.25, 0.5, 7), ROT45[0, 3:12], (1, 1, 1)))
    r = np.concatenate([ray((0.1, 0.2, -4), (0.01, 0.02, 1)), ray((5, 0.2, -4), (0.01, 0.02, 1)), ray((0.1, 0.2, 0.3), (0.3, 0.1, 1), 0.25)])
    assert not sr.unsafe_rays(r, ROT45, 2).any()
    graze = ray((np.sqrt(2), 0, -4), (1e-9, 1e-9, 1))                # past the diamond's corner by the rounding of sqrt(2)
    assert sr.unsafe_rays(graze, ROT45, 2).all()
    assert sr.unsafe_rays(r[:1], np.concatenate([ROT45, ROT45]), 2).all()
    assert sr.unsafe_rays(ray((0, 0, -4), (0, 0, 1)), UNIT, 2).all()
    three = np.concatenate([ROT45, far_box, far_box])
    assert sr.unsafe_rays(r[:1], three, 2).all() and not sr.unsafe_rays(r[:1], three, 1).any()
    b_in, b_out, deg = sr.interval_bounds(r, ROT45)
    assert not deg.any() and b_in[0, 0] > 0 and b_out[0, 0] > 0 and b_in[2, 0] == 0 and 0 < b_in[0, 0] < 1e-5


@pytest.mark.parametrize("n_box, seed, scale", TABLES)
def test_c_oracle_hits_against_float64(n_box, seed, scale):
    """20 000 pinhole rays against a seeded table, max_hits 2 and 8.  Outside the unsafe rays (_setup_ref.unsafe_rays: a decision
    whose float64 margin is below the derived bound; at most 1 %, a condition) counts and kept boxes are EQUAL and every kept
    depth lies inside interval_bounds of float64's.  The numpy float32 restatement equals the C oracle bit for bit everywhere."""
    rays = scene_rays()
    box = synthetic.random_boxes(n_box, seed=seed)[0].numpy()
    box[:, 12:15] *= scale
    chunks = [slice(i, i + 4000) for i in range(0, rays.shape[0], 4000)]
    h64 = [np.concatenate(x) for x in zip(*(sr.bbox_hits64(rays[c], box) for c in chunks))]
    b_in, b_out, _ = [np.concatenate(x) for x in zip(*(sr.interval_bounds(rays[c], box) for c in chunks))]
    h32 = sr.bbox_hits32(rays, box)
    for mh in (2, 8):
        unsafe = np.concatenate([sr.unsafe_rays(rays[c], box, mh) for c in chunks])
        print("table of %d boxes x %g, max_hits %d: %.3f %% of the rays excluded as unsafe, largest count %d"
              % (n_box, scale, mh, 100.0 * unsafe.mean(), sr.bbox_hits64(rays[::50], box)[2].sum(1).max()))
        assert unsafe.mean() <= 0.01
        c_t, c_b, c_n = co.bbox_hits(rays, box, mh)
        for got, ref in zip((c_t, c_b, c_n), sr.kept_lists(*h32, mh)):
            assert got.tobytes() == ref.tobytes()
        t64, b64, n64 = sr.kept_lists(*h64, mh)
        keep = ~unsafe
        assert np.array_equal(c_n[keep], n64[keep]) and np.array_equal(c_b[keep], b64[keep])
        assert n64[keep].max() >= 2                          # the scene is not trivial
        sel = keep[:, None] & (b64 >= 0)
        idx = np.maximum(b64, 0).astype(np.int64)
        worst = 0.0
        for end, b in enumerate((b_in, b_out)):
            tol = np.take_along_axis(b, idx, 1)
            err = np.abs(c_t[..., end].astype(np.float64) - t64[..., end])
            assert (err[sel] <= tol[sel]).all(), (mh, end, float((err[sel] - tol[sel]).max()))
            worst = max(worst, float((err[sel] / np.maximum(tol[sel], 1e-300)).max()))
        print("  worst |t32 - t64| / bound = %.3f" % worst)


def strat_rays(R, seed):
    rng = np.random.default_rng(seed)
    rays = np.zeros((R, 8), np.float32)
    rays[:, 6] = rng.uniform(0.05, 4.0, R)
    rays[:, 7] = rays[:, 6] + rng.uniform(0.0, 120.0, R)
    rays[0, 6:8] = (0.5, 100.0)
    rays[1, 6:8] = (2.0, 2.0)               # near == far
    rays[2, 6:8] = (3.0, 1.0)               # far < near
    return rays


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("jitter", [False, True])
def test_c_oracle_depths_against_float64_at_every_n(lindisp, jitter):
    rays = strat_rays(24, 5)
    rng = np.random.default_rng(11)
    worst = 0.0
    for N in range(1, 259):
        tr = rng.random((24, N)).astype(np.float32) if jitter else None
        if jitter:
            tr[3], tr[4] = 0.0, np.float32(1.0 - 2.0 ** -24)
        z = co.stratified(rays, N, lindisp, tr)
        ref, tol = sr.stratified64(rays, N, lindisp, tr), sr.stratified_bound(rays, N, lindisp, jitter)
        err = np.abs(z.astype(np.float64) - ref)
        assert (err <= tol).all(), (N, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
        if not jitter and not lindisp:
            assert (z[:, 0] == rays[:, 6]).all() and (N == 1 or (z[:, -1] == rays[:, 7]).all())
    print("lindisp %d jitter %d: worst |z32 - z64| / bound = %.3f" % (lindisp, jitter, worst))
    assert worst > 0.01         # the bound is not vacuous


def test_c_oracle_points_labels_hull():
    rays = scene_rays(3000)
    box, ids = synthetic.random_boxes(64, seed=1)
    box, ids = box.numpy(), ids.numpy()
    box[:, 12:15] *= 4.0                            # big boxes: every list overflows, intervals overlap
    rng = np.random.default_rng(2)
    for mh, N in ((1, 7), (3, 33), (8, 64)):
        ht, hb, hc = co.bbox_hits(rays, box, mh)
        assert hc.max() > mh
        out = co.restrict_rays(rays, ht, hc)
        assert out.tobytes() == sr.hull_loops(rays, ht, hc).tobytes()
        assert np.array_equal(out.astype(np.float64), sr.restrict64(rays, ht, hc))
        for use in (rays, out):
            z = co.stratified(use, N, False, rng.random((rays.shape[0], N)).astype(np.float32))
            z[::7, 0] = ht[::7, 0, 0]                    # samples exactly on an interval's ends
            z[::7, -1] = ht[::7, 0, 1]
            ls, li = co.sample_labels(z, ht, hb, hc, ids)
            a, b = sr.labels_vec(z, ht, hb, hc, ids)
            assert np.array_equal(ls, a) and np.array_equal(li, b)
            assert (ls >= 0).any() and (use is out or (ls < 0).any())
            a, b = sr.labels_loops(z[:200], ht[:200], hb[:200], hc[:200], ids)
            assert np.array_equal(ls[:200], a) and np.array_equal(li[:200], b)
            pts = co.points(use, z)
            err = np.abs(pts.astype(np.float64) - sr.points64(use, z))
            assert (err <= sr.points_bound(use, z)).all()


def embed_inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 30.0, (n, 3)).astype(np.float32)
    k = min(n, 4)
    x[:k] = np.array([[150.0, -150.0, 0.0], [-150.0, 150.0, 149.99], [0.0, -0.0, 1e-30], [3.1415927, 1.5707964, 100.0]], np.float32)[:k]
    return x


def test_c_oracle_embed_against_float64():
    x = embed_inputs(1001)
    for L in range(17):
        e = co.embed(x, L)
        ref = sr.embed64(x, L)
        assert e.shape == ref.shape == (1001, 3 + 6 * L)
        assert e[:, :3].tobytes() == x.tobytes()
        if L:
            err = np.abs(e[:, 3:].astype(np.float64) - ref[:, 3:])
            assert err.max() <= m32.TRIG_BOUND, (L, float(err.max()))
    print("host sinf / cosf: worst |float32 - float64| = %.3g at L = 16 (bound %.3g)" % (err.max(), m32.TRIG_BOUND))


# ------------------------------------------------------------------------------------------------------------------- refusals
PTR = ctypes.c_void_p(0x10000)          # a non-null, 32-byte aligned address that is never touched
ODD = ctypes.c_void_p(0x10004)
NULL = ctypes.c_void_p(0)


def _einval(rc, *words):
    assert rc == -1
    msg = _lib.load().pnr_last_error().decode()
    for w in words:
        assert w in msg, msg


def _rng(call=PTR, ray_base=0, tag=1, scale=1.0):
    return ctypes.byref(_lib.RngDesc(call.value, ray_base, tag, scale))


def test_stratified_points_embed_einval():
    lib = _lib.load()
    for R, N in ((-1, 4), (4, 0), (4, -2)):
        _einval(lib.pnr_stratified(PTR, R, N, 0, NULL, PTR, None), "pnr_stratified", "bad size")
        _einval(lib.pnr_stratified_rng(PTR, R, N, 0, _rng(), PTR, None), "pnr_stratified_rng")
        _einval(lib.pnr_points(PTR, PTR, R, N, PTR, None), "pnr_points", "bad size")
    _einval(lib.pnr_stratified_rng(PTR, 4, (1 << 26) + 1, 0, _rng(), PTR, None), "pnr_stratified_rng", "bad size")
    for rays, z in ((NULL, PTR), (PTR, NULL)):
        _einval(lib.pnr_stratified(rays, 4, 4, 0, NULL, z, None), "pnr_stratified", "null pointer")
        _einval(lib.pnr_stratified_rng(rays, 4, 4, 0, _rng(), z, None), "pnr_stratified_rng", "null pointer")
    for a in ((NULL, PTR, PTR), (PTR, NULL, PTR), (PTR, PTR, NULL)):
        _einval(lib.pnr_points(a[0], a[1], 4, 4, a[2], None), "pnr_points", "null pointer")
    _einval(lib.pnr_stratified_rng(PTR, 4, 4, 0, None, PTR, None), "pnr_stratified_rng", "null rng")
    _einval(lib.pnr_stratified_rng(PTR, 4, 4, 0, _rng(call=NULL), PTR, None), "pnr_stratified_rng", "null rng")
    for tag in (0, 256):
        _einval(lib.pnr_stratified_rng(PTR, 4, 4, 0, _rng(tag=tag), PTR, None), "pnr_stratified_rng", "tag")
    _einval(lib.pnr_stratified_rng(PTR, 4, 4, 0, _rng(scale=-1.0), PTR, None), "pnr_stratified_rng", "scale")
    _einval(lib.pnr_stratified_rng(PTR, 4, 4, 0, _rng(ray_base=(1 << 32) - 3), PTR, None), "pnr_stratified_rng", "ray_base")
    _einval(lib.pnr_stratified_rng(PTR, 4, 4, 0, _rng(call=ODD), PTR, None), "pnr_stratified_rng", "aligned")
    for n, L in ((-1, 4), (4, -1), (4, 17)):
        _einval(lib.pnr_embed(PTR, n, L, PTR, None), "pnr_embed", "bad size")
    _einval(lib.pnr_embed(NULL, 4, 4, PTR, None), "pnr_embed", "null pointer")
    _einval(lib.pnr_embed(PTR, 4, 4, NULL, None), "pnr_embed", "null pointer")
    # empty calls are no-ops, never refusals
    assert lib.pnr_stratified(NULL, 0, 4, 0, NULL, NULL, None) == 0 and lib.pnr_points(NULL, NULL, 0, 4, NULL, None) == 0
    assert lib.pnr_embed(NULL, 0, 16, NULL, None) == 0 and lib.pnr_stratified_rng(NULL, 0, 4, 0, _rng(), NULL, None) == 0


def test_bbox_labels_restrict_einval():
    lib = _lib.load()
    for i in range(4):
        a = [PTR, PTR, PTR, PTR]
        a[i] = NULL
        _einval(lib.pnr_bbox_hits(a[0], 4, PTR, 2, 2, a[1], a[2], a[3], None), "pnr_bbox_hits", "null pointer")
    _einval(lib.pnr_bbox_hits(PTR, 4, PTR, -1, 2, PTR, PTR, PTR, None), "pnr_bbox_hits", "bad box table")
    _einval(lib.pnr_bbox_hits(PTR, 4, NULL, 2, 2, PTR, PTR, PTR, None), "pnr_bbox_hits", "bad box table")
    for mh in (0, 65, -1):
        _einval(lib.pnr_bbox_hits(PTR, 4, PTR, 2, mh, PTR, PTR, PTR, None), "pnr_bbox_hits", "max_hits")
    assert lib.pnr_bbox_hits(NULL, 0, NULL, 0, 64, NULL, NULL, NULL, None) == 0

    def labels(z=PTR, R=4, N=4, ht=PTR, hb=PTR, hc=PTR, mh=2, ids=PTR, ls=PTR, li=PTR):
        return lib.pnr_sample_labels(z, R, N, ht, hb, hc, mh, ids, ls, li, None)
    for k in ("z", "ht", "hb", "hc", "ids", "ls", "li"):
        _einval(labels(**{k: NULL}), "pnr_sample_labels", "null pointer")
    for kw in (dict(N=0), dict(mh=0)):
        _einval(labels(**kw), "pnr_sample_labels", "bad size")
    assert labels(R=0, z=NULL, ls=NULL) == 0

    def restrict(rays=PTR, R=4, ht=PTR, hc=PTR, mh=2, out=PTR):
        return lib.pnr_restrict_rays(rays, R, ht, hc, mh, out, None)
    for kw in (dict(R=-1), dict(mh=0)):
        _einval(restrict(**kw), "pnr_restrict_rays", "bad size")
    for k in ("rays", "ht", "hc", "out"):
        _einval(restrict(**{k: NULL}), "pnr_restrict_rays", "null pointer")
    for k in ("rays", "out"):
        _einval(restrict(**{k: ODD}), "pnr_restrict_rays", "aligned")
    assert restrict(R=0, rays=NULL, out=NULL) == 0


def test_ray_setup_einval():
    lib = _lib.load()

    def plain(rays=PTR, R=4, box=PTR, M=2, mh=2, ids=PTR, N=4, tr=NULL, ht=PTR, hb=PTR, hc=PTR, z=PTR, ls=PTR, li=PTR):
        return lib.pnr_ray_setup(rays, R, box, M, mh, ids, N, 0, tr, 0, ht, hb, hc, z, ls, li, None)

    def twin(rays=PTR, R=4, box=PTR, M=2, mh=2, ids=PTR, N=4, tr=NULL, ht=PTR, hb=PTR, hc=PTR, z=PTR, ls=PTR, li=PTR):
        return lib.pnr_ray_setup_rng(rays, R, box, M, mh, ids, N, 0, _rng(), 0, ht, hb, hc, z, ls, li, None)

    for call in (plain, twin):
        for kw in (dict(R=-1), dict(N=0)):
            _einval(call(**kw), "pnr_ray_setup", "bad size")
        for mh in (0, 9, -1):
            _einval(call(mh=mh), "pnr_ray_setup", "max_hits", "[1,8]")
        _einval(call(M=-1), "pnr_ray_setup", "bad box table")
        _einval(call(box=NULL), "pnr_ray_setup", "bad box table")
        for k in ("rays", "ht", "hb", "hc", "z"):
            _einval(call(**{k: NULL}), "pnr_ray_setup", "null pointer")
        _einval(call(ls=NULL), "pnr_ray_setup", "labels need both outputs")
        _einval(call(li=NULL), "pnr_ray_setup", "labels need both outputs")
        _einval(call(ids=NULL), "pnr_ray_setup", "labels need both outputs and box_ids")
        _einval(call(rays=ODD), "pnr_ray_setup", "aligned")
        _einval(call(rays=ctypes.c_void_p(0x10008)), "pnr_ray_setup", "aligned")
        _einval(call(ht=ODD), "pnr_ray_setup", "aligned")
        assert call(R=0, rays=NULL, z=NULL) == 0
    _einval(lib.pnr_ray_setup_rng(PTR, 4, PTR, 2, 2, PTR, 4, 0, None, 0, PTR, PTR, PTR, PTR, PTR, PTR, None), "pnr_ray_setup_rng", "null rng")
    _einval(lib.pnr_ray_setup_rng(PTR, 4, PTR, 2, 2, PTR, 4, 0, _rng(tag=0), 0, PTR, PTR, PTR, PTR, PTR, PTR, None), "pnr_ray_setup_rng", "tag")
    _einval(lib.pnr_ray_setup_rng(PTR, 4, PTR, 2, 2, PTR, (1 << 26) + 1, 0, _rng(), 0, PTR, PTR, PTR, PTR, PTR, PTR, None),
            "pnr_ray_setup_rng", "n_samples", "2^26")
