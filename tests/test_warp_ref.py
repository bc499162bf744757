"""Pins tests/_warp_ref.py, the CPU references of cross-view reprojection (include/pnr.h "cross-view reprojection"), before
anything on the GPU is measured against them: closed-form answers that both restatements must give and that each corrupted
variant of the rule must miss, then float32 against float64 on whole frames of the two benchmark shapes.

float32 against float64: reproject32 and reproject64 must give the same code and the same target pixel everywhere outside an
excluded set, the pixels where the float64 u + 0.5 or v + 0.5 lies within the chain's float32 error bound of an integer, or
|e - dt| within its bound of the threshold.  The bound is derived from the roundings of the chain per pixel
(_warp_ref.E: running error analysis; _warp_ref.S: the same to first order with correlations kept, on the pixels E cannot
clear), never from the difference of the two evaluations.  Condition: at most 1 % of the pixels that have depth are excluded,
per pairing.  Measured here (whole frames, poses 0.5 m and 3 degrees apart, cameras inside a 15 m sphere):
    pinhole -> pinhole   0.12 % excluded,   26 pixels differ, all inside the excluded set
    fisheye -> fisheye   0.45 % excluded,  174 pixels differ, all inside (E's bound alone would exclude 1.5 %)
    fisheye -> pinhole   0.19 % excluded,   14 pixels differ, all inside
"""
import numpy as np
import pytest

import _camera_ref as cr
import _warp_ref as wr

f32 = lambda a: np.asarray(a, np.float32)
PIN_SMALL = (40.0, 41.0, 31.5, 23.5)
W1, H1 = 64, 48
FISH_SMALL = tuple(v * s for v, s in zip(cr.KITTI_FISHEYE, (1, 1, 1, 96 / 1400, 96 / 1400, 0, 0)))[:5] + (48.66, 47.9)
W2 = H2 = 96


def _view(model, cam, pose, w, h):
    return (model, f32(cam), f32(pose), w, h)


def _w2c(c2w):
    return f32(cr.invert_pose(f32(c2w).astype(np.float64)))


def _grid(w, h):
    return cr.pixel_grid(w, h)


# ------------------------------------------------------------------------------------------------ closed forms
def closed_form_failures(fn, variant=None):
    """Names of the closed-form checks that `fn` (reproject32 / reproject64), run with `variant`, does NOT pass."""
    bad = []
    kw = dict(variant=variant)

    def check(name, ok):
        if not ok:
            bad.append(name)

    # (1) the same camera, pose and depth image on both sides: every pixel with depth lands on itself
    c2w = cr.pose(0.3, -0.1, (0.5, 1.55, -1.0))
    for tag, model, cam, w, h in (("pinhole", wr.PINHOLE, PIN_SMALL, W1, H1), ("fisheye", wr.FISHEYE, FISH_SMALL, W2, H2)):
        i, j = _grid(w, h)
        depth = f32(6.0 + 2.0 * np.sin(i / 9.0) + np.cos(j / 7.0))
        depth[(i > 10) & (i < 14) & (j > 5) & (j < 9)] = 0.0
        depth[5] = np.nan
        depth[7] = np.inf
        depth[9] = -2.0
        out = fn(_view(model, cam, c2w, w, h), depth, _view(model, cam, _w2c(c2w), w, h), depth, tol=(0.0, 1e-5), **kw)
        m = out["match"]
        lens = np.ones(w * h, bool) if model == wr.PINHOLE else cr.unproject64(cam, w, h)[1]
        has = lens & (depth > 0) & np.isfinite(depth)
        check("identity_" + tag, np.array_equal(m[has], np.flatnonzero(has)))
        # (4a) zero, negative, NaN, Inf source depth and pixels outside the lens: nothing to reproject
        check("nothing_" + tag, (m[~has] == wr.NOTHING).all() and (~has).sum() > 10 and (model == wr.PINHOLE or (~lens).sum() > 100))
        check("stats_" + tag, np.array_equal(out["stats"], [has.sum(), (~has).sum(), 0, 0, 0]))
    # (2) a pinhole pair translated along camera x in front of a fronto-parallel plane: columns shift by round(fx b / Z)
    fx, Z, b = PIN_SMALL[0], 8.0, 0.66                      # fx b / Z = 3.3
    i, j = _grid(W1, H1)
    ca, cb = cr.pose(0.0), cr.pose(0.0, 0.0, (b, 0.0, 0.0))
    plane = np.full(W1 * H1, Z, np.float32)
    src, tgt = _view(wr.PINHOLE, PIN_SMALL, ca, W1, H1), _view(wr.PINHOLE, PIN_SMALL, _w2c(cb), W1, H1)
    m = fn(src, plane, tgt, plane, **kw)["match"]
    shift = int(round(fx * b / Z))
    want = np.where(i - fx * b / Z >= -0.5, j * W1 + i - shift, wr.LEFT_VIEW)
    check("shift", shift == 3 and np.array_equal(m, want))
    check("shift_no_depth_test", np.array_equal(fn(src, plane, tgt, None, **kw)["match"], want))
    # (3) a nearer surface in the target's depth image occludes exactly where it covers; so does a farther one (the test is two-sided)
    for name, other in (("nearer", Z / 2), ("farther", 2 * Z)):
        dt = plane.copy().reshape(H1, W1)
        dt[10:20, 30:45] = other
        covered = (j >= 10) & (j < 20) & (i - shift >= 30) & (i - shift < 45)
        m = fn(src, plane, tgt, dt, **kw)["match"]
        check("occluded_" + name, covered.sum() == 150 and np.array_equal(m, np.where(covered, wr.OCCLUDED, want)))
    # (4b) a zero (or NaN) target depth: unknown
    dt = plane.copy().reshape(H1, W1)
    dt[10:20, 30:45] = 0.0
    dt[12, 33] = np.nan
    check("unknown", np.array_equal(fn(src, plane, tgt, dt, **kw)["match"], np.where(covered, wr.UNKNOWN, want)))
    # (4c) a target that looks the other way: every point is behind it
    back = _view(wr.PINHOLE, PIN_SMALL, _w2c(cr.pose(np.pi, 0.0, (b, 0.0, 0.0))), W1, H1)
    check("behind", (fn(src, plane, back, plane, **kw)["match"] == wr.LEFT_VIEW).all())
    # (5) depth conventions across the models: a fisheye source (range) in a sphere around it, a pinhole target (z-depth) at
    # the same place: every pixel that lands in the other image is visible at the default 2 % (the nearest pixel's depth differs
    # by up to half a pixel's depth gradient, 0.6 % here)
    c2w = cr.pose(0.2, 0.05, (0.0, 1.5, 0.0))
    centre = c2w[:, 3]
    fs = _view(wr.FISHEYE, FISH_SMALL, c2w, W2, H2)
    ds = wr.sphere_depth(wr.FISHEYE, FISH_SMALL, c2w, W2, H2, centre, 9.0)
    dp = wr.sphere_depth(wr.PINHOLE, PIN_SMALL, c2w, W1, H1, centre, 9.0)
    m = fn(fs, ds, _view(wr.PINHOLE, PIN_SMALL, _w2c(c2w), W1, H1), dp, tol=(0.0, 0.02), **kw)["match"]
    check("cross_model", (m >= 0).sum() > 1000 and not (m <= wr.UNKNOWN).any())
    m = fn(_view(wr.PINHOLE, PIN_SMALL, c2w, W1, H1), dp, (fs[0], fs[1], _w2c(c2w), W2, H2), ds, tol=(0.0, 0.02), **kw)["match"]
    check("cross_model_back", (m >= 0).sum() > 1000 and not (m <= wr.UNKNOWN).any())
    return bad


@pytest.mark.parametrize("fn", [wr.reproject32, wr.reproject64], ids=["float32", "float64"])
def test_closed_forms(fn):
    assert closed_form_failures(fn) == []


@pytest.mark.parametrize("variant", wr.VARIANTS)
def test_corrupted_variants_fail_the_closed_forms(variant):
    """the checks can fail: each deliberately wrong rule misses at least one of them, in both precisions"""
    for fn in (wr.reproject32, wr.reproject64):
        bad = closed_form_failures(fn, variant)
        print(variant, fn.__name__, "fails", bad)
        assert bad, variant
    assert len(wr.VARIANTS) >= 3


def test_labels_and_counters():
    """agree counts visible pixels with both labels in range; pix lists index the source image; out-of-image indices are -1"""
    i, j = _grid(W1, H1)
    plane = np.full(W1 * H1, 8.0, np.float32)
    src = _view(wr.PINHOLE, PIN_SMALL, cr.pose(0.0), W1, H1)
    tgt = _view(wr.PINHOLE, PIN_SMALL, _w2c(cr.pose(0.0, 0.0, (0.66, 0.0, 0.0))), W1, H1)
    ls = (i // 16).astype(np.int32)
    lt = ((i + 3) // 16).astype(np.int32)               # the target's labels, shifted with the view: they agree everywhere
    lt[j == 4] = -1
    lt[j == 5] = 7
    out = wr.reproject32(src, plane, tgt, plane, label_src=ls, label_tgt=lt, n_classes=4)
    seen = (out["match"] >= 0) & (j != 4) & (j != 5)
    assert np.array_equal(out["agree"], np.diag(np.bincount(ls[seen], minlength=4)))
    assert out["agree"].sum() == seen.sum() < (out["match"] >= 0).sum()
    pix = np.array([5, 100, -3, W1 * H1, 77], np.int64)
    sub = wr.reproject32(src, plane, tgt, plane, pix=pix)
    assert np.array_equal(sub["match"], [out["match"][5], out["match"][100], -1, -1, out["match"][77]])
    assert np.array_equal(sub["stats"], [3, 2, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ float32 against float64
PIN = (552.554261, 552.554261, 682.049453, 238.769549)
POSE_A = cr.pose(0.0, 0.0, (0.0, 1.55, 0.0))
POSE_B = cr.pose(0.05, -0.03, (0.3, 1.5, 0.4))            # 0.5 m and 3.3 degrees from A
SPHERE = ((1.0, 0.0, 3.0), 15.0)
MAX_EXCLUDED = 0.01


def frame_pair(kind_s, kind_t):
    """(src, depth_src, tgt, depth_tgt) of one pairing on whole benchmark-shaped frames: both cameras inside a sphere (a
    smooth analytic depth image on either side, in each model's own convention); the target's depth is modulated by +-3 % so
    that the 2 % depth test passes and fails over smooth regions."""
    mk = {"pinhole": lambda: (wr.PINHOLE, f32(PIN), 1408, 376), "fisheye": lambda: (wr.FISHEYE, f32(cr.KITTI_FISHEYE), 1400, 1400)}
    ms, cs, ws, hs = mk[kind_s]()
    mt, ct, wt, ht = mk[kind_t]()
    ca, cb = f32(POSE_A), f32(POSE_B)
    ds = wr.sphere_depth(ms, cs, ca, ws, hs, *SPHERE)
    dt = wr.sphere_depth(mt, ct, cb, wt, ht, *SPHERE).reshape(-1)
    i, j = _grid(wt, ht)
    dt = (dt * (1.0 + 0.03 * np.sin(i / 97.0) * np.cos(j / 61.0))).astype(np.float32)
    return (ms, cs, ca, ws, hs), ds, (mt, ct, _w2c(cb), wt, ht), dt


@pytest.mark.parametrize("kind_s,kind_t", [("pinhole", "pinhole"), ("fisheye", "fisheye"), ("fisheye", "pinhole")])
def test_float32_against_float64_on_whole_frames(kind_s, kind_t):
    src, ds, tgt, dt = frame_pair(kind_s, kind_t)
    tol = (0.0, 0.02)
    a = wr.reproject32(src, ds, tgt, dt, tol)
    b = wr.reproject64(src, ds, tgt, dt, tol)
    ex, du = wr.excluded(b, src, ds, tgt, tol)
    have = b["have"]
    share = ex.sum() / have.sum()
    differ = a["match"] != b["match"]
    both = have & (a["match"] != wr.LEFT_VIEW) & (b["match"] != wr.LEFT_VIEW) & np.isfinite(du)
    err = np.abs(a["uv"].astype(np.float64) - b["uv"]).max(-1)
    print("%s -> %s: %d pixels with depth, %.3f %% excluded, %d differ (%d outside the excluded set); codes %s; max |uv32 - uv64| = %.2e px"
          % (kind_s, kind_t, have.sum(), 100 * share, differ.sum(), (differ & ~ex).sum(), a["stats"].tolist(), err[both].max()))
    assert share <= MAX_EXCLUDED
    assert not (differ & ~ex).any()
    # the comparison is not vacuous: every code occurs (no unknown: the sphere is seen everywhere), and the bound holds where it is finite
    assert (a["stats"][[0, 2, 4]] > 1000).all() and (kind_s == "pinhole" or a["stats"][1] > 1000)
    assert (err[both] <= wr.INFLATE * (du[both] + wr.U32 * 1408.0)).all()          # (uv is u without the + 0.5: one rounding less)
