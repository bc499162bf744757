"""Pins tests/_tsdf_ref.py, the CPU references of depth fusion (include/pnr.h "depth fusion"), before anything on the GPU is
measured against them: the two float32 restatements agree bit for bit; closed forms worked by hand that integrate32 must give
and that each corrupted variant of the rule must miss; float32 against float64 per lattice point; the extract filter.

float32 against float64: one frame fused into an empty volume, per camera of _tsdf_ref.CAMERAS, on a 33^3 lattice round the
whole sphere.  Outside an excluded set the two must make the same decision (fused or not) and their tsdf must agree within
_tsdf_ref.single_frame_bound, which is derived from the roundings of the chain (_splat_ref.project_bound, then one subtraction
and one division), never from the difference of the two evaluations.  Condition: at most 1 % of the points excluded, per view.
Measured here (35 937 points, trunc 0.8):
    pinhole_a   0.003 % excluded    pinhole_b   0.008 %         no decision differs in any view, excluded points included;
    fisheye_a   0.019 %             fisheye_b   0.019 %         the largest |tsdf32 - tsdf64| uses 0.32 .. 0.61 of its bound
    equirect_a  0.000 %             equirect_b  0.017 %
(equirect_a stands at y = 1.07, not 1.0: at 1.0 one whole lattice plane lies on the horizon, which is the border between two
pixel rows, and 3 % of the points are rightly excluded for their pixel choice.)
"""
import numpy as np
import pytest
import torch

import _camera_ref as cr
import _mesh_ref as mr
import _pano_ref as pr
import _tsdf_ref as tr
from panopticnerf_amd import fusion

f32 = lambda a: np.asarray(a, np.float32)
EYE = f32(cr.pose(0.0))
PIN = f32((20.0, 20.0, 15.5, 11.5))
PW, PH = 32, 24
FISH = f32(tr._FISH)
KEYS = ("tsdf", "weight", "rgb", "rgb_weight", "label", "conf")


def same_bits(a, b):
    return all(k in b and a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a) and set(a) == set(b)


def const_frame(model, cam, w, h, depth, rgb=None, sem=None, inst=None):
    full = lambda v, dt, tail=(): None if v is None else np.full((h, w) + tail, v, dt)
    return tr.frame((model, cam, EYE, w, h), full(depth, np.float32), full(rgb, np.uint8, (3,)), full(sem, np.int16), full(inst, np.int16))


# ------------------------------------------------------------------------------------------------ 1: the two restatements
def test_loops_equal_vectorised():
    lo, hi, res = (-2.5, -1.0, 4.5), (3.0, 3.0, 8.0), (9, 7, 6)
    pts = tr.points(lo, hi, res)
    few = {"n_sem": 2, "n_inst": 1}                 # few keys: votes meet
    frames = [tr.sphere_frame("pinhole_a", 1, **few), tr.sphere_frame("fisheye_a", 2, inst=False, **few), tr.sphere_frame("equirect_b", 3, **few),
              tr.sphere_frame("pinhole_b", 4, depth=False), tr.sphere_frame("equirect_a", 5, sem=False), tr.sphere_frame("fisheye_b", 6, **few),
              tr.sphere_frame("pinhole_a", 7, **few)]
    frames[0]["depth"][::3, ::2] = 0.0
    frames[2]["depth"][5, :] = np.nan
    frames[5]["depth"][:, 40] = np.inf
    frames[6]["depth"][10:20] = -1.0
    touched = 0
    for trunc, w_max, max_depth, color, labels in ((0.4, np.inf, np.inf, True, True), (2.5, 3.0, np.inf, True, False), (1.0, 1.0, 6.0, False, True),
                                                   (0.9, np.inf, 5.5, False, False)):
        st0 = tr.new_state(len(pts), color, labels)
        a = tr.integrate_loops(st0, frames, pts, trunc, max_depth, w_max)
        b = tr.integrate32(st0, frames, pts, trunc, max_depth, w_max)
        assert same_bits(a, b), (trunc, w_max)
        assert (b["weight"] > 0).sum() > 20 and ((b["weight"] == 0).sum() > 0 or trunc > 2.0)
        # a split call accumulates to the same bits
        c = tr.integrate32(tr.integrate32(st0, frames, pts, trunc, max_depth, w_max, 0, 3), frames, pts, trunc, max_depth, w_max, 3, 7)
        assert same_bits(b, c)
        if w_max == 3.0:
            assert b["weight"].max() == 3.0 and b["rgb_weight"].max() == 3.0
        if labels:
            assert (b["label"] >= 0).any() and (b["conf"] > 1).any() and (b["label"][b["weight"] == 0] == -1).all()
        touched += int((b["weight"] > 0).sum())
    assert touched > 200


# ------------------------------------------------------------------------------------------------ 2: closed forms and variants
def closed_form_failures(variant=None):
    """Names of the closed-form checks that integrate32, run with `variant`, does NOT pass."""
    bad = []

    def check(name, ok):
        if not bool(ok):
            bad.append(name)

    def run(frames, pts, trunc, color=False, labels=False, **kw):
        pts = f32(pts).reshape(-1, 3)
        return tr.integrate32(tr.new_state(len(pts), color, labels), frames, pts, trunc, variant=variant, **kw)

    # (1) the plane z = 2 seen by an axis-aligned pinhole camera: p_cam.z = Z exactly, every value below a multiple of 1/8
    lo, hi, res = (-0.5, -0.5, 1.0), (0.5, 0.5, 3.5), (3, 3, 10)
    pts = tr.points(lo, hi, res)
    st = run([const_frame(tr.PINHOLE, PIN, PW, PH, 2.0)], pts, 0.5)
    z = pts[:, 2]
    want = np.clip((z - np.float32(2.0)) / np.float32(0.5), -1.0, None).astype(np.float32)
    hidden = z - 2.0 > 0.5
    check("plane", np.array_equal(st["tsdf"][~hidden], want[~hidden]) and (st["weight"][~hidden] == 1).all() and (want[~hidden] <= 0.75).all()
          and (want == -1).sum() == 18 and (want == 0.75).sum() == 9)
    check("plane_hidden", (st["tsdf"][hidden] == 0).all() and (st["weight"][hidden] == 0).all() and hidden.sum() == 36)
    # (2) the band's two ends belong to it: s == trunc is fused with phi = 1, s == -trunc is coloured; just beyond neither
    fr = const_frame(tr.PINHOLE, PIN, PW, PH, 2.0, rgb=200)
    st = run([fr], [[0, 0, 2.5], [0, 0, 2.625], [0, 0, 1.5], [0, 0, 1.375]], 0.5, color=True)
    check("boundary_trunc", st["tsdf"].tolist() == [1.0, 0.0, -1.0, -1.0] and st["weight"].tolist() == [1.0, 0.0, 1.0, 1.0])
    check("boundary_colour", st["rgb_weight"].tolist() == [1.0, 0.0, 1.0, 0.0] and st["rgb"][:, 1].tolist() == [200.0, 0.0, 200.0, 0.0])
    # (3) the nearest pixel, halves up: u = x / z with the unit camera; column c holds the depth 0.5 + c / 64
    unit = f32((1.0, 1.0, 0.0, 0.0))
    depth = np.broadcast_to(0.5 + np.arange(32, dtype=np.float32) / 64, (8, 32))
    st = run([tr.frame((tr.PINHOLE, unit, EYE, 32, 8), depth)], [[10.7, 3, 1], [10.5, 3, 1], [10.3, 3, 1]], 1.0)
    check("nearest_pixel", st["tsdf"].tolist() == [1.0 - (0.5 + 11 / 64), 1.0 - (0.5 + 11 / 64), 1.0 - (0.5 + 10 / 64)])
    # (4) a fisheye camera at the centre of a sphere of constant RANGE 2: phi = (|X| - 2) / trunc, whatever the direction
    g = np.random.default_rng(0)
    d = g.normal(size=(200, 3)) * (1, 1, 0.3) + (0, 0, 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    X = f32(d * g.uniform(1.6, 2.4, (200, 1)))
    st = run([const_frame(tr.FISHEYE, FISH, 80, 80, 2.0)], X, 0.5)
    seen = st["weight"] == 1
    want = (np.linalg.norm(X.astype(np.float64), axis=1) - 2.0) / 0.5
    check("fisheye_sphere", seen.sum() > 100 and np.abs(st["tsdf"][seen] - want[seen]).max() < 1e-6 and np.abs(want[seen]).max() > 0.5)
    # ... while a pinhole view of a plane stores z: off the axis the range would be wrong
    st = run([const_frame(tr.PINHOLE, PIN, PW, PH, 2.0)], [[0.5, 0.25, 2.25]], 0.5)
    check("pinhole_z", st["tsdf"].tolist() == [0.5])
    # (5) the running mean of two and three frames (phi = 0.2, -0.2, -0.6), its weights, and w_max = 1
    frames = [const_frame(tr.PINHOLE, PIN, PW, PH, dd, rgb=c) for dd, c in ((1.9, 10), (2.1, 20), (2.3, 60))]
    P = [[0, 0, 2.0]]
    st1, st2, st3 = run(frames[:1], P, 0.5, color=True), run(frames[:2], P, 0.5, color=True), run(frames, P, 0.5, color=True)
    check("mean1", abs(st1["tsdf"][0] - 0.2) < 1e-6 and st1["weight"][0] == 1)
    check("mean2", abs(st2["tsdf"][0] - 0.0) < 1e-6 and st2["weight"][0] == 2 and abs(st2["rgb"][0, 0] - 15.0) < 1e-5)
    check("mean3", abs(st3["tsdf"][0] + 0.2) < 1e-6 and st3["weight"][0] == 3 and abs(st3["rgb"][0, 2] - 30.0) < 1e-5 and st3["rgb_weight"][0] == 3)
    stc = run(frames, P, 0.5, color=True, w_max=1.0)
    check("w_max_1", abs(stc["tsdf"][0] + 0.3) < 1e-6 and stc["weight"][0] == 1 and abs(stc["rgb"][0, 0] - 37.5) < 1e-5 and stc["rgb_weight"][0] == 1)
    # ... max_depth: the third frame's 2.3 is beyond 2.2 and is ignored
    stm = run(frames, P, 0.5, max_depth=2.2)
    check("max_depth", stm["weight"][0] == 2 and abs(stm["tsdf"][0]) < 1e-6)
    # (6) Boyer-Moore votes: sequences of (sem, inst) keys, and a pixel without a label
    a, b, c = (3, 7), (4, -1), (3, 8)
    for name, seq, want in (("vote_aab", (a, a, b), (a, 1)), ("vote_abb", (a, b, b), (b, 1)), ("vote_abc", (a, b, c), (c, 1)),
                            ("vote_aaa", (a, a, a), (a, 3)), ("vote_a_none_a", (a, (-1, 5), a), (a, 2)), ("vote_none", ((-1, 5),), None)):
        frames = [const_frame(tr.PINHOLE, PIN, PW, PH, 2.0, sem=s, inst=i) for s, i in seq]
        st = run(frames, P, 0.5, labels=True)
        lab, cf = int(st["label"][0]), int(st["conf"][0])
        if want is None:
            check(name, lab == -1 and cf == 0)
        else:
            sem, inst = tr.unpack(st["label"])
            check(name, lab == tr.pack(*want[0]) and cf == want[1] and (int(sem[0]), int(inst[0])) == want[0])
    # ... a frame without inst votes with inst = -1; one without sem does not vote; one without depth does nothing
    frames = [const_frame(tr.PINHOLE, PIN, PW, PH, 2.0, sem=2), const_frame(tr.PINHOLE, PIN, PW, PH, 2.0, inst=9),
              const_frame(tr.PINHOLE, PIN, PW, PH, None, sem=1, inst=1)]
    st = run(frames, P, 0.5, labels=True)
    check("vote_missing_images", int(st["label"][0]) == tr.pack(2, -1) and int(st["conf"][0]) == 1 and st["weight"][0] == 2)
    return bad


def test_closed_forms():
    assert closed_form_failures() == []


@pytest.mark.parametrize("variant, named", [("sign", "plane"), ("ge", "boundary_trunc"), ("weight_first", "mean3"), ("trunc_pixel", "nearest_pixel"),
                                            ("z_fisheye", "fisheye_sphere"), ("vote_replace", "vote_abb")])
def test_corrupted_variants_fail(variant, named):
    assert variant in tr.VARIANTS
    bad = closed_form_failures(variant)
    assert named in bad, (variant, bad)


def test_variants_all_covered():
    assert len(tr.VARIANTS) >= 6


def test_equirect_sphere_and_its_mesh():
    """an Equirect camera at the centre of a sphere of constant range r: tsdf = (|X| - r) / trunc in the band, and the filtered
    mesh of the fused volume has the volume of the mesh of the analytic field on the same lattice, within 0.1 %"""
    r, trunc, res = 0.6, 0.35, (24, 24, 24)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    pts = tr.points(lo, hi, res)
    cam = f32(pr.equirect_cam(64, 32))
    st = tr.integrate32(tr.new_state(len(pts)), [const_frame(tr.EQUIRECT, cam, 64, 32, r)], pts, trunc)
    rad = np.linalg.norm(pts.astype(np.float64), axis=1)
    band = np.abs(rad - r) < trunc - 1e-4
    assert band.sum() > 3000 and (st["weight"][band] == 1).all()
    assert np.abs(st["tsdf"][band] - (rad[band] - r) / trunc).max() < 1e-6
    assert (st["tsdf"][rad < r - trunc - 1e-4] == -1).all() and (st["weight"][rad > r + trunc + 1e-4] == 0).all()
    observed = (st["weight"] >= 1).reshape(24, 24, 24)
    field = np.where(observed, st["tsdf"].reshape(24, 24, 24), np.float32(-1.0)).astype(np.float32)
    v, t, s = mr.extract(field, lo, hi, 0.0)
    fv, ft, fs, _ = tr.filter_mesh(v, t, s, observed)
    assert 0 < len(ft) < len(t)                     # the shell at r + trunc is gone
    exact = ((rad - r) / trunc).astype(np.float32).reshape(24, 24, 24)
    ev, et, _ = mr.extract(exact, lo, hi, 0.0)
    vol, want = mr.volume(fv, ft), mr.volume(ev, et)
    print("fused %.6f analytic %.6f sphere %.6f" % (vol, want, -4.0 / 3.0 * np.pi * r ** 3))
    assert abs(want + 4.0 / 3.0 * np.pi * r ** 3) < 0.02 * abs(want)       # (inside is BEHIND the surface: the normals point inwards)
    assert abs(vol - want) <= 1e-3 * abs(want)
    assert len(ft) == len(et) and mr.is_closed_oriented(ft, len(fv))


# ------------------------------------------------------------------------------------------------ 3: float32 against float64
@pytest.mark.parametrize("name", list(tr.CAMERAS))
def test_float32_against_float64(name):
    lo, hi, res = (-6.5, -5.5, -6.0), (7.0, 7.5, 7.0), (33, 33, 33)
    trunc = 0.8
    pts = tr.points(lo, hi, res)
    fr = tr.sphere_frame(name, 0, rgb=False, sem=False, inst=False)
    st0 = tr.new_state(len(pts))
    a = tr.integrate32(st0, [fr], pts, trunc)
    b, info = tr.integrate64(tr.new_state(len(pts), dtype=np.float64), [fr], pts, trunc)
    bound, excl = tr.single_frame_bound(fr, pts, trunc, info[0])
    share = excl.mean()
    ok = ~excl
    fused32, fused64 = a["weight"] == 1, b["weight"] == 1
    diff = np.abs(a["tsdf"].astype(np.float64) - b["tsdf"])
    worst = float((diff[ok & fused64] / np.maximum(bound[ok & fused64], 1e-300)).max())
    print("%s: %.3f %% excluded, %d fused, %d decisions differ (all excluded: %s), largest share of the bound %.3f"
          % (name, 100 * share, fused64.sum(), (fused32 != fused64).sum(), bool((fused32 == fused64)[ok].all()), worst))
    assert share <= 0.01
    assert fused64[ok].sum() > 2000
    assert np.array_equal(fused32[ok], fused64[ok])
    assert (diff[ok] <= bound[ok]).all()
    assert bound[ok].max() < 1e-4                   # the bound is no blank cheque


# ------------------------------------------------------------------------------------------------ 4: the extract filter
def test_extract_filter():
    g = np.random.default_rng(5)
    res = (6, 5, 4)
    lo, hi = (0.0, 0.0, 0.0), (6.0, 5.0, 4.0)
    field = g.normal(size=(4, 5, 6)).astype(np.float32)
    observed = np.ones((4, 5, 6), bool)
    observed[0, 0, 0] = observed[3, 4, 5] = observed[1, 2, 5] = False       # two corners and a face point
    observed[2, :, 0] = False                                                # a line
    v, t, s = mr.extract(field, lo, hi, 0.0)
    fv, ft, fs, idx = tr.filter_mesh(v, t, s, observed)
    assert 0 < len(fv) < len(v) and 0 < len(ft) < len(t)
    # the definition, checked directly: every lattice neighbour (+-1 per axis, inside the lattice) of every surviving src is observed
    for n in fs:
        iz, iy, ix = np.unravel_index(int(n), observed.shape)
        assert observed[max(iz - 1, 0):iz + 2, max(iy - 1, 0):iy + 2, max(ix - 1, 0):ix + 2].all()
    assert (np.diff(idx) > 0).all() and np.array_equal(fv, v[idx]) and np.array_equal(fs, s[idx])
    assert sorted(set(ft.reshape(-1).tolist())) == list(range(len(fv)))         # no vertex without a face
    # the kept faces are the faces whose three sources pass, in order, renumbered
    bad = tr.unobserved_near(observed).reshape(-1)
    kept = [k for k in range(len(t)) if not bad[s[t[k]]].any()]
    assert np.array_equal(idx[ft], t[kept])
    # fusion's torch implementation is the same function
    tv, tt, ts, ti = fusion.filter_mesh(torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(s), torch.from_numpy(observed))
    assert tt.dtype == torch.int32 and ts.dtype == torch.int64
    assert np.array_equal(tv.numpy(), fv) and np.array_equal(tt.numpy(), ft) and np.array_equal(ts.numpy(), fs) and np.array_equal(ti.numpy(), idx)
    assert np.array_equal(fusion.unobserved_near(torch.from_numpy(observed)).numpy(), tr.unobserved_near(observed))
    for shape in ((1, 1, 1), (1, 4, 2), (3, 1, 5)):
        o = g.random(shape) < 0.7
        assert np.array_equal(fusion.unobserved_near(torch.from_numpy(o)).numpy(), tr.unobserved_near(o)), shape
    # everything observed: nothing changes; nothing observed: nothing is left
    full = tr.filter_mesh(v, t, s, np.ones_like(observed))
    assert np.array_equal(full[0], v) and np.array_equal(full[1], t)
    none = fusion.filter_mesh(torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(s), torch.zeros(4, 5, 6, dtype=torch.bool))
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)
