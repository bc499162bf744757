"""CPU tests that pin tests/_raycast_ref.py, the restatement k_tsdf_raycast is compared with bit for bit on the GPU
(include/pnr.h "volume ray casting"): the two float32 forms agree on every case here, closed forms worked out by hand, six
corrupted variants that each fail a named check, the hit depth against the exact ray-sphere root inside a derived bound, and
float32 against float64 per pixel."""
import numpy as np
import pytest

import _pano_ref as pr
import _raycast_ref as rr
import _tsdf_ref as tr
import _warp_ref as wr

f32 = np.float32
BOX = rr.BOX
TRUNC = 0.6


def same_bits(a, b):
    return all(a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("depth", "normal", "src", "code"))


def both(view, near, far, lat, tsdf, weight, pix=None, **kw):
    """raycast32's result, after checking that the loops give the same bits"""
    a = rr.raycast32(view, near, far, lat, tsdf, weight, pix=pix, **kw)
    b = rr.raycast_loops(view, near, far, lat, tsdf, weight, pix=pix, **kw)
    assert same_bits(a, b), kw
    off = a["code"] != rr.HIT
    assert not a["depth"][off].any() and not a["normal"][off].any() and (a["src"][off] == -1).all() and (a["src"][~off] >= 0).all()
    return a


# ------------------------------------------------------------------------------------------------ the plane, by hand
# Lattice 4 x 4 x 8 at step 1 from the origin: positions 0.5, 1.5, ...  tsdf = (Z - 4) / 4 is linear, so trilinear interpolation
# is exact: the surface is the plane Z = 4, positive behind it for a camera that looks along +z.  The camera stands at
# (1.5, 1.5, -1): its central pixel runs along the lattice line g = (1, 1, .), og_z = -1.5, so the ray enters at t = 1.5 and its
# samples at dt = 0.5 sit at g_z = 0, 0.5, 1, ...: sample 6 has g_z = 3 (Z = 3.5, v = -0.125), sample 7 g_z = 3.5 (Z = 4, v = 0):
# r = 1, t* = 4.5 + 0.5 = 5 = the plane's z-depth.  At t*: cell (1, 1, 3), fraction (0, 0, 0.5) -> nearest corner (1, 1, 4), flat
# index (4 * 4 + 1) * 4 + 1 = 69; the gradient is (0, 0, 0.25), the normal (0, 0, -1).
LAT = rr.lattice((0, 0, 0), (4, 4, 8), (4, 4, 8))
CENTRE = 2 * 5 + 2


def plane(weight_edit=None):
    z = np.arange(8, dtype=np.float64) + 0.5
    t = np.broadcast_to(((z - 4.0) / 4.0)[:, None, None], (8, 4, 4)).astype(f32)
    w = np.ones((8, 4, 4), f32)
    if weight_edit is not None:
        weight_edit(w)
    return np.ascontiguousarray(t).reshape(-1), w.reshape(-1)


def axis_view(origin, back=False):
    c2w = np.zeros((3, 4), f32)
    c2w[0, 0], c2w[1, 1], c2w[2, 2] = (-1, 1, -1) if back else (1, 1, 1)
    c2w[:, 3] = origin
    return (rr.PINHOLE, np.asarray((16.0, 16.0, 2.0, 2.0), f32), c2w, 5, 5)


FRONT = axis_view((1.5, 1.5, -1.0))


def check_plane_hit(variant=None):
    out = rr.raycast32(FRONT, 0.0, 100.0, LAT, *plane(), dt=0.5, variant=variant)
    return out["code"][CENTRE] == rr.HIT and out["depth"][CENTRE] == f32(5.0)


def check_plane_normal(variant=None):
    out = rr.raycast32(FRONT, 0.0, 100.0, LAT, *plane(), dt=0.5, variant=variant)
    return np.array_equal(out["normal"][CENTRE], np.asarray((0.0, 0.0, -1.0), f32))


def check_plane_src(variant=None):
    return rr.raycast32(FRONT, 0.0, 100.0, LAT, *plane(), dt=0.5, variant=variant)["src"][CENTRE] == 69


def check_weight_equal_to_min_weight_is_observed(variant=None):
    return rr.raycast32(FRONT, 0.0, 100.0, LAT, *plane(), min_weight=1.0, dt=0.5, variant=variant)["code"][CENTRE] == rr.HIT


def slab(layer):
    def edit(w):
        w[layer] = 0.0
    return edit


def check_crossing_next_to_unobserved(variant=None):
    """layer 3 (Z = 3.5) unobserved: sample 6 (cell 3: layers 3, 4) is unobserved, so the crossing between samples 6 and 7 does
    not count, and nothing crosses after it"""
    return rr.raycast32(FRONT, 0.0, 100.0, LAT, *plane(slab(3)), dt=0.5, variant=variant)["code"][CENTRE] == rr.NO_SURFACE


def check_far_face_cell(variant=None):
    """a ray along the lattice's last plane g_x = res_x - 1 = 3 samples cell (2, ., .) at fraction 1, so with column 2 unobserved
    it sees nothing"""
    def edit(w):
        w[:, :, 2] = 0.0
    view = axis_view((3.5, 1.5, -1.0))
    return rr.raycast32(view, 0.0, 100.0, LAT, *plane(edit), dt=0.5, variant=variant)["code"][CENTRE] == rr.NO_SURFACE


CHECKS = {"sign": check_plane_hit, "ge": check_weight_equal_to_min_weight_is_observed, "unobserved_ok": check_crossing_next_to_unobserved,
          "no_clamp": check_far_face_cell, "normal_sign": check_plane_normal, "src_floor": check_plane_src}


def test_every_variant_fails_its_named_check():
    assert set(CHECKS) == set(rr.VARIANTS)
    for name, check in CHECKS.items():
        assert check(), name
        assert not check(name), name
    # and each variant is a rule of its own on the sphere: it changes some output there, in both float32 forms alike
    lat = rr.lattice(*BOX, (16, 12, 10))
    tsdf, weight = rr.sphere_volume(lat, TRUNC)
    m, cam, c2w, w, h = tr.CAMERAS["pinhole_a"]
    view = (m, np.asarray(cam, f32), np.asarray(c2w, f32), w, h)
    pix = np.arange(0, w * h, 53)
    base = rr.raycast32(view, 0.1, 100.0, lat, tsdf, weight, pix=pix)
    for name in rr.VARIANTS:
        assert same_bits(rr.raycast32(view, 0.1, 100.0, lat, tsdf, weight, pix=pix, variant=name),
                         rr.raycast_loops(view, 0.1, 100.0, lat, tsdf, weight, pix=pix, variant=name)), name
        if name not in ("ge", "no_clamp"):                          # (those two need weights of exactly min_weight / a ray on the far face)
            assert not same_bits(base, rr.raycast32(view, 0.1, 100.0, lat, tsdf, weight, pix=pix, variant=name)), name


def test_plane_closed_forms():
    out = both(FRONT, 0.0, 100.0, LAT, *plane(), dt=0.5)
    assert check_plane_hit() and check_plane_normal() and check_plane_src()
    # every pixel of the 5 x 5 image hits the plane at z-depth 5 (a pinhole's parameter), to rounding
    assert (out["code"] == rr.HIT).all() and np.abs(out["depth"] - 5.0).max() <= 8 * 5.0 * rr.U32
    assert np.abs(out["normal"] - np.asarray((0, 0, -1), f32)).max() <= 1e-6
    # the same plane from behind: the volume goes from + to -, which is no crossing
    back = both(axis_view((1.5, 1.5, 9.0), back=True), 0.0, 100.0, LAT, *plane(), dt=0.5)
    assert (back["code"] == rr.NO_SURFACE).all()
    # a ray that STARTS behind the surface (camera at Z = 5) never crosses from - to +
    inside = both(axis_view((1.5, 1.5, 5.0)), 0.0, 100.0, LAT, *plane(), dt=0.5)
    assert (inside["code"] == rr.NO_SURFACE).all()


def test_unobserved_slab_in_front_of_the_crossing():
    # layer 1 (Z = 1.5): samples 0 .. 3 (cells 0 and 1) are unobserved, samples 4 .. are not touched; the crossing at 6 | 7 counts
    far_slab = both(FRONT, 0.0, 100.0, LAT, *plane(slab(1)), dt=0.5)
    assert far_slab["code"][CENTRE] == rr.HIT and far_slab["depth"][CENTRE] == f32(5.0) and far_slab["src"][CENTRE] == 69
    # layer 3 touches sample 6: no hit; layer 4 touches both
    for layer in (3, 4):
        out = both(FRONT, 0.0, 100.0, LAT, *plane(slab(layer)), dt=0.5)
        assert out["code"][CENTRE] == rr.NO_SURFACE, layer
    assert check_crossing_next_to_unobserved()
    # layer 5 (Z = 5.5) is behind both samples (cells 3: layers 3, 4) but inside the cell of t* only if t* sat in cell 4: it does not
    out = both(FRONT, 0.0, 100.0, LAT, *plane(slab(5)), dt=0.5)
    assert out["code"][CENTRE] == rr.HIT and np.array_equal(out["normal"][CENTRE], np.asarray((0, 0, -1), f32))
    # garbage where weight fails the test cannot leak
    t, w = plane(slab(1))
    for junk in (np.nan, np.inf, -np.inf, 1e30):
        t2 = t.copy()
        t2[w == 0] = junk
        assert same_bits(both(FRONT, 0.0, 100.0, LAT, t2, w, dt=0.5), far_slab), junk
    # a hit with a zero gradient keeps its depth and src and gets the zero normal: tsdf -0.25 in layers 0 .. 3 and 0 from layer 4
    # on, dt = 1: samples at g_z = 3 (v = -0.25) and 4 (v = 0) cross with r = 1, so t* = t_1 = 5.5 in cell 4, where the field is flat
    flat_t = np.where(np.arange(t.size) // 16 >= 4, 0.0, -0.25).astype(f32)
    out = both(FRONT, 0.0, 100.0, LAT, flat_t, np.ones_like(w), dt=1.0)
    assert out["code"][CENTRE] == rr.HIT and out["depth"][CENTRE] == f32(5.5)
    assert not out["normal"][CENTRE].any() and out["src"][CENTRE] == (4 * 4 + 1) * 4 + 1


def test_axis_parallel_rays_clip_and_limits():
    t, w = plane()
    # dg_x = dg_y = 0 on the central pixel: inside the lattice it marches (above); outside on x, on y, beyond the last plane: MISSED
    for origin in ((-1.0, 1.5, -1.0), (1.5, 4.75, -1.0), (3.75, 1.5, -1.0)):
        out = both(axis_view(origin), 0.0, 100.0, LAT, t, w, dt=0.5)
        assert out["code"][CENTRE] == rr.MISSED, origin
    # exactly on the first and the last plane (og = 0 and og = res - 1) is inside
    for origin in ((0.5, 1.5, -1.0), (3.5, 3.5, -1.0)):
        out = both(axis_view(origin), 0.0, 100.0, LAT, t, w, dt=0.5)
        assert out["code"][CENTRE] == rr.HIT and out["depth"][CENTRE] == f32(5.0), origin
    assert check_far_face_cell()
    # near beyond the box (the ray leaves at t = 8.5), far in front of it (it enters at 1.5)
    assert (both(FRONT, 20.0, 100.0, LAT, t, w, dt=0.5)["code"] == rr.MISSED).all()
    assert (both(FRONT, 0.0, 1.25, LAT, t, w, dt=0.5)["code"] == rr.MISSED).all()
    # far between the entry and the surface: NO_SURFACE; near inside the box in front of the surface: the march starts there
    assert (both(FRONT, 0.0, 4.0, LAT, t, w, dt=0.5)["code"] == rr.NO_SURFACE).all()
    out = both(FRONT, 3.25, 100.0, LAT, t, w, dt=0.5)               # samples at g_z = 1.75, ..., 3.25 (v = -0.0625), 3.75 (v = 0.0625)
    assert out["code"][CENTRE] == rr.HIT and out["depth"][CENTRE] == f32(5.0)
    # max_steps 0 and 1 cannot see a crossing (it takes two samples); 8 samples reach it, 7 do not
    for ms, want in ((0, rr.NO_SURFACE), (1, rr.NO_SURFACE), (7, rr.NO_SURFACE), (8, rr.HIT)):
        assert both(FRONT, 0.0, 100.0, LAT, t, w, dt=0.5, max_steps=ms)["code"][CENTRE] == want, ms
    # a dt larger than the box: one sample
    assert (both(FRONT, 0.0, 100.0, LAT, t, w, dt=50.0)["code"] == rr.NO_SURFACE).all()
    # the defaults: half the smallest step, and enough samples for the diagonal
    assert rr.default_dt(LAT[1]) == f32(0.5) and rr.default_max_steps(LAT[2], LAT[1], 0.5) == int(np.sqrt(9 + 9 + 49) / 0.5) + 2
    assert both(FRONT, 0.0, 100.0, LAT, t, w)["depth"][CENTRE] == f32(5.0)


def view_of(name):
    m, cam, c2w, w, h = tr.CAMERAS[name]
    return (m, np.asarray(cam, f32), np.asarray(c2w, f32), w, h)


def test_fisheye_pixels_outside_the_lens_see_no_ray():
    lat = rr.lattice(*BOX, (8, 6, 5))
    tsdf, weight = rr.sphere_volume(lat, TRUNC)
    view = view_of("fisheye_a")
    pix = np.concatenate([np.arange(0, 6400, 41), [0, 79, 6399]])
    out = both(view, 0.1, 100.0, lat, tsdf, weight, pix=pix)
    _, _, ok = pr._rays(np.float32, view, pix)
    assert (~ok).sum() >= 3 and ok.sum() > 50
    assert (out["code"][~ok] == rr.NO_RAY).all() and (out["code"][ok] != rr.NO_RAY).all()


# ------------------------------------------------------------------------------------------------ the sphere
def exact_depth(name):
    m, cam, c2w, w, h = view_of(name)
    d = pr.sphere_depth(cam, c2w, w, h, *tr.SPHERE) if m == rr.EQUIRECT else wr.sphere_depth(m, cam, c2w, w, h, *tr.SPHERE)
    return d.reshape(-1).astype(np.float64)


def sphere_error(name, res):
    """(|depth - exact root|, bound, hit mask) over the pixels of CAMERAS[name] on the sphere volume at `res`"""
    lat = rr.lattice(*BOX, res)
    tsdf, weight = rr.sphere_volume(lat, TRUNC)
    view = view_of(name)
    out = rr.raycast32(view, 0.1, 100.0, lat, tsdf, weight)
    hit = out["code"] == rr.HIT
    o, d, _ = pr._rays(np.float32, view, np.arange(view[3] * view[4]))
    o, d = o.astype(np.float64), d.astype(np.float64)
    t = exact_depth(name)
    centre, R = tr.SPHERE
    nrm = (o + t[:, None] * d - np.asarray(centre)) / R
    norm_d = np.sqrt((d * d).sum(-1))
    with np.errstate(all="ignore"):
        slope = (d * nrm).sum(-1)                                   # |d| cos(ray, normal): how fast the distance grows along t
        h, dt = float(np.abs(lat[1]).max()), float(rr.default_dt(lat[1]))
        rho = R - TRUNC
        E = h * h / (4.0 * rho) + dt * dt * norm_d ** 2 / (8.0 * rho)
        bound = rr.INFLATE * E / slope + 64 * rr.U32 * (t + 1.0)
    return np.abs(out["depth"].astype(np.float64) - t), bound, hit, (out, nrm)


@pytest.mark.parametrize("name", ["pinhole_a", "fisheye_b", "equirect_a"])
def test_sphere_depth_against_the_exact_root(name):
    """The bound.  The volume holds phi = g / trunc with g(X) = |X - c| - R, a distance function: its Hessian is (I - n n^T) / rho
    at distance rho from the centre, so the pure second derivatives sum to 2 / rho, and rho >= R - trunc inside the band.
      * Trilinear interpolation on a cell of steps h_k errs by at most sum_k h_k^2 / 8 max|g_kk| <= h^2 / (4 (R - trunc)) in
        units of g, h the largest step.  (trunc is 3.5 h or more at both resolutions, and a sample in front of the crossing lies
        at most dt |d| + a cell diagonal < trunc from the surface, so no clamped or unobserved point enters the two samples.)
      * Along the ray g is convex with g'' <= |d|^2 / rho, so the chord between two samples dt apart leaves g by at most
        dt^2 |d|^2 / (8 rho).  The secant through the two INTERPOLATED samples therefore stays within
        E = h^2 / (4 rho) + dt^2 |d|^2 / (8 rho) of g between them, and at its root t* we have |g(t*)| <= E.
      * g grows along the ray at the rate g' = d . n = |d| cos(ray, normal), and by convexity a value of E costs at most
        E / g'(root) in t on the far side (and E / g'(t*) on the near side, which the inflation by 1 + 2^-4 covers: g' changes by
        |d|^2 / rho * 1e-3 over such a distance).  Hence |t* - root| <= (1 + 2^-4) E / (|d| cos), divided by the cosine and in units of
        the ray parameter.
      * float32: 64 u (t + 1) for the rounding of the volume, the ray and the march.
    E is proportional to h^2 (dt is half the smallest step): the bound quarters when the lattice step halves.  At step 0.172 and
    the image centre it is 1.5e-3; a prototype of the rule measured a largest error of 9.4e-4 there and 2.4e-4 at step 0.086."""
    err1, bound1, hit1, (out, nrm) = sphere_error(name, (32, 32, 32))
    err2, bound2, hit2, _ = sphere_error(name, (64, 64, 64))
    for err, bound, hit in ((err1, bound1, hit1), (err2, bound2, hit2)):
        print("%s: %d hits, largest error %.3g, largest error / bound %.3f" % (name, hit.sum(), err[hit].max(), (err[hit] / bound[hit]).max()))
        assert hit.sum() > 200 and (err[hit] <= bound[hit]).all()
    slack = 64 * rr.U32 * (exact_depth(name) + 1.0)
    both_hit = hit1 & hit2
    assert np.allclose((bound2 - slack)[both_hit] * 4.0, (bound1 - slack)[both_hit], rtol=1e-12)
    assert err2[both_hit].max() < 0.5 * err1[both_hit].max()
    # the normal points from the surface into the sphere, towards the camera: -n of the exact sphere, to the interpolant's slope error
    seen = hit1 & (np.abs(out["normal"]).sum(-1) > 0)
    assert seen.sum() > 0.9 * hit1.sum()
    assert np.abs(np.linalg.norm(out["normal"][seen], axis=-1) - 1.0).max() < 1e-6
    assert ((out["normal"][seen] * -nrm[seen]).sum(-1) > 0.99).all()
    # src is the lattice point nearest the hit: within half a cell diagonal of it
    lat = rr.lattice(*BOX, (32, 32, 32))
    pts = tr.points(*BOX, (32, 32, 32))[out["src"][hit1]]
    o, d, _ = pr._rays(np.float32, view_of(name), np.nonzero(hit1)[0])
    X = o + out["depth"][hit1][:, None] * d
    assert (np.abs(pts - X) <= 0.5 * np.abs(lat[1]) * (1 + 1e-4)).all()


def test_float32_against_float64_per_pixel():
    """Codes equal on every pixel; where both runs pick the same crossing (the same sample number n), |depth32 - depth64| stays
    inside _raycast_ref.depth_bound, derived there.  Excluded: the pixels whose two runs pick different crossings or whose
    samples sit within rounding of a cell boundary -- at most 1 % (a prototype saw none differ in 20 000 rays and a largest
    difference of 7.7e-7)."""
    lat = rr.lattice(*BOX, (32, 32, 32))
    tsdf, weight = rr.sphere_volume(lat, TRUNC)
    total = excluded = hits = 0
    worst = 0.0
    for name in tr.CAMERAS:
        view = view_of(name)
        a, _ = rr.raycast32(view, 0.1, 100.0, lat, tsdf, weight, info=True), None
        out32, info32 = a
        out64, info64 = rr.raycast64(view, 0.1, 100.0, lat, tsdf, weight)
        assert np.array_equal(out32["code"], out64["code"]), name
        bound, doubt = rr.depth_bound(lat, info64)
        hit = out64["code"] == rr.HIT
        out = hit & ((info32["n"] != info64["n"]) | doubt)
        use = hit & ~out
        diff = np.abs(out32["depth"].astype(np.float64) - info64["depth"])
        assert (diff[use] <= bound[use]).all(), name
        assert np.array_equal(out32["src"][use], out64["src"][use]) or (out32["src"][use] != out64["src"][use]).mean() < 0.01
        assert np.abs(out32["normal"][use] - info64["normal"][use]).max() < 1e-3
        total, excluded, hits = total + hit.size, excluded + int(out.sum()), hits + int(use.sum())
        worst = max(worst, float(diff[use].max()) if use.any() else 0.0)
        print("%s: %d hits, %d excluded, largest difference %.3g, largest difference / bound %.3f"
              % (name, hit.sum(), out.sum(), diff[use].max() if use.any() else 0.0, (diff[use] / bound[use]).max() if use.any() else 0.0))
    assert total > 20000 and hits > 5000 and excluded <= 0.01 * total
    assert worst < 1e-5


def test_loops_and_vectorised_agree_on_the_sphere():
    hits = {}
    for res, box, trunc in rr.LATTICES:
        lat = rr.lattice(*box, res)
        tsdf, weight = rr.sphere_volume(lat, trunc)
        for k, name in enumerate(tr.CAMERAS):
            view = view_of(name)
            pix = np.arange(k, view[3] * view[4], 97)
            out = both(view, 0.1, 100.0, lat, tsdf, weight, pix=pix)
            for kw in ({"dt": 0.25 * float(np.abs(lat[1]).min())}, {"dt": 4.0 * float(np.abs(lat[1]).max())}, {"min_weight": 3.0}, {"max_steps": 5}):
                both(view, 0.1, 100.0, lat, tsdf, weight, pix=pix[::3], **kw)
            hits[res] = hits.get(res, 0) + int((out["code"] == rr.HIT).sum())
    assert hits[(16, 16, 16)] > 40 and all(n > 0 for n in hits.values()), hits
