"""CPU tests of the rule of include/pnr.h "mesh ray casting" as tests/_meshcast_ref.py restates it: the index is conservative (the
slab walk's winner is brute force's on adversarial rays, at every offset and resolution), the ray-triangle test is watertight where
plain Moller-Trumbore is not, and box_mesh through the rule agrees with synthetic.room_depth's float64 closed form.  No GPU."""
import numpy as np
import pytest

import _icp_ref as ir
import _meshcast_ref as mc
from panopticnerf_amd import mesh, synthetic

f32 = np.float32
N_ = lambda t: t.detach().cpu().numpy()


def icosphere(subdiv, offset=0.0):
    m = synthetic.icosphere(subdiv)
    return (N_(m.vertices) + f32(offset)).astype(f32), N_(m.faces)


def grid_for(V, F, res):
    use = mc.usable_faces(V, F)
    pts = V[F[use]].reshape(-1, 3)
    bounds = np.concatenate([pts.min(0), pts.max(0)]).astype(f32)
    lo, cell, res = mesh.grid_box(bounds, int(use.sum()), res)
    return mc.make_grid(res, lo, cell)


# ------------------------------------------------------------------------------------------------ the index only prunes
RESOLUTIONS = ((1, 1, 1), (2, 3, 5), (16, 16, 16), (37, 5, 11), (1, 2, 300))


def adversarial_rays(V, F, grid, offset, seed):
    g = np.random.default_rng(seed)
    res, lo, inv, _ = grid
    off = f32(offset)
    rays = []
    tg = mc.edge_targets(V, F[mc.usable_faces(V, F)])
    tg = tg[np.isfinite(tg).all(1)]
    tg = tg[g.choice(len(tg), 40, replace=False)]
    for org in (np.array([0.03, -0.02, 0.05], f32) + off, np.array([3.0, 1.0, -2.0], f32) + off, np.zeros(3, f32) + off):
        rays.append(mc.rays_to(org, tg))
        axis = np.concatenate([np.eye(3, dtype=f32), -np.eye(3, dtype=f32)])
        rays.append(mc.rays_to(org, org + axis))
        rays.append(mc.rays_to(org, org + g.standard_normal((12, 3)).astype(f32)))
    # rays lying in cell boundary planes: through the corner of cell (1, 1, 1), along every axis and both ways
    corner = (lo + f32(1) / inv).astype(f32)
    for k in range(3):
        d = np.zeros(3, f32)
        d[k] = 1
        rays.append(mc.rays_to((corner - d * f32(5)).astype(f32), corner[None]))
        rays.append(mc.rays_to((corner + d * f32(5)).astype(f32), corner[None]))
    rays = np.concatenate(rays)
    rays[::7, 6], rays[::7, 7] = f32(0.5), f32(2.5)                  # some with a near and a far that cut hits away
    return rays


@pytest.mark.parametrize("offset", [0.0, 7.0, 3000.0, -1e5])
def test_walk_finds_the_brute_force_winner(offset):
    """the winner of the slab walk -- binning, clip, layers, the early stop -- is brute force's key on every ray: aimed at vertices
    and edge points, axis-parallel, lying in cell boundary planes, from inside, outside and the exact centre"""
    Vs, Fs = icosphere(2)
    Vq, Fq = mc.soup(120, 200, seed=3)
    V = (np.concatenate([Vs, Vq]) + f32(offset)).astype(f32)
    F = np.concatenate([Fs, np.where(Fq < len(Vq), Fq + len(Vs), Fq + len(Vs))]).astype(np.int32)
    walked = hits = stopped_early = 0
    for n, res in enumerate(RESOLUTIONS):
        grid = grid_for(V, F, res)
        cells = mc.bin_faces(V, F, grid)
        rays = adversarial_rays(V, F, grid, offset, seed=n)
        keys = mc.face_times(rays, V, F)
        want = keys.min(1)
        for q in range(len(rays)):
            got = mc.walk(rays[q], grid, cells, keys[q])
            assert got is not None, (offset, res, rays[q])
            assert got[0] == want[q], (offset, res, rays[q], got, want[q])
            walked += 1
            hits += want[q] != mc.EMPTY
            stopped_early += got[2] < grid[0][int(np.argmax(np.abs(rays[q, 3:6] * grid[2])))] and want[q] != mc.EMPTY
    assert walked > 500 and hits > walked // 3 and stopped_early > 50, (walked, hits, stopped_early)


def test_a_far_origin_takes_the_plain_loop():
    V, F = icosphere(1)
    grid = grid_for(V, F, (16, 16, 16))
    cells = mc.bin_faces(V, F, grid)
    near_by = mc.rays_to((0.0, 0.0, -3.0), V[:4])
    far_off = mc.rays_to((0.0, 0.0, -3.0e4), V[:4])
    keys = mc.face_times(np.concatenate([near_by, far_off]), V, F)
    assert all(mc.walk(near_by[q], grid, cells, keys[q]) is not None for q in range(4))
    assert all(mc.walk(far_off[q], grid, cells, keys[4 + q]) is None for q in range(4))
    # the threshold: the ray's reach against 4096 of the smallest cell
    assert mc.within_reach(near_by[0, :3], grid) and not mc.within_reach(far_off[0, :3], grid)
    og = (far_off[0, :3] - grid[1]) * grid[2]
    assert np.abs(og).max() + 17 > mc.MAX_REACH


def test_unequal_cells_walk_or_take_the_plain_loop():
    """a grid of unequal cells (never RayIndex's own: grid_box makes cubes) is still exact: where the reach allows the walk its
    winner is brute force's, and very unequal cells send the rays from outside to the plain loop"""
    V, F = icosphere(2)
    lo = (V.min(0) - f32(0.01)).astype(f32)
    ext = (V.max(0) + f32(0.01) - lo).astype(f32)
    rays = np.concatenate([mc.rays_to(o, mc.edge_targets(V, F)[::9]) for o in ((0.03, -0.02, 0.05), (6.0, 1.0, -2.0))])
    keys = mc.face_times(rays, V, F)
    walked = looped = 0
    for res in ((37, 5, 11), (8, 8, 8), (1, 1, 1000)):
        grid = mc.make_grid(res, lo, (ext / np.asarray(res, f32)).astype(f32))
        cells = mc.bin_faces(V, F, grid)
        for q in range(len(rays)):
            got = mc.walk(rays[q], grid, cells, keys[q])
            assert got is None or got[0] == keys[q].min(), (res, rays[q])
            walked += got is not None
            looped += got is None and res == (1, 1, 1000)
    assert walked > len(rays) and looped > len(rays) // 3


def _bounds_of(V, F):
    pts = V[F[mc.usable_faces(V, F)]].reshape(-1, 3)
    return np.concatenate([pts.min(0), pts.max(0)]).astype(f32)


GRAZING_RES = ((1, 1, 1), (8, 8, 8), (32, 32, 32), (100, 30, 20))


def test_grazing_rays_against_large_faces():
    """rays in the plane of a face much larger than a cell, whose t is cancellation noise (mc.grazing_cases: the reviewer's case
    and 23 from a seed).  With the rule, the walk's winner is the plain loop's at every resolution, case by case and on all
    cases as one mesh; without the box test -- the cases' teeth -- the walk loses the plain loop's winner in several."""
    cases = mc.grazing_cases()
    lost_without = 0
    for V, ray in cases:
        new, old = mc.face_times(ray[None], V, mc.PAIR)[0], mc.face_times(ray[None], V, mc.PAIR, box=False)[0]
        assert old[0] != mc.EMPTY and new[0] == mc.EMPTY            # the claimed hit is away from its face: the rule refuses it
        for res in GRAZING_RES:
            grid = grid_for(V, mc.PAIR, res)
            cells = mc.bin_faces(V, mc.PAIR, grid)
            assert mc.walk(ray, grid, cells, new)[0] == new.min(), (res, V.tolist(), ray.tolist())
            lost_without += mc.walk(ray, grid, cells, old)[0] != old.min()
    assert lost_without >= 5, lost_without
    V, F, rays = mc.grazing_scene()
    keys = mc.face_times(rays, V, F)
    for res in GRAZING_RES[1:]:
        grid = grid_for(V, F, res)
        cells = mc.bin_faces(V, F, grid)
        for q in range(len(rays)):
            assert mc.walk(rays[q], grid, cells, keys[q])[0] == keys[q].min(), (res, q)


MEASURED_SPAN = 1.575e-7                   # wall 5 cm 1.15e-07, wall 1 cm 1.32e-07, floors 1.58e-07, 1.45e-07, 1.55e-07: 2.6 x 2^-24
SPAN_DEPTH_ERR = 4 * MEASURED_SPAN


def span_error(out, V, F, rays, exact):
    """|depth - exact| over the span of the face hit along the ray: max |corner - origin| component / max |d_k|"""
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    M = np.abs(V[F[out["face"]]].astype(np.float64) - o[:, None, :]).max((1, 2))
    return np.abs(out["depth"] - exact) / (M / np.abs(d).max(1))


def close_wall_exact(name, V, rays):
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    if name.startswith("floor"):
        return -o[:, 2] / d[:, 2]
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(d != 0, (np.where(d > 0, hi, lo) - o) / d, np.inf).min(1)


@pytest.mark.parametrize("case", range(5))
def test_no_holes_next_to_large_faces(case):
    """a wide pinhole 1 cm or 5 cm from a wall far larger than that, a camera above a floor 100 to 1000 times its height: every
    ray hits, with and without the box test under the same key (its tolerance is 2^-17 of the largest corner component, which
    bounds the error of t d).  The depth: t is a mean of the corners' depths along the ray, so its error is a few 2^-24 of the
    face's SPAN along the ray, not of t -- 1 cm in front of a 10 m wall float32 cannot give t to 4e-6 (measured against the
    float64 closed form: 4.3e-05 of t there, 7.0e-05 above the 1000 m floor).  Relative to the span the largest error measured
    on the CPU is 1.58e-07 = 2.6 x 2^-24 over the five scenes; the bound is four times that, 6.3e-07, here and on the GPU."""
    name, V, F, rays, ok = mc.close_wall_views()[case]
    out = mc.cast(rays, V, F, ok)
    assert (out["code"] == mc.HIT).all(), (name, int((out["code"] != mc.HIT).sum()))
    assert np.array_equal(mc.face_times(rays, V, F), mc.face_times(rays, V, F, box=False)), name
    err = span_error(out, V, F, rays, close_wall_exact(name, V, rays))
    print("%s: largest depth error over the face's span %.3e" % (name, err.max()))
    assert err.max() <= SPAN_DEPTH_ERR


def test_box_test_leaves_ordinary_hits_alone():
    """on rays that cross faces at an angle the box test changes no key: icosphere and soup, from inside and outside"""
    Vs, Fs = icosphere(2)
    Vq, Fq = mc.soup(120, 200, seed=3)
    for V, F in ((Vs, Fs), (Vq, Fq)):
        tg = mc.edge_targets(V, F[mc.usable_faces(V, F)])
        tg = tg[np.isfinite(tg).all(1)][:600]
        for org in ((0.03, -0.02, 0.05), (3.0, 1.0, -2.0)):
            rays = mc.rays_to(org, tg)
            assert np.array_equal(mc.face_times(rays, V, F), mc.face_times(rays, V, F, box=False))


# ------------------------------------------------------------------------------------------------ watertight
@pytest.mark.parametrize("origin", [(0.03, -0.02, 0.05), (0.0, 0.0, 0.0)])
def test_rule_is_watertight_where_moller_trumbore_is_not(origin):
    """every vertex, and five points along every edge, of icosphere(2) seen from inside: every ray hits -- while the plain
    float32 Moller-Trumbore test leaves holes on the same rays"""
    V, F = icosphere(2)
    rays = mc.rays_to(origin, mc.edge_targets(V, F))
    assert len(rays) == 162 + 5 * 480
    out = mc.cast(rays, V, F)
    assert (out["code"] == mc.HIT).all(), np.nonzero(out["code"] != mc.HIT)[0]
    assert (out["side"] == -1).all()                                 # from inside: the back of every face
    holes = int((~mc.moller_trumbore(rays, V, F)).sum())
    print("Moller-Trumbore leaves %d holes in %d rays from %r" % (holes, len(rays), origin))
    assert holes > 0


# ------------------------------------------------------------------------------------------------ analytic cross-check
MEASURED_REL = 1.022e-6                    # pinhole 3.03e-07, fisheye 1.02e-06, equirect 3.13e-07, against the float64 closed form
REL_DEPTH_ERR = 4 * MEASURED_REL


def room_depth64(cam, c2w, room=ir.ROOM):
    """synthetic.room_depth's closed form kept in float64 (that function rounds its result to float32): flat, 0 off the lens"""
    m = np.asarray(c2w, np.float32).astype(np.float64).reshape(3, 4)
    dc, ok = synthetic.camera_directions(cam)
    d = dc.numpy().reshape(-1, 3) @ m[:, :3].T
    wall = np.where(d > 0, np.asarray(room[1], np.float64), np.asarray(room[0], np.float64))
    with np.errstate(all="ignore"):
        t = np.where(d != 0, (wall - m[:, 3]) / d, np.inf).min(1)
    return np.where(ok.numpy().reshape(-1), t, 0.0)


@pytest.mark.parametrize("name", ["pinhole", "fisheye", "equirect"])
def test_box_mesh_against_room_depth(name):
    """box_mesh through the rule against synthetic.room_depth's closed form in float64 at a tilted pose.
    The largest relative depth error of the float32 rule measured on the CPU: pinhole 3.03e-07, fisheye 1.02e-06, equirect
    3.13e-07; the bound is four times the largest, 4.09e-06 -- the GPU executes the same float32 operations.  The normals of an
    axis-aligned box are exact, and every wall is met on the side its winding normal points to."""
    cam = ir.cameras()[name]
    c2w = np.asarray(ir.TRUE_POSE, f32)
    box = synthetic.box_mesh(*ir.ROOM)
    view = (cam.word, np.asarray(cam.params, f32), c2w, cam.width, cam.height)
    rays, ok = mc.camera_rays(view, 0.0, 100.0)
    out = mc.cast(rays, N_(box.vertices), N_(box.faces), ok)
    depth, normal = room_depth64(cam, c2w), ir.room_maps(cam, c2w)[1].reshape(-1, 3)
    sees = depth > 0
    assert np.array_equal(out["code"] == mc.HIT, sees) and np.array_equal(out["code"] == mc.NO_RAY, ~sees)
    assert (name == "fisheye") == bool((~sees).any())
    rel = np.abs(out["depth"][sees] - depth[sees]) / depth[sees]
    print("%s: largest relative depth error %.3e over %d pixels" % (name, rel.max(), sees.sum()))
    assert rel.max() <= REL_DEPTH_ERR
    assert np.array_equal(out["normal"], normal)                     # (== on values: exact, 0 off the lens)
    assert (out["side"][sees] == 1).all() and (out["side"][~sees] == 0).all()
    assert (out["bary"][sees].sum(1) > 0.999).all()
