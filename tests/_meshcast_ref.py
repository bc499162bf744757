"""The rule of include/pnr.h "mesh ray casting" restated in numpy float32, operation by operation: `cast` is brute force over all
faces -- the DEFINITION of every output of pnr_mesh_raycast / pnr_mesh_cast_rays, which the GPU tests compare bit for bit -- and
`bin_faces` / `walk` restate the index (csrc/pnr_meshcast.hip mc_scatter, mc_walk) so that the exactness argument of DESIGN.md
"Mesh ray casting" is guarded without a GPU: the walk's winner must be brute force's.  `moller_trumbore` is the plain float32
test the rule replaces, kept ONLY to show that the watertightness inputs have teeth.  A test helper, not a test."""
import functools
import itertools

import numpy as np

import _pano_ref as pr

f32, f64 = np.float32, np.float64
HIT, NO_RAY, MISSED = 0, 1, 2
PAD = f32(0.0625)                   # PNR_MESHCAST_PAD
BOX_TOL = f32(2.0 ** -17)           # PNR_MESHCAST_BOX_TOL
MAX_REACH = f32(4096.0)             # PNR_MESHCAST_MAX_REACH
MAX_RES = 1024
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
FMAX = np.finfo(f32).max
PINHOLE, FISHEYE, EQUIRECT = pr.PINHOLE, pr.FISHEYE, pr.EQUIRECT
KEYS = ("depth", "face", "code", "bary", "vertex", "normal", "side")


def camera_rays(view, near, far):
    """(rays (R, 8) float32, ok (R) bool) of every pixel of view = (model word, cam, c2w, width, height): pnr_camera_ray"""
    m, cam, c2w, w, h = view
    o, d, ok = pr._rays(f32, view, np.arange(w * h))
    rays = np.zeros((w * h, 8), f32)
    rays[:, :3], rays[:, 3:6] = np.asarray(o, f32), d
    rays[:, 6], rays[:, 7] = np.where(ok, f32(near), f32(0)), np.where(ok, f32(far), f32(0))
    return rays, ok


def usable_faces(V, F):
    """(F,) bool: every index in range and every corner finite"""
    F = np.asarray(F).reshape(-1, 3)
    inr = ((F >= 0) & (F < len(V))).all(1)
    Fc = np.where(inr[:, None], F, 0)
    return inr & (np.isfinite(V[Fc]).all((1, 2)) if len(V) else np.zeros(len(F), bool))


def ray_ok(rays, ok=None):
    o, d, near, far = rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    with np.errstate(invalid="ignore"):
        good = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1) & (near >= 0) & (near <= far)
    return good if ok is None else good & ok


def shear(d):
    """kx, ky, kz (R) and Sx, Sy, Sz (R) of rays with directions d (R, 3), d != 0"""
    ad = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    kz[ad[:, 1] > ad[:, 0]] = 1
    kz[ad[:, 2] > ad[np.arange(len(d)), kz]] = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    r = np.arange(len(d))
    dz = d[r, kz]
    neg = dz < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        return kx, ky, kz, d[r, kx] / dz, d[r, ky] / dz, f32(1) / dz


def test(o, d, near, far, k, c, box=True):
    """the ray-triangle test of R rays against F faces: c = (v0, v1, v2) each (F, 3).  Returns hit (R, F), t, U, V, W, det.
    box=False leaves the box test out: NOT the rule, kept to show that the grazing rays of the tests have teeth."""
    kx, ky, kz, Sx, Sy, Sz = k

    def sheared(v):
        P = v[None, :, :] - o[:, None, :]
        pz = np.take_along_axis(P, kz[:, None, None], 2)[..., 0]
        px = np.take_along_axis(P, kx[:, None, None], 2)[..., 0]
        py = np.take_along_axis(P, ky[:, None, None], 2)[..., 0]
        boxes.append(P)
        return px - Sx[:, None] * pz, py - Sy[:, None] * pz, Sz[:, None] * pz
    boxes = []
    with np.errstate(all="ignore"):
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sheared(c[0]), sheared(c[1]), sheared(c[2])
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        z = (U == 0) | (V == 0) | (W == 0)
        if z.any():
            U = np.where(z, (Cx.astype(f64) * By - Cy.astype(f64) * Bx).astype(f32), U)
            V = np.where(z, (Ax.astype(f64) * Cy - Ay.astype(f64) * Cx).astype(f32), V)
            W = np.where(z, (Bx.astype(f64) * Ay - By.astype(f64) * Ax).astype(f32), W)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        t = ((U * Az + V * Bz) + W * Cz) / det + f32(0)
        hit = ~mixed & (det != 0) & (t >= near[:, None]) & (t <= far[:, None])
        if box:                                                      # the box test: t d inside the box of A, B, C, widened
            q = t[:, :, None] * d[:, None, :]
            lo, hi = np.fmin(np.fmin(boxes[0], boxes[1]), boxes[2]), np.fmax(np.fmax(boxes[0], boxes[1]), boxes[2])
            e = (BOX_TOL * np.fmax(np.abs(lo), np.abs(hi)).max(2))[:, :, None]          # 2^-17 of the largest |component| of A, B, C
            hit &= ((q >= lo - e) & (q <= hi + e)).all(2)
            assert q.dtype == f32 and e.dtype == f32
    assert t.dtype == f32 and U.dtype == f32 and det.dtype == f32
    return hit, t, U, V, W, det


def keys_of(hit, t, faces):
    """(R, F) uint64 keys, EMPTY off a hit; faces (F) the face index of each column"""
    key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | faces.astype(np.uint64)[None, :]
    return np.where(hit, key, EMPTY)


def face_times(rays, V, F, chunk=256, box=True):
    """(R, F) uint64: the key of every ray-face pair, EMPTY where there is no hit (rays that are no rays included)"""
    V, F = np.asarray(V, f32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    use = usable_faces(V, F)
    Fc = np.where(use[:, None], F, 0)
    c = tuple(V[Fc[:, j]] if len(V) else np.zeros((len(F), 3), f32) for j in range(3))
    good = ray_ok(rays)
    out = np.full((len(rays), len(F)), EMPTY, np.uint64)
    idx = np.nonzero(good)[0]
    for s in range(0, len(idx), chunk):
        q = idx[s:s + chunk]
        hit, t, _, _, _, _ = test(rays[q, :3], rays[q, 3:6], rays[q, 6], rays[q, 7], shear(rays[q, 3:6]), c, box)
        out[q] = keys_of(hit & use[None, :], t, np.arange(len(F)))
    return out


def cast(rays, V, F, ok=None, chunk=256):
    """Brute force over all faces: the outputs of R rays as a dict of flat arrays (KEYS)"""
    V, F = np.asarray(V, f32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    rays = np.asarray(rays, f32).reshape(-1, 8)
    R = len(rays)
    good = ray_ok(rays, ok)
    best = face_times(rays, V, F, chunk).min(1) if len(F) else np.full(R, EMPTY)
    best = np.where(good, best, EMPTY)
    out = {"depth": np.zeros(R, f32), "face": np.full(R, -1, np.int32), "code": np.where(good, MISSED, NO_RAY).astype(np.uint8),
           "bary": np.zeros((R, 3), f32), "vertex": np.full(R, -1, np.int32), "normal": np.zeros((R, 3), f32), "side": np.zeros(R, np.int8)}
    q = np.nonzero(best != EMPTY)[0]
    if not len(q):
        return out
    face = (best[q] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out["code"][q] = HIT
    out["face"][q] = face
    out["depth"][q] = (best[q] >> np.uint64(32)).astype(np.uint32).view(f32)
    v0, v1, v2 = V[F[face, 0]], V[F[face, 1]], V[F[face, 2]]
    o, d = rays[q, :3], rays[q, 3:6]
    k = shear(d)
    r = np.arange(len(q))
    U, Vv, W, det = (np.empty(len(q), f32) for _ in range(4))
    for s in range(0, len(q), chunk):            # (the diagonal of a chunk x chunk test: the winner's own U, V, W)
        e = slice(s, s + chunk)
        _, _, u, v, w, dt = test(o[e], d[e], rays[q[e], 6], rays[q[e], 7], tuple(a[e] for a in k), (v0[e], v1[e], v2[e]))
        n = np.arange(u.shape[0])
        U[e], Vv[e], W[e], det[e] = u[n, n], v[n, n], w[n, n], dt[n, n]
    with np.errstate(all="ignore"):
        b = np.stack([U / det, Vv / det, W / det], 1)
        kb = np.zeros(len(q), np.int64)
        kb[b[:, 1] > b[:, 0]] = 1
        kb[b[:, 2] > b[r, kb]] = 2
        e1, e2 = v1 - v0, v2 - v0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        dot = (nx * d[:, 0] + ny * d[:, 1]) + nz * d[:, 2]
        side = np.where(dot < 0, 1, -1).astype(np.int8)
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        fine = (ln > 0) & (ln <= FMAX)
        u3 = np.stack([nx / ln, ny / ln, nz / ln], 1)
        u3 = np.where((side > 0)[:, None], u3, -u3)
    out["bary"][q] = b
    out["vertex"][q] = F[face, kb]
    out["side"][q] = side
    out["normal"][q] = np.where(fine[:, None], u3, f32(0))
    assert out["bary"].dtype == f32 and out["normal"].dtype == f32
    return out


def moller_trumbore(rays, V, F):
    """(R,) bool: some face is hit by the plain float32 Moller-Trumbore test (t >= 0).  NOT the rule: it leaves holes on edges."""
    o, d = rays[:, :3], rays[:, 3:6]
    hit = np.zeros(len(rays), bool)
    for a, b, c in F:
        e1, e2 = V[b] - V[a], V[c] - V[a]
        with np.errstate(all="ignore"):
            p = np.cross(d, e2).astype(f32)
            det = (p * e1).sum(1, dtype=f32)
            inv = f32(1) / det
            s = o - V[a]
            u = (s * p).sum(1, dtype=f32) * inv
            q = np.cross(s, e1).astype(f32)
            v = (d * q).sum(1, dtype=f32) * inv
            t = (q * e2).sum(1, dtype=f32) * inv
            hit |= (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
    return hit


# ------------------------------------------------------------------------------------------------ the index
def _cell(g, res):
    """mc_cell: floor, clamped as a float, then converted (NaN gives 0)"""
    with np.errstate(invalid="ignore"):
        c = np.fmin(np.fmax(np.floor(f32(g)), f32(0)), f32(res - 1))
    return int(c) if c == c else 0


def make_grid(res, lo, cell):
    lo, cell = np.asarray(lo, f32), np.asarray(cell, f32)
    return tuple(int(r) for r in res), lo, (f32(1) / cell).astype(f32), cell


def within_reach(o, grid):
    """mc_walk's first test: the ray's reach against PNR_MESHCAST_MAX_REACH smallest cells"""
    res, lo, inv, cell = grid
    with np.errstate(all="ignore"):
        og = ((np.asarray(o, f32) - lo) * inv).astype(f32)
        reach = ((np.abs(og) + (np.asarray(res) + 1).astype(f32)) * cell).astype(f32).max()
        return bool(np.isfinite(og).all() and reach <= MAX_REACH * cell.min())


def bin_faces(V, F, grid):
    """mc_scatter: {(cx, cy, cz): [faces]} of the usable faces"""
    res, lo, inv, _ = grid
    V, F = np.asarray(V, f32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    cells = {}
    for t in np.nonzero(usable_faces(V, F))[0]:
        g = ((V[F[t]] - lo) * inv).astype(f32)                     # (3 corners, 3 axes)
        rng = [range(_cell(g[:, k].min() - PAD, res[k]), _cell(g[:, k].max() + PAD, res[k]) + 1) for k in range(3)]
        for c in itertools.product(*rng):
            cells.setdefault(c, []).append(int(t))
    return cells


def walk(ray, grid, cells, keys):
    """mc_walk for one ray (8 floats): keys (F,) uint64 are the ray's brute-force keys per face (EMPTY: no hit), so that the walk is
    restated apart from the test.  Returns None where the ray takes the plain loop, else (best key, faces tested, layers visited)."""
    res, lo, inv, _ = grid
    o, d, near, far = ray[:3].astype(f32), ray[3:6].astype(f32), f32(ray[6]), f32(ray[7])
    with np.errstate(all="ignore"):
        og, dg = ((o - lo) * inv).astype(f32), (d * inv).astype(f32)
        if not (within_reach(o, grid) and (np.abs(dg) <= FMAX).all()):
            return None
        kz = 0
        if abs(dg[1]) > abs(dg[0]):
            kz = 1
        if abs(dg[2]) > abs(dg[kz]):
            kz = 2
        kx, ky = (1 if kz == 0 else 0), (1 if kz == 2 else 2)
        dz, oz = dg[kz], og[kz]
        if dz == 0:
            return None
        t_in, t_out = near, far
        for k in range(3):
            a, b = -PAD, f32(res[k]) + PAD
            if dg[k] == 0:
                if og[k] < a or og[k] > b:
                    return EMPTY, 0, 0
            else:
                ta, tb = (a - og[k]) / dg[k], (b - og[k]) / dg[k]
                t_in, t_out = np.fmax(t_in, np.fmin(ta, tb)), np.fmin(t_out, np.fmax(ta, tb))
        if not (abs(t_in) <= FMAX and abs(t_out) <= FMAX):
            return None
        if not t_in <= t_out:
            return EMPTY, 0, 0
        up = dz > 0
        gz_in = oz + t_in * dz
        L = _cell(gz_in - PAD if up else gz_in + PAD, res[kz])
        best, tested, layers = EMPTY, 0, 0
        while 0 <= L < res[kz]:
            layers += 1
            za, zb = (f32(L), f32(L + 1)) if up else (f32(L + 1), f32(L))
            ta, tb = (za - oz) / dz, (zb - oz) / dz
            ta, tb = np.fmin(np.fmax(ta, t_in), t_out), np.fmin(np.fmax(tb, t_in), t_out)
            xa, xb, ya, yb = og[kx] + ta * dg[kx], og[kx] + tb * dg[kx], og[ky] + ta * dg[ky], og[ky] + tb * dg[ky]
            x0, x1 = _cell(np.fmin(xa, xb) - PAD, res[kx]), _cell(np.fmax(xa, xb) + PAD, res[kx])
            y0, y1 = _cell(np.fmin(ya, yb) - PAD, res[ky]), _cell(np.fmax(ya, yb) + PAD, res[ky])
            for cy in range(y0, y1 + 1):
                for cx in range(x0, x1 + 1):
                    c = [0, 0, 0]
                    c[kz], c[kx], c[ky] = L, cx, cy
                    for t in cells.get(tuple(c), ()):
                        tested += 1
                        best = min(best, keys[t])
            if best != EMPTY:
                tb_ = np.uint32(int(best) >> 32).view(f32)
                gzb = oz + tb_ * dz
                if ((zb - gzb) if up else (gzb - zb)) > PAD:
                    break
            if tb >= t_out:
                break
            L += 1 if up else -1
    return best, tested, layers


# ------------------------------------------------------------------------------------------------ shared scenes
EDGE_WEIGHTS = (0.5, 0.25, 0.125, 0.3, 0.7)


def edge_targets(V, F):
    """every vertex, and five points along every edge, of a mesh: float32 points whose rays pass exactly through or within an
    ulp of a shared edge or vertex"""
    E = np.asarray(sorted({(min(a, b), max(a, b)) for t in np.asarray(F) for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}))
    out = [np.asarray(V, f32)]
    for w in EDGE_WEIGHTS:
        out.append((V[E[:, 0]] * f32(1 - w) + V[E[:, 1]] * f32(w)).astype(f32))
    return np.concatenate(out)


def rays_to(origin, targets, near=0.0, far=1e30):
    """(n, 8) rays from one origin through every target, d = target - origin in float32 (targets equal to the origin left out)"""
    o = np.asarray(origin, f32)
    d = (np.asarray(targets, f32) - o).astype(f32)
    d = d[(d != 0).any(1)]
    rays = np.zeros((len(d), 8), f32)
    rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, f32(near), f32(far)
    return rays


def soup(n_vertices=300, n_faces=500, seed=1, spread=0.7):
    """a random triangle soup with the edge cases of the rule: faces 1 and 3 repeat face 0 (a tie goes to the lowest index),
    faces 4 .. 6 have zero area, face 7 has a NaN corner (its own vertex) and face 8 an index out of range"""
    g = np.random.default_rng(seed)
    V = (g.standard_normal((n_vertices + 1, 3)) * spread).astype(f32)
    F = g.integers(0, n_vertices, (n_faces, 3)).astype(np.int32)
    F[0] = (0, 1, 2)
    F[1] = F[3] = F[0]
    F[4], F[5], F[6] = (5, 5, 9), (7, 7, 7), (11, 12, 11)
    V[n_vertices] = (np.nan, 0.0, 0.0)
    F[7] = (3, n_vertices, 4)
    F[8] = (3, n_vertices + 1, 4)
    return V, F


# the reviewer's case of a ray in the plane of a face, found on the rule WITHOUT the box test: there face 0 "hit" at t = 2.131, far
# outside its own box, and an index finer than 16^3 stopped on face 1 without ever testing it
GRAZING_V = np.array([[-0.9428961277008057, 0.7392842173576355, 0.15818531811237335], [0.8466171622276306, 0.7523073554039001, 0.08670332282781601],
                      [-0.51825350522995, 0.36794155836105347, -0.09832806140184402], [-0.41287708282470703, 0.7554562091827393, 0.2041945606470108],
                      [-0.44577115774154663, 0.7677369117736816, 0.12117549777030945], [-0.3799830377101898, 0.8293725252151489, 0.164453387260437]], f32)
GRAZING_RAY = np.array([-0.9159047603607178, 1.1438058614730835, 0.4157823920249939, 0.23498500883579254, -0.16799211502075195,
                        -0.11795687675476074, 0.0, 1e30], f32)
PAIR = np.array([[0, 1, 2], [3, 4, 5]], np.int32)


@functools.lru_cache(maxsize=None)
def grazing_cases(n_cases=24, seed=11, outside=0.03):
    """[(V (6, 3), ray (8,))]: two-face meshes with teeth.  Face 0 is a large triangle and the ray lies in its plane, from an
    origin in that plane outside it, up to float32 rounding: U, V, W are cancellation noise and, WITHOUT the box test, face 0
    "hits" at a t whose point lies more than `outside` beyond its own box.  Face 1 is a small triangle across the ray just behind
    that point.  There the plain loop and an index disagree unless the rule ties a hit to its face.  The first case is the
    reviewer's; the rest are drawn from a seed."""
    g = np.random.default_rng(seed)
    cases = [(GRAZING_V, GRAZING_RAY)]
    while len(cases) < n_cases:
        Vf = g.uniform(-1, 1, (3, 3)).astype(f32)
        n = 20000
        w = g.uniform(-3, 3, (n, 2, 2))
        w = np.concatenate([w, 1 - w.sum(2, keepdims=True)], 2)
        P = np.einsum("rpc,ck->rpk", w, Vf.astype(f64))
        rays = np.zeros((n, 8), f32)
        rays[:, :3], rays[:, 3:6], rays[:, 7] = P[:, 0].astype(f32), (P[:, 1] - P[:, 0]).astype(f32), f32(1e30)
        old = face_times(rays, Vf, PAIR[:1], box=False)[:, 0]
        idx = np.nonzero(old != EMPTY)[0]
        t = (old[idx] >> np.uint64(32)).astype(np.uint32).view(f32).astype(f64)
        p = rays[idx, :3].astype(f64) + t[:, None] * rays[idx, 3:6].astype(f64)
        far_out = np.maximum(Vf.min(0) - p, p - Vf.max(0)).max(1) > outside
        for q, tq in zip(idx[far_out][:4], t[far_out][:4]):
            o, d = rays[q, :3].astype(f64), rays[q, 3:6].astype(f64)
            u = np.cross(d, (1.0, 0.3, -0.7))
            u /= np.linalg.norm(u)
            v = np.cross(d, u)
            v /= np.linalg.norm(v)
            m = o + tq * 1.002 * d
            T = np.array([m + 0.05 * u, m - 0.025 * u + 0.043 * v, m - 0.025 * u - 0.043 * v]).astype(f32)
            cases.append((np.concatenate([Vf, T]), rays[q].copy()))
    return cases[:n_cases]


def grazing_scene(n_cases=24):
    """(V, F, rays): the cases of grazing_cases as one mesh and one ray list"""
    cases = grazing_cases(n_cases)
    V = np.concatenate([c[0] for c in cases])
    F = np.concatenate([PAIR + 6 * k for k in range(len(cases))]).astype(np.int32)
    return V, F, np.stack([c[1] for c in cases])


def close_wall_views():
    """[(name, V, F, rays, ok)]: ordinary rays next to faces far larger than the origin's distance to them -- a wide pinhole
    1 cm and 5 cm from a wall of a 10 x 10 x 3 room, and 4000 unit rays from 1.5 m / 5 cm above a two-triangle floor of
    half-size 100 / 1000 / 10 at floor points around the camera's foot.  Every one must hit: none is near grazing."""
    from panopticnerf_amd import Pinhole, synthetic
    import _camera_ref as cr
    out = []
    room = synthetic.box_mesh((-5.0, -5.0, -1.5), (5.0, 5.0, 1.5))
    cam = Pinhole(12.0, 12.0, 31.5, 23.5, 64, 48)
    for x in (4.95, 4.99):
        view = (cam.word, np.asarray(cam.params, f32), np.asarray(cr.pose(np.pi / 2, 0.0, (x, 0.3, 0.2)), f32), 64, 48)
        rays, ok = camera_rays(view, 0.0, 100.0)
        out.append(("room wall at %.2f" % (5.0 - x), room.vertices.numpy(), room.faces.numpy(), rays, ok))
    g = np.random.default_rng(2)
    for half, height, within in ((100.0, 1.5, 3.0), (1000.0, 1.5, 3.0), (10.0, 0.05, 0.1)):
        V = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], f32)
        F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
        o = np.array([0.3, -0.2, height])
        tg = np.concatenate([g.uniform(-within, within, (4000, 2)) + o[:2], np.zeros((4000, 1))], 1)
        d = tg - o
        rays = np.zeros((4000, 8), f32)
        rays[:, :3], rays[:, 3:6], rays[:, 7] = o.astype(f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32), f32(1e4)
        out.append(("floor %g from %g" % (half, height), V, F, rays, np.ones(4000, bool)))
    return out
