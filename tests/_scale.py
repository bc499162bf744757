"""Inputs and chunked references of tests/test_gpu_geometry_scale.py: the geometry ops at the sizes where their kernels change
behaviour -- three trips of a grid-stride loop, three steps of k_scan_top's carried loop, a 64-bit scan total.  The launch and
scan rules are RESTATED here from csrc/pnr_common.h (pnr_grid_cap: 8 workgroups of 256 threads per compute unit),
csrc/pnr_nn.hip (k_cloud_metrics: min(1024, 4 per CU) workgroups) and csrc/pnr_scan_dev.h (tiles of 1024 items, summed 256
tiles a step), never asked of the library.  Every reference is one of the existing restatements (_cc_ref, _nn_ref,
_meshcast_ref, _reduce_ref), called in chunks where its working set would not fit, or a vectorised form of one that
tests/test_scale_ref.py pins to it on a small input.  Test support, not part of the product package."""
import numpy as np

import _cc_ref as cr
import _meshcast_ref as mc
import _nn_ref as nr

f32 = np.float32
BLOCK = 256                     # threads of a workgroup of every kernel here
PER_CU = 8                      # pnr_grid_cap's default
CM_MAX_BLOCKS, CM_PER_CU = 1024, 4
SCAN_TILE, SCAN_BLOCK = 1024, 256
SCAN3 = 2 * SCAN_BLOCK * SCAN_TILE + 77
BRUTE_BUDGET = 5 * 10 ** 7      # entries of the (m, n) matrices nr.brute builds, over a whole case
FRAME = (376, 1408)             # a KITTI-360 perspective frame
CLAMP_FACES = 32800             # x 65535 points = 2 149 548 000 > 2^31 - 1
CU_RANGE = (32, 64, 80, 104, 128, 228, 256, 304)


def ceil_div(a, b):
    return -(-a // b)


def stride3(cus):
    return 2 * PER_CU * cus * BLOCK + 77


def cm3(cus):
    return 2 * min(CM_MAX_BLOCKS, CM_PER_CU * cus) * BLOCK + 77


def items(cus):
    """the item count of a case that has both a grid-stride loop and a scan"""
    return max(stride3(cus), SCAN3)


def per_trip(cus, per_cu=PER_CU, max_blocks=None):
    """items one trip of a launch covers once the grid is capped"""
    blocks = cus * per_cu if max_blocks is None else min(max_blocks, cus * per_cu)
    return blocks * BLOCK


def trips(n, cus, per_cu=PER_CU, max_blocks=None, unit=BLOCK):
    """trips of the grid-stride loop of a launch over n items, `unit` of them a workgroup and trip"""
    blocks = max(1, min(ceil_div(n, unit), cus * per_cu if max_blocks is None else min(max_blocks, cus * per_cu)))
    return ceil_div(n, blocks * unit)


def scan_steps(n):
    """steps of k_scan_top's loop for a scan of n items"""
    return ceil_div(ceil_div(n, SCAN_TILE), SCAN_BLOCK)


def image_shape(cus):
    """(height, width): odd sides that straddle the 32 x 8 tile, at least items(cus) pixels; 1029 x 1021 on 256 compute units"""
    w = 1021
    h = ceil_div(items(cus), w)
    return (h + 1 - h % 2, w)


def lattice_shape(cus):
    """(res_z, res_y, res_x), no side a multiple of the 8 x 8 x 4 tile's; 65 x 129 x 127 on 256 compute units"""
    ry, rx = 129, 127
    rz = ceil_div(items(cus), ry * rx)
    return (rz + (rz % 4 == 0), ry, rx)


def tiles_of(shape, tile):
    """tiles of k_cc_tile over shape ([rz,] ry, rx); tile (tx, ty[, tz])"""
    t = tuple(tile)[::-1]
    return int(np.prod([ceil_div(s, ti) for s, ti in zip(shape, t)]))


def sizes(cus):
    """name -> (items, trips, scan steps or None) of every case of the GPU module at `cus` compute units"""
    n, img, lat = items(cus), image_shape(cus), lattice_shape(cus)
    V, F = ribbon_counts(mesh_faces_min(cus))
    m_big, n_small = query_sizes(cus)
    out = {
        "image": (img[0] * img[1], trips(img[0] * img[1], cus), scan_steps(img[0] * img[1])),
        "image tiles": (tiles_of(img, (32, 8)), trips(tiles_of(img, (32, 8)), cus, unit=1), None),
        "lattice": (int(np.prod(lat)), trips(int(np.prod(lat)), cus), scan_steps(int(np.prod(lat)))),
        "lattice tiles": (tiles_of(lat, (8, 8, 4)), trips(tiles_of(lat, (8, 8, 4)), cus, unit=1), None),
        "mesh faces": (F, trips(F, cus), None),
        "mesh vertices": (V, trips(V, cus), scan_steps(V)),
        "nn reference cloud": (n, trips(n, cus), None),
        "nn table": (1 << 20, None, scan_steps(1 << 20)),
        "nn queries": (m_big, trips(m_big, cus), None),
        "cloud metrics": (cm3(cus), trips(cm3(cus), cus, CM_PER_CU, CM_MAX_BLOCKS), None),
        "sample count faces": (n, trips(n, cus), scan_steps(n)),
        "sample emit points": (stride3(cus), trips(stride3(cus), cus), None),
        "cell table": (81 ** 3, None, scan_steps(81 ** 3)),
    }
    return out


def check_sizes(cus):
    """every case takes at least three trips and three scan steps at `cus` compute units"""
    for name, (n, t, s) in sizes(cus).items():
        assert t is None or t >= 3, (cus, name, n, t)
        assert s is None or s >= 3, (cus, name, n, s)
    half = ceil_div(image_shape(cus)[0] * image_shape(cus)[1], 2)          # the checkerboard's components: k_cc_stats_init
    assert trips(half, cus) >= 2, (cus, half)
    return True


# ------------------------------------------------------------------------------------------------------ the shared scan

def exclusive(counts):
    """(n + 1,) int32: what pnr_scan_i32 leaves of n counts whose total fits an int32"""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int32)


def scan_restated(counts, drop_carry=False):
    """pnr_scan_i32 launch by launch in numpy: tile sums, k_scan_top's loop over 256 tiles a step with its 64-bit carry, the
    tiles applied; returns ((n + 1,) int32, the 64-bit total).  drop_carry: THE PLANTED FAULT -- a step starts from 0 again."""
    c = np.asarray(counts, np.int64).reshape(-1)
    n = len(c)
    tiles = ceil_div(n, SCAN_TILE)
    pad = np.zeros(tiles * SCAN_TILE, np.int64)
    pad[:n] = c
    sums = pad.reshape(tiles, SCAN_TILE).sum(1)
    top, carry, total = np.zeros(tiles, np.int64), 0, 0
    for s in range(0, tiles, SCAN_BLOCK):
        part = sums[s:s + SCAN_BLOCK]
        top[s:s + SCAN_BLOCK] = carry + np.concatenate([[0], np.cumsum(part)[:-1]])
        total += int(part.sum())
        carry = 0 if drop_carry else carry + int(part.sum())
    inside = np.cumsum(pad.reshape(tiles, SCAN_TILE), 1) - pad.reshape(tiles, SCAN_TILE)
    out = (top[:, None] + inside).reshape(-1)[:n]
    last = out[-1] + c[-1] if n else 0
    return np.concatenate([out, [last]]).astype(np.int32), total


def counts_per_step(counts):
    """the sum of the counts of every step of k_scan_top: all non-zero where a lost carry is to show"""
    c = np.asarray(counts, np.int64).reshape(-1)
    step = SCAN_TILE * SCAN_BLOCK
    return [int(c[s:s + step].sum()) for s in range(0, len(c), step)]


def check_start(start, counts, what=""):
    """THE comparison of every scanned table: all n + 1 entries equal the exclusive sums of the counts"""
    want = exclusive(counts)
    start = np.asarray(start)
    assert start.shape == want.shape and start.dtype == np.int32, (what, start.shape, start.dtype)
    bad = np.nonzero(start != want)[0]
    assert not len(bad), "%s: %d of %d scan entries differ, the first at %d (step %d of k_scan_top): %d for %d" % (
        what, len(bad), len(want), bad[0], bad[0] // (SCAN_TILE * SCAN_BLOCK), start[bad[0]], want[bad[0]])
    return True


# ---------------------------------------------------------------------------------------------------------- components

def check_labels(got, want, what=""):
    """THE comparison of a labelling: got and want are (labels, count, size) with size possibly None on the got side"""
    lab, count, size = got
    assert count == want[1], (what, count, want[1])
    bad = np.nonzero(np.asarray(lab).reshape(-1) != np.asarray(want[0]).reshape(-1))[0]
    assert not len(bad), "%s: %d labels differ, the first at flat index %d" % (what, len(bad), bad[0])
    if size is not None:
        bad = np.nonzero(np.asarray(size).reshape(-1) != np.asarray(want[2]).reshape(-1))[0]
        assert not len(bad), "%s: %d sizes differ, the first at flat index %d" % (what, len(bad), bad[0])
    return True


def foreground_per_trip(keys, cus):
    """foreground elements in every trip's index range of a grid-stride launch over the keys"""
    fg = (np.asarray(keys).reshape(-1) >= 0)
    step = per_trip(cus)
    return [int(fg[s:s + step].sum()) for s in range(0, fg.size, step)]


def values_of(keys):
    """(float32 values, tol) that the values mode links exactly as the keys mode links `keys`: 1 + key / 2 on the foreground --
    distinct keys are at least 0.5 apart and tol is just below it -- and on the background a cycle of every kind of value that is
    no foreground: NaN, +inf, -inf, 0, -0, a negative number"""
    keys = np.asarray(keys)
    bad = np.resize(np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5], f32), keys.size).reshape(keys.shape)
    return np.where(keys >= 0, f32(1.0) + f32(0.5) * keys.astype(f32), bad).astype(f32), np.nextafter(f32(0.5), f32(0))


def stats(labels, count):
    """cr.stats vectorised: (sizes (count,) int32, boxes (count, 6) int32); cr.stats scans the image once per component"""
    labels = np.asarray(labels)
    l3 = labels.reshape((1,) * (3 - labels.ndim) + labels.shape)
    z, y, x = np.nonzero(l3 >= 0)
    c = l3[z, y, x].astype(np.int64)
    sizes = np.bincount(c, minlength=count).astype(np.int32)
    boxes = np.zeros((count, 6), np.int32)
    for k, a in enumerate((x, y, z)):
        lo, hi = np.full(count, np.iinfo(np.int64).max), np.full(count, -1, np.int64)
        np.minimum.at(lo, c, a)
        np.maximum.at(hi, c, a)
        boxes[:, k], boxes[:, 3 + k] = lo, hi
    return sizes, boxes


# --------------------------------------------------------------------------------------------------------- the big mesh

RIBBON = 1023                   # faces of one ribbon


def ribbon_counts(n_faces_min, ribbon=RIBBON):
    """(vertices, faces) of ribbon_mesh"""
    R = ceil_div(n_faces_min, ribbon)
    return R * (ribbon + 2) + 1, R * ribbon + R - len(set(_cuts(R)) | {R - 1})


def mesh_faces_min(cus):
    """the n_faces_min of the big mesh: items(cus), raised a ribbon at a time until the last trip over the faces holds at least
    100 of them -- the unusable faces and the last rays' targets lie there"""
    n = items(cus)
    while (ribbon_counts(n)[1] - 1) % per_trip(cus) < 100:
        n += RIBBON
    return n


def _cuts(R):
    """the ribbons after which no bridge follows: seven pieces of unequal size"""
    return sorted(set(min(R - 1, max(0, int(R * f))) for f in (0.03, 0.11, 0.37, 0.5, 0.52, 0.9)))


def ribbon_mesh(n_faces_min, ribbon=RIBBON, seed=0):
    """(V (nv, 3) float32, F (nf, 3) int32, info): at least n_faces_min faces as R parallel ribbons of `ribbon` triangles, every
    ribbon a strip (j, j + 1, j + 2) over its own ribbon + 2 vertices from np.arange, on a wavy sheet (a true 3-D surface: the
    ray-casting grid has several layers).  A bridge triangle joins each ribbon to the next, except after the ribbons of `cuts`:
    several disjoint pieces of unequal size, each spanning many trips' worth of indices.  The ribbons' blocks of faces come in a
    seeded random order, so a piece's faces lie in every trip and the face order is not the vertex order.  Three faces near the
    END of the list are no faces of a ray cast: one with an index == nv (out of range), one with -1, and one whose corner is
    the last vertex, which is NaN and used by nothing else (that face is valid for cc_mesh, which reads no coordinates).
    info: pieces, the cut list, the three unusable faces."""
    L = ribbon
    R = ceil_div(n_faces_min, L)
    nv = R * (L + 2) + 1
    j = np.arange(L + 2)
    r = np.arange(R)
    x = 0.01 * j[None, :] + 0.0 * r[:, None]
    y = 0.02 * r[:, None] + 0.015 * (j % 2)[None, :]
    z = 0.2 * np.sin(0.37 * x * 10.0 + 0.11 * r[:, None]) * np.cos(0.05 * r[:, None])
    V = np.concatenate([np.stack([x, y, z], -1).reshape(-1, 3), [[np.nan, 0.0, 0.0]]]).astype(f32)
    base = (r * (L + 2))[:, None]
    k = np.arange(L)[None, :]
    strip = np.stack([base + k, base + k + 1, base + k + 2], -1)                                  # (R, L, 3)
    bridge = np.stack([base[:, 0] + L + 1, base[:, 0] + L, base[:, 0] + (L + 2) + L + 1], -1)     # the ends of ribbons r and r + 1
    cuts = _cuts(R)
    has = np.ones(R, bool)
    has[cuts] = False
    has[R - 1] = False
    blocks = np.concatenate([strip, bridge[:, None, :]], 1)                                       # (R, L + 1, 3)
    keep = np.ones((R, L + 1), bool)
    keep[:, L] = has
    order = np.random.default_rng(seed).permutation(R)
    F = blocks[order][keep[order]].astype(np.int32)
    nf = len(F)
    bad = (nf - 97, nf - 41, nf - 7)
    F[bad[0], 1] = nv
    F[bad[1], 0] = -1
    F[bad[2], 2] = nv - 1
    assert V.shape == (nv, 3) and (nv, nf) == ribbon_counts(n_faces_min, L) and nf >= n_faces_min
    return V, F, {"pieces": len(cuts) + 1, "cuts": cuts, "unusable": bad, "ribbons": R, "order": order}


def aimed_rays(V, F, cus, n=16):
    """(n, 8) rays at the big mesh whose winners lie in the first, a middle and the last trip's range of face indices: straight down
    on a face's centroid from 1 above it, obliquely from one far origin at centroids, at a vertex several faces share (a tie
    goes to the lowest face), one that points away (a miss) and one with d = 0 (no ray)"""
    nf, step = len(F), per_trip(cus)
    use = mc.usable_faces(V, F)
    last = min((trips(nf, cus) - 1) * step, nf - 2000)
    picks = [3, step - 2, step + 5, (nf // 2) | 1, 2 * step - 1, last + 1, nf - 1500, nf - 99, nf - 40, nf - 1]
    picks = [p for p in picks if 0 <= p < nf and use[p]]
    cen = V[F[picks]].astype(np.float64).mean(1)
    rays = np.zeros((n, 8), f32)
    rays[:, 7] = f32(1e30)
    k = len(picks)
    rays[:k, :3], rays[:k, 3:6] = (cen + (0.0, 0.0, 1.0)).astype(f32), f32([0.0, 0.0, -1.0])
    far = np.asarray([5.0, 10.0, 6.0])
    for i, p in enumerate((0, 4, 7)):                                       # oblique: whatever lies in front wins
        rays[k + i, :3], rays[k + i, 3:6] = far.astype(f32), (cen[p % k] - far).astype(f32)
    v = V[F[picks[1], 1]]                                                   # a shared vertex, from straight above
    rays[k + 3, :3], rays[k + 3, 3:6] = (v + f32([0, 0, 1])).astype(f32), f32([0.0, 0.0, -1.0])
    rays[k + 4, :3], rays[k + 4, 3:6] = (cen[0] + (0.0, 0.0, 1.0)).astype(f32), f32([0.0, 0.0, 1.0])
    rays[k + 5:, :3] = f32([1.0, 1.0, 1.0])                                 # d = 0: no rays
    return rays


def cast_chunked(rays, V, F, chunk=1 << 17):
    """mc.cast over all faces, `chunk` faces at a time: brute force keeps, per ray, the smallest key (bits(t), face), and every
    other output is a function of the ray and the winning face alone -- so the winner over all faces is the best of the
    chunks' winners, with its outputs as that chunk computed them"""
    V, F = np.asarray(V, f32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    rays = np.asarray(rays, f32).reshape(-1, 8)
    best, out = np.full(len(rays), mc.EMPTY), None
    for s in range(0, max(len(F), 1), chunk):
        part = mc.cast(rays, V, F[s:s + chunk])
        hit = part["code"] == mc.HIT
        part["face"] = np.where(hit, part["face"] + s, -1).astype(np.int32)
        key = np.where(hit, (part["depth"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.maximum(part["face"], 0).astype(np.uint64), mc.EMPTY)
        if out is None:
            out, best = part, key
            continue
        take = key < best
        best = np.where(take, key, best)
        for name in mc.KEYS:
            out[name][take] = part[name][take]
    return out


def bin_counts(V, F, grid):
    """mc.bin_faces vectorised, as counts: (cells,) int64, cell = (cz res_y + cy) res_x + cx, the entries mc_scatter gives every
    cell -- a face enters every cell of its padded box, so a box adds +-1 at its eight corners of a difference array and three
    running sums give the counts.  grid: mc.make_grid's."""
    res, lo, inv, _ = grid
    V, F = np.asarray(V, f32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    Fu = F[mc.usable_faces(V, F)]
    g = ((V[Fu] - lo) * inv).astype(f32)                                    # (faces, corners, axes)
    top = np.asarray(res, f32) - f32(1)
    with np.errstate(invalid="ignore"):
        c0 = np.fmin(np.fmax(np.floor(g.min(1) - mc.PAD), f32(0)), top)
        c1 = np.fmin(np.fmax(np.floor(g.max(1) + mc.PAD), f32(0)), top)
    c0, c1 = np.nan_to_num(c0, nan=0.0).astype(np.int64), np.nan_to_num(c1, nan=0.0).astype(np.int64) + 1
    rx, ry, rz = res
    diff = np.zeros((rz + 1) * (ry + 1) * (rx + 1), np.int64)
    for sz, cz in ((1, c0[:, 2]), (-1, c1[:, 2])):
        for sy, cy in ((1, c0[:, 1]), (-1, c1[:, 1])):
            for sx, cx in ((1, c0[:, 0]), (-1, c1[:, 0])):
                np.add.at(diff, (cz * (ry + 1) + cy) * (rx + 1) + cx, sz * sy * sx)
    d = diff.reshape(rz + 1, ry + 1, rx + 1).cumsum(0).cumsum(1).cumsum(2)
    return d[:rz, :ry, :rx].reshape(-1)


def bin_counts_scalar(V, F, grid):
    """the same counts from mc.bin_faces' dictionary"""
    rx, ry, rz = grid[0]
    out = np.zeros(rx * ry * rz, np.int64)
    for (cx, cy, cz), faces in mc.bin_faces(V, F, grid).items():
        out[(cz * ry + cy) * rx + cx] = len(faces)
    return out


# -------------------------------------------------------------------------------------------------- nearest neighbours

D = 0.25
PITCH = f32(D) / f32(4)         # every coordinate is an integer multiple: distances of exactly D, exact ties


def query_sizes(cus):
    """(m, n) of the big query set: m queries against n <= 48 reference points, m n within the budget"""
    m = stride3(cus)
    return m, min(48, BRUTE_BUDGET // m)


def lattice_points(n, half, seed):
    return (np.random.default_rng(seed).integers(-half, half + 1, size=(n, 3)).astype(f32) * PITCH).astype(f32)


def big_reference(cus, seed=1):
    """(ref (n, 3), q (m, 3)), n = items(cus): lattice points in a cube of 801^3 sites -- about one to a cell of the hash, a
    neighbour within D for about half of them --, the first 50 repeated at the END (a tie goes to the lowest index: the answer
    lies in the first trip, its twin in the last), a NaN and an inf row in the last trip.  q: a few dozen queries, m n within the
    budget: reference points of the first, a middle and the last trip themselves and shifted by exactly D along an axis,
    lattice points, one NaN row."""
    n = items(cus)
    ref = lattice_points(n, 400, seed)
    ref[n - 50:] = ref[:50]
    ref[n - 60, 1], ref[n - 61, 2] = np.nan, np.inf
    m = min(48, BRUTE_BUDGET // n)
    step = per_trip(cus)
    at = [0, 7, step - 1, step, n // 2, 2 * step + 3, n - 62, n - 59, n - 50, n - 43, n - 1]
    shifted = ref[at].copy()
    shifted[np.arange(len(at)), np.arange(len(at)) % 3] += f32(D) * f32([1, -1])[np.arange(len(at)) % 2]
    q = np.concatenate([ref[at], shifted, f32([[np.nan, 0, 0]]), lattice_points(m, 400, seed + 1)])[:m].astype(f32)
    return ref, q


def big_queries(cus, seed=2):
    """(ref (n, 3), q (m, 3)), m = stride3(cus) and n a few dozen: lattice queries around a small cloud, a quarter to a half of
    them with a neighbour; in the LAST trip's range a NaN row, a +inf and a -inf row, and queries exactly D from a reference
    point along every axis (the same at the start of the first trip)"""
    m, n = query_sizes(cus)
    ref = lattice_points(n, 12, seed)
    q = lattice_points(m, 16, seed + 1)
    shifted = np.concatenate([ref[:6] + f32(D) * np.eye(3, dtype=f32)[np.arange(6) % 3], ref[6:12] - f32(D) * np.eye(3, dtype=f32)[np.arange(6) % 3]])
    q[:12] = shifted
    q[m - 40:m - 28] = shifted
    q[m - 20] = (np.nan, 0, 0)
    q[m - 13, 1] = np.inf
    q[m - 5, 2] = -np.inf
    return ref, q.astype(f32)


def brute_chunked(q, ref, max_dist, chunk=None):
    """nr.brute over the queries in chunks whose (chunk, n) matrices stay small: (index, dist2, stats)"""
    q, ref = nr.f32(q).reshape(-1, 3), nr.f32(ref).reshape(-1, 3)
    chunk = max(1, (1 << 22) // max(len(ref), 1)) if chunk is None else chunk
    index, dist2, stats = [], [], [0, 0, 0]
    for s in range(0, len(q), chunk):
        i, d, st = nr.brute(q[s:s + chunk], ref, max_dist)
        index.append(i)
        dist2.append(d)
        stats = [a + b for a, b in zip(stats, st)]
    if not index:
        return np.zeros(0, np.int32), np.zeros(0, f32), stats
    return np.concatenate(index), np.concatenate(dist2), stats


def metrics_case(m, seed=0):
    """the rows of test_gpu_geometry_eval's order test at any m: (index, dist2, query, root, active) with dist2 the square of
    k 2^e, k < 2^12 -- exact in float32 with an exact root -- over 44 binades, a seventh of the rows without a neighbour, a
    seventh with a NaN dist2 and a seventh with a query that is not finite"""
    rng = np.random.default_rng([seed, m])
    root = np.ldexp(rng.integers(1, 4096, m).astype(f32), rng.integers(-50, -6, m)).astype(f32)
    dist2 = root * root
    index = rng.integers(0, 1000, m).astype(np.int32)
    q = rng.uniform(-4, 4, size=(m, 3)).astype(f32)
    lost, nan, bad = (rng.choice(m, max(m // 7, 1), replace=False) for _ in range(3))
    index[lost], dist2[lost] = -1, np.inf
    dist2[nan] = np.nan
    q[bad, rng.integers(0, 3, bad.size)] = np.resize(f32([np.nan, np.inf, -np.inf]), bad.size)
    active = ~np.isnan(dist2) & nr.finite_rows(q)
    return index, dist2, q, root, active


# -------------------------------------------------------------------------------------------------------- mesh sampling

def small_triangles(F, seed=3, mean_count=0.3):
    """(vertices (3 F, 3), faces (F, 3), rho): F triangles of edge about 0.02 scattered in the unit cube and the density at which a
    face gets `mean_count` points on average; near the END a face with an index out of range and one with a NaN corner"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1, 1, size=(F, 1, 3)) + rng.uniform(-0.02, 0.02, size=(F, 3, 3))).astype(f32).reshape(-1, 3)
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    p = v.reshape(F, 3, 3).astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    f[F - 3, 1] = 3 * F
    v[3 * (F - 11)] = np.nan
    return v, f, float(mean_count / area.mean())


def large_triangles(n_points_min, n_faces=48, seed=4):
    """(vertices, faces, rho = 1): a few dozen right triangles of unequal area, each below the clamp of 65535 points, together a
    little above n_points_min"""
    rng = np.random.default_rng(seed)
    mean = 1.06 * n_points_min / n_faces
    target = mean * (0.6 + 0.8 * np.arange(n_faces) / (n_faces - 1))
    assert target.max() < 0.95 * nr.MAX_PER_FACE, "more triangles are needed for %d points" % n_points_min
    s = np.sqrt(2.0 * target)
    p0 = rng.uniform(-50, 50, size=(n_faces, 3))
    v = np.stack([p0, p0 + np.stack([s, 0 * s, 0.1 * s], -1), p0 + np.stack([0 * s, s, -0.2 * s], -1)], 1).astype(f32).reshape(-1, 3)
    return v, np.arange(3 * n_faces, dtype=np.int32).reshape(n_faces, 3), 1.0


def clamped_triangles(n_faces=CLAMP_FACES):
    """(vertices, faces, rho = 1): every face has area 80000 and gets the clamp's 65535 points"""
    i = np.arange(n_faces, dtype=np.float64)
    v = np.stack([np.stack([i, 0 * i, 0 * i], -1), np.stack([i + 400, 0 * i, 0 * i], -1), np.stack([i, 0 * i + 400, 0 * i], -1)], 1)
    return v.astype(f32).reshape(-1, 3), np.arange(3 * n_faces, dtype=np.int32).reshape(n_faces, 3), 1.0
