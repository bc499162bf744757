"""numpy restatement of include/pnr.h "nearest neighbours": the nearest-neighbour rule twice (brute force over all n, and the
hashed search: cells, buckets, box), the cloud metrics on math.fsum, and the mesh sampler through tests/_philox.py.  Every
float32 operation is one numpy float32 operation in the order the header gives.  Not part of the product package."""
import math

import numpy as np

import _philox

PAD = np.float32(1.0009765625)
CLAMP = np.float32(1048576.0)
HX, HY, HZ = np.uint32(73856093), np.uint32(19349663), np.uint32(83492791)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_PER_FACE = 65535
OFFSETS_D = ((0.0, 0.25), (7.0, 3.0), (3000.0, 0.05), (-1e5, 0.5), (0.0, 1e-3))


def f32(a):
    return np.asarray(a, dtype=np.float32)


def finite_rows(p):
    return np.isfinite(p).all(axis=1)


def d2_matrix(q, ref):
    """(m, n) float32: d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded"""
    with np.errstate(all="ignore"):
        d = f32(q)[:, None, :] - f32(ref)[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _answer(keys):
    best = keys.min(axis=1) if keys.shape[1] else np.full(keys.shape[0], EMPTY)
    none = best == EMPTY
    index = np.where(none, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    dist2 = np.where(none, np.uint32(0x7F800000), (best >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    return index, dist2


def _keys(q, ref, D, allowed=None):
    """(m, n) uint64 keys, EMPTY where ref[j] is no candidate of query i (or not `allowed`)"""
    q, ref = f32(q), f32(ref)
    r2 = np.float32(D) * np.float32(D)
    d2 = d2_matrix(q, ref)
    with np.errstate(invalid="ignore"):
        cand = (d2 <= r2) & finite_rows(ref)[None, :] & finite_rows(q)[:, None]
    if allowed is not None:
        cand &= allowed
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(ref.shape[0], dtype=np.uint64)[None, :]
    return np.where(cand, key, EMPTY)


def brute(q, ref, D):
    """(index int32, dist2 float32, stats [found, none, invalid]) of the rule, over all n"""
    q = f32(q).reshape(-1, 3)
    ref = f32(ref).reshape(-1, 3)
    index, dist2 = _answer(_keys(q, ref, D))
    ok = finite_rows(q)
    return index, dist2, [int((index >= 0).sum()), int((ok & (index < 0)).sum()), int((~ok).sum())]


def grid(ref, D):
    """(origin float32[3], Dp, inv) of the spatial hash"""
    ref = f32(ref).reshape(-1, 3)
    o = ref[0] if ref.shape[0] and np.isfinite(ref[0]).all() else np.zeros(3, np.float32)
    Dp = np.float32(D) * PAD
    h = np.float32(2.0) * Dp
    return o, Dp, np.float32(1.0) / h


def cell(p, o, inv):
    """int64 cell coordinates of the float32 points p (..., 3)"""
    with np.errstate(all="ignore"):
        c = np.floor((f32(p) - o) * inv)
        return np.clip(c, -CLAMP, CLAMP).astype(np.int64)


def bucket(c, T):
    c = c.astype(np.int64).astype(np.uint32)            # two's complement words
    with np.errstate(over="ignore"):
        return ((c[..., 0] * HX) ^ (c[..., 1] * HY) ^ (c[..., 2] * HZ)) & np.uint32(T - 1)


def table(ref, D, T):
    """(bucket of every finite reference point or -1, start (T + 1) int32) of the build"""
    ref = f32(ref).reshape(-1, 3)
    o, _, inv = grid(ref, D)
    ok = finite_rows(ref)
    b = np.where(ok, bucket(cell(np.where(ok[:, None], ref, 0), o, inv), T).astype(np.int64), -1)
    count = np.bincount(b[ok], minlength=T)
    return b, np.concatenate([[0], np.cumsum(count)]).astype(np.int32)


def hashed(q, ref, D, T):
    """(index, dist2, largest cell span of a query's box) by the structure: only records in the buckets of the box are tested"""
    q = f32(q).reshape(-1, 3)
    ref = f32(ref).reshape(-1, 3)
    o, Dp, inv = grid(ref, D)
    b_ref, _ = table(ref, D, T)
    okq = finite_rows(q)
    qs = np.where(okq[:, None], q, 0)
    c0, c1 = cell(qs - Dp, o, inv), cell(qs + Dp, o, inv)
    span = int((c1 - c0)[okq].max()) if okq.any() else 0
    allowed = np.zeros((q.shape[0], ref.shape[0]), dtype=bool)
    for dz in range(span + 1):
        for dy in range(span + 1):
            for dx in range(span + 1):
                c = c0 + np.array([dx, dy, dz])
                inside = (c <= c1).all(axis=1)
                allowed |= inside[:, None] & (bucket(c, T).astype(np.int64)[:, None] == b_ref[None, :])
    index, dist2 = _answer(_keys(q, ref, D, allowed))
    return index, dist2, span


def adversarial(n, m, offset, D, seed=0):
    """(ref (n, 3), q (m, 3)) float32: a lattice of pitch D / 4 (distances of exactly D and exact ties), the first 50 reference
    points repeated at the end (a tie goes to the lowest index), a Gaussian blob of width 4 D, one NaN row and one row with an inf;
    queries: lattice points, a blob of width 5 D, reference points shifted by exactly D along one axis, one NaN query.  ref[0] is an
    isolated point and q[0] lies exactly D from it, so at offset 0 one answer has dist2 == r2 and the index 0, not n - n_rep."""
    rng = np.random.default_rng([seed, n, m])
    D32, off = np.float32(D), np.float32(offset)
    pitch = D32 / np.float32(4)

    def lattice(k, span):
        return off + rng.integers(-span, span + 1, size=(k, 3)).astype(np.float32) * pitch

    n_rep = min(50, n // 4)
    n_bad = 2 if n >= 8 else 0
    n_lat = (n - n_rep - n_bad) // 2
    n_blob = n - n_rep - n_bad - n_lat
    ref = np.concatenate([lattice(n_lat, 24), off + f32(rng.normal(size=(n_blob, 3))) * (np.float32(4) * D32)]).astype(np.float32)
    if n_bad:
        bad = np.tile(off, (2, 3)).astype(np.float32)
        bad[0, 1], bad[1, 2] = np.nan, np.inf
        ref = np.concatenate([ref[: len(ref) // 2], bad, ref[len(ref) // 2:]])
    if n >= 8:                                          # an isolated point, 10 blob widths out: ref[0], repeated at the end with the first 50
        ref[0] = off + f32([40, 0, 0]) * D32
    ref = np.concatenate([ref, ref[:n_rep]]).astype(np.float32)
    assert ref.shape == (n, 3)
    m_bad = 1 if m >= 4 else 0
    m_lat = (m - m_bad) // 3
    m_shift = min((m - m_bad) // 4, n)
    m_blob = m - m_bad - m_lat - m_shift
    good = ref[finite_rows(ref)]
    if len(good):
        pick = good[rng.integers(0, len(good), size=m_shift)].copy()
        axis = rng.integers(0, 3, size=m_shift)
        pick[np.arange(m_shift), axis] = pick[np.arange(m_shift), axis] + D32 * rng.choice(f32([-1, 1]), size=m_shift)
    else:
        pick = lattice(m_shift, 24)
    q = np.concatenate([lattice(m_lat, 36), off + f32(rng.normal(size=(m_blob, 3))) * (np.float32(5) * D32), pick]).astype(np.float32)
    if m_bad:
        q = np.concatenate([q[: len(q) // 2], f32([[np.nan, off, off]]), q[len(q) // 2:]])
        q[0] = ref[0] + f32([0, 1, 0]) * D32             # exactly D from the isolated point (at offset 0), which ties with its repeat
    assert q.shape == (m, 3)
    return ref, q


def cloud_metrics(index, dist2, D, taus, query=None):
    """(sums [d, d^2] by math.fsum on float64, counts [n, missing, per threshold ...]) of pnr_cloud_metrics"""
    index, dist2 = np.asarray(index), f32(dist2)
    keep = ~np.isnan(dist2)
    if query is not None:
        keep &= finite_rows(f32(query).reshape(-1, 3))
    found = index >= 0
    with np.errstate(invalid="ignore"):
        d = np.where(found, np.sqrt(dist2.astype(np.float64)), np.float64(np.float32(D)))[keep]
    counts = [int(keep.sum()), int((keep & ~found).sum())]
    for t in taus:
        t2 = np.float32(t) * np.float32(t)
        counts.append(int((keep & found & (dist2 <= t2)).sum()))
    return [math.fsum(d.tolist()), math.fsum((d * d).tolist())], counts


def summarize(pred_side, gt_side, n_tau):
    """Evaluator.summarize's geom_* keys from the two (sums, counts) pairs"""
    out = {}
    (sp, cp), (sg, cg) = pred_side, gt_side
    mean = lambda v, n: v / n if n else math.nan
    acc, comp = mean(sp[0], cp[0]), mean(sg[0], cg[0])
    out["geom_accuracy"], out["geom_completeness"], out["geom_chamfer"] = acc, comp, 0.5 * (acc + comp)
    out["geom_accuracy_rms"] = math.sqrt(mean(sp[1], cp[0])) if cp[0] else math.nan
    out["geom_completeness_rms"] = math.sqrt(mean(sg[1], cg[0])) if cg[0] else math.nan
    out["geom_precision"] = [mean(cp[2 + k], cp[0]) for k in range(n_tau)]
    out["geom_recall"] = [mean(cg[2 + k], cg[0]) for k in range(n_tau)]
    out["geom_fscore"] = [2.0 * p * r / (p + r) if p + r > 0 else math.nan for p, r in zip(out["geom_precision"], out["geom_recall"])]
    out["geom_n_pred"], out["geom_n_gt"], out["geom_missing_pred"], out["geom_missing_gt"] = cp[0], cg[0], cp[1], cg[1]
    return out


def _uniform(w):
    return ((w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def sample_counts(vertices, faces, rho, seed):
    """(k_t int64 per triangle, p0, e1, e2 float32 with zeros for a triangle whose indices are out of range)"""
    v, f = f32(vertices).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = f.shape[0]
    ok = ((f >= 0) & (f < v.shape[0])).all(axis=1) if F else np.zeros(0, bool)
    fs = np.where(ok[:, None], f, 0)
    z = np.zeros((F, 3), np.float32)
    if v.shape[0] == 0:
        p0 = e1 = e2 = z
    else:
        with np.errstate(all="ignore"):
            p0 = np.where(ok[:, None], v[fs[:, 0]], z)
            e1 = np.where(ok[:, None], v[fs[:, 1]] - p0, z)
            e2 = np.where(ok[:, None], v[fs[:, 2]] - p0, z)
    with np.errstate(all="ignore"):
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        s = (nx * nx + ny * ny) + nz * nz
        area = np.float32(0.5) * np.sqrt(s)
        ctr = np.zeros((F, 4), dtype=np.uint32)
        ctr[:, 0] = np.arange(F, dtype=np.uint32)
        seed &= 2 ** 64 - 1
        key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
        u = _uniform(_philox.philox4x32_10(ctr, key)[:, 0]) if F else np.zeros(0, np.float32)
        x = np.floor(area * np.float32(rho) + u)
        k = np.where(ok & np.isfinite(area), np.minimum(np.nan_to_num(x, nan=0.0, posinf=MAX_PER_FACE), MAX_PER_FACE), 0).astype(np.int64)
    return k, p0, e1, e2


def sample(vertices, faces, rho, seed):
    """(points (N, 3) float32, face (N,) int32) of the sampler"""
    k, p0, e1, e2 = sample_counts(vertices, faces, rho, seed)
    face = np.repeat(np.arange(len(k), dtype=np.int64), k)
    start = np.concatenate([[0], np.cumsum(k)])
    j = np.arange(len(face), dtype=np.int64) - start[face]
    ctr = np.zeros((len(face), 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1] = face.astype(np.uint32), (1 + j).astype(np.uint32)
    seed &= 2 ** 64 - 1
    w = _philox.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)) if len(face) else np.zeros((0, 4), np.uint32)
    u, v = _uniform(w[:, 0]), _uniform(w[:, 1])
    flip = (u + v) > np.float32(1.0)
    u, v = np.where(flip, np.float32(1.0) - u, u), np.where(flip, np.float32(1.0) - v, v)
    with np.errstate(all="ignore"):
        pts = (p0[face] + u[:, None] * e1[face]) + v[:, None] * e2[face]
    return pts.astype(np.float32), face.astype(np.int32)
