"""The connected-components rule of include/pnr.h "connected components" restated in plain numpy and Python, written from the
rule and not from the kernels: a flood fill in raster order for lattices (so the numbering by lowest flat index needs no
renumbering), a sequential union-find for meshes; and the case generators of test_cc_ref.py and test_gpu_components.py.  Test
support, not part of the product package."""
from collections import deque

import numpy as np

KEYS, VALUES = 0, 1


def offsets(rank, full):
    """the neighbour offsets (dz, dy, dx) of an element: 4 / 8 in an image (dz = 0), 6 / 26 in a volume"""
    out = []
    for dz in ((-1, 0, 1) if rank == 3 else (0,)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nz = (dz != 0) + (dy != 0) + (dx != 0)
                if nz == 0 or (not full and nz != 1):
                    continue
                out.append((dz, dy, dx))
    return out


def foreground(data, mode):
    data = np.asarray(data)
    if mode == KEYS:
        return data >= 0
    with np.errstate(invalid="ignore"):
        return np.isfinite(data) & (data > 0)


def linked(a, b, mode, tol):
    """the mode's test on two foreground elements: equal keys, or one float32 subtraction against tol"""
    if mode == KEYS:
        return a == b
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(np.abs(np.float32(a) - np.float32(b)) <= np.float32(tol))


def label(data, mode=KEYS, tol=0.0, full=False):
    """(labels int32 of data's shape, count, size int32 of data's shape) by the rule; data 2-D or 3-D"""
    data = np.asarray(data)
    rank = data.ndim
    d3 = data.reshape((1,) + data.shape) if rank == 2 else data
    rz, ry, rx = d3.shape
    fg = foreground(d3, mode)
    lab = np.full(d3.shape, -1, np.int32)
    offs = offsets(rank, full)
    sizes = []
    for iz in range(rz):
        for iy in range(ry):
            for ix in range(rx):
                if not fg[iz, iy, ix] or lab[iz, iy, ix] >= 0:
                    continue
                c = len(sizes)
                lab[iz, iy, ix] = c
                todo, n = deque([(iz, iy, ix)]), 0
                while todo:
                    z, y, x = todo.popleft()
                    n += 1
                    for dz, dy, dx in offs:
                        jz, jy, jx = z + dz, y + dy, x + dx
                        if not (0 <= jz < rz and 0 <= jy < ry and 0 <= jx < rx):
                            continue
                        if fg[jz, jy, jx] and lab[jz, jy, jx] < 0 and linked(d3[z, y, x], d3[jz, jy, jx], mode, tol):
                            lab[jz, jy, jx] = c
                            todo.append((jz, jy, jx))
                sizes.append(n)
    sizes = np.asarray(sizes, np.int32).reshape(-1)
    size = np.where(lab >= 0, sizes[np.maximum(lab, 0)] if len(sizes) else 0, 0).astype(np.int32)
    return lab.reshape(data.shape), len(sizes), size.reshape(data.shape)


def stats(labels, count):
    """(sizes (count,) int32, boxes (count, 6) int32 = ix_min, iy_min, iz_min, ix_max, iy_max, iz_max)"""
    labels = np.asarray(labels)
    l3 = labels.reshape((1,) * (3 - labels.ndim) + labels.shape)
    sizes, boxes = np.zeros(count, np.int32), np.zeros((count, 6), np.int32)
    for c in range(count):
        z, y, x = np.nonzero(l3 == c)
        sizes[c] = len(z)
        boxes[c] = (x.min(), y.min(), z.min(), x.max(), y.max(), z.max())
    return sizes, boxes


def largest(labels, sizes, k):
    """bool mask of the k largest components; a tie goes to the lower number"""
    order = sorted(range(len(sizes)), key=lambda c: (-int(sizes[c]), c))[:k]
    return np.isin(labels, order) & (np.asarray(labels) >= 0)


def renumber(comp, used=None):
    """arbitrary component ids (one per element) -> numbers by lowest member; elements with used False get -1"""
    comp = np.asarray(comp).reshape(-1)
    out, seen = np.full(comp.shape, -1, np.int32), {}
    for i, c in enumerate(comp):
        if used is not None and not used[i]:
            continue
        if c not in seen:
            seen[c] = len(seen)
        out[i] = seen[c]
    return out, len(seen)


def label_mesh(faces, n_vertices):
    """(vertex_label (V,), face_label (F,), face_size (F,) int32, count) by the rule: a sequential union-find over the vertices"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(n_vertices))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    ok = ((faces >= 0) & (faces < n_vertices)).all(axis=1) if len(faces) else np.zeros(0, bool)
    used = np.zeros(n_vertices, bool)
    for f in faces[ok]:
        used[f] = True
        for a, b in ((f[0], f[1]), (f[1], f[2])):
            ra, rb = find(int(a)), find(int(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    vlab, count = renumber([find(v) for v in range(n_vertices)], used)
    flab = np.where(ok, vlab[np.clip(faces[:, 0], 0, max(n_vertices - 1, 0))] if n_vertices else -1, -1).astype(np.int32) if len(faces) \
        else np.zeros(0, np.int32)
    per = np.bincount(flab[flab >= 0], minlength=count).astype(np.int32)
    fsize = np.where(flab >= 0, per[np.maximum(flab, 0)] if count else 0, 0).astype(np.int32)
    return vlab, flab, fsize, count


def select(vertices, faces, mask):
    """Mesh.select restated: (vertices, faces int32, index) of the masked faces; faces with an index out of range are dropped"""
    faces = np.asarray(faces, np.int64)[np.asarray(mask, bool)]
    V = len(vertices)
    faces = faces[((faces >= 0) & (faces < V)).all(axis=1)]
    index = np.unique(faces.reshape(-1))
    new = np.full(V, -1, np.int64)
    new[index] = np.arange(len(index))
    return np.asarray(vertices)[index], new[faces].astype(np.int32), index


def despeckle(depth, max_diff, min_size, full=False):
    depth = np.asarray(depth, np.float32)
    _, _, size = label(depth, VALUES, max_diff, full)
    return np.where((size > 0) & (size < min_size), np.float32(0), depth)


# ---------------------------------------------------------------------------------------------------------------- the cases

def axis_sizes(t):
    return (1, t - 1, t, t + 1, 2 * t + 1)


def shapes_2d(tile, small=5):
    """(height, width): every size of axis_sizes on each axis, the other axis small; and the largest of both"""
    tx, ty = tile
    out = [(small, n) for n in axis_sizes(tx)] + [(n, small) for n in axis_sizes(ty)] + [(1, 1), (2 * ty + 1, 2 * tx + 1)]
    return sorted(set(s for s in out if min(s) >= 1))


def shapes_3d(tile, small=3):
    tx, ty, tz = tile
    out = [(small, small, n) for n in axis_sizes(tx)] + [(small, n, small) for n in axis_sizes(ty)] + [(n, small, small) for n in axis_sizes(tz)]
    out += [(1, 1, 1), (1, 1, 37), (2 * tz + 1, 2 * ty + 1, 2 * tx + 1)]
    return sorted(set(s for s in out if min(s) >= 1))


PERCOLATION = {2: 0.593, 3: 0.312}            # site percolation, 4-linked square and 6-linked cubic lattices


def bernoulli(shape, p, seed):
    return np.where(np.random.default_rng(seed).random(shape) < p, 0, -1).astype(np.int32)


def serpentine(shape):
    """one path through every row between walls: rows 0, 2, 4, .. are foreground, the odd rows only at alternating ends (in a
    volume the slices are joined the same way along z at one corner)"""
    m = np.full(shape, -1, np.int32)
    img = m.reshape((-1,) + shape[-2:])
    for z in range(img.shape[0]):
        if len(shape) == 3 and z % 2:
            img[z, 0 if (z // 2) % 2 else shape[-2] - 1 - (shape[-2] - 1) % 2, 0] = 0
            continue
        for y in range(shape[-2]):
            if y % 2 == 0:
                img[z, y, :] = 0
            else:
                img[z, y, -1 if (y // 2) % 2 == 0 else 0] = 0
    return m


def spiral(shape):
    """an inward spiral of width 1 with a gap of 1, in the last two axes (every slice of a volume the same): a walk that turns
    right whenever the next cell is outside or the cell behind it is taken"""
    h, w = shape[-2:]
    img = np.full((h, w), -1, np.int32)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y, x, d, turned = 0, 0, 0, 0
    img[0, 0] = 0
    while turned < 2:
        dy, dx = dirs[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < h and 0 <= nx < w and img[ny, nx] < 0 and not (0 <= ay < h and 0 <= ax < w and img[ay, ax] >= 0):
            y, x, turned = ny, nx, 0
            img[y, x] = 0
        else:
            d, turned = (d + 1) % 4, turned + 1
    return np.broadcast_to(img, shape).copy() if len(shape) == 3 else img


def comb(shape):
    """teeth along the last axis' even columns that join only in the last row (of the last slice, in a volume)"""
    m = np.full(shape, -1, np.int32)
    m[..., ::2] = 0
    if len(shape) == 3:
        m[-1, -1, :] = 0
    else:
        m[-1, :] = 0
    return m


def u_shape(shape):
    """two teeth at the first and last column that join only in the last row"""
    m = np.full(shape, -1, np.int32)
    m[..., 0] = 0
    m[..., -1] = 0
    if len(shape) == 3:
        m[-1, -1, :] = 0
    else:
        m[-1, :] = 0
    return m


def checkerboard(shape):
    idx = np.indices(shape).sum(axis=0)
    return np.where(idx % 2 == 0, 0, -1).astype(np.int32)


def corner_pair(shape, tile):
    """two elements touching only at the corner where 4 (8) tiles meet: t - 1 and t on every axis; None where the shape is too
    small.  tile is (tx, ty[, tz]), the shape ([rz,] ry, rx)."""
    t = tuple(tile)[::-1]
    if any(s <= ti for s, ti in zip(shape, t)):
        return None
    m = np.full(shape, -1, np.int32)
    m[tuple(ti - 1 for ti in t)] = 0
    m[t] = 0
    return m


def stripes(shape):
    """one-element-wide stripes of alternating keys 1, 2 along the last axis, with a background stripe every fifth"""
    k = np.arange(shape[-1])
    row = np.where(k % 5 == 4, -1, 1 + k % 2).astype(np.int32)
    return np.broadcast_to(row, shape).copy()


def multikey(shape, seed):
    return np.random.default_rng(seed).integers(-1, 4, size=shape).astype(np.int32)


def key_patterns(shape, tile, seed=0):
    """name -> int32 keys of `shape`"""
    rank = len(shape)
    one = np.full(shape, -1, np.int32)
    one[tuple(s // 2 for s in shape)] = 3
    out = {"background": np.full(shape, -1, np.int32), "foreground": np.zeros(shape, np.int32), "one": one,
           "p20": bernoulli(shape, 0.2, seed + 1), "p45": bernoulli(shape, 0.45, seed + 2), "p90": bernoulli(shape, 0.9, seed + 3),
           "percolation": bernoulli(shape, PERCOLATION[rank], seed + 4), "serpentine": serpentine(shape), "spiral": spiral(shape),
           "comb": comb(shape), "u": u_shape(shape), "checkerboard": checkerboard(shape), "multikey": multikey(shape, seed + 5),
           "stripes": stripes(shape)}
    cp = corner_pair(shape, tile)
    if cp is not None:
        out["corner"] = cp
    return out


def value_cases(shape, seed=0):
    """name -> (float32 values of `shape`, tol)"""
    f = np.float32
    n = int(np.prod(shape))
    tol = f(0.25)
    up = np.nextafter(tol, f(np.inf), dtype=np.float32)
    ramp = (f(1.0) + tol * np.arange(n, dtype=np.float32)).astype(np.float32).reshape(shape)           # exact: multiples of 2^-2
    # up and 2 up alternate like a checkerboard: axis neighbours differ by exactly up (2 up = 0.5 + 2^-24 is a float32)
    steep = np.where(np.indices(shape).sum(axis=0) % 2 == 0, up, f(2.0) * up).astype(np.float32)
    g = np.random.default_rng(seed)
    noisy = (f(2.0) + g.random(shape, dtype=np.float32)).astype(np.float32)
    holes = noisy.copy().reshape(-1)
    bad = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5]
    holes[g.choice(n, min(n, 3 * len(bad)), replace=False)] = np.resize(np.asarray(bad, np.float32), min(n, 3 * len(bad)))
    chain = np.zeros(shape, np.float32)
    flat = chain.reshape(-1)
    flat[:min(3, shape[-1])] = [1.0, 1.25, 1.5][:min(3, shape[-1])]                                      # a ~ b ~ c, |a - c| = 2 tol
    quant = (f(1.0) + np.floor(g.random(shape) * 4).astype(np.float32)).astype(np.float32)
    return {"ramp_at_tol": (ramp, tol), "ramp_above_tol": (steep, tol), "chain": (chain, tol), "holes": (holes.reshape(shape), f(0.3)),
            "tol_zero": (quant, f(0.0)), "tol_inf": (holes.reshape(shape), f(np.inf)), "noisy": (noisy, f(0.2))}
