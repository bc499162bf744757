"""CPU restatements of the stereo-matching rule of include/pnr.h ("stereo matching"), the reference of tests/test_sgm_ref.py and
tests/test_gpu_sgm.py.  Two of them, written independently:

  * numpy, vectorised over everything but the position along the path (census / cost / aggregate / select / depth / sgm);
  * plain Python integers, one pixel, one direction and one disparity at a time (loop_census / loop_sgm), for tiny images.

`variant` names a deliberately WRONG form of the vectorised rule (VARIANTS); the closed forms of test_sgm_ref.py must tell each
from the rule."""
import numpy as np

DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))        # (dy, dx), the rule's order
VARIANTS = ("census_le", "no_minus_m", "swap_p", "ties_high", "trunc_div", "uniq_le")
BIG = 1 << 20


def _popcount64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int32)


# ---------------------------------------------------------------- vectorised
def census(img, variant=None):
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape
    pad = np.pad(img, ((3, 3), (4, 4)), mode="edge").astype(np.int32)
    c = img.astype(np.int32)
    w = np.zeros((H, W), dtype=np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            nb = pad[3 + dy:3 + dy + H, 4 + dx:4 + dx + W]
            bit = (nb <= c) if variant == "census_le" else (nb < c)
            w = (w << np.uint64(1)) | bit.astype(np.uint64)
    return w.view(np.int64)


def cost(cl, cr, D):
    cl, cr = np.asarray(cl).view(np.uint64), np.asarray(cr).view(np.uint64)
    H, W = cl.shape
    C = np.full((H, W, D), 63, dtype=np.int32)
    for d in range(min(D, W)):
        C[:, d:, d] = _popcount64(cl[:, d:] ^ cr[:, :W - d])
    return C


def _step(c, prev, p1, p2, variant):
    """one step of a path for a batch of paths: c, prev (n, D)"""
    if variant == "swap_p":
        p1, p2 = p2, p1
    m = prev.min(axis=1, keepdims=True)
    lo = np.full_like(prev, BIG)
    hi = np.full_like(prev, BIG)
    lo[:, 1:] = prev[:, :-1]
    hi[:, :-1] = prev[:, 1:]
    best = np.minimum(np.minimum(prev, lo + p1), np.minimum(hi + p1, m + p2))
    return c + best if variant == "no_minus_m" else c + best - m


def path_costs(C, dy, dx, p1, p2, variant=None):
    """L_r (H, W, D) of one direction.  One loop along the path: over the columns for a horizontal direction, else over the rows
    (every pixel of row y has its predecessor in row y - dy)."""
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2, variant)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    cols = np.arange(W)
    for i, y in enumerate(ys):
        L[y] = C[y]
        if i == 0:
            continue
        has = (cols - dx >= 0) & (cols - dx < W)
        L[y, cols[has]] = _step(C[y, cols[has]], L[y - dy, cols[has] - dx], p1, p2, variant)
    return L


def aggregate(cl, cr, D, p1, p2, paths, variant=None):
    C = cost(cl, cr, D)
    S = np.zeros(C.shape, dtype=np.int32)
    for dy, dx in DIRECTIONS[:paths]:
        S += path_costs(C, dy, dx, p1, p2, variant)
    assert S.max() <= 2040 or variant is not None
    return S.astype(np.uint16)


def right_disparity(S, variant=None):
    S = np.asarray(S).astype(np.int32)
    H, W, D = S.shape
    cand = np.full((H, W, D), BIG, dtype=np.int32)
    for k in range(min(D, W)):
        cand[:, :W - k, k] = S[:, k:, k]
    return _argmin(cand, variant).astype(np.int16)


def _argmin(a, variant):
    if variant == "ties_high":
        return a.shape[-1] - 1 - np.argmin(a[..., ::-1], axis=-1)
    return np.argmin(a, axis=-1)


def select(S, uniqueness, lr_tol, variant=None):
    """(d16, disp_right) of a summed volume"""
    S = np.asarray(S).astype(np.int64)
    H, W, D = S.shape
    ds = _argmin(S, variant)
    best = np.take_along_axis(S, ds[..., None], axis=-1)[..., 0]
    k = np.arange(D)[None, None, :]
    far = np.abs(k - ds[..., None]) > 1
    second = np.where(far, S, BIG).min(axis=-1)
    dR = right_disparity(S, variant)
    x = np.arange(W)[None, :] + np.zeros((H, 1), dtype=np.int64)
    y = np.arange(H)[:, None] + np.zeros((1, W), dtype=np.int64)
    no_right = x - ds < 0
    if variant == "uniq_le":
        not_unique = far.any(axis=-1) & (second * (100 - uniqueness) <= best * 100)
    else:
        not_unique = far.any(axis=-1) & (second * (100 - uniqueness) < best * 100)
    lr = np.zeros((H, W), dtype=bool)
    if lr_tol >= 0:
        lr = np.abs(dR[y, np.clip(x - ds, 0, W - 1)].astype(np.int64) - ds) > lr_tol
    sm = np.take_along_axis(S, np.clip(ds - 1, 0, D - 1)[..., None], axis=-1)[..., 0]
    sp = np.take_along_axis(S, np.clip(ds + 1, 0, D - 1)[..., None], axis=-1)[..., 0]
    den = sm + sp - 2 * best
    num = 8 * (sm - sp)
    flat = (ds == 0) | (ds == D - 1) | (den == 0)
    den1 = np.where(flat, 1, den)
    if variant == "trunc_div":
        q = 2 * num + den1
        off = np.sign(q) * (np.abs(q) // (2 * den1))
    else:
        off = (2 * num + den1) // (2 * den1)            # numpy's // floors toward -inf
    off = np.where(flat, 0, off)
    d16 = 16 * ds + off
    d16 = np.where(lr, -3, d16)
    d16 = np.where(not_unique, -2, d16)
    d16 = np.where(no_right, -1, d16)
    return d16.astype(np.int16), dR


def depth(d16, fb, d_min, d_max):
    d16 = np.asarray(d16)
    fb, d_min, d_max = np.float32(fb), np.float32(d_min), np.float32(d_max)
    disp = d16.astype(np.float32) * np.float32(0.0625)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (fb / np.where(d16 > 0, disp, np.float32(1.0))).astype(np.float32)
    keep = (d16 > 0) & (z >= d_min) & (z <= d_max)
    return np.where(keep, z, np.float32(0.0)).astype(np.float32)


def sgm(left, right, max_disp=128, p1=10, p2=120, paths=8, uniqueness=5, lr_tol=1, variant=None):
    """the whole rule up to d16: dict(census_l, census_r, S, d16, disp_right)"""
    cl, cr = census(left, variant), census(right, variant)
    S = aggregate(cl, cr, max_disp, p1, p2, paths, variant)
    d16, dR = select(S, uniqueness, lr_tol, variant)
    return {"census_l": cl, "census_r": cr, "S": S, "d16": d16, "disp_right": dR}


# ---------------------------------------------------------------- plain loops over Python integers
def loop_census(img):
    H, W = len(img), len(img[0])
    out = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            centre, word = int(img[y][x]), 0
            for j in range(y - 3, y + 4):
                for i in range(x - 4, x + 5):
                    if j == y and i == x:
                        continue
                    jj, ii = min(max(j, 0), H - 1), min(max(i, 0), W - 1)
                    word = word * 2 + (1 if int(img[jj][ii]) < centre else 0)
            out[y][x] = word
    return out


def loop_sgm(left, right, D, p1, p2, paths, uniqueness, lr_tol):
    """(census_l, census_r, S, d16, disp_right) as nested lists of Python integers"""
    left, right = [[int(v) for v in row] for row in left], [[int(v) for v in row] for row in right]
    H, W = len(left), len(left[0])
    cl, cr = loop_census(left), loop_census(right)

    def C(y, x, d):
        return bin(cl[y][x] ^ cr[y][x - d]).count("1") if x - d >= 0 else 63

    S = [[[0] * D for _ in range(W)] for _ in range(H)]
    for dy, dx in DIRECTIONS[:paths]:
        L = {}
        order_y = range(H) if dy >= 0 else range(H - 1, -1, -1)
        order_x = range(W) if dx >= 0 else range(W - 1, -1, -1)
        for y in order_y:
            for x in order_x:
                py, px = y - dy, x - dx
                inside = 0 <= py < H and 0 <= px < W
                if inside:
                    prev = L[(py, px)]
                    m = min(prev)
                cur = []
                for d in range(D):
                    if not inside:
                        cur.append(C(y, x, d))
                        continue
                    terms = [prev[d], m + p2]
                    if d - 1 >= 0:
                        terms.append(prev[d - 1] + p1)
                    if d + 1 < D:
                        terms.append(prev[d + 1] + p1)
                    cur.append(C(y, x, d) + min(terms) - m)
                L[(y, x)] = cur
                for d in range(D):
                    S[y][x][d] += cur[d]
    dR = [[0] * W for _ in range(H)]
    for y in range(H):
        for xr in range(W):
            arg, val = None, None
            for k in range(D):
                if xr + k >= W:
                    break
                if val is None or S[y][xr + k][k] < val:
                    arg, val = k, S[y][xr + k][k]
            dR[y][xr] = arg
    d16 = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            row = S[y][x]
            best = min(row)
            ds = row.index(best)
            others = [row[k] for k in range(D) if abs(k - ds) > 1]
            if x - ds < 0:
                d16[y][x] = -1
            elif others and min(others) * (100 - uniqueness) < best * 100:
                d16[y][x] = -2
            elif lr_tol >= 0 and abs(dR[y][x - ds] - ds) > lr_tol:
                d16[y][x] = -3
            else:
                off = 0
                if 0 < ds < D - 1:
                    den = row[ds - 1] + row[ds + 1] - 2 * best
                    if den:
                        off = (2 * 8 * (row[ds - 1] - row[ds + 1]) + den) // (2 * den)      # Python's // floors
                d16[y][x] = 16 * ds + off
    return cl, cr, S, d16, dR
