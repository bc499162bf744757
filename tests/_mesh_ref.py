"""CPU restatements of the mesh-extraction rule (include/pnr.h "mesh extraction"): marching tetrahedra on the Kuhn split of the
lattice Network.query_grid defines.  Twice: `extract_loops` is plain Python over points, cubes, tetrahedra and triangles with
numpy.float32 scalars, `extract` is vectorised numpy float32 in the rule's op order.  The two agree bit for bit, and the GPU
equals `extract` bit for bit (tests/test_mesh_ref.py, tests/test_gpu_mesh.py).  Both return (vertices (V, 3) float32, faces
(T, 3) int32, src (V,) int64).

`extract_loops(corrupt=...)` breaks the rule in one named way; the closed-form checks at the bottom must notice each."""
import numpy as np

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # xyz xzy yxz yzx zxy zyx
PARITY = (0, 1, 1, 0, 0, 1)
# FLIP[case][parity of the permutation]: 1 = the triangle's second and third vertex are swapped.  case: bit k = corner w_k inside.
FLIP = ((0, 0), (0, 1), (1, 0), (0, 1), (0, 1), (1, 0), (0, 1), (0, 1),
        (1, 0), (0, 1), (1, 0), (1, 0), (0, 1), (0, 1), (1, 0), (0, 0))
CORRUPTIONS = ("ge", "from_inside", "diagonal", "winding", "src_outside")
MAX_POINTS = (2 ** 31 - 1) // 12


def tet_codes(tet):
    """corner codes (x + 2 y + 4 z of the offset from the cube's corner) of w0 .. w3"""
    p = PERMS[tet]
    c1 = 1 << p[0]
    return (0, c1, c1 | (1 << p[1]), 7)


def case_triangles(case):
    """the rule's triangles of a case before winding: a list of three (inside corner, outside corner) pairs each"""
    I = [k for k in range(4) if case >> k & 1]
    O = [k for k in range(4) if not case >> k & 1]
    if len(I) == 1:
        return [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
    if len(I) == 3:
        return [[(I[0], O[0]), (I[1], O[0]), (I[2], O[0])]]
    if len(I) == 2:
        q = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def derive_flip():
    """FLIP from geometry: vertices at edge midpoints of the unit tetrahedron, normal against (outside mean - inside mean)"""
    out = []
    for case in range(16):
        row = [None, None]
        for tet in range(6):
            w = np.array([[(c >> a) & 1 for a in range(3)] for c in tet_codes(tet)], dtype=np.float64)
            flips = set()
            I = [k for k in range(4) if case >> k & 1]
            O = [k for k in range(4) if not case >> k & 1]
            for tri in case_triangles(case):
                p = [(w[a] + w[b]) / 2 for a, b in tri]
                s = float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), w[O].mean(0) - w[I].mean(0)))
                assert abs(s) > 1e-9
                flips.add(int(s < 0))
            if flips:
                assert len(flips) == 1
                f = flips.pop()
                assert row[PARITY[tet]] in (None, f)        # the swap depends on the case and the parity only
                row[PARITY[tet]] = f
        out.append(tuple(0 if v is None else v for v in row))
    return tuple(out)


def tet_table():
    """TAB[tet][case] = list of triangles, each three (owner corner code, kind) pairs, winding applied"""
    tab = []
    for tet in range(6):
        c = tet_codes(tet)
        rows = []
        for case in range(16):
            tris = []
            for tri in case_triangles(case):
                v = [(c[min(a, b)], (c[max(a, b)] ^ c[min(a, b)]) - 1) for a, b in tri]
                if FLIP[case][PARITY[tet]]:
                    v[1], v[2] = v[2], v[1]
                tris.append(v)
            rows.append(tris)
        tab.append(rows)
    return tab


TAB = tet_table()


def lattice(lo, hi, res):
    """(lo32, step32) of query_grid: float32 lo, (hi32 - lo32) / res32; res = (res_x, res_y, res_z)"""
    lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
    hi32 = np.asarray(hi, dtype=np.float32).reshape(3)
    with np.errstate(all="ignore"):
        return lo32, ((hi32 - lo32) / np.asarray(res, dtype=np.float32)).astype(np.float32)


def _empty():
    return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0,), np.int64)


# ---------------------------------------------------------------- plain loops
def extract_loops(field, lo, hi, level, corrupt=None):
    f = np.ascontiguousarray(field, dtype=np.float32)
    rz, ry, rx = f.shape
    assert corrupt is None or corrupt in CORRUPTIONS
    if min(rx, ry, rz) < 2:
        return _empty()
    lo32, step = lattice(lo, hi, (rx, ry, rz))
    level = np.float32(level)
    half, zero, one = np.float32(0.5), np.float32(0.0), np.float32(1.0)
    res = (rx, ry, rz)

    def val(i):
        return f[i[2], i[1], i[0]]

    def inside(i):
        return bool(val(i) >= level) if corrupt == "ge" else bool(val(i) > level)

    def flat(i):
        return (i[2] * ry + i[1]) * rx + i[0]

    def pos(i):
        return [np.float32(np.float32(np.float32(i[a]) + half) * step[a]) + lo32[a] for a in range(3)]

    ids, verts, src = {}, [], []
    with np.errstate(all="ignore"):
        for iz in range(rz):
            for iy in range(ry):
                for ix in range(rx):
                    a = (ix, iy, iz)
                    for kind in range(7):
                        off = ((kind + 1) & 1, (kind + 1) >> 1 & 1, (kind + 1) >> 2 & 1)
                        b = tuple(a[k] + off[k] for k in range(3))
                        if any(b[k] >= res[k] for k in range(3)) or inside(a) == inside(b):
                            continue
                        s, e = (b, a) if (corrupt == "from_inside" and inside(b)) else (a, b)
                        fs, fe = val(s), val(e)
                        t = np.float32(level - fs) / np.float32(fe - fs)
                        t = half if np.isnan(t) else (zero if t < zero else (one if t > one else t))
                        ps, pe = pos(s), pos(e)
                        ids[(flat(a), kind)] = len(verts)
                        verts.append([ps[k] + np.float32(t * np.float32(pe[k] - ps[k])) for k in range(3)])
                        want_inside = corrupt != "src_outside"
                        src.append(flat(a) if inside(a) == want_inside else flat(b))
    faces = []
    for iz in range(rz - 1):
        for iy in range(ry - 1):
            for ix in range(rx - 1):
                for tet in range(6):
                    codes = tet_codes(tet)
                    if corrupt == "diagonal" and tet == 0:          # xyz walks x, y, z; here its middle corner is taken from xzy
                        codes = (0, 1, 5, 7)
                    w = [(ix + (c & 1), iy + (c >> 1 & 1), iz + (c >> 2 & 1)) for c in codes]
                    case = sum(int(inside(w[k])) << k for k in range(4))
                    for tri in case_triangles(case):
                        v = []
                        for p, q in tri:
                            a, b = w[min(p, q)], w[max(p, q)]
                            kind = (b[0] - a[0]) + 2 * (b[1] - a[1]) + 4 * (b[2] - a[2]) - 1
                            v.append(ids[(flat(a), kind)])
                        flip = FLIP[case][PARITY[tet]]
                        if corrupt == "winding" and case == 6:
                            flip = 1 - flip
                        if flip:
                            v[1], v[2] = v[2], v[1]
                        faces.append(v)
    if not verts:
        return _empty()[0], np.asarray(faces, np.int32).reshape(-1, 3), _empty()[2]
    return (np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3),
            np.asarray(src, dtype=np.int64))


# ---------------------------------------------------------------- vectorised
_POP = np.array([bin(i).count("1") for i in range(128)], dtype=np.int64)
_NTRI = np.array([len(case_triangles(c)) for c in range(16)], dtype=np.int64)
# per (tet, case, triangle, corner): owner code and kind (zeros where the case has no such triangle)
_OWN = np.zeros((6, 16, 2, 3), dtype=np.int64)
_KIND = np.zeros((6, 16, 2, 3), dtype=np.int64)
for _t in range(6):
    for _c in range(16):
        for _j, _tri in enumerate(TAB[_t][_c]):
            for _s, (_o, _k) in enumerate(_tri):
                _OWN[_t, _c, _j, _s], _KIND[_t, _c, _j, _s] = _o, _k


def classify(field, level):
    """(mask (N,) the 7-bit crossing mask of the edges each point owns, ntri (N,) the triangle count of the cube at each point)"""
    f = np.ascontiguousarray(field, dtype=np.float32)
    rz, ry, rx = f.shape
    ins = f > np.float32(level)
    mask = np.zeros((rz, ry, rx), dtype=np.int64)
    ntri = np.zeros((rz, ry, rx), dtype=np.int64)
    if min(rx, ry, rz) < 2:
        return mask.reshape(-1), ntri.reshape(-1)
    for code in range(1, 8):
        ox, oy, oz = code & 1, code >> 1 & 1, code >> 2 & 1
        a = ins[:rz - oz, :ry - oy, :rx - ox]
        b = ins[oz:, oy:, ox:]
        mask[:rz - oz, :ry - oy, :rx - ox] |= (a != b).astype(np.int64) << (code - 1)
    corner = [ins[(c >> 2 & 1):rz - 1 + (c >> 2 & 1), (c >> 1 & 1):ry - 1 + (c >> 1 & 1), (c & 1):rx - 1 + (c & 1)].astype(np.int64)
              for c in range(8)]
    for tet in range(6):
        c = tet_codes(tet)
        case = corner[c[0]] | corner[c[1]] << 1 | corner[c[2]] << 2 | corner[c[3]] << 3
        ntri[:rz - 1, :ry - 1, :rx - 1] += _NTRI[case]
    return mask.reshape(-1), ntri.reshape(-1)


def extract(field, lo, hi, level):
    f = np.ascontiguousarray(field, dtype=np.float32)
    rz, ry, rx = f.shape
    if min(rx, ry, rz) < 2:
        return _empty()
    assert rx * ry * rz <= MAX_POINTS
    lo32, step = lattice(lo, hi, (rx, ry, rz))
    level = np.float32(level)
    flat_f = f.reshape(-1)
    ins = flat_f > level
    mask, _ = classify(f, level)
    base_v = np.cumsum(_POP[mask]) - _POP[mask]
    # vertices in (owner, kind) order
    own, kind = np.nonzero((mask[:, None] >> np.arange(7)[None, :]) & 1)
    code = kind + 1
    off = np.stack((code & 1, code >> 1 & 1, code >> 2 & 1), 1)
    far = own + off[:, 0] + off[:, 1] * rx + off[:, 2] * rx * ry
    ia = np.stack((own % rx, own // rx % ry, own // (rx * ry)), 1)
    half = np.float32(0.5)
    with np.errstate(all="ignore"):
        pa = (ia.astype(np.float32) + half) * step[None, :] + lo32[None, :]
        pb = ((ia + off).astype(np.float32) + half) * step[None, :] + lo32[None, :]
        fa, fb = flat_f[own], flat_f[far]
        t = (level - fa) / (fb - fa)
        t = np.where(np.isnan(t), half, np.where(t < 0, np.float32(0.0), np.where(t > 1, np.float32(1.0), t))).astype(np.float32)
        verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
    src = np.where(ins[own], own, far).astype(np.int64)
    # triangles in (cube, tetrahedron, triangle) order, over the cubes that have any
    ins3 = ins.reshape(rz, ry, rx)
    corner = [ins3[(c >> 2 & 1):rz - 1 + (c >> 2 & 1), (c >> 1 & 1):ry - 1 + (c >> 1 & 1), (c & 1):rx - 1 + (c & 1)] for c in range(8)]
    cm = sum(corner[c].astype(np.int64) << c for c in range(8))
    cz, cy, cx = np.nonzero((cm != 0) & (cm != 255))
    cube = (cz * ry + cy) * rx + cx                     # ascending: nonzero walks in row-major order
    cmv = cm[cz, cy, cx]
    K = cube.shape[0]
    tri_ids = np.zeros((K, 6, 2, 3), dtype=np.int64)
    valid = np.zeros((K, 6, 2), dtype=bool)
    corner_off = np.array([(c & 1) + (c >> 1 & 1) * rx + (c >> 2 & 1) * rx * ry for c in range(8)], dtype=np.int64)
    for tet in range(6):
        c = tet_codes(tet)
        case = (cmv >> c[0] & 1) | (cmv >> c[1] & 1) << 1 | (cmv >> c[2] & 1) << 2 | (cmv >> c[3] & 1) << 3
        valid[:, tet, :] = _NTRI[case][:, None] > np.arange(2)[None, :]
        owner = cube[:, None, None] + corner_off[_OWN[tet][case]]                   # (K, 2, 3)
        k = _KIND[tet][case]
        tri_ids[:, tet] = base_v[owner] + _POP[mask[owner] & ((1 << k) - 1)]
    faces = tri_ids[valid].astype(np.int32).reshape(-1, 3)
    return verts.reshape(-1, 3), faces, src


# ---------------------------------------------------------------- closed forms
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]), 0)


def edge_pairing(faces, n_vertices):
    """(count of each directed edge, count of its reverse), per distinct directed edge"""
    e = directed_edges(faces)
    n = max(int(n_vertices), 1)
    key, cnt = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    rev = (key % n) * n + key // n
    pos = np.searchsorted(key, rev)
    pos = np.minimum(pos, len(key) - 1)
    rcnt = np.where(key[pos] == rev, cnt[pos], 0) if len(key) else cnt
    return key, cnt, rcnt


def is_closed_oriented(faces, n_vertices):
    """every directed edge appears once, and so does its reverse"""
    _, cnt, rcnt = edge_pairing(faces, n_vertices)
    return len(cnt) > 0 and bool((cnt == 1).all() and (rcnt == 1).all())


def euler(faces, n_vertices=None):
    """V - E + F over the vertices the faces use"""
    f = np.asarray(faces, dtype=np.int64)
    e = np.sort(directed_edges(f), 1)
    n = int(f.max()) + 1 if f.size else 1
    return len(np.unique(f)) - len(np.unique(e[:, 0] * n + e[:, 1])) + len(f)


def volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def area(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float(np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum() / 2.0)


def positions(lo, hi, res):
    """the lattice's coordinates per axis, float32, as query_grid makes them: (x (res_x), y (res_y), z (res_z))"""
    lo32, step = lattice(lo, hi, res)
    return [((np.arange(res[a]).astype(np.float32) + np.float32(0.5)) * step[a] + lo32[a]).astype(np.float32) for a in range(3)]


def interior_edges_paired(verts, faces, lo, hi, res):
    """on any lattice: every mesh edge that does not lie in one of the lattice's six boundary planes is in exactly two
    triangles, in opposite directions.  Returns (holds, number of such edges)."""
    x, y, z = positions(lo, hi, res)
    v = np.asarray(verts)
    key, cnt, rcnt = edge_pairing(faces, len(v))
    n = max(len(v), 1)
    a, b = key // n, key % n
    on = np.zeros(len(key), dtype=bool)
    for k, c in enumerate((x, y, z)):
        for plane in (c[0], c[-1]):
            on |= (v[a, k] == plane) & (v[b, k] == plane)
    inner = ~on
    return bool((cnt[inner] == 1).all() and (rcnt[inner] == 1).all()), int(inner.sum())
