"""The mesh-extraction rule (include/pnr.h "mesh extraction") on the CPU: its two restatements in tests/_mesh_ref.py agree bit
for bit, the closed forms hold on both, and each of five corrupted variants of the rule is noticed by them."""
import os
import re

import numpy as np
import pytest

import _mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def sdf(kind, res, **kw):
    x, y, z = R.positions(UNIT[0], UNIT[1], (res,) * 3)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    if kind == "sphere":
        return (np.float32(kw["r"]) - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    q = np.sqrt(X * X + Y * Y) - np.float32(kw["R"])
    return (np.float32(kw["a"]) - np.sqrt(q * q + Z * Z)).astype(np.float32)


# ---------------------------------------------------------------- the tables
def test_winding_table_is_the_geometric_one_and_the_headers():
    assert R.derive_flip() == R.FLIP
    assert all(R.FLIP[c][0] != R.FLIP[c][1] for c in range(1, 15))          # an odd tetrahedron is the mirror image of an even one
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    rows = {name: [int(v) for v in re.search(r"\*\s+%s((?:\s+[01]){16})\s*\n" % name, hdr).group(1).split()] for name in ("even", "odd")}
    assert rows["even"] == [r[0] for r in R.FLIP] and rows["odd"] == [r[1] for r in R.FLIP]
    src = open(os.path.join(ROOT, "panopticnerf_amd", "csrc", "pnr_mesh.hip")).read()
    body = re.search(r"MESH_FLIP\[16\]\[2\] = \{(.*?)\};", src, re.S).group(1)
    assert [int(v) for v in re.findall(r"[01]", body)] == [v for r in R.FLIP for v in r]


def test_the_six_tetrahedra_tile_the_cube_and_share_the_diagonal():
    vol = 0.0
    for tet in range(6):
        w = np.array([[(c >> a) & 1 for a in range(3)] for c in R.tet_codes(tet)], dtype=np.float64)
        vol += abs(np.linalg.det(w[1:] - w[0])) / 6.0
        assert R.tet_codes(tet)[0] == 0 and R.tet_codes(tet)[3] == 7
        sign = np.sign(np.linalg.det(w[1:] - w[0]))
        assert sign == (1 if R.PARITY[tet] == 0 else -1)
    assert abs(vol - 1.0) < 1e-12
    assert len({R.tet_codes(t) for t in range(6)}) == 6
    for case in range(16):
        assert len(R.case_triangles(case)) == (0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0)[case]


# ---------------------------------------------------------------- loops == vectorised
@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 3, 2), (3, 3, 3), (1, 5, 5), (5, 1, 4), (4, 6, 5), (6, 5, 7)])
def test_the_two_restatements_agree_bit_for_bit(shape):
    rng = np.random.default_rng(sum(shape) * 31 + shape[0])
    for level, (lo, hi) in ((0.0, UNIT), (0.7, ((-3.0, 0.5, 10.0), (2.0, 0.75, 47.0))), (-0.3, ((1e-3, 1e3, -7.0), (2e-3, 1e3 + 1, 9.0)))):
        f = rng.standard_normal(shape).astype(np.float32)
        a, b = R.extract_loops(f, lo, hi, level), R.extract(f, lo, hi, level)
        assert same(a, b), (shape, level)
        mask, ntri = R.classify(f, level)
        assert int(R._POP[mask].sum()) == len(a[0]) and int(ntri.sum()) == len(a[1])
        if min(shape) < 2:
            assert len(a[0]) == 0 and len(a[1]) == 0


def test_noise_exercises_every_case_of_every_tetrahedron():
    """what the GPU parity test relies on: Gaussian noise at both of its levels meets all 16 cases of all six tetrahedra"""
    f = np.random.default_rng(0).standard_normal((31, 33, 65)).astype(np.float32)
    for level in (0.0, 0.7):
        ins = f > np.float32(level)
        rz, ry, rx = f.shape
        corner = [ins[(c >> 2 & 1):rz - 1 + (c >> 2 & 1), (c >> 1 & 1):ry - 1 + (c >> 1 & 1), (c & 1):rx - 1 + (c & 1)].astype(int) for c in range(8)]
        for tet in range(6):
            c = R.tet_codes(tet)
            case = corner[c[0]] | corner[c[1]] << 1 | corner[c[2]] << 2 | corner[c[3]] << 3
            assert len(np.unique(case)) == 16, (level, tet)


def test_edge_inputs_agree_too():
    rng = np.random.default_rng(5)
    f = rng.standard_normal((4, 5, 6)).astype(np.float32)
    flat = f.reshape(-1)
    flat[rng.choice(flat.size, 30, replace=False)] = np.tile(np.array([np.nan, np.inf, -np.inf, 0.25, 0.25], np.float32), 6)
    for level in (0.25, 0.0):
        assert same(R.extract_loops(f, *UNIT, level), R.extract(f, *UNIT, level))
    for const in (1.0, -1.0, np.nan, np.inf, -np.inf, 0.25):
        g = np.full((3, 4, 5), const, np.float32)
        for fn in (R.extract_loops, R.extract):
            v, t, s = fn(g, *UNIT, 0.25)
            assert v.shape == (0, 3) and t.shape == (0, 3) and s.shape == (0,)
            assert v.dtype == np.float32 and t.dtype == np.int32 and s.dtype == np.int64


# ---------------------------------------------------------------- closed forms, on any implementation of the rule
def one_point():
    f = np.zeros((3, 3, 3), np.float32)
    f[1, 1, 1] = 1.0
    return f, ((-0.5,) * 3, (2.5,) * 3)            # unit step, point i at coordinate i


def closed_form_failures(fn, sphere_res=(8,)):
    """names of the closed-form checks that `fn(field, lo, hi, level)` fails"""
    bad = []

    def check(name, ok):
        if not ok:
            bad.append(name)

    # one inside point, peak 1, level 0.5: an octahedron-like cell of 14 vertices and 24 triangles, volume 0.5
    f, box = one_point()
    v, t, s = fn(f, *box, 0.5)
    check("one point: counts", (len(v), len(t)) == (14, 24))
    check("one point: closed and oriented", R.is_closed_oriented(t, len(v)))
    check("one point: euler", len(t) and R.euler(t) == 2)
    check("one point: volume", len(t) and abs(R.volume(v, t) - 0.5) < 1e-6)
    check("one point: src", len(s) == 14 and set(s.tolist()) == {13})
    # values equal to level are outside: the same cell when the background sits AT the level
    g = np.full((3, 3, 3), 0.5, np.float32)
    g[1, 1, 1] = 1.0
    v, t, s = fn(g, *box, 0.5)
    check("equal to level is outside", (len(v), len(t)) == (14, 24))
    # non-finite ends, always from the owner: (owner value, far value) -> t
    lo, hi = (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)       # points at 0.5 and 1.5
    for fa, fb, t_want in ((-np.inf, 1.0, 0.5), (0.0, np.inf, 0.0), (np.inf, 0.0, 0.5), (1.0, -np.inf, 0.0), (np.nan, 1.0, 0.5),
                           (1.0, np.nan, 0.5), (0.5, 1.0, 0.0), (1.0, 0.5, 1.0), (0.25, 1.0, 1.0 / 3.0)):
        g = np.full((2, 2, 2), fa, np.float32)
        g[:, :, 1] = fb                              # every x edge crosses; so do the diagonals with an x component
        v, t, s = fn(g, lo, hi, 0.5)
        x_want = np.float32(0.5) + np.float32(t_want) * np.float32(1.0)
        check("non-finite ends (%r, %r)" % (fa, fb), len(v) == 9 and np.array_equal(v[:, 0], np.full(9, x_want, np.float32))
              and bool((g.reshape(-1)[s] > 0.5).all()))
    # the sphere: closed, oriented, genus 0, positive volume; the label source is inside
    for res in sphere_res:
        f = sdf("sphere", res, r=0.7)
        v, t, s = fn(f, *UNIT, 0.0)
        check("sphere %d: closed and oriented" % res, R.is_closed_oriented(t, len(v)))
        check("sphere %d: euler" % res, len(t) and R.euler(t) == 2)
        check("sphere %d: volume sign" % res, len(t) and R.volume(v, t) > 0)
        check("sphere %d: src inside" % res, len(s) and bool((f.reshape(-1)[s] > 0).all()))
    # noise: watertight away from the lattice's boundary
    f = np.random.default_rng(3).standard_normal((5, 6, 7)).astype(np.float32)
    v, t, s = fn(f, *UNIT, 0.1)
    ok, n = R.interior_edges_paired(v, t, *UNIT, (7, 6, 5))
    check("noise: interior edges paired", ok and n > 100)
    check("noise: src inside", bool((f.reshape(-1)[s] > np.float32(0.1)).all()))
    return bad


def test_closed_forms_hold_on_both_restatements():
    assert closed_form_failures(R.extract_loops) == []
    assert closed_form_failures(R.extract, sphere_res=(8, 16)) == []


@pytest.mark.parametrize("corrupt", R.CORRUPTIONS)
def test_each_corrupted_variant_is_noticed(corrupt):
    assert len(R.CORRUPTIONS) >= 5
    bad = closed_form_failures(lambda f, lo, hi, level: R.extract_loops(f, lo, hi, level, corrupt=corrupt))
    assert bad, corrupt
    expect = {"ge": "equal to level is outside", "from_inside": "non-finite ends (-inf, 1.0)", "diagonal": "sphere 8: closed and oriented",
              "winding": "noise: interior edges paired", "src_outside": "one point: src"}[corrupt]
    assert expect in bad, (corrupt, bad)


def test_sphere_converges_at_second_order():
    """r = 0.7 in [-1, 1]^3 at res 8 / 16 / 32: closed, consistently oriented, genus 0, signed volume positive; the relative volume
    error (a float64 prototype of the rule measured -6.27 % / -1.59 % / -0.40 %) shrinks by a factor between 3 and 5 per
    doubling; no vertex is farther than h^2 from the sphere (the prototype measured 0.33 / 0.46 / 0.52 h^2)."""
    exact = 4.0 / 3.0 * np.pi * 0.7 ** 3
    errs = []
    for res in (8, 16, 32):
        f = sdf("sphere", res, r=0.7)
        v, t, s = R.extract(f, *UNIT, 0.0)
        assert R.is_closed_oriented(t, len(v)) and R.euler(t) == 2
        vol = R.volume(v, t)
        assert vol > 0
        errs.append((vol - exact) / exact)
        h = 2.0 / res
        far = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.7).max()
        print("sphere res %d: volume error %.4f %%, largest distance %.3f h^2" % (res, 100 * errs[-1], far / h ** 2))
        assert far <= h * h
    assert all(e < 0 for e in errs)
    assert 3.0 < errs[0] / errs[1] < 5.0 and 3.0 < errs[1] / errs[2] < 5.0


def test_torus_has_genus_one():
    f = sdf("torus", 16, R=0.6, a=0.25)
    v, t, s = R.extract(f, *UNIT, 0.0)
    assert len(t) > 0 and R.is_closed_oriented(t, len(v)) and R.euler(t) == 0 and R.volume(v, t) > 0
    assert (f.reshape(-1)[s] > 0).all()


@pytest.mark.parametrize("c", [0.1, -0.37, 0.125])
def test_plane(c):
    """field x - c: every vertex has x == c to one rounding -- |x - float32(c)| is at most one float32 spacing at c -- and
    the area is the cross-section's"""
    res = (8, 5, 6)
    x, y, z = R.positions(*UNIT, res)
    f = np.broadcast_to((x - np.float32(c))[None, None, :], (6, 5, 8)).astype(np.float32)
    v, t, s = R.extract(f, *UNIT, 0.0)
    dev = np.abs(v[:, 0].astype(np.float64) - float(np.float32(c))).max()
    print("plane c = %r: largest |x - c| = %.3e, one spacing = %.3e" % (c, dev, float(np.spacing(np.float32(abs(c))))))
    assert len(v) > 0 and dev <= float(np.spacing(np.float32(abs(c))))
    want = float(y[-1] - y[0]) * float(z[-1] - z[0])
    assert abs(R.area(v, t) - want) <= 1e-6 * want
    assert (f.reshape(-1)[s] > 0).all()
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]).astype(np.float64)
    assert (n[:, 0] <= 0).all() and (n[:, 0] < 0).any()           # inside is x > c: the normals point to -x


def test_noise_is_watertight_away_from_the_boundary():
    rng = np.random.default_rng(11)
    for shape, level in (((9, 8, 7), 0.0), ((6, 12, 5), 0.7)):
        f = rng.standard_normal(shape).astype(np.float32)
        v, t, s = R.extract(f, *UNIT, level)
        ok, n = R.interior_edges_paired(v, t, *UNIT, shape[::-1])
        assert ok and n > 500
        assert (f.reshape(-1)[s] > np.float32(level)).all()
        assert t.min() >= 0 and t.max() == len(v) - 1 and len(np.unique(t)) == len(v)          # every vertex is used


def test_a_lattice_without_cubes_is_empty():
    rng = np.random.default_rng(2)
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1)):
        f = rng.standard_normal(shape).astype(np.float32)
        for fn in (R.extract_loops, R.extract):
            v, t, s = fn(f, *UNIT, 0.0)
            assert len(v) == 0 and len(t) == 0 and len(s) == 0
        mask, ntri = R.classify(f, 0.0)
        assert not mask.any() and not ntri.any()
