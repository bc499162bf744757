"""CPU tests of tests/_scale.py, the inputs and chunked references of test_gpu_geometry_scale.py: the chunked and vectorised
forms equal the restatements they stand for on small inputs, the generators are deterministic, the size rule gives three trips
and three scan steps at every compute-unit count, and the inputs have teeth -- a scan that loses its carry between two steps
of k_scan_top and a label map whose second trip was never written both fail the comparisons the GPU module makes."""
import numpy as np
import pytest

import _cc_ref as cr
import _meshcast_ref as mc
import _nn_ref as nr
import _scale as sc

CUS = 256
SENTINEL_BITS = np.float32(-7.5e33).view(np.int32)          # what an unwritten int32 of a guarded arena holds (_arena.SENTINEL)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------------------ the sizes
@pytest.mark.parametrize("cus", range(32, 305, 8))
def test_three_trips_and_three_scan_steps_at_every_cu_count(cus):
    """the rule restated from pnr_common.h and pnr_scan_dev.h: a launch of min(ceil(n / 256), 8 cus) workgroups covers
    8 cus 256 items a trip, k_scan_top 256 tiles of 1024 items a step"""
    assert sc.trips(8 * cus * 256, cus) == 1 and sc.trips(8 * cus * 256 + 1, cus) == 2 and sc.trips(sc.stride3(cus), cus) == 3
    assert sc.trips(sc.cm3(cus), cus, sc.CM_PER_CU, sc.CM_MAX_BLOCKS) == 3
    assert sc.scan_steps(262144) == 1 and sc.scan_steps(262145) == 2 and sc.scan_steps(sc.SCAN3) == 3 and sc.scan_steps(64 ** 3) == 1
    assert sc.check_sizes(cus)
    h, w = sc.image_shape(cus)
    rz, ry, rx = sc.lattice_shape(cus)
    assert h % 2 and w % 2 and h % 8 and w % 32 and rz % 4 and ry % 8 and rx % 8
    assert h * w >= sc.items(cus) and rz * ry * rx >= sc.items(cus)
    V, F = sc.ribbon_counts(sc.mesh_faces_min(cus))
    assert F >= sc.items(cus) and V >= sc.SCAN3 and F - (sc.trips(F, cus) - 1) * sc.per_trip(cus) >= 100
    m, n = sc.query_sizes(cus)
    assert m * n <= sc.BRUTE_BUDGET and n >= 24 and sc.items(cus) * min(48, sc.BRUTE_BUDGET // sc.items(cus)) <= sc.BRUTE_BUDGET


def test_sizes_on_a_full_device():
    assert sc.stride3(256) == 1048653 and sc.cm3(256) == 524365 and sc.SCAN3 == 524365
    assert sc.image_shape(256) == (1029, 1021) and sc.lattice_shape(256) == (65, 129, 127)
    assert sc.trips(sc.FRAME[0] * sc.FRAME[1], 256) == 2 and sc.FRAME[0] * sc.FRAME[1] - sc.per_trip(256) == 5120
    assert sc.CLAMP_FACES * nr.MAX_PER_FACE == 2149548000 > 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ chunked = unchunked
@pytest.mark.parametrize("offset,D", nr.OFFSETS_D)
def test_chunked_brute_is_brute(offset, D):
    ref, q = nr.adversarial(257, 130, offset, D)
    want = nr.brute(q, ref, D)
    for chunk in (1, 7, 64, 130, 1000, None):
        got = sc.brute_chunked(q, ref, D, chunk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and got[2] == want[2], chunk
    assert sc.brute_chunked(q[:0], ref, D)[2] == [0, 0, 0]


def test_chunked_cast_is_cast():
    V, F = mc.soup()
    rays = np.concatenate([mc.rays_to((0.2, -0.1, -2.5), mc.edge_targets(V, F[9:60])[::3]),mc.rays_to((3.0, 0.1, 0.2), V[:40]), np.zeros((2, 8), np.float32)])
    want = mc.cast(rays, V, F)
    assert (want["code"] == mc.HIT).sum() > 100 and (want["code"] == mc.MISSED).any() and (want["code"] == mc.NO_RAY).sum() >= 2
    for chunk in (7, 64, 499, 500, 4096):
        got = sc.cast_chunked(rays, V, F, chunk)
        for k in mc.KEYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(bits(got[k]), bits(want[k])), (chunk, k)
    assert len({int(f) // 64 for f in want["face"] if f >= 0}) > 4          # the winners come from many chunks


@pytest.mark.parametrize("res", [(1, 1, 1), (2, 3, 5), (16, 16, 16), (40, 7, 1)])
def test_vectorised_binning_is_bin_faces(res):
    from panopticnerf_amd import mesh
    V, F = mc.soup()
    use = mc.usable_faces(V, F)
    P = V[F[use]].reshape(-1, 3)
    lo, cell, _ = mesh.grid_box(np.concatenate([P.min(0), P.max(0)]), int(use.sum()), res)
    grid = mc.make_grid(res, lo, cell)
    got, want = sc.bin_counts(V, F, grid), sc.bin_counts_scalar(V, F, grid)
    assert np.array_equal(got, want) and got.sum() >= use.sum() and got.shape == (res[0] * res[1] * res[2],)
    # a grid that does not cover the mesh: the clamp of mc_cell on both sides
    tight = mc.make_grid(res, lo + cell * np.float32(0.4) * np.asarray(res, np.float32), cell * np.float32(0.3))
    assert np.array_equal(sc.bin_counts(V, F, tight), sc.bin_counts_scalar(V, F, tight))


def test_vectorised_stats_are_cr_stats():
    for shape in ((17, 65), (9, 17, 17)):
        for name in ("percolation", "multikey", "checkerboard", "background", "comb"):
            lab, count, _ = cr.label(cr.key_patterns(shape, (32, 8) if len(shape) == 2 else (8, 8, 4), seed=3)[name])
            got, want = sc.stats(lab, count), cr.stats(lab, count)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].dtype == want[1].dtype, (shape, name)


def test_values_of_keys_link_as_the_keys_do():
    """the values-mode case of the GPU module takes cr.label of the KEYS as its reference: on these values the two modes are
    the same partition, foreground and numbering, by cr.label itself"""
    for shape in ((17, 65), (5, 9, 11)):
        keys = cr.multikey(shape, 7)
        values, tol = sc.values_of(keys)
        assert values.dtype == np.float32 and tol < 0.5 and np.isnan(values).any() and np.isinf(values).any() and (values == 0).any()
        assert np.array_equal(cr.foreground(values, cr.VALUES), keys >= 0)
        for full in (False, True):
            a, b = cr.label(values, cr.VALUES, tol, full), cr.label(keys, cr.KEYS, 0.0, full)
            assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        assert cr.label(values, cr.VALUES, np.float32(0.5), False)[1] < cr.label(keys)[1]          # tol itself matters


# --------------------------------------------------------------------------------------------------------- generators
def test_generators_are_deterministic_and_as_described():
    for make in (lambda: sc.ribbon_mesh(5000, 63), lambda: sc.big_reference(32), lambda: sc.big_queries(32), lambda: sc.metrics_case(5000),
                 lambda: sc.small_triangles(4000), lambda: sc.large_triangles(70000, 4), lambda: sc.clamped_triangles(50)):
        a, b = make(), make()
        for x, y in zip(a, b):
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y))
            elif isinstance(x, dict):
                assert sorted(x) == sorted(y) and all(np.array_equal(x[k], y[k]) for k in x)
            else:
                assert x == y
    V, F, info = sc.ribbon_mesh(5000, 63)
    assert V.dtype == np.float32 and F.dtype == np.int32 and (len(V), len(F)) == sc.ribbon_counts(5000, 63)
    vlab, flab, fsize, n = cr.label_mesh(F, len(V))
    assert n == info["pieces"] == 7 and len(set(np.bincount(flab[flab >= 0]))) == 7                # seven pieces, all of another size
    use = mc.usable_faces(V, F)
    assert sorted(np.nonzero(~use)[0]) == sorted(info["unusable"]) and min(info["unusable"]) > len(F) - 100
    assert (flab[list(info["unusable"][:2])] == -1).all() and flab[info["unusable"][2]] >= 0       # the NaN corner is cc_mesh's face
    first = np.array([np.nonzero(flab == c)[0].min() for c in range(n)])
    assert (first < len(F) // 2).sum() >= 4 and not np.array_equal(np.sort(F[:, 0]), F[:, 0])       # pieces and faces interleave
    v, f, rho = sc.small_triangles(4000)
    k = nr.sample_counts(v, f, rho, 5)[0]
    assert 0.2 < k.mean() < 0.4 and k[-3] == 0 and k[-11] == 0
    v, f, rho = sc.large_triangles(70000, 4)
    k = nr.sample_counts(v, f, rho, 6)[0]
    assert k.sum() >= 70000 and k.max() < nr.MAX_PER_FACE and len(set(k)) == 4
    v, f, rho = sc.clamped_triangles(50)
    assert (nr.sample_counts(v, f, rho, 7)[0] == nr.MAX_PER_FACE).all()


def test_aimed_rays_win_in_every_trip():
    cus = 2                                              # a toy device: 4096 faces a trip
    V, F, info = sc.ribbon_mesh(3 * sc.per_trip(cus) + 77, 63)
    rays = sc.aimed_rays(V, F, cus)
    want = mc.cast(rays, V, F)
    face = want["face"][want["code"] == mc.HIT]
    trip = face // sc.per_trip(cus)
    assert rays.shape == (16, 8) and len(face) >= 12 and {0, 1, int(sc.trips(len(F), cus) - 1)} <= set(trip.tolist())
    assert (want["code"] == mc.MISSED).sum() == 1 and (want["code"] == mc.NO_RAY).sum() >= 1
    assert not set(face.tolist()) & set(info["unusable"])


# ------------------------------------------------------------------------------------------------------ planted faults
def scan_inputs():
    """name -> the counts of every scan the GPU module checks entry by entry, at the sizes of a full device"""
    ref, _ = sc.big_reference(CUS)
    b, _ = nr.table(ref, sc.D, 1 << 20)
    v, f, rho = sc.small_triangles(sc.items(CUS))
    V, F = mc.soup()
    from panopticnerf_amd import mesh
    use = mc.usable_faces(V, F)
    P = V[F[use]].reshape(-1, 3)
    lo, cell, _ = mesh.grid_box(np.concatenate([P.min(0), P.max(0)]), int(use.sum()), (81, 81, 81))
    checker = cr.checkerboard(sc.image_shape(CUS)).reshape(-1)
    return {"nn table": np.bincount(b[b >= 0], minlength=1 << 20), "sample counts": nr.sample_counts(v, f, rho, 5)[0],
            "cell table": sc.bin_counts(V, F, mc.make_grid((81, 81, 81), lo, cell)),
            "root flags of the checkerboard": (checker >= 0).astype(np.int64)}


def test_planted_fault_dropped_scan_carry_is_caught():
    """pnr_scan_i32 restated launch by launch equals the plain exclusive sums; restated with k_scan_top's carry dropped between
    two steps it fails check_start, the comparison the GPU module makes, on every scanned input: each has counts in every step"""
    for name, counts in scan_inputs().items():
        assert sc.scan_steps(len(counts)) >= 3 and all(s > 0 for s in sc.counts_per_step(counts)), name
        good, total = sc.scan_restated(counts)
        assert total == int(counts.sum()) and sc.check_start(good, counts, name)
        lost, total = sc.scan_restated(counts, drop_carry=True)
        assert total == int(counts.sum())
        with pytest.raises(AssertionError, match=r"scan entries differ, the first at %d \(step 1 of k_scan_top\)" % (sc.SCAN_TILE * sc.SCAN_BLOCK)):
            sc.check_start(lost, counts, name)
        assert np.array_equal(lost[:sc.SCAN_TILE * sc.SCAN_BLOCK], good[:sc.SCAN_TILE * sc.SCAN_BLOCK])      # one step: nothing to lose
    # the 64-bit total past the int32 range, the last entry wrapped
    k = np.full(sc.CLAMP_FACES, nr.MAX_PER_FACE)
    start, total = sc.scan_restated(k)
    assert total == 2149548000 and int(start[-1]) == total - 2 ** 32


def test_planted_fault_unwritten_second_trip_is_caught():
    """a label map whose second trip's elements were never written -- left as the arena's sentinel, or as background -- fails
    check_labels, the comparison the GPU module makes, for every pattern it runs: each has foreground in every trip"""
    step = sc.per_trip(CUS)
    shape = sc.image_shape(CUS)
    cases = {"frame": (cr.bernoulli(sc.FRAME, cr.PERCOLATION[2], 11), sc.FRAME)}
    for name in ("percolation", "serpentine", "spiral", "comb", "multikey", "checkerboard"):
        keys = cr.checkerboard(shape) if name == "checkerboard" else cr.comb(shape) if name == "comb" else cr.serpentine(shape) if name == "serpentine" \
            else cr.spiral(shape) if name == "spiral" else cr.multikey(shape, 5) if name == "multikey" else cr.bernoulli(shape, cr.PERCOLATION[2], 4)
        cases[name] = (keys, shape)
    cases["lattice"] = (cr.bernoulli(sc.lattice_shape(CUS), cr.PERCOLATION[3], 6), sc.lattice_shape(CUS))
    for name, (keys, shp) in cases.items():
        per = sc.foreground_per_trip(keys, CUS)
        assert len(per) == sc.trips(keys.size, CUS) >= 2 and all(p > 0 for p in per), (name, per)
    # the comparison itself, on the labellings whose reference is cheap or a closed form
    checker = cr.checkerboard(shape)
    one = lambda keys: (np.where(keys >= 0, 0, -1).astype(np.int32), 1, np.where(keys >= 0, int((keys >= 0).sum()), 0).astype(np.int32))
    wants = {"frame": cr.label(cases["frame"][0]), "serpentine": one(cases["serpentine"][0]), "comb": one(cases["comb"][0]),
             "checkerboard": (np.where(checker >= 0, np.cumsum(checker.reshape(-1) >= 0).reshape(shape) - 1, -1).astype(np.int32),
                              int((checker >= 0).sum()), (checker >= 0).astype(np.int32))}
    for name, want in wants.items():
        assert sc.check_labels((want[0], want[1], want[2]), want, name)
        for stale in (SENTINEL_BITS, -1):
            lab = want[0].copy().reshape(-1)
            lab[step:2 * step] = stale
            with pytest.raises(AssertionError, match="labels differ, the first at flat index"):
                sc.check_labels((lab.reshape(want[0].shape), want[1], want[2]), want, name)
            size = want[2].copy().reshape(-1)
            size[step:2 * step] = 0 if stale == -1 else stale
            with pytest.raises(AssertionError, match="sizes differ, the first at flat index"):
                sc.check_labels((want[0], want[1], size.reshape(want[0].shape)), want, name)
