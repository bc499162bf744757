"""The newest geometry ops on an MI355X at frame scale: nearest neighbours and cloud metrics, mesh sampling, mesh ray casting
and connected components at the sizes where their kernels change behaviour -- three trips of every grid-stride loop sized by
pnr_grid_cap (CC_GRID_STRIDE, CC_BLOCK_STRIDE and k_cc_tile's tile loop, k_nn_count / _fill / _query, k_mesh_sample_count /
_emit, k_meshcast_bounds / _count / _fill, the k_cc_mesh_* kernels, k_cc_stats_init / k_cc_stats, k_cloud_metrics), three and
more steps of k_scan_top's carried loop at all five call sites of pnr_scan_i32 (with out[n] written by the last thread of the
last tile), and a scan total above 2^31 - 1.  The sizes follow the device's compute-unit count (tests/_scale.py; a device with
fewer units just takes more trips) and are printed once.

Every comparison is exact equality with the existing CPU restatements (_cc_ref, _nn_ref, _meshcast_ref, _reduce_ref), called
in chunks or vectorised as tests/_scale.py states and tests/test_scale_ref.py pins; the one bound is test_gpu_geometry_eval's
for the metric sums against math.fsum, unchanged.  Outputs and workspaces of the component and table builds are interior
views of a guarded arena, and a second call on the same buffers gives the same bits.  References are computed once per
process and shared.  The slowest case, reference included, on an MI355X host with 256 compute units:
test_image_labels_at_three_trips[multikey-8], 1.9 s (cr.label of a million pixels at 8-connectivity); the module, 19 s.  On a
slower CPU the longest is test_cast_at_three_trips_of_faces: brute force of 16 rays over a million faces, about 5 s."""
import functools

import numpy as np
import pytest
import torch

import _cc_ref as cr
import _meshcast_ref as mc
import _nn_ref as nr
import _reduce_ref as rr
import _scale as sc
import test_gpu_meshcast as tm
from _arena import Arena
from panopticnerf_amd import mesh, ops
from test_gpu_geometry_eval import close
from test_gpu_nn import check_table, run_in_arena

pytestmark = pytest.mark.gpu

GUARD = 64
N_ = lambda t: t.detach().cpu().numpy()


def G(a, dev):
    """a device copy of a (read-only) numpy array"""
    return torch.from_numpy(np.array(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def even(n):
    return max(n + n % 2, 2)


def CU(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def report(what, n, cus, scan=None, per_cu=sc.PER_CU, max_blocks=None, unit=sc.BLOCK):
    """print, and require, three trips of a launch over n items (and three scan steps of a scan over `scan` items)"""
    t = sc.trips(n, cus, per_cu, max_blocks, unit)
    s = None if scan is None else sc.scan_steps(scan)
    print("%s: %d items, %d trips%s" % (what, n, t, "" if s is None else "; a scan of %d entries, %d steps of k_scan_top" % (scan, s)))
    assert t >= 3 and (s is None or s >= 3), (what, n, t, s)


def test_sizes_give_three_trips_and_three_scan_steps_on_this_device(dev):
    cus = CU(dev)
    assert tuple(ops.CC_TILE_2D) == (32, 8) and tuple(ops.CC_TILE_3D) == (8, 8, 4)        # what _scale.sizes restates
    print("%d compute units: STRIDE3 %d, CM3 %d, SCAN3 %d" % (cus, sc.stride3(cus), sc.cm3(cus), sc.SCAN3))
    for name, (n, t, s) in sc.sizes(cus).items():
        print("  %-20s %9d items  trips %-4s scan steps %s" % (name, n, "-" if t is None else t, "-" if s is None else s))
    assert sc.check_sizes(cus)


# ---------------------------------------------------------------------------------------------------------- components
@functools.lru_cache(maxsize=None)
def keys_of(name, shape):
    rank = len(shape)
    k = {"percolation": lambda: cr.bernoulli(shape, cr.PERCOLATION[rank], 4 + rank), "multikey": lambda: cr.multikey(shape, 5),
         "serpentine": lambda: cr.serpentine(shape), "spiral": lambda: cr.spiral(shape), "comb": lambda: cr.comb(shape),
         "checkerboard": lambda: cr.checkerboard(shape)}[name]()
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def labelled(name, shape, full):
    """cr.label of a pattern: (labels, count, size), computed once, never written"""
    out = cr.label(keys_of(name, shape), cr.KEYS, 0.0, full)
    out[0].setflags(write=False)
    out[2].setflags(write=False)
    return out


def label_twice(dev, data, full, tol=None):
    """ops.cc_label with every output and the workspace inside a guarded arena, called twice on the same buffers: the second
    call's (labels, count, size) as numpy, equal to the first's"""
    data = np.ascontiguousarray(data)
    n = data.size
    words = ops.cc_workspace_bytes(n) // 8
    arena = Arena(dev, [("count", 2, GUARD), ("labels", even(n), GUARD), ("size", even(n), GUARD), ("ws", 2 * words, GUARD)])
    i32 = lambda name: arena.view(name).view(torch.int32)[:n].reshape(data.shape)
    labels, size, count = i32("labels"), i32("size"), arena.view("count").view(torch.int64)
    d = G(data, dev)
    runs = []
    for _ in range(2):
        ops.cc_label(d, full, tol, labels=labels, size=size, count=count, workspace=arena.view("ws").view(torch.int64))
        torch.cuda.synchronize()
        assert arena.guards_intact()
        runs.append((N_(labels).copy(), int(count.item()), N_(size).copy()))
    assert runs[0][1] == runs[1][1] and np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2]), "the second call differs"
    return runs[1]


def report_lattice(what, shape, cus):
    n = int(np.prod(shape))
    report(what + " elements", n, cus, scan=n)
    tile = tuple(ops.CC_TILE_2D) if len(shape) == 2 else tuple(ops.CC_TILE_3D)
    report(what + " tiles of k_cc_tile", sc.tiles_of(shape, tile), cus, unit=1)


IMAGE_CASES = [("percolation", False), ("percolation", True), ("multikey", False), ("multikey", True), ("serpentine", False), ("spiral", False),
               ("comb", True)]


@pytest.mark.parametrize("name,full", IMAGE_CASES, ids=["%s-%d" % (n, 8 if f else 4) for n, f in IMAGE_CASES])
def test_image_labels_at_three_trips(dev, name, full):
    cus = CU(dev)
    shape = sc.image_shape(cus)
    report_lattice("image %d x %d" % shape, shape, cus)
    keys = keys_of(name, shape)
    assert all(p > 0 for p in sc.foreground_per_trip(keys, cus))
    assert sc.check_labels(label_twice(dev, keys, full), labelled(name, shape, full), "%s full=%d" % (name, full))


def test_image_values_mode_at_three_trips(dev):
    """the multikey image as values: 1 + key / 2 on the foreground, NaN / +-inf / +-0 / a negative on the background, tol just
    below the gap -- the partition cr.label gives the keys (test_scale_ref.py: cr.label of these values is cr.label of the keys)"""
    cus = CU(dev)
    shape = sc.image_shape(cus)
    values, tol = sc.values_of(keys_of("multikey", shape))
    for full in (False, True):
        assert sc.check_labels(label_twice(dev, values, full, tol=float(tol)), labelled("multikey", shape, full), "values full=%d" % full)


@pytest.mark.parametrize("full", [False, True], ids=["6", "26"])
def test_lattice_labels_at_three_trips(dev, full):
    cus = CU(dev)
    shape = sc.lattice_shape(cus)
    report_lattice("lattice %d x %d x %d" % shape, shape, cus)
    keys = keys_of("percolation", shape)
    assert all(p > 0 for p in sc.foreground_per_trip(keys, cus))
    assert sc.check_labels(label_twice(dev, keys, full), labelled("percolation", shape, full), "lattice full=%d" % full)


def test_a_perspective_frame(dev):
    """376 x 1408, the frame the product labels: on 256 compute units a second, ragged trip of 5120 elements"""
    cus = CU(dev)
    n = sc.FRAME[0] * sc.FRAME[1]
    print("frame %d x %d: %d elements, %d trips, the last of %d; %d scan steps" % (sc.FRAME + (n, sc.trips(n, cus), n - (sc.trips(n, cus) - 1) * sc.per_trip(cus),
                                                                                 sc.scan_steps(n))))
    assert sc.check_labels(label_twice(dev, keys_of("percolation", sc.FRAME), False), labelled("percolation", sc.FRAME, False), "frame")


@pytest.mark.parametrize("name", ["percolation", "checkerboard"])
def test_stats_at_three_trips(dev, name):
    """cc_stats over the image: k_cc_stats strides over the elements, and on the checkerboard -- every foreground pixel its own
    component, more than one trip's worth of them -- k_cc_stats_init strides over the components"""
    cus = CU(dev)
    shape = sc.image_shape(cus)
    want = labelled(name, shape, False)
    lab, count, size = label_twice(dev, keys_of(name, shape), False)
    assert sc.check_labels((lab, count, size), want, name)
    print("%s: %d components, %d trips of k_cc_stats_init" % (name, count, sc.trips(count, cus)))
    assert name != "checkerboard" or (count == sc.ceil_div(lab.size, 2) and sc.trips(count, cus) >= 2)
    arena = Arena(dev, [("sizes", even(count), GUARD), ("boxes", even(6 * count), GUARD)])
    sizes = arena.view("sizes").view(torch.int32)[:count]
    boxes = arena.view("boxes").view(torch.int32)[:6 * count].reshape(count, 6)
    want_sizes, want_boxes = sc.stats(want[0], want[1])
    for _ in range(2):
        ops.cc_stats(G(lab, dev), G(size, dev), count, sizes=sizes, boxes=boxes)
        torch.cuda.synchronize()
        assert arena.guards_intact()
        assert np.array_equal(N_(sizes), want_sizes) and np.array_equal(N_(boxes), want_boxes)


@functools.lru_cache(maxsize=None)
def big_mesh(cus):
    """(V, F, info) of the mesh that cc_mesh and the ray-casting build share, read-only"""
    V, F, info = sc.ribbon_mesh(sc.mesh_faces_min(cus))
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F, info


def test_mesh_components_at_three_trips(dev):
    cus = CU(dev)
    V, F, info = big_mesh(cus)
    nv, nf = len(V), len(F)
    report("cc_mesh faces", nf, cus)
    report("cc_mesh vertices", nv, cus, scan=nv)
    words = ops.cc_workspace_bytes(nv) // 8
    arena = Arena(dev, [("count", 2, GUARD), ("v", even(nv), GUARD), ("f", even(nf), GUARD), ("s", even(nf), GUARD), ("ws", 2 * words, GUARD)])
    i32 = lambda name, n: arena.view(name).view(torch.int32)[:n]
    count = arena.view("count").view(torch.int64)
    vlab, flab, fsize, n = cr.label_mesh(F, nv)
    assert n == info["pieces"] and len(set(np.bincount(flab[flab >= 0]).tolist())) == n
    Fd = G(F, dev)
    for _ in range(2):
        ops.cc_mesh(Fd, nv, i32("v", nv), i32("f", nf), i32("s", nf), count, arena.view("ws").view(torch.int64))
        torch.cuda.synchronize()
        assert arena.guards_intact()
        assert int(count.item()) == n
        assert np.array_equal(N_(i32("v", nv)), vlab) and np.array_equal(N_(i32("f", nf)), flab) and np.array_equal(N_(i32("s", nf)), fsize)


# ---------------------------------------------------------------------------------------- nearest neighbours and metrics
def test_a_big_reference_cloud(dev):
    """n points into 2^20 buckets: k_nn_count and k_nn_fill over three trips, the table scan over four steps.  start entry by
    entry including start[T], every bucket's multiset of records, and a few dozen queries against brute force over all n"""
    cus = CU(dev)
    ref, q = sc.big_reference(cus)
    n, m = len(ref), len(q)
    report("nn_build reference points", n, cus, scan=1 << 20)
    assert m * n <= sc.BRUTE_BUDGET and m >= 24
    b_ref, start_ref = nr.table(ref, sc.D, 1 << 20)
    assert all(s > 0 for s in sc.counts_per_step(np.diff(start_ref)))
    runs = [run_in_arena(dev, ref, q, sc.D, 20) for _ in range(2)]
    start, records, index, dist2, stats, T = runs[0]
    assert T == 1 << 20 and sc.check_start(start, np.diff(start_ref), "nn table")
    check_table(ref, sc.D, T, start, records)
    bi, bd, bstats = sc.brute_chunked(q, ref, sc.D, 8)
    assert np.array_equal(index, bi) and np.array_equal(dist2.view(np.uint32), bd.view(np.uint32)) and stats == bstats
    step = sc.per_trip(cus)
    assert {0, 1, int((n - 1) // step)} <= set((bi[bi >= 0] // step).tolist()) and (bi < 0).any()             # answers from every trip's range
    assert (bd[11:22] == np.float32(sc.D) * np.float32(sc.D)).any() and bi[22] == -1 and bstats[2] == 1
    assert np.array_equal(bi[[0, 1, 8, 9, 10]], [0, 7, 0, 7, 49])                # a twin at the end loses the tie to the lowest index
    assert np.array_equal(runs[1][0], start) and np.array_equal(runs[1][2], index) and np.array_equal(bits(runs[1][3]), bits(dist2)) and runs[1][4] == stats


def test_a_big_query_set(dev):
    """m queries against a few dozen points: k_nn_query over three trips; NaN and Inf rows and queries exactly max_dist away in
    the last trip's range"""
    cus = CU(dev)
    ref, q = sc.big_queries(cus)
    n, m = len(ref), len(q)
    report("nn_query queries", m, cus)
    assert m * n <= sc.BRUTE_BUDGET and n >= 24
    bi, bd, bstats = sc.brute_chunked(q, ref, sc.D)
    last = slice((sc.trips(m, cus) - 1) * sc.per_trip(cus), m)
    r2 = np.float32(sc.D) * np.float32(sc.D)
    assert bstats[2] == 3 and (~nr.finite_rows(q[last])).sum() == 3 and (bd[last] == r2).sum() >= 3 and 0.1 < bstats[0] / m < 0.9
    start, records, index, dist2, stats, T = run_in_arena(dev, ref, q, sc.D, None)
    bad = np.nonzero((index != bi) | (dist2.view(np.uint32) != bd.view(np.uint32)))[0]
    assert not len(bad), "%d answers differ, the first at query %d (trip %d)" % (len(bad), bad[0], bad[0] // sc.per_trip(cus))
    assert stats == bstats
    check_table(ref, sc.D, T, start, records)


def test_cloud_metrics_at_three_trips(dev):
    """counts exact; the sums within test_gpu_geometry_eval's bound of math.fsum (its REL, the tighter form of m 2^-53), equal to
    _reduce_ref's restatement of the order bit for bit, and the same bits from a second run"""
    cus = CU(dev)
    m = sc.cm3(cus)
    report("cloud_metrics rows", m, cus, per_cu=sc.CM_PER_CU, max_blocks=sc.CM_MAX_BLOCKS)
    max_dist, taus = 1.7, (0.05, 0.5, 1.7)
    index, dist2, q, root, active = sc.metrics_case(m)
    grid = rr.blocks_for(m, sc.CM_MAX_BLOCKS, cus, sc.CM_PER_CU)
    d = np.where(index >= 0, root.astype(np.float64), np.float64(np.float32(max_dist)))
    terms = np.where(active[:, None], np.stack([d, d * d], -1), 0.0)
    want = rr.total(terms, active, grid)
    assert (want != rr.total(terms[::-1], active[::-1], grid)).all(), "the data do not tell two orders apart"
    want_s, want_c = nr.cloud_metrics(index, dist2, max_dist, taus, query=q)
    assert want_c[0] == int(active.sum()) and 0 < want_c[2] < want_c[3] < want_c[4] <= want_c[0] - want_c[1]
    i_d, d_d, q_d = G(index, dev), G(dist2, dev), G(q, dev)
    sums, counts = ops.cloud_metrics(i_d, d_d, max_dist, taus, query=q_d)
    assert counts.tolist() == want_c + [0] * (ops.CLOUD_COUNTS - len(want_c))
    close(float(sums[0]), want_s[0], "sum d over %d rows" % m)
    close(float(sums[1]), want_s[1], "sum d^2 over %d rows" % m)
    assert np.array_equal(N_(sums).view(np.uint64), want.view(np.uint64)), (m, grid, N_(sums), want)
    sums2, counts2 = ops.cloud_metrics(i_d, d_d, max_dist, taus, query=q_d)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)) and torch.equal(counts, counts2)


# -------------------------------------------------------------------------------------------------------- mesh sampling
def pad4(n):
    return n + (-n) % 4


def test_sample_count_at_three_trips_and_scan_steps(dev):
    """F small triangles at a mean count well below 1: k_mesh_sample_count over three trips and the scan, in place (in == out),
    over three and more steps of k_scan_top: all F + 1 entries of start and the total"""
    cus = CU(dev)
    F = sc.items(cus)
    report("mesh_sample_count faces", F, cus, scan=F)
    v, f, rho = sc.small_triangles(F)
    k = nr.sample_counts(v, f, rho, 5)[0]
    assert k.mean() < 0.5 and all(s > 0 for s in sc.counts_per_step(k)) and k[F - 3] == 0 and k[F - 11] == 0
    arena = Arena(dev, [("total", 2, GUARD), ("start", pad4(F + 1), GUARD)])
    start, total = arena.view("start")[:F + 1].view(torch.int32), arena.view("total").view(torch.int64)
    vd, fd = G(v, dev), G(f, dev)
    for _ in range(2):
        t2, s2 = ops.mesh_sample_count(vd, fd, rho, 5, start=start, total=total)
        torch.cuda.synchronize()
        assert s2 is start and t2 is total and arena.guards_intact()
        assert int(total.item()) == int(k.sum()) and sc.check_start(N_(start), k, "mesh sample counts")


def test_sample_emit_at_three_trips(dev):
    """a few dozen large triangles, each below the clamp, at least STRIDE3 points: k_mesh_sample_emit over three trips"""
    cus = CU(dev)
    v, f, rho = sc.large_triangles(sc.stride3(cus))
    k = nr.sample_counts(v, f, rho, 6)[0]
    N = int(k.sum())
    report("mesh_sample_emit points", N, cus)
    assert k.max() < nr.MAX_PER_FACE and k.min() > 0 and 24 <= len(f) <= 64
    arena = Arena(dev, [("start", pad4(len(f) + 1), GUARD), ("points", pad4(3 * N), GUARD), ("face", pad4(N), GUARD)])
    start = arena.view("start")[:len(f) + 1].view(torch.int32)
    points, face = arena.view("points")[:3 * N].view(N, 3), arena.view("face")[:N].view(torch.int32)
    vd, fd = G(v, dev), G(f, dev)
    total, _ = ops.mesh_sample_count(vd, fd, rho, 6, start=start)
    assert int(total.item()) == N and sc.check_start(N_(start), k, "large triangles")
    rp, rf = nr.sample(v, f, rho, 6)
    for _ in range(2):
        ops.mesh_sample_emit(vd, fd, 6, start, points, face)
        torch.cuda.synchronize()
        assert arena.guards_intact()
        bad = np.nonzero(N_(face) != rf)[0]
        assert not len(bad), "%d faces differ, the first at point %d (trip %d)" % (len(bad), bad[0], bad[0] // sc.per_trip(cus))
        bad = np.nonzero((N_(points).view(np.uint32) != rp.view(np.uint32)).any(1))[0]
        assert not len(bad), "%d points differ, the first at point %d (trip %d)" % (len(bad), bad[0], bad[0] // sc.per_trip(cus))


def test_a_total_above_int32_is_counted_in_64_bits_and_refused(dev, monkeypatch):
    """32 800 faces at the clamp of 65 535 points: the device's own 64-bit total is 2 149 548 000, Mesh.sample refuses it by name
    and launches no emit.  (The int32 start has wrapped by then; include/pnr.h promises nothing about it.)"""
    v, f, rho = sc.clamped_triangles()
    want = sc.CLAMP_FACES * nr.MAX_PER_FACE
    assert want == 2149548000 > ops.NN_MAX_POINTS and int(nr.sample_counts(v, f, rho, 7)[0].sum()) == want
    vd, fd = G(v, dev), G(f, dev)
    total, start = ops.mesh_sample_count(vd, fd, rho, 7)
    assert total.dtype == torch.int64 and int(total.item()) == want
    emits = []
    emit = ops.mesh_sample_emit
    monkeypatch.setattr(ops, "mesh_sample_emit", lambda *a, **kw: (emits.append(a), emit(*a, **kw))[1])
    m = mesh.Mesh.from_arrays(vd, fd)
    with pytest.raises(ValueError, match=r"Mesh.sample: density 1.0 asks for 2149548000 points, more than 2\^31 - 1"):
        m.sample(density=rho, seed=7)
    assert not emits
    small = mesh.Mesh.from_arrays(vd[:30], fd[:10])                      # the spy itself: an ordinary call does reach the emit
    pts, _ = small.sample(density=1e-3, seed=7)
    assert len(emits) == 1 and pts.shape[0] > 0


# ---------------------------------------------------------------------------------------------------- mesh ray casting
@functools.lru_cache(maxsize=None)
def big_index(dev):
    """the ray-casting index of the big mesh, built once through the ops with start between guards: a dict of what each step gave"""
    cus = CU(dev)
    V, F, _ = big_mesh(cus)
    Vd, Fd = G(V, dev), G(F, dev)
    bounds = N_(ops.mesh_grid_bounds(Vd, Fd))
    usable = int(bounds.view(np.int32)[6])
    lo, cell, res = mesh.grid_box(bounds[:6], usable, None)
    cells = res[0] * res[1] * res[2]
    arena = Arena(dev, [("total", 2, GUARD), ("start", pad4(cells + 1), GUARD)])
    start, total = arena.view("start")[:cells + 1].view(torch.int32), arena.view("total").view(torch.int64)
    _, _, ws = ops.mesh_grid_count(Vd, Fd, res, lo, cell, start=start, total=total)
    n = int(total.item())
    records = torch.empty((n, 12), device=dev, dtype=torch.float32)
    ops.mesh_grid_fill(Vd, Fd, res, lo, cell, start, records, ws)
    torch.cuda.synchronize()
    return {"V": Vd, "F": Fd, "bounds": bounds, "usable": usable, "lo": lo, "cell": cell, "res": res, "start": start, "total": n, "records": records,
            "arena": arena}


def test_ray_index_build_at_three_trips(dev):
    """k_meshcast_bounds / _count / _fill over three trips of faces, with an out-of-range index and a NaN corner in the last
    trip's range: the bounds and the usable-face count, the entry total and every entry of start against a recount"""
    cus = CU(dev)
    V, F, info = big_mesh(cus)
    report("ray-casting build faces", len(F), cus)
    use = mc.usable_faces(V, F)
    assert sorted(np.nonzero(~use)[0].tolist()) == sorted(info["unusable"]) and min(info["unusable"]) >= (sc.trips(len(F), cus) - 1) * sc.per_trip(cus)
    idx = big_index(dev)
    P = V[F[use]].reshape(-1, 3)
    assert idx["usable"] == int(use.sum()) and np.array_equal(bits(idx["bounds"][:6]), bits(np.concatenate([P.min(0), P.max(0)])))
    assert idx["bounds"].view(np.uint32)[7] == 0 and idx["arena"].guards_intact()
    counts = sc.bin_counts(V, F, mc.make_grid(idx["res"], idx["lo"], idx["cell"]))
    print("grid %d x %d x %d: %d cells, %d entries" % (tuple(idx["res"]) + (len(counts), int(counts.sum()))))
    assert idx["total"] == int(counts.sum()) and sc.check_start(N_(idx["start"]), counts, "cell table of the big mesh")
    face = N_(idx["records"][:, 9].contiguous()).view(np.int32)                    # every usable face has records, no other
    assert np.array_equal(np.unique(face), np.nonzero(use)[0])


def test_cast_at_three_trips_of_faces(dev):
    """16 rays against brute force over all faces, every output bit for bit; the winners lie in the first, a middle and the
    last trip's range of face indices"""
    cus = CU(dev)
    V, F, info = big_mesh(cus)
    idx = big_index(dev)
    rays = sc.aimed_rays(V, F, cus)
    want = sc.cast_chunked(rays, V, F)
    trip = want["face"][want["code"] == mc.HIT] // sc.per_trip(cus)
    assert {0, 1, sc.trips(len(F), cus) - 1} <= set(trip.tolist()) and (want["code"] == mc.MISSED).any() and (want["code"] == mc.NO_RAY).any()
    assert not set(want["face"].tolist()) & set(info["unusable"])
    g = tm.guarded_outputs(dev, (len(rays),))
    for _ in range(2):
        ops.mesh_cast_rays(G(rays, dev), idx["V"], idx["F"], idx["res"], idx["lo"], idx["cell"], idx["start"], idx["records"], {k: gd.view for k, gd in g.items()})
        torch.cuda.synchronize()
        assert tm.same(g, want, "the big mesh")


def test_a_cell_table_of_three_scan_steps(dev):
    """the soup in a grid of 81^3 = 531 441 cells: the cell-table scan with its carry.  start equals the recount, and the cast
    equals the cast through one cell and the brute-force reference, bit for bit"""
    res = (81, 81, 81)
    assert sc.scan_steps(res[0] * res[1] * res[2]) >= 3
    print("cell table: %d cells, %d steps of k_scan_top" % (res[0] * res[1] * res[2], sc.scan_steps(res[0] * res[1] * res[2])))
    m, V, F, _ = tm.scene("soup")
    idx = mesh.RayIndex(m, res)
    counts = sc.bin_counts(V, F, mc.make_grid(idx.res, idx.lo, idx.cell))
    assert all(s > 0 for s in sc.counts_per_step(counts))
    assert idx.records.shape[0] == int(counts.sum()) and sc.check_start(N_(idx.start), counts, "cell table of the soup")
    want = tm.reference("soup", "pinhole")
    for index in (idx, tm.index_of("soup", (1, 1, 1))):
        g = tm.guarded_outputs(dev, (tm.H, tm.W))
        tm.launch("soup", "pinhole", index, g)
        torch.cuda.synchronize()
        assert tm.same(g, want, ("soup", index.res))
