"""GPU tests of connected components (ops.cc_label / cc_mesh / cc_stats, components, and what mesh, fusion, depth and stereo
build on them) against tests/_cc_ref.py, the restatement test_cc_ref.py pins.  Every comparison is exact equality of int32
arrays; nothing has a tolerance.  The outputs of the ops are interior views of a guarded arena.  The shapes straddle the tiles
the library exports (ops.CC_TILE_2D, ops.CC_TILE_3D): on each axis 1, t - 1, t, t + 1 and 2 t + 1."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _cc_ref as cr
import _depth_ref as dr
from _arena import Arena
from panopticnerf_amd import Pinhole, components, depth, fusion, make_network, mesh, ops, stereo, synthetic
from panopticnerf_amd.data import FrameSet

pytestmark = pytest.mark.gpu

T2, T3 = tuple(ops.CC_TILE_2D), tuple(ops.CC_TILE_3D)
SHAPES = cr.shapes_2d(T2) + cr.shapes_3d(T3)
GUARD = 64
N_ = lambda t: t.detach().cpu().numpy()


def _even(n):
    return max(n + n % 2, 2)


def _label(dev, data, full, tol=None, want_size=True):
    """ops.cc_label with every output and the workspace inside a guarded arena: (labels, size, count) as numpy"""
    data = np.ascontiguousarray(data)
    n = data.size
    words = ops.cc_workspace_bytes(n) // 8
    arena = Arena(dev, [("count", 2, GUARD), ("labels", _even(n), GUARD), ("size", _even(n), GUARD), ("ws", 2 * words, GUARD)])
    i32 = lambda name: arena.view(name).view(torch.int32)[:n].reshape(data.shape)
    labels, size = i32("labels"), i32("size") if want_size else False
    count = arena.view("count").view(torch.int64)
    got = ops.cc_label(torch.from_numpy(data).to(dev), full, tol, labels=labels, size=size, count=count, workspace=arena.view("ws").view(torch.int64))
    torch.cuda.synchronize()
    assert arena.guards_intact()
    assert got[0].data_ptr() == labels.data_ptr() and got[2].data_ptr() == count.data_ptr()
    return N_(labels).copy(), (N_(size).copy() if want_size else None), int(count.item())


def _check_stats(dev, lab, size, count):
    arena = Arena(dev, [("sizes", _even(count), GUARD), ("boxes", _even(6 * count), GUARD)])
    sizes = arena.view("sizes").view(torch.int32)[:count]
    boxes = arena.view("boxes").view(torch.int32)[:6 * count].reshape(count, 6)
    ops.cc_stats(torch.from_numpy(lab).to(dev), torch.from_numpy(size).to(dev), count, sizes=sizes, boxes=boxes)
    torch.cuda.synchronize()
    assert arena.guards_intact()
    want_sizes, want_boxes = cr.stats(lab, count)
    assert np.array_equal(N_(sizes), want_sizes) and np.array_equal(N_(boxes), want_boxes)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_key_patterns_equal_the_restatement(dev, shape):
    rank = len(shape)
    for name, keys in cr.key_patterns(shape, T2 if rank == 2 else T3, seed=sum(shape)).items():
        for full in (False, True):
            want_lab, want_count, want_size = cr.label(keys, cr.KEYS, 0.0, full)
            lab, size, count = _label(dev, keys, full)
            what = "%s full=%d" % (name, full)
            assert count == want_count, what
            assert np.array_equal(lab, want_lab), what
            assert np.array_equal(size, want_size), what
            if name in ("p45", "percolation", "multikey", "checkerboard", "corner", "one", "background"):
                _check_stats(dev, lab, size, count)
    lab, size, _ = _label(dev, cr.bernoulli(shape, 0.5, 9), False, want_size=False)
    assert size is None and np.array_equal(lab, cr.label(cr.bernoulli(shape, 0.5, 9))[0])


def test_corner_pair_is_joined_only_by_the_full_neighbourhood(dev):
    for tile, shape in ((T2, (2 * T2[1] + 1, 2 * T2[0] + 1)), (T3, (2 * T3[2] + 1, 2 * T3[1] + 1, 2 * T3[0] + 1))):
        keys = cr.corner_pair(shape, tile)
        assert _label(dev, keys, False)[2] == 2 and _label(dev, keys, True)[2] == 1


@pytest.mark.parametrize("shape", [(1, 1), (5, T2[0] + 1), (2 * T2[1] + 1, 2 * T2[0] + 1), (1, 1, 1), (1, 1, 37), (T3[2] + 1, T3[1] + 1, T3[0] + 1),
                                   (2 * T3[2] + 1, T3[1], 2 * T3[0] + 1)], ids=lambda s: "x".join(str(v) for v in s))
def test_values_mode_equals_the_restatement(dev, shape):
    for name, (values, tol) in cr.value_cases(shape, seed=sum(shape)).items():
        for full in (False, True):
            want_lab, want_count, want_size = cr.label(values, cr.VALUES, tol, full)
            lab, size, count = _label(dev, values, full, tol=float(tol))
            what = "%s full=%d" % (name, full)
            assert count == want_count and np.array_equal(lab, want_lab) and np.array_equal(size, want_size), what
            if name == "holes":
                assert ((lab >= 0) == (np.isfinite(values) & (values > 0))).all()


def test_values_mode_closed_forms(dev):
    cases = cr.value_cases((1, 24))
    for full in (False, True):
        assert _label(dev, cases["ramp_at_tol"][0], full, tol=0.25)[2] == 1
        assert _label(dev, cases["ramp_above_tol"][0], full, tol=0.25)[2] == 24
        lab, _, count = _label(dev, cases["chain"][0], full, tol=0.25)
        assert count == 1 and list(lab[0, :4]) == [0, 0, 0, -1]
    quant = cases["tol_zero"][0]
    assert np.array_equal(_label(dev, quant, False, tol=0.0)[0], _label(dev, quant.astype(np.int32), False)[0])


def test_zero_elements(dev):
    count = torch.full((1,), 77, dtype=torch.int64, device=dev)
    v, f, s, c = ops.cc_mesh(torch.zeros((0, 3), dtype=torch.int32, device=dev), 0, count=count)
    assert v.shape == (0,) and f.shape == (0,) and s.shape == (0,) and int(count.item()) == 0
    v, f, s, c = ops.cc_mesh(torch.zeros((3, 3), dtype=torch.int32, device=dev), 0)
    assert int(c.item()) == 0 and f.tolist() == [-1] * 3 and s.tolist() == [0] * 3
    sizes, boxes = ops.cc_stats(f, s, 0)
    assert sizes.shape == (0,) and boxes.shape == (0, 6)


def test_components_record(dev):
    mask, count, sizes = synthetic.blobs((20, 19, 18), 1)
    keys = np.where(mask.numpy(), 0, -1).astype(np.int32)
    want_lab, want_count, want_size = cr.label(keys)
    assert want_count == count
    for x in (mask, torch.from_numpy(keys), torch.from_numpy(keys).to(torch.int16)):         # (uint8 has no background: below)
        c = components.label(x.to(dev))
        assert c.connectivity == 6 and np.array_equal(N_(c.labels), want_lab) and np.array_equal(N_(c.size), want_size)
        assert c.n == count and np.array_equal(N_(c.sizes()), sizes) and np.array_equal(N_(c.boxes()), cr.stats(want_lab, count)[1])
    c = components.label(mask.to(dev), connectivity=26)
    assert c.connectivity == 26 and c.n == count
    u8 = components.label((mask.to(torch.uint8) * 2).to(dev))                 # keys 0 and 2: the background is a component too
    assert np.array_equal(N_(u8.labels), cr.label(mask.numpy().astype(np.int32) * 2)[0])
    for k in (int(sizes.min()), int(sizes.max()), int(sizes.max()) + 1, 0):
        assert np.array_equal(N_(c.keep(k)), want_size >= max(k, 1))
    for k in (0, 1, 2, count + 3):
        assert np.array_equal(N_(c.largest(k)), cr.largest(want_lab, sizes, k))
    lo, step = (-1.0, 0.5, 2.0), (0.25, 0.5, 0.125)
    b = cr.stats(want_lab, count)[1].astype(np.float32)
    world = np.stack([np.asarray(lo, np.float32) + b[:, :3] * np.asarray(step, np.float32),
                      np.asarray(lo, np.float32) + (b[:, 3:] + 1) * np.asarray(step, np.float32)], axis=1)
    assert np.array_equal(N_(c.boxes(lo, step)), world)
    # a size tie goes to the lower number
    two = torch.zeros((3, 9), dtype=torch.bool)
    two[0, :3] = two[2, 5:8] = True
    t = components.label(two.to(dev))
    assert t.n == 2 and np.array_equal(N_(t.largest(1)), N_(t.labels) == 0)
    # float32 needs tol; 2-D defaults to 4
    img = torch.from_numpy(cr.value_cases((9, 11))["noisy"][0])
    v = components.label(img.to(dev), tol=0.2, connectivity=8)
    assert v.connectivity == 8 and np.array_equal(N_(v.labels), cr.label(img.numpy(), cr.VALUES, 0.2, True)[0])
    with pytest.raises(TypeError, match="int64 keys are not taken"):
        components.label(torch.zeros((3, 3), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="connectivity must be 4 or 8 for a 2-D tensor"):
        components.label(img.to(dev), tol=0.1, connectivity=6)
    with pytest.raises(ValueError, match="need tol"):
        components.label(img.to(dev))


def test_repeatable(dev):
    """the schedule-independence claim: five runs of a percolation-threshold case, all equal (and equal to the restatement)"""
    for shape in ((70, 70), (20, 19, 18)):
        keys = cr.bernoulli(shape, cr.PERCOLATION[len(shape)], 123)
        want = cr.label(keys)
        x = torch.from_numpy(keys).to(dev)
        for _ in range(5):
            lab, size, count = ops.cc_label(x)
            assert np.array_equal(N_(lab), want[0]) and int(count.item()) == want[1] and np.array_equal(N_(size), want[2])


# ------------------------------------------------------------------------------------------------------------------ meshes

def _mesh_case(dev, faces, V):
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F = len(faces)
    words = ops.cc_workspace_bytes(V) // 8
    arena = Arena(dev, [("count", 2, GUARD), ("v", _even(V), GUARD), ("f", _even(F), GUARD), ("s", _even(F), GUARD), ("ws", max(2 * words, 2), GUARD)])
    i32 = lambda name, n: arena.view(name).view(torch.int32)[:n]
    count = arena.view("count").view(torch.int64)
    ops.cc_mesh(torch.from_numpy(faces).to(dev), V, i32("v", V), i32("f", F), i32("s", F), count, arena.view("ws").view(torch.int64))
    torch.cuda.synchronize()
    assert arena.guards_intact()
    vlab, flab, fsize, n = cr.label_mesh(faces, V)
    assert int(count.item()) == n
    assert np.array_equal(N_(i32("v", V)), vlab) and np.array_equal(N_(i32("f", F)), flab) and np.array_equal(N_(i32("s", F)), fsize)
    return n, fsize


def test_meshes_equal_the_restatement(dev):
    g = np.random.default_rng(4)
    ico, box = synthetic.icosphere(2), synthetic.box_mesh((2, 2, 2), (3, 3, 3))
    Vi = ico.vertices.shape[0]
    faces, V = np.concatenate([ico.faces.numpy(), box.faces.numpy() + Vi]), Vi + 8
    n, fsize = _mesh_case(dev, faces, V)
    assert n == 2 and set(fsize[:320]) == {320} and set(fsize[320:]) == {12}              # 20 * 4^2 faces and 12
    shuffled = g.permutation(V).astype(np.int32)[faces][g.permutation(len(faces))]
    assert _mesh_case(dev, shuffled, V)[0] == 2
    strip = np.stack([np.arange(3000), np.arange(1, 3001), np.arange(2, 3002)], axis=1)
    assert _mesh_case(dev, strip, 3002)[0] == 1
    assert _mesh_case(dev, g.permutation(3002)[strip], 3002)[0] == 1                      # a long strip, vertex numbers shuffled
    assert _mesh_case(dev, faces, V + 7)[0] == 2                                           # unused vertices
    assert _mesh_case(dev, np.concatenate([faces, [[0, 1, V], [-1, 2, 3]]]), V)[0] == 2    # faces with an index out of range
    assert _mesh_case(dev, np.zeros((0, 3), np.int32), 5)[0] == 0                          # F = 0
    _mesh_case(dev, g.integers(0, 400, size=(150, 3)), 400)
    # MeshComponents: sizes in faces, through cc_stats over the faces as a 1 x 1 x F lattice
    both = mesh.Mesh.from_arrays(np.concatenate([ico.vertices.numpy(), box.vertices.numpy()]), faces, device=dev)
    mc = both.components()
    assert isinstance(mc, components.MeshComponents) and mc.n == 2 and mc.sizes().tolist() == [320, 12]
    assert int(mc.keep(13).sum()) == 320 and int(mc.largest().sum()) == 320
    empty = mesh.Mesh.from_arrays(np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32), device=dev).components()
    assert empty.n == 0 and empty.sizes().shape == (0,)


def test_extracted_spheres_select_and_largest(dev):
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 24
    big = synthetic.sdf_grid("sphere", lo, hi, res, center=(-0.45, 0.0, 0.0), radius=0.4)
    small = synthetic.sdf_grid("sphere", lo, hi, res, center=(0.6, 0.1, 0.0), radius=0.25)
    m = mesh.extract(torch.maximum(big, small).to(dev), lo, hi, 0.0)
    m.attributes["tag"] = torch.arange(m.vertices.shape[0], device=dev)
    mc = m.components()
    vlab, flab, fsize, n = cr.label_mesh(N_(m.faces), m.vertices.shape[0])
    assert mc.n == n == 2 and np.array_equal(N_(mc.face_label), flab) and np.array_equal(N_(mc.face_size), fsize)
    alone = mesh.extract(big.to(dev), lo, hi, 0.0)
    top = m.largest()
    assert top.faces.shape[0] == alone.faces.shape[0] == int(fsize.max()) and top.res == m.res and top.level == m.level
    assert torch.equal(top.vertices, alone.vertices) and torch.equal(top.src, alone.src)       # the larger sphere alone, src carried
    assert torch.equal(top.attributes["tag"], torch.nonzero(torch.from_numpy(vlab == np.argmax(np.bincount(flab))).to(dev)).reshape(-1))
    assert m.remove_small(int(fsize.min()) + 1).faces.shape[0] == int(fsize.max()) and m.remove_small(0).faces.shape[0] == m.faces.shape[0]
    # select against numpy, on a random mask
    mask = np.random.default_rng(8).random(m.faces.shape[0]) < 0.3
    sv, sf, index = cr.select(N_(m.vertices), N_(m.faces), mask)
    got = m.select(torch.from_numpy(mask).to(dev))
    assert np.array_equal(N_(got.vertices), sv) and np.array_equal(N_(got.faces), sf) and np.array_equal(N_(got.src), N_(m.src)[index])
    assert np.array_equal(N_(got.attributes["tag"]), index) and got.faces.dtype == torch.int32
    with pytest.raises(ValueError, match="face_mask must be a"):
        m.select(torch.ones(3, dtype=torch.bool, device=dev))


def _same_mesh(a, b):
    return (torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and torch.equal(a.src, b.src)
            and sorted(a.attributes) == sorted(b.attributes) and all(torch.equal(a.attributes[k], b.attributes[k]) for k in a.attributes))


def test_min_faces_zero_is_todays_result_and_a_bound_removes_floaters(dev):
    torch.manual_seed(3)
    net = make_network(NS(D=2, W=128, skips=[], N_importance=0, num_classes=5, num_instances=3)).to(dev).eval()
    lo, hi, res = (-1.0, -0.5, 2.0), (1.0, 1.5, 4.0), (12, 10, 9)
    level = float(net.query_grid(lo, hi, res, want=("sigma",))["sigma"].median())
    plain = mesh.from_network(net, lo, hi, res, level)
    assert _same_mesh(plain, mesh.from_network(net, lo, hi, res, level, min_faces=0))
    sizes = plain.components().sizes()
    kept = mesh.from_network(net, lo, hi, res, level, min_faces=int(sizes.max()))
    assert kept.faces.shape[0] == int(sizes[sizes == sizes.max()].sum()) and sorted(kept.attributes) == sorted(plain.attributes)
    # a fused volume: a plane seen once
    H, W = 24, 32
    cam = Pinhole(30.0, 30.0, (W - 1) / 2.0, (H - 1) / 2.0, W, H)
    frames = FrameSet(dev, capacity=1)
    frames.add(cam, torch.eye(4)[:3], 0.1, 10.0, torch.zeros((H, W, 3), dtype=torch.uint8), depth=torch.full((H, W), 2.0))
    vol = fusion.Volume((-1.0, -0.8, 1.2), (1.0, 0.8, 2.8), (20, 16, 16), dev)
    fusion.integrate(vol, frames, 0.5)
    a, b = fusion.extract(vol), fusion.extract(vol, min_faces=0)
    assert a.faces.shape[0] > 0 and _same_mesh(a, b)
    assert fusion.extract(vol, min_faces=a.faces.shape[0] + 1).faces.shape[0] == 0
    with pytest.raises(ValueError, match="min_faces must be an integer >= 0"):
        fusion.extract(vol, min_faces=-1)


# ------------------------------------------------------------------------------------------------------------ conveniences

def _speckled_depth():
    h, w = 40, 56
    plane = (2.0 + 0.01 * np.arange(w, dtype=np.float32))[None, :].repeat(h, 0).astype(np.float32)
    img = dr.noisy(plane, 3, rel=0.001, speckle=6)
    img[10:12, 20:22] = 5.0                                 # a planted blob of 5 pixels, far from the plane
    img[12, 20] = 5.0
    img[30, 5:9] = 0.0                                      # and a hole
    return img


def test_depth_despeckle(dev):
    img = _speckled_depth()
    for conn, min_size in ((4, 6), (8, 6), (4, 5), (4, 0)):
        got = N_(depth.despeckle(torch.from_numpy(img).to(dev), 0.05, min_size, connectivity=conn))
        want = cr.despeckle(img, 0.05, min_size, conn == 8)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        gone = got != img
        assert (got[gone] == 0).all()                                           # removed pixels are 0, every other pixel its own bits
        if min_size == 6:
            assert got[10, 20] == 0 and got[12, 20] == 0 and 6 <= gone.sum() <= 5 + 6 and got[0, 0] == img[0, 0]
        if min_size == 5:
            assert got[10, 20] == 5.0
        if min_size == 0:
            assert not gone.any()


def test_stereo_despeckle_and_depth_from_pair(dev):
    H, W = 48, 96
    left, right, disp, visible = synthetic.stereo_pair(H, W, layers=((0, None), (9, (0.3, 0.7, 0.4, 0.8))), seed=2, device=dev)
    res = stereo.sgm(left, right, max_disp=16)
    d16 = N_(res["d16"])
    zero = (d16 == 0)
    assert zero.sum() > 500                                   # a region of true disparity 0 that matched
    out = stereo.despeckle(res, max_diff=1.0, min_size=50)
    assert sorted(out) == sorted(res)
    _, _, size = cr.label((d16.astype(np.int32) + 1).astype(np.float32), cr.VALUES, 16.0, False)
    gone = (size > 0) & (size < 50)
    want = np.where(gone, np.int16(-4), d16)
    assert np.array_equal(N_(out["d16"]), want) and stereo.CODES[-4] == "speckle"
    assert np.array_equal(N_(out["valid"]), want >= 0) and np.array_equal(N_(out["code"]), np.where(want >= 0, 0, want))
    assert np.array_equal(N_(out["disparity"]), np.where(want >= 0, want.astype(np.float32) * np.float32(0.0625), np.float32(0)))
    assert (N_(out["d16"])[zero & (size >= 50)] == 0).all() and (zero & (size >= 50)).sum() > 500      # disparity 0 stayed foreground
    assert out["disp_right"] is res["disp_right"] and gone.any()
    # without the + 1 the zero region would have been background: labelling d16 itself gives it size 0
    assert (cr.label(d16.astype(np.float32), cr.VALUES, 16.0, False)[2][zero] == 0).all()
    cam = Pinhole(100.0, 100.0, (W - 1) / 2.0, (H - 1) / 2.0, W, H)
    plain = stereo.depth_from_pair(left, right, cam, 0.5, max_disp=16)
    assert torch.equal(plain, stereo.depth_from_pair(left, right, cam, 0.5, speckle=None, max_disp=16))
    assert torch.equal(stereo.depth_from_pair(left, right, cam, 0.5, speckle=(1.0, 50), max_disp=16), stereo.depth(out, cam, 0.5))


def test_label_and_despeckle_in_a_graph(dev):
    """components.label + depth.despeckle captured on a side stream: every replay equals the restatement of the input it saw"""
    img = _speckled_depth()
    x = torch.from_numpy(img).to(dev)
    run = lambda: (components.label(x, tol=0.05), depth.despeckle(x, 0.05, 6))
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream(dev)):
        c, clean = run()
    for edit in (None, (slice(20, 23), slice(30, 32))):
        if edit is not None:
            img = img.copy()
            img[edit] = 7.0
            img[0, :] = 0.0
            x.copy_(torch.from_numpy(img).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        want_lab, want_count, want_size = cr.label(img, cr.VALUES, 0.05, False)
        assert np.array_equal(N_(c.labels), want_lab) and int(c.count.item()) == want_count and np.array_equal(N_(c.size), want_size)
        assert np.array_equal(N_(clean).view(np.uint32), cr.despeckle(img, 0.05, 6).view(np.uint32))
