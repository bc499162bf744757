"""Depth fusion on an MI355X: k_tsdf_integrate (csrc/pnr_fusion.hip) and fusion.* against tests/_tsdf_ref.py's restatement of
the rule (include/pnr.h "depth fusion").  No tolerance anywhere: every volume array must equal integrate32's bit pattern, and the
extracted mesh the CPU extractor's on the same volume.  Every caller-owned array sits between canaries.
tests/test_tsdf_ref.py pins the restatement on the CPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _mesh_ref as mr
import _tsdf_ref as tr
from panopticnerf_amd import Equirect, Fisheye, FrameSet, Pinhole, _lib, camera, fusion, ops, pointcloud, stereo, synthetic

pytestmark = pytest.mark.gpu

BOX = ((-2.5, -1.0, 4.5), (3.0, 3.0, 8.0))          # straddles the sphere's surface in front of every camera of _tsdf_ref.CAMERAS
ALL6 = tuple(tr.CAMERAS)
GUARD = 64
REC = ctypes.sizeof(_lib.Frame)
ARRAYS = ("tsdf", "weight", "rgb", "rgb_weight", "label", "conf")


def N_(t):
    return t.detach().cpu().numpy()


def camera_of(name):
    m, cam, _, w, h = tr.CAMERAS[name]
    if m == tr.PINHOLE:
        c = Pinhole(*cam, w, h)
    elif m == tr.FISHEYE:
        c = Fisheye(*cam, w, h)
    else:
        c = Equirect(w, h, **(tr.EQUIRECT_B_DEGREES if name == "equirect_b" else {}))
    assert np.array_equal(np.asarray(c.params, np.float32), np.asarray(cam, np.float32)), name
    return c


def make_set(dev, specs, capacity=None):
    """FrameSet + reference frames of specs = [(camera name, sphere_frame keywords, edit(frame) or None)]; the reference uses
    the rows of the set's own w2c table."""
    frames = FrameSet(dev, capacity=capacity or max(len(specs), 1))
    refs = []
    T = lambda a: None if a is None else torch.from_numpy(a)
    for k, (name, kw, edit) in enumerate(specs):
        fr = tr.sphere_frame(name, seed=k + 1, **kw)
        if edit is not None:
            edit(fr)
        frames.add(camera_of(name), torch.from_numpy(fr["c2w"]), 0.1, 100.0, T(fr["rgb"]), depth=T(fr["depth"]), pseudo_label=T(fr["sem"]),
                   instance_label=T(fr["inst"]))
        refs.append(fr)
    if specs:
        table = frames.w2c_table()
        assert tuple(table.shape) == (frames.capacity, 12) and table.dtype == torch.float32
        for k, fr in enumerate(refs):
            assert torch.equal(table[k].cpu(), camera.invert_pose(torch.from_numpy(fr["c2w"])).reshape(12))
            m, cam, _, w, h = fr["view"]
            fr["view"] = (m, cam, N_(table[k]).reshape(3, 4), w, h)
        assert frames.w2c_table() is table
    return frames, refs


class Guarded:
    """a tensor with GUARD canary elements before and after it, in one allocation"""

    def __init__(self, like):
        n = like.numel()
        self.canary = -7.25e30 if like.dtype.is_floating_point else -1234567
        self.buf = torch.full((n + 2 * GUARD,), self.canary, dtype=like.dtype, device=like.device)
        self.n = n
        self.view = self.buf[GUARD:GUARD + n].view(like.shape)
        self.view.copy_(like)

    def intact(self):
        return bool((self.buf[:GUARD] == self.canary).all()) and bool((self.buf[GUARD + self.n:] == self.canary).all())


def guarded_volume(dev, res, color=True, labels=True, box=BOX):
    vol = fusion.Volume(box[0], box[1], res, dev, color=color, labels=labels)
    guards = []
    for name in ARRAYS:
        if getattr(vol, name) is not None:
            g = Guarded(getattr(vol, name))
            setattr(vol, name, g.view)
            guards.append(g)
    return vol, guards


def state_of(vol):
    st = {}
    for name in ARRAYS:
        t = getattr(vol, name)
        if t is not None:
            st[name] = N_(t).reshape(-1, 3) if name == "rgb" else N_(t).reshape(-1)
    return st


def same(vol, guards, want, what=""):
    got = state_of(vol)
    assert set(got) == set(want), what
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
    assert all(g.intact() for g in guards), what
    return True


def fresh(vol):
    rx, ry, rz = vol.res
    return tr.new_state(rx * ry * rz, vol.rgb is not None, vol.label is not None)


def pts_of(vol):
    return tr.points(vol.lo, vol.hi, vol.res)


PLAIN = [(name, {}, None) for name in ALL6]


@pytest.fixture(scope="module")
def six(dev):
    return make_set(dev, PLAIN)


# ------------------------------------------------------------------------------------------------ 1: lattices
@pytest.mark.parametrize("res, box", [((1, 1, 1), BOX), ((2, 3, 5), BOX), ((17, 9, 4), BOX), ((64, 5, 3), BOX), ((33, 33, 33), BOX),
                                      ((12, 7, 5), ((-4.0, 0.5, 5.75), (4.0, 2.5, 6.25)))])       # the last: an anisotropic box
def test_lattices_bit_for_bit(dev, six, res, box):
    frames, refs = six
    vol, guards = guarded_volume(dev, res, box=box)
    assert fusion.integrate(vol, frames, 0.6) is vol
    want = tr.integrate32(fresh(vol), refs, pts_of(vol), 0.6)
    assert same(vol, guards, want, res)
    assert (want["weight"] > 0).any() and (want["weight"] >= 2).sum() >= want["weight"].size // 4
    if res[0] * res[1] * res[2] > 100:
        assert (want["label"] >= 0).any() and (want["rgb_weight"] > 0).any() and (want["weight"] > want["rgb_weight"]).any()
    sem, inst = tr.unpack(want["label"])
    assert np.array_equal(N_(vol.sem_label).reshape(-1), sem) and np.array_equal(N_(vol.inst_label).reshape(-1), inst)
    assert np.array_equal(N_(vol.colors()).reshape(-1, 3), np.rint(want["rgb"]).astype(np.uint8))


def test_three_grid_stride_trips(dev):
    """a lattice of more than two full grids of PNR_TSDF_BLOCK-point blocks: the third trip and the tail, checked on the z slices
    that hold the first and last points and the points either side of every trip boundary"""
    per_trip = torch.cuda.get_device_properties(dev).multi_processor_count * ops.TSDF_BLOCKS_PER_CU * ops.TSDF_BLOCK
    rx, ry = 255, 64                                            # 255: slices straddle blocks, and the tail block is partial
    rz = (2 * per_trip) // (rx * ry) + 2
    n = rx * ry * rz
    assert -(-n // per_trip) >= 3 and n % ops.TSDF_BLOCK != 0
    frames, refs = make_set(dev, [(name, {}, None) for name in ("pinhole_a", "fisheye_b", "equirect_b")])
    vol, guards = guarded_volume(dev, (rx, ry, rz))
    fusion.integrate(vol, frames, 0.5)
    slices = sorted({0, rz - 1} | {min(max(b // (rx * ry) + d, 0), rz - 1) for b in (per_trip, 2 * per_trip) for d in (-1, 0, 1)})
    x, y, z = mr.positions(vol.lo, vol.hi, vol.res)
    got = state_of(vol)
    touched = 0
    for iz in slices:
        Y, X = np.meshgrid(y, x, indexing="ij")
        pts = np.stack([X, Y, np.full_like(X, z[iz])], -1).reshape(-1, 3).astype(np.float32)
        want = tr.integrate32(tr.new_state(rx * ry, True, True), refs, pts, 0.5)
        a, b = iz * rx * ry, (iz + 1) * rx * ry
        for k in want:
            assert np.array_equal(got[k][a:b].view(np.uint32), want[k].view(np.uint32)), (iz, k)
        touched += int((want["weight"] > 0).sum())
    assert touched > 1000 and all(g.intact() for g in guards)
    # and the whole volume: a point is fused iff some frame sees it, nothing else is left at a value no frame could give
    assert np.isfinite(got["tsdf"]).all() and (np.abs(got["tsdf"]) <= 1).all() and (got["weight"] <= 3).all()


# ------------------------------------------------------------------------------------------------ 2: frame counts and edge frames
SPHERE2 = ((0.1, 0.2, 0.3), 2.5)
BOX2 = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0))        # res 16: positions -3.75 + 0.5 i, exact in float32; the cameras stand on lattice points


def _pose_at(name, origin):
    c2w = np.asarray(tr.CAMERAS[name][2], np.float64).copy()
    c2w[:, 3] = origin
    return c2w


def _bad_pixels(fr):
    d = fr["depth"]
    d[::5, ::3] = 0.0
    d[1::7, :] = -2.0
    d[:, 2::9] = np.nan
    d[3::11, 1::4] = np.inf
    d[2::13, 5::6] = -np.inf


EDGE = [("pinhole_a", {"sphere": SPHERE2, "c2w": _pose_at("pinhole_a", (0.25, 0.25, -0.25))}, _bad_pixels),
        ("fisheye_a", {"sphere": SPHERE2, "c2w": _pose_at("fisheye_a", (-0.25, 0.25, 0.25)), "inst": False}, None),
        ("equirect_b", {"sphere": SPHERE2, "c2w": _pose_at("equirect_b", (0.25, -0.25, 0.75))}, None),
        ("pinhole_b", {"sphere": SPHERE2, "c2w": _pose_at("pinhole_b", (0.75, 0.25, 0.25)), "depth": False}, None),
        ("equirect_a", {"sphere": SPHERE2, "c2w": _pose_at("equirect_a", (0.25, 0.25, 0.25)), "sem": False}, _bad_pixels),
        ("fisheye_b", {"sphere": SPHERE2, "c2w": _pose_at("fisheye_b", (-0.25, -0.25, -0.25)), "n_sem": 2, "n_inst": 1}, _bad_pixels),
        ("pinhole_a", {"sphere": SPHERE2, "c2w": _pose_at("pinhole_a", (0.25, 0.25, -0.75)), "n_sem": 2, "n_inst": 1}, None)]


@pytest.fixture(scope="module")
def edge(dev):
    return make_set(dev, EDGE, capacity=9)


def test_frame_counts_and_edge_frames(dev, edge):
    frames, refs = edge
    pts = tr.points(BOX2[0], BOX2[1], (16, 16, 16))
    # the lattice holds every camera centre, and points behind the pinhole cameras
    for fr in refs:
        assert (pts == fr["c2w"][:, 3]).all(axis=1).sum() == 1, fr["name"]
    assert ((pts - refs[0]["c2w"][:, 3]) @ refs[0]["c2w"][:, 2] < 0).sum() > 1000
    for F in (0, 1, 2, 7):
        vol, guards = guarded_volume(dev, 16, box=BOX2)
        fusion.integrate(vol, frames, 0.7, last=F)
        want = tr.integrate32(fresh(vol), refs, pts, 0.7, f1=F)
        assert same(vol, guards, want, F)
        if F == 0:
            assert not want["weight"].any() and (want["label"] == -1).all()
        if F == 7:
            assert want["weight"].max() >= 4 and (want["conf"] >= 2).any() and (want["weight"] == 0).any()
            # the frame without depth changes nothing; frames without sem / inst vote less / with inst = -1
            again = tr.integrate32(fresh(vol), refs[:3] + refs[4:], pts, 0.7)
            assert all(np.array_equal(again[k], want[k]) for k in want)
            assert (tr.unpack(want["label"])[1][want["label"] >= 0] == -1).any()
    empty = FrameSet(dev, capacity=2)
    vol, guards = guarded_volume(dev, (5, 4, 3))
    fusion.integrate(vol, empty, 0.7)
    assert same(vol, guards, fresh(vol), "empty set")


# ------------------------------------------------------------------------------------------------ 3: parameters
@pytest.mark.parametrize("color, labels", list(itertools.product((False, True), (False, True))))
def test_parameters_and_optional_arrays(dev, edge, six, color, labels):
    for (frames, refs), box, res, limit in ((edge, BOX2, (16, 16, 16), 2.25), (six, BOX, (17, 9, 4), 6.0)):
        for trunc, w_max, max_depth in ((0.15, np.inf, np.inf), (3.0, 3.0, np.inf), (0.7, 1.0, np.inf), (0.7, np.inf, limit), (1.0, 3.0, limit)):
            vol, guards = guarded_volume(dev, res, color, labels, box)
            fusion.integrate(vol, frames, trunc, max_depth=max_depth, w_max=w_max)
            want = tr.integrate32(fresh(vol), refs, pts_of(vol), trunc, max_depth, w_max)
            assert same(vol, guards, want, (trunc, w_max, max_depth, res))
            assert (want["weight"] > 0).any() and want["weight"].max() <= w_max
            if w_max < np.inf and max_depth == np.inf:
                assert want["weight"].max() == w_max
    # the cap and the depth limit bite in the edge scene
    frames, refs = edge
    pts = tr.points(BOX2[0], BOX2[1], (16, 16, 16))
    free = tr.integrate32(tr.new_state(len(pts)), refs, pts, 0.7)
    capped = tr.integrate32(tr.new_state(len(pts)), refs, pts, 0.7, w_max=1.0)
    near = tr.integrate32(tr.new_state(len(pts)), refs, pts, 0.7, max_depth=2.25)
    assert free["weight"].max() > 3 and not np.array_equal(free["tsdf"], capped["tsdf"]) and (near["weight"] < free["weight"]).any()


# ------------------------------------------------------------------------------------------------ 4: launch equivalences
def test_launch_equivalences(dev):
    frames, refs = make_set(dev, EDGE, capacity=9)              # its own set: the test adds a frame
    F = len(refs)
    res = (16, 16, 16)
    one, g1 = guarded_volume(dev, res, box=BOX2)
    fusion.integrate(one, frames, 0.7, w_max=3.0)
    want = tr.integrate32(fresh(one), refs, pts_of(one), 0.7, w_max=3.0)
    assert same(one, g1, want)
    each, g2 = guarded_volume(dev, res, box=BOX2)
    for f in range(F):
        fusion.integrate(each, frames, 0.7, first=f, last=f + 1, w_max=3.0)
    assert same(each, g2, want, "F launches")
    for k in (1, 3, 6):
        two, g3 = guarded_volume(dev, res, box=BOX2)
        fusion.integrate(two, frames, 0.7, last=k, w_max=3.0)
        fusion.integrate(two, frames, 0.7, first=k, w_max=3.0)
        assert same(two, g3, want, k)
    # a second call accumulates
    fusion.integrate(one, frames, 0.7, w_max=3.0)
    twice = tr.integrate32(want, refs, pts_of(one), 0.7, w_max=3.0)
    assert same(one, g1, twice, "second call") and not np.array_equal(twice["tsdf"], want["tsdf"])
    one.reset()
    assert same(one, g1, fresh(one), "reset")
    # the ops front end on a set that grew: the table is extended, not rebuilt
    table = frames.w2c_table()
    before = table.clone()
    fr = tr.sphere_frame("pinhole_b", seed=40, sphere=SPHERE2, c2w=_pose_at("pinhole_b", (0.25, 0.75, 0.25)))
    frames.add(camera_of("pinhole_b"), torch.from_numpy(fr["c2w"]), 0.1, 100.0, torch.from_numpy(fr["rgb"]), depth=torch.from_numpy(fr["depth"]),
               pseudo_label=torch.from_numpy(fr["sem"]), instance_label=torch.from_numpy(fr["inst"]))
    assert frames.w2c_table() is table and torch.equal(table[:F], before[:F]) and table[F].abs().sum() > 0
    m, cam, _, w, h = fr["view"]
    fr["view"] = (m, cam, N_(table[F]).reshape(3, 4), w, h)
    grown, g4 = guarded_volume(dev, res, box=BOX2)
    fusion.integrate(grown, frames, 0.7)
    assert same(grown, g4, tr.integrate32(fresh(grown), refs + [fr], pts_of(grown), 0.7), "grown set")


def test_captured_graph_reads_the_table_and_the_images_when_it_runs(dev):
    frames, refs = make_set(dev, [(name, {"n_sem": 2, "n_inst": 2}, None) for name in ("pinhole_a", "equirect_a", "fisheye_a")])
    vol, guards = guarded_volume(dev, (17, 9, 4))
    pts = pts_of(vol)
    fusion.integrate(vol, frames, 0.6)                          # warm call: module loading and the w2c upload are not capturable
    vol.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fusion.integrate(vol, frames, 0.6)
    vol.reset()
    g.replay()
    torch.cuda.synchronize()
    want = tr.integrate32(fresh(vol), refs, pts, 0.6)
    assert same(vol, guards, want, "first replay") and (want["weight"] == 3).any()
    # a second replay accumulates
    g.replay()
    torch.cuda.synchronize()
    assert same(vol, guards, tr.integrate32(want, refs, pts, 0.6), "second replay")
    # edit the depth image of frame 0 and the record of frame 1 (its depth address: the frame leaves the fusion)
    refs[0]["depth"][:, :48] += np.float32(0.25)
    frames.frames[0]["depth"].copy_(torch.from_numpy(refs[0]["depth"]))
    frames.table[REC + _lib.Frame.depth.offset:REC + _lib.Frame.depth.offset + 8].zero_()
    refs[1]["depth"] = None
    vol.reset()
    g.replay()
    torch.cuda.synchronize()
    want2 = tr.integrate32(fresh(vol), refs, pts, 0.6)
    assert not np.array_equal(want2["tsdf"], want["tsdf"]) and want2["weight"].max() == 2
    assert same(vol, guards, want2, "edited")


# ------------------------------------------------------------------------------------------------ 5: end to end
def read_ply(path):
    """the binary little-endian PLY Mesh.save_ply writes: (vertex record array, faces (T, 3))"""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    n_v = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    n_f = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    stop = [i for i, ln in enumerate(lines) if ln.startswith("element face")][0]
    kinds = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    dt = np.dtype([(ln.split()[2], kinds[ln.split()[1]]) for ln in lines[:stop] if ln.startswith("property")])
    verts = np.frombuffer(body, dt, n_v)
    faces = np.frombuffer(body, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), n_f, n_v * dt.itemsize)
    assert n_v * dt.itemsize + 13 * n_f == len(body) and (faces["n"] == 3).all()
    return verts, faces["v"]


def test_stereo_depth_to_a_labelled_mesh(dev, tmp_path):
    H, W, trunc = 64, 128, 0.6
    left, right, _, _ = synthetic.stereo_pair(H, W, layers=((16, None),), seed=3)
    cam, baseline = Pinhole(120.0, 120.0, (W - 1) / 2.0, (H - 1) / 2.0, W, H), 0.6       # the plane stands at 120 * 0.6 / 16 = 4.5
    depth = stereo.depth_from_pair(left.to(dev), right.to(dev), cam, baseline, max_disp=32)
    assert float((depth > 0).float().mean()) > 0.8
    g = np.random.default_rng(11)
    rgb = g.integers(0, 256, (H, W, 3)).astype(np.uint8)
    sem, inst = g.integers(-1, 3, (H, W)).astype(np.int16), g.integers(-1, 40, (H, W)).astype(np.int16)
    c2w = np.asarray(tr.cr.pose(0.0), np.float32)
    frames = FrameSet(dev, capacity=1)
    frames.add(cam, torch.from_numpy(c2w), 0.1, 100.0, torch.from_numpy(rgb), depth=depth, pseudo_label=torch.from_numpy(sem),
               instance_label=torch.from_numpy(inst))
    lo, hi, res = (-1.6, -0.8, 3.6), (1.6, 0.8, 5.4), (32, 16, 18)             # step 0.1: trunc is 6 steps
    vol = fusion.Volume(lo, hi, res, dev, color=True, labels=True)
    fusion.integrate(vol, frames, trunc)
    m = fusion.extract(vol)
    # the reference on the same images
    fr = tr.frame((tr.PINHOLE, np.asarray(cam.params, np.float32), N_(frames.w2c_table()[0]).reshape(3, 4), W, H), N_(depth), rgb, sem, inst)
    want = tr.integrate32(tr.new_state(32 * 16 * 18, True, True), [fr], tr.points(lo, hi, res), trunc)
    got = state_of(vol)
    assert all(np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)) for k in want)
    observed = (want["weight"] >= 1).reshape(18, 16, 32)
    field = np.where(observed, want["tsdf"].reshape(18, 16, 32), np.float32(-1.0)).astype(np.float32)
    v, t, s = mr.extract(field, lo, hi, 0.0)
    fv, ft, fs, _ = tr.filter_mesh(v, t, s, observed)
    assert len(ft) > 500 and len(ft) < len(t)
    assert np.array_equal(N_(m.vertices).view(np.uint32), fv.view(np.uint32)) and np.array_equal(N_(m.faces), ft) and np.array_equal(N_(m.src), fs)
    assert m.faces.dtype == torch.int32 and m.src.dtype == torch.int64 and m.res == res
    # attributes, through src
    rsem, rinst = tr.unpack(want["label"])
    assert sorted(m.attributes) == ["inst_label", "rgb", "sem_label"]
    assert np.array_equal(N_(m.attributes["sem_label"]), rsem[fs]) and np.array_equal(N_(m.attributes["inst_label"]), rinst[fs])
    assert np.array_equal(N_(m.attributes["rgb"]), np.rint(want["rgb"]).astype(np.uint8)[fs]) and m.attributes["rgb"].dtype == torch.uint8
    assert (rsem[fs] >= 0).mean() > 0.5
    path = str(tmp_path / "fused.ply")
    m.save_ply(path, colors=m.attributes["rgb"], labels=m.attributes["sem_label"])
    pv, pf = read_ply(path)
    assert pv.dtype.names == ("x", "y", "z", "red", "green", "blue", "label")
    assert np.array_equal(np.stack([pv["x"], pv["y"], pv["z"]], -1), fv) and np.array_equal(pf, ft)
    assert np.array_equal(np.stack([pv["red"], pv["green"], pv["blue"]], -1), N_(m.attributes["rgb"])) and np.array_equal(pv["label"], rsem[fs])
    # the vertices, splatted back into the view, land within trunc of the depth that made them, wherever both exist
    back = pointcloud.splat(cam, torch.from_numpy(c2w), m.vertices)
    both = (back["depth"] > 0) & (depth > 0)
    err = (back["depth"] - depth).abs()[both]
    print("splatted vertices: %d pixels with both depths, largest |difference| %.4f (trunc %.2f)" % (int(both.sum()), float(err.max()), trunc))
    assert int(both.sum()) > 1000 and float(err.max()) <= trunc
    # min_weight above every weight: nothing is observed, nothing is left
    none = fusion.extract(vol, min_weight=2.0)
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3) and none.attributes["rgb"].shape == (0, 3)
