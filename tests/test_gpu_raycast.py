"""Volume ray casting on an MI355X: k_tsdf_raycast (csrc/pnr_fusion.hip) and fusion.raycast against tests/_raycast_ref.py's
restatement of the rule (include/pnr.h "volume ray casting").  No tolerance on the kernel: every output array must equal
raycast32's bit pattern.  Every caller-owned array sits between canaries.  tests/test_raycast_ref.py pins the restatement on
the CPU.  (The grid is not capped -- one workgroup per four 8 x 8 tiles -- so there is no tile-stride trip to cover; the images
below run from one partial tile to several workgroups with partial tiles on both edges.)"""
import numpy as np
import pytest
import torch

import _camera_ref as cr
import _pano_ref as pr
import _raycast_ref as rr
import _tsdf_ref as tr
from panopticnerf_amd import consistency, fusion, ops, pointcloud
from panopticnerf_amd.evaluate import Evaluator
from test_gpu_tsdf import BOX, N_, camera_of, make_set, state_of

pytestmark = pytest.mark.gpu

assert BOX == rr.BOX
f32 = np.float32
GUARD = 64
NAMES = {rr.PINHOLE: "pinhole", rr.FISHEYE: "fisheye", rr.EQUIRECT: "equirect"}
KEYS = ("depth", "normal", "src", "code")
NEAR, FAR = 0.1, 100.0


class Guarded:
    """an output array filled with junk, with GUARD canary elements before and after it, in one allocation"""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape))
        self.canary, junk = (-7.25e30, 3.5e12) if dtype.is_floating_point else (0xA5, 0x5A) if dtype == torch.uint8 else (-1234567, 7654321)
        self.buf = torch.full((n + 2 * GUARD,), self.canary, dtype=dtype, device=dev)
        self.n = n
        self.view = self.buf[GUARD:GUARD + n].view(shape)
        self.view.fill_(junk)

    def intact(self):
        return bool((self.buf[:GUARD] == self.canary).all()) and bool((self.buf[GUARD + self.n:] == self.canary).all())


def outputs(dev, w, h, normal=True, src=True):
    g = {"depth": Guarded((h, w), torch.float32, dev), "code": Guarded((h, w), torch.uint8, dev)}
    if normal:
        g["normal"] = Guarded((h, w, 3), torch.float32, dev)
    if src:
        g["src"] = Guarded((h, w), torch.int32, dev)
    return g


def launch(view, lat, tsdf, weight, g, near=NEAR, far=FAR, **kw):
    m, cam, c2w, w, h = view
    ops.tsdf_raycast(NAMES[m], cam, c2w, w, h, near, far, lat[0], lat[1], tsdf, weight, g["depth"].view, g["code"].view,
                     normal=g["normal"].view if "normal" in g else None, src=g["src"].view if "src" in g else None, **kw)


def same(g, want, what=""):
    for k, gd in g.items():
        got = N_(gd.view).reshape(want[k].shape)
        assert got.dtype == want[k].dtype and np.array_equal(got.view(np.uint8), want[k].view(np.uint8)), (what, k)
        assert gd.intact(), (what, k)
    return True


def on_device(dev, lat, tsdf, weight):
    rx, ry, rz = lat[2]
    return torch.from_numpy(tsdf.reshape(rz, ry, rx)).to(dev), torch.from_numpy(weight.reshape(rz, ry, rx)).to(dev)


def check(dev, view, lat, tsdf, weight, dev_arrays=None, normal=True, src=True, near=NEAR, far=FAR, **kw):
    """launch on fresh guarded outputs and compare with raycast32; returns the restatement's result"""
    t, w = dev_arrays if dev_arrays is not None else on_device(dev, lat, tsdf, weight)
    g = outputs(dev, view[3], view[4], normal, src)
    launch(view, lat, t, w, g, near, far, **kw)
    want = rr.raycast32(view, near, far, lat, tsdf, weight, **kw)
    assert same(g, want, (view[0], view[3], view[4], lat[2], kw))
    return want


def view_of(name, c2w=None):
    m, cam, own, w, h = tr.CAMERAS[name]
    return (m, np.asarray(cam, f32), np.asarray(own if c2w is None else c2w, f32), w, h)


def sized(model, w, h, c2w):
    """a camera of `model` at any image size, looking the way of pose c2w"""
    if model == rr.PINHOLE:
        cam = (0.6 * max(w, h), 0.65 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0 + 0.25)
    elif model == rr.FISHEYE:
        s = max(w, h) / 1400.0
        xi, k1, k2, g1, g2, _, _ = cr.KITTI_FISHEYE
        cam = (xi, k1, k2, g1 * s, g2 * s, (w - 1) / 2.0, (h - 1) / 2.0)
    else:
        cam = pr.equirect_cam(w, h)
    return (model, np.asarray(cam, f32), np.asarray(c2w, f32), w, h)


# the six cameras of _tsdf_ref stand OUTSIDE the box and look at it (the equirect ones all round); three more stand inside it, and
# one looks away from it
VIEWS = {name: view_of(name) for name in tr.CAMERAS}
VIEWS.update(inside_pinhole=view_of("pinhole_a", cr.pose(0.2, -0.1, (0.5, 1.0, 5.5))),
             inside_fisheye=view_of("fisheye_a", cr.pose(-0.3, 0.1, (1.0, 0.5, 5.0))),
             inside_equirect=view_of("equirect_a", cr.pose(1.0, 0.0, (-1.0, 2.0, 6.0))),
             away=view_of("pinhole_a", cr.pose(np.pi, 0.0, (0.0, 1.2, 0.3))))


def sphere(res, box, trunc):
    lat = rr.lattice(*box, res)
    return (lat,) + rr.sphere_volume(lat, trunc)


# ------------------------------------------------------------------------------------------------ 1: lattices x cameras
@pytest.mark.parametrize("res, box, trunc", rr.LATTICES)
def test_lattices_and_cameras_bit_for_bit(dev, res, box, trunc):
    lat, tsdf, weight = sphere(res, box, trunc)
    arrays = on_device(dev, lat, tsdf, weight)
    codes = np.zeros(4, np.int64)
    for name, view in VIEWS.items():
        want = check(dev, view, lat, tsdf, weight, arrays)
        codes += np.bincount(want["code"], minlength=4)
        if name == "away":
            assert (want["code"] == rr.MISSED).all()
        if name.startswith("inside") and res == (16, 16, 16):       # (the smaller lattices' hulls do not hold these cameras)
            assert not (want["code"] == rr.MISSED).any()            # a ray from inside the lattice always meets it
    assert codes.all(), codes                                       # every code occurs on every lattice


# ------------------------------------------------------------------------------------------------ 2: images
@pytest.mark.parametrize("w, h", [(1, 1), (7, 5), (8, 8), (9, 17), (65, 3), (70, 41)])
def test_image_sizes_and_partial_tiles(dev, w, h):
    lat, tsdf, weight = sphere(*rr.LATTICES[2])
    arrays = on_device(dev, lat, tsdf, weight)
    hits = 0
    for model in (rr.PINHOLE, rr.FISHEYE, rr.EQUIRECT):
        for c2w in (tr.CAMERAS["pinhole_a"][2], cr.pose(0.2, -0.1, (0.5, 1.0, 5.5))):
            want = check(dev, sized(model, w, h, c2w), lat, tsdf, weight, arrays)
            hits += int((want["code"] == rr.HIT).sum())
    assert hits > 0


# ------------------------------------------------------------------------------------------------ 3: volumes
def test_unobserved_volume_and_garbage_where_weight_fails(dev):
    lat, tsdf, weight = sphere(*rr.LATTICES[2])
    for name in ("pinhole_a", "fisheye_b", "equirect_a", "inside_pinhole"):
        view = VIEWS[name]
        base = check(dev, view, lat, tsdf, weight)
        assert (base["code"] == rr.HIT).any()
        # nothing observed: no pixel is a hit, whatever tsdf holds
        none = check(dev, view, lat, tsdf, np.zeros_like(weight))
        assert set(np.unique(none["code"])) <= {rr.NO_RAY, rr.MISSED, rr.NO_SURFACE}
        assert np.array_equal(none["code"] == rr.NO_SURFACE, (base["code"] == rr.NO_SURFACE) | (base["code"] == rr.HIT))
        # NaN and +-Inf wherever weight is 0: the results do not change
        for junk in (np.nan, np.inf, -np.inf):
            t2 = tsdf.copy()
            t2[weight == 0] = junk
            got = check(dev, view, lat, t2, weight)
            assert all(np.array_equal(got[k].view(np.uint8), base[k].view(np.uint8)) for k in KEYS), (name, junk)
    assert (weight == 0).sum() > 100


@pytest.fixture(scope="module")
def fused(dev):
    """a volume fusion.integrate made from the six sphere frames: (volume, lattice, tsdf, weight) with the arrays copied back"""
    frames, _ = make_set(dev, [(name, {}, None) for name in tr.CAMERAS])
    vol = fusion.Volume(BOX[0], BOX[1], (16, 16, 16), dev, color=True, labels=True)
    fusion.integrate(vol, frames, 0.9)
    st = state_of(vol)
    lat = (vol.lo32, vol.step, vol.res)
    ref = rr.lattice(BOX[0], BOX[1], vol.res)
    assert np.array_equal(ref[0], lat[0]) and np.array_equal(ref[1], lat[1])
    assert st["weight"].max() >= 3 and (st["weight"] == 0).any()
    return vol, lat, st["tsdf"], st["weight"]


def test_integrated_volume_and_parameters(dev, fused):
    vol, lat, tsdf, weight = fused
    arrays = (vol.tsdf, vol.weight)
    smallest, largest = float(np.abs(lat[1]).min()), float(np.abs(lat[1]).max())
    seen = {}
    for name in ("pinhole_b", "fisheye_a", "equirect_b", "inside_pinhole"):
        view = VIEWS[name]
        for kw in ({}, {"dt": 0.25 * smallest}, {"dt": 4.0 * largest}, {"min_weight": 3.0}, {"min_weight": 6.0}, {"max_steps": 0}, {"max_steps": 1},
                   {"max_steps": 5}, {"max_steps": 5, "dt": largest}, {"min_weight": 3.0, "dt": 1.3 * largest, "max_steps": 40}):
            want = check(dev, view, lat, tsdf, weight, arrays, **kw)
            key = tuple(sorted(kw.items()))
            seen[key] = seen.get(key, 0) + int((want["code"] == rr.HIT).sum())
            if kw.get("max_steps", 2) <= 1:
                assert not (want["code"] == rr.HIT).any()
    # (the six frames leave weight 6 almost everywhere they leave any: min_weight 3 costs nothing here, 6 does)
    assert seen[()] > 500 and 0 < seen[(("min_weight", 6.0),)] < seen[(("min_weight", 3.0),)] <= seen[()]
    assert seen[(("max_steps", 5),)] < seen[()] and 0 < seen[(("dt", largest), ("max_steps", 5))] < seen[()]
    assert 0 < seen[(("dt", 4.0 * largest),)] and seen[(("dt", 0.25 * smallest),)] > 500
    # near and far cut the march short
    for near, far in ((0.0, 5.0), (5.5, 7.0), (30.0, 31.0)):
        want = check(dev, VIEWS["pinhole_a"], lat, tsdf, weight, arrays, near=near, far=far)
    assert (want["code"] == rr.MISSED).all()


def test_skipped_outputs_reruns_and_contiguity(dev, fused):
    vol, lat, tsdf, weight = fused
    arrays = (vol.tsdf, vol.weight)
    view = VIEWS["fisheye_b"]
    full = check(dev, view, lat, tsdf, weight, arrays)
    for normal, src in ((False, True), (True, False), (False, False)):
        check(dev, view, lat, tsdf, weight, arrays, normal=normal, src=src)
    # two runs give the same bits, on outputs that held the first run's values
    g = outputs(dev, view[3], view[4])
    launch(view, lat, *arrays, g)
    first = {k: gd.view.clone() for k, gd in g.items()}
    launch(view, lat, *arrays, g)
    assert all(torch.equal(first[k].view(torch.uint8), g[k].view.view(torch.uint8)) for k in g) and same(g, full)
    # contiguity and the device, by name
    with pytest.raises(ValueError, match="tsdf_raycast: depth: tensor must be contiguous"):
        ops.tsdf_raycast("fisheye", view[1], view[2], 80, 80, NEAR, FAR, lat[0], lat[1], *arrays, torch.zeros((80, 80), device=dev).t(), g["code"].view)
    with pytest.raises(ValueError, match="tsdf_raycast: tsdf: tensor must be contiguous"):
        ops.tsdf_raycast("fisheye", view[1], view[2], 80, 80, NEAR, FAR, lat[0], lat[1], vol.tsdf.transpose(0, 1), vol.weight, g["depth"].view, g["code"].view)
    with pytest.raises(RuntimeError, match="tsdf_raycast: code: expected a GPU tensor"):
        ops.tsdf_raycast("fisheye", view[1], view[2], 80, 80, NEAR, FAR, lat[0], lat[1], *arrays, g["depth"].view, torch.zeros((80, 80), dtype=torch.uint8))
    assert all(gd.intact() for gd in g.values())


def test_captured_graph_sees_what_was_integrated_since(dev):
    frames, _ = make_set(dev, [(name, {}, None) for name in tr.CAMERAS])
    vol = fusion.Volume(BOX[0], BOX[1], (16, 16, 16), dev)
    lat = (vol.lo32, vol.step, vol.res)
    view = VIEWS["inside_pinhole"]
    fusion.integrate(vol, frames, 0.9, last=1)
    g = outputs(dev, view[3], view[4])
    launch(view, lat, vol.tsdf, vol.weight, g)                      # warm call: module loading is not capturable
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch(view, lat, vol.tsdf, vol.weight, g)
    graph.replay()
    torch.cuda.synchronize()
    st = state_of(vol)
    one = rr.raycast32(view, NEAR, FAR, lat, st["tsdf"], st["weight"])
    assert same(g, one, "first replay")
    fusion.integrate(vol, frames, 0.9, first=1)
    graph.replay()
    torch.cuda.synchronize()
    st = state_of(vol)
    six = rr.raycast32(view, NEAR, FAR, lat, st["tsdf"], st["weight"])
    assert same(g, six, "after five more frames")
    assert not np.array_equal(one["depth"], six["depth"]) and (six["code"] == rr.HIT).all()


# ------------------------------------------------------------------------------------------------ 4: end to end
def _blocks(fr):
    """labels a surface can carry: constant over 12 x 8 pixel blocks"""
    h, w = fr["depth"].shape
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fr["sem"] = ((ii // 12 + 3 * (jj // 8)) % 5).astype(np.int16)
    fr["inst"] = (ii // 12 + 8 * (jj // 8)).astype(np.int16)


def _neighbour_step(depth):
    """the largest |difference| of two horizontally or vertically neighbouring pixels that both have depth"""
    best = 0.0
    for a, b in ((depth[:, 1:], depth[:, :-1]), (depth[1:], depth[:-1])):
        both = (a > 0) & (b > 0)
        best = max(best, float(np.abs(a - b)[both].max()))
    return best


def test_frames_to_volume_to_image(dev):
    """Sphere frames -> integrate -> raycast from the first frame's pose.  The bound on |depth - the frame's depth|: a hit lies
    between a sample whose cell has a negative corner and one, dt |d| further, whose cell has a corner >= 0.  A fused value has
    the sign of the point's true side of the surface unless the point is within delta of it, delta = the largest depth
    difference of neighbouring pixels (the nearest-pixel lookup) over 0.7 (a z-depth difference is the distance along the
    frame's ray times the cosine to the optical axis, 0.72 in the corners of these images); trunc = 0.9 exceeds a cell diagonal,
    so the cells of both samples are inside the band.  The distance to the surface is 1-Lipschitz, so the hit point is within
    diag + dt |d| + delta of the surface, and within that over cos(ray, normal) along the ray parameter (|d| >= 1)."""
    trunc, res = 0.9, (32, 32, 32)
    frames, refs = make_set(dev, [("pinhole_a", {"inst": True}, _blocks), ("fisheye_a", {"sem": False, "inst": False}, None),
                                  ("equirect_a", {"sem": False, "inst": False}, None)])
    vol = fusion.Volume(BOX[0], BOX[1], res, dev, color=True, labels=True)
    fusion.integrate(vol, frames, trunc)
    cam, c2w = camera_of("pinhole_a"), torch.from_numpy(refs[0]["c2w"])
    maps = fusion.raycast(vol, cam, c2w, NEAR, FAR)
    h, w = cam.height, cam.width
    assert sorted(maps) == ["code", "depth", "inst_label", "normal", "rgb", "sem_label", "src", "valid"]
    assert all(tuple(maps[k].shape[:2]) == (h, w) for k in maps) and maps["valid"].dtype == torch.bool and maps["rgb"].dtype == torch.uint8
    # the restatement on the integrated arrays, and the attributes through src
    st = state_of(vol)
    lat = (vol.lo32, vol.step, vol.res)
    view = view_of("pinhole_a", refs[0]["c2w"])
    want = rr.raycast32(view, NEAR, FAR, lat, st["tsdf"], st["weight"])
    for k in KEYS:
        assert np.array_equal(N_(maps[k]).reshape(want[k].shape).view(np.uint8), want[k].view(np.uint8)), k
    valid = want["code"] == rr.HIT
    assert np.array_equal(N_(maps["valid"]).reshape(-1), valid) and valid.sum() > 1500
    sem, inst = tr.unpack(st["label"])
    at = np.maximum(want["src"], 0)
    assert np.array_equal(N_(maps["sem_label"]).reshape(-1), np.where(valid, sem[at], -1))
    assert np.array_equal(N_(maps["inst_label"]).reshape(-1), np.where(valid, inst[at], -1))
    assert np.array_equal(N_(maps["rgb"]).reshape(-1, 3), np.where(valid[:, None], np.rint(st["rgb"]).astype(np.uint8)[at], 0))
    # depth against the frame's input depth, first on the restatement
    d_in = refs[0]["depth"].reshape(-1).astype(np.float64)
    delta = max(_neighbour_step(fr["depth"]) for fr in refs) / 0.7
    o, d, _ = pr._rays(np.float32, view, np.arange(w * h))
    X = o + d_in[:, None] * d
    nrm = (X - np.asarray(tr.SPHERE[0])) / tr.SPHERE[1]
    cos = (d * nrm).sum(-1) / np.sqrt((d * d).sum(-1))
    norm_d = np.sqrt((d * d).sum(-1))
    bound = (float(np.sqrt((lat[1] ** 2).sum())) + float(rr.default_dt(lat[1])) * norm_d + delta) / cos
    err_ref = np.abs(want["depth"].astype(np.float64) - d_in)
    err = np.abs(N_(maps["depth"]).reshape(-1).astype(np.float64) - d_in)
    print("ray-cast depth against the frame's: %d valid pixels, largest |difference| %.4f, smallest bound %.3f" % (valid.sum(), err[valid].max(), bound[valid].min()))
    assert (err_ref[valid] <= bound[valid]).all() and (err[valid] <= bound[valid]).all()
    # the labels of the frame come back in its own view on at least the share the restatement reaches
    share_ref = (np.where(valid, sem[at], -1) == refs[0]["sem"].reshape(-1))[valid].mean()
    share = (N_(maps["sem_label"]).reshape(-1) == refs[0]["sem"].reshape(-1))[valid].mean()
    print("sem_label equals the frame's label on %.1f %% of the valid pixels" % (100.0 * share))
    assert share >= share_ref > 0.7
    # the result is a view: reprojection against a render_view-shaped view, lifting, and the depth metrics
    other = (camera_of("pinhole_b"), torch.from_numpy(np.asarray(tr.CAMERAS["pinhole_b"][2], f32)),
             {"depth_0": torch.zeros(64, 96, device=dev), "depth_1": torch.from_numpy(tr.sphere_frame("pinhole_b")["depth"]).to(dev)})
    match = consistency.reproject((cam, c2w, maps), other)
    assert tuple(match.shape) == (h, w) and int((match >= 0).sum()) > 500
    back = consistency.reproject(other, (cam, c2w, maps))
    assert int((back >= 0).sum()) > 500
    points, pix = pointcloud.lift((cam, c2w, maps))
    assert points.shape[0] == int(valid.sum()) and np.array_equal(N_(pix), np.nonzero(valid)[0])
    radius = np.linalg.norm(N_(points).astype(np.float64) - np.asarray(tr.SPHERE[0]), axis=1)
    assert np.abs(radius - tr.SPHERE[1]).max() <= bound[valid].max()
    ev = Evaluator()
    assert ev.evaluate_depth(maps, torch.from_numpy(refs[0]["depth"]).to(dev), valid=maps["valid"]) == "depth"
    got = ev.summarize()
    assert got["depth_n"] == int(valid.sum()) and got["depth_mae"] <= bound[valid].max()
    # without normals and attributes
    bare = fusion.raycast(vol, cam, c2w, NEAR, FAR, normals=False, attributes=False)
    assert sorted(bare) == ["code", "depth", "src", "valid"] and torch.equal(bare["depth"], maps["depth"]) and torch.equal(bare["src"], maps["src"])
    plain = fusion.raycast(fusion.Volume(BOX[0], BOX[1], 4, dev), cam, c2w, NEAR, FAR)
    assert sorted(plain) == ["code", "depth", "normal", "src", "valid"] and not plain["valid"].any()
