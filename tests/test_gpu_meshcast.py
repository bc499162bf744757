"""Mesh ray casting on an MI355X: k_mesh_cast and the index kernels (csrc/pnr_meshcast.hip), mesh.RayIndex, mesh.raycast and
mesh.cast_rays against tests/_meshcast_ref.py's brute-force restatement of the rule (include/pnr.h "mesh ray casting").  No
tolerance on the kernels: every output array equals the restatement's bit pattern, at every index resolution.  Every
caller-owned array sits between canaries.  tests/test_meshcast_ref.py pins the restatement and the walk on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _camera_ref as cr
import _icp_ref as ir
import _meshcast_ref as mc
from panopticnerf_amd import Equirect, Fisheye, Pinhole, consistency, fusion, mesh, ops, pointcloud, synthetic
from panopticnerf_amd.evaluate import Evaluator
from test_meshcast_ref import REL_DEPTH_ERR, SPAN_DEPTH_ERR, close_wall_exact, span_error

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64
W, H = 70, 45                       # 8 x 8 tiles partial on both edges, three workgroups
NEAR, FAR = 0.05, 100.0
N_ = lambda t: t.detach().cpu().numpy()
DEV = torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Guarded:
    """an output array filled with junk, with GUARD canary elements before and after it, in one allocation"""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape))
        self.canary, junk = (-7.25e30, 3.5e12) if dtype.is_floating_point else (0x55, 0x2A) if dtype in (torch.uint8, torch.int8) else (-1234567, 7654321)
        self.buf = torch.full((n + 2 * GUARD,), self.canary, dtype=dtype, device=dev)
        self.n = n
        self.view = self.buf[GUARD:GUARD + n].view(shape)
        self.view.fill_(junk)

    def intact(self):
        return bool((self.buf[:GUARD] == self.canary).all()) and bool((self.buf[GUARD + self.n:] == self.canary).all())


def guarded_outputs(dev, lead, keys=mc.KEYS):
    return {n: Guarded(lead + tail, dt, dev) for n, dt, tail in ops.MESHCAST_OUTPUTS if n in keys}


def same(g, want, what=""):
    for k, gd in g.items():
        got = N_(gd.view).reshape(want[k].shape)
        assert got.dtype == want[k].dtype, (what, k, got.dtype)
        assert np.array_equal(bits(got), bits(want[k])), (what, k, int((got != want[k]).sum()))
        assert gd.intact(), (what, k)
    return True


def camera_of(model, w=W, h=H):
    if model == "pinhole":
        return Pinhole(0.6 * w, 0.65 * w, (w - 1) / 2.0, (h - 1) / 2.0 + 0.25, w, h)
    if model == "fisheye":
        xi, k1, k2, g1, g2, _, _ = cr.KITTI_FISHEYE
        s = max(w, h) / 1400.0
        return Fisheye(xi, k1, k2, g1 * s, g2 * s, (w - 1) / 2.0, (h - 1) / 2.0, w, h)
    return Equirect(w, h)


def view_of(cam, c2w):
    return (cam.word, np.asarray(cam.params, f32), np.asarray(c2w, f32), cam.width, cam.height)


OUTSIDE = np.asarray(cr.pose(0.1, -0.05, (0.2, -0.1, -2.5)), f32)
INSIDE_ROOM = np.asarray(ir.TRUE_POSE, f32)
LATTICE = ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(mesh on the GPU, vertices, faces as numpy, the pose its cameras stand at)"""
    if name == "box":
        m, pose = synthetic.box_mesh(*ir.ROOM, device=DEV), INSIDE_ROOM
    elif name in ("sphere", "torus", "torus32"):
        kind, res = name.rstrip("32"), 32 if name.endswith("32") else 16
        m, pose = mesh.extract(synthetic.sdf_grid(kind, *LATTICE, res, device=DEV), *LATTICE, 0.0), OUTSIDE
    else:
        V, F = mc.soup()
        m, pose = mesh.Mesh.from_arrays(V, F, device=DEV), OUTSIDE
    return m, N_(m.vertices), N_(m.faces), pose


@functools.lru_cache(maxsize=None)
def index_of(name, res):
    return mesh.RayIndex(scene(name)[0], res)


@functools.lru_cache(maxsize=None)
def reference(name, model):
    """the brute-force restatement of scene `name` in camera `model`, computed once and shared"""
    _, V, F, pose = scene(name)
    rays, ok = mc.camera_rays(view_of(camera_of(model), pose), NEAR, FAR)
    return mc.cast(rays, V, F, ok)


def launch(name, model, idx, g):
    m, _, _, pose = scene(name)
    cam = camera_of(model)
    ops.mesh_raycast(cam.model, cam.params, torch.from_numpy(pose), cam.width, cam.height, NEAR, FAR, m.vertices, m.faces, idx.res, idx.lo, idx.cell,
                     idx.start, idx.records, {k: gd.view for k, gd in g.items()})


# ------------------------------------------------------------------------------------------------ 1: bit for bit
@pytest.mark.parametrize("name", ["box", "sphere", "torus", "soup"])
@pytest.mark.parametrize("res", [(1, 1, 1), (2, 3, 5), None])
@pytest.mark.parametrize("model", ["pinhole", "fisheye", "equirect"])
def test_every_output_bit_for_bit(dev, model, res, name):
    m, V, F, _ = scene(name)
    assert 12 <= len(F) <= 3200
    idx = index_of(name, res)
    assert res is None or idx.res == res
    g = guarded_outputs(dev, (H, W))
    launch(name, model, idx, g)
    want = reference(name, model)
    assert same(g, want, (name, model, idx.res))
    codes = set(np.unique(want["code"]))
    assert mc.HIT in codes and (model != "fisheye" or mc.NO_RAY in codes) and (name == "box" or mc.MISSED in codes)
    if name == "box":
        assert not (want["code"] == mc.MISSED).any()                # from inside a closed room every ray hits


def test_soup_edge_cases_are_in_the_reference():
    """the soup's duplicated faces, zero-area faces, NaN corner and out-of-range index do what the rule says"""
    _, V, F, _ = scene("soup")
    use = mc.usable_faces(V, F)
    assert not use[7] and not use[8] and use[:7].all() and np.array_equal(F[0], F[1]) and np.array_equal(F[0], F[3])
    centre = V[F[0]].astype(np.float64).mean(0).astype(f32)
    rays = mc.rays_to((0.0, 0.0, -3.0), centre[None])
    keys = mc.face_times(rays, V, F)[0]
    assert keys[0] != mc.EMPTY and (keys[0] >> np.uint64(32)) == (keys[1] >> np.uint64(32)) == (keys[3] >> np.uint64(32))
    out = mc.cast(np.concatenate([rays, mc.rays_to((0.0, 0.0, -3.0), V[F[7, 0]][None])]), V, F)
    assert out["face"][0] not in (1, 3, 4, 5, 6, 7, 8) and out["face"][1] not in (7, 8)
    assert not (mc.face_times(rays, V, F)[:, 4:9] != mc.EMPTY).any()


def test_skipped_outputs_and_reruns(dev):
    idx = index_of("sphere", None)
    want = reference("sphere", "fisheye")
    for keys in (("depth", "face", "code"), ("depth", "face", "code", "vertex"), ("depth", "face", "code", "normal", "side")):
        g = guarded_outputs(dev, (H, W), keys)
        launch("sphere", "fisheye", idx, g)
        assert same(g, want, keys)
    g = guarded_outputs(dev, (H, W))
    launch("sphere", "fisheye", idx, g)
    launch("sphere", "fisheye", idx, g)                             # on outputs that held the first run's values
    assert same(g, want, "second run")


# ------------------------------------------------------------------------------------------------ 2: the index only prunes
def test_index_independence(dev):
    """the torus at 32^3 at five resolutions, and from a far origin through the walk and through the plain loop: identical arrays"""
    m, V, F, pose = scene("torus32")
    cam = camera_of("pinhole", 48, 32)
    got = []
    for res in ((1, 1, 1), (7, 7, 2), (16, 16, 16), None, (1, 1, 1024)):
        idx = mesh.RayIndex(m, res)
        maps = mesh.raycast(m, cam, torch.from_numpy(pose), NEAR, FAR, index=idx)
        got.append({k: N_(maps[k]) for k in mc.KEYS})
    assert (got[0]["code"] == mc.HIT).sum() > 50 and (got[0]["code"] == mc.MISSED).sum() > 50
    for other in got[1:]:
        for k in mc.KEYS:
            assert np.array_equal(bits(got[0][k]), bits(other[k])), k
    # a far origin: within reach of a coarse grid (the walk), beyond the reach of a fine one (the plain loop)
    far = mc.rays_to((30.0, -12.0, 38.0), mc.edge_targets(V, F)[::7], NEAR, 1e4)
    lists = []
    for res, walks in (((12, 12, 4), True), ((220, 220, 60), False)):
        idx = mesh.RayIndex(m, res)
        assert mc.within_reach(far[0, :3], mc.make_grid(idx.res, idx.lo, idx.cell)) == walks
        out = mesh.cast_rays(m, torch.from_numpy(far).to(dev), index=idx)
        lists.append({k: N_(out[k]) for k in mc.KEYS})
    assert (lists[0]["code"] == mc.HIT).sum() > len(far) // 2
    for k in mc.KEYS:
        assert np.array_equal(bits(lists[0][k]), bits(lists[1][k])), k
    # and they are the restatement's on the rows that cross the torus
    rays, ok = mc.camera_rays(view_of(cam, pose), NEAR, FAR)
    rows = slice(12 * 48, 20 * 48)
    want = mc.cast(rays[rows], V, F, ok[rows])
    for k in mc.KEYS:
        assert np.array_equal(bits(got[0][k].reshape((-1,) + want[k].shape[1:])[rows]), bits(want[k])), k


@pytest.mark.parametrize("res", [(1, 1, 1), (8, 8, 8), (32, 32, 32), (64, 64, 64), (100, 30, 20), None])
def test_grazing_rays_bit_for_bit(dev, res):
    """rays in the plane of faces much larger than a cell, whose t is cancellation noise (mc.grazing_cases: without the rule's box
    test an index finer than the faces loses the plain loop's winner there): every array equals brute force's at every resolution"""
    V, F, rays = mc.grazing_scene()
    m = mesh.Mesh.from_arrays(V, F, device=dev)
    idx = mesh.RayIndex(m, res)
    g = guarded_outputs(dev, (len(rays),))
    ops.mesh_cast_rays(torch.from_numpy(rays).to(dev), m.vertices, m.faces, idx.res, idx.lo, idx.cell, idx.start, idx.records,
                       {k: gd.view for k, gd in g.items()})
    want = grazing_reference()
    assert same(g, want, idx.res) and (want["code"] == mc.HIT).sum() >= len(rays) // 2


@functools.lru_cache(maxsize=None)
def grazing_reference():
    V, F, rays = mc.grazing_scene()
    return mc.cast(rays, V, F)


@pytest.mark.parametrize("case", range(5))
def test_no_holes_next_to_large_faces(dev, case):
    """a camera 1 cm or 5 cm from a wall, or low above a floor, far larger than that distance (mc.close_wall_views): no ray falls
    through, every array is brute force's at the default and at a fine resolution, the depth within the CPU test's bound"""
    name, V, F, rays, ok = mc.close_wall_views()[case]
    rays = np.where(ok[:, None], rays, 0).astype(f32)                # (a pixel that is no ray: d = 0, as the camera's own rays have it)
    m = mesh.Mesh.from_arrays(V, F, device=dev)
    want = mc.cast(rays, V, F)
    for res in (None, (24, 24, 24)):
        idx = mesh.RayIndex(m, res)
        g = guarded_outputs(dev, (len(rays),))
        ops.mesh_cast_rays(torch.from_numpy(rays).to(dev), m.vertices, m.faces, idx.res, idx.lo, idx.cell, idx.start, idx.records,
                           {k: gd.view for k, gd in g.items()})
        assert bool((g["code"].view == mc.HIT).all()), "%s: %d rays fell through" % (name, int((g["code"].view != mc.HIT).sum()))
        assert same(g, want, (name, idx.res))
        got = {"depth": N_(g["depth"].view), "face": N_(g["face"].view)}
        assert span_error(got, V, F, rays, close_wall_exact(name, V, rays)).max() <= SPAN_DEPTH_ERR


# ------------------------------------------------------------------------------------------------ 3: watertight
@pytest.mark.parametrize("origin", [(0.03, -0.02, 0.05), (0.0, 0.0, 0.0)])
def test_edge_aimed_rays_all_hit(dev, origin):
    ico = synthetic.icosphere(2, device=dev)
    V, F = N_(ico.vertices), N_(ico.faces)
    rays = mc.rays_to(origin, mc.edge_targets(V, F))
    idx = mesh.RayIndex(ico)
    g = guarded_outputs(dev, (len(rays),))
    ops.mesh_cast_rays(torch.from_numpy(rays).to(dev), ico.vertices, ico.faces, idx.res, idx.lo, idx.cell, idx.start, idx.records,
                       {k: gd.view for k, gd in g.items()})
    assert bool((g["code"].view == mc.HIT).all()), "a ray through an edge or a vertex fell through the mesh"
    assert same(g, mc.cast(rays, V, F))


def test_panorama_from_inside_a_closed_mesh_is_valid_everywhere(dev):
    ico = synthetic.icosphere(3, radius=2.0, center=(0.3, -0.2, 0.1), device=dev)
    maps = mesh.raycast(ico, Equirect(64, 32), torch.from_numpy(np.asarray(cr.pose(0.4, 0.2, (0.5, 0.1, -0.3)), f32)), 0.0, 50.0)
    assert bool(maps["valid"].all()) and bool((maps["side"] == -1).all())
    assert float((maps["normal"].norm(dim=-1) - 1).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ 4: two ray sources, one body
@pytest.mark.parametrize("model", ["pinhole", "fisheye", "equirect"])
def test_raycast_equals_cast_rays_of_the_cameras_rays(dev, model):
    m, _, _, pose = scene("torus")
    cam, c2w = camera_of(model), torch.from_numpy(pose)
    idx = index_of("torus", None)
    img = mesh.raycast(m, cam, c2w, NEAR, FAR, index=idx)
    lst = mesh.cast_rays(m, cam.rays(c2w, NEAR, FAR, device=dev), index=idx)
    assert sorted(img) == sorted(lst) == sorted(mc.KEYS + ("valid",))
    for k in img:
        assert tuple(img[k].shape[:2]) == (H, W) and torch.equal(img[k].reshape(lst[k].shape).view(torch.uint8), lst[k].view(torch.uint8)), k
    no_ray = N_(img["code"]).reshape(-1) == mc.NO_RAY
    assert np.array_equal(no_ray, reference("torus", model)["code"] == mc.NO_RAY) and (model == "fisheye") == bool(no_ray.any())


def test_bad_rays_are_no_rays_and_empty_inputs_are_no_ops(dev):
    m = scene("box")[0]
    idx = index_of("box", None)
    good = [0.1, 0.0, 0.2, 0.0, 0.0, 1.0, 0.0, 50.0]
    rows = [good]
    for col, v in ((0, np.nan), (4, np.inf), (6, -1.0), (6, np.nan), (7, np.nan), (6, 60.0)):
        r = list(good)
        r[col] = v
        rows.append(r)
    rows.append([0.1, 0.0, 0.2, 0.0, 0.0, 0.0, 0.0, 50.0])
    rows.append(good[:7] + [np.inf])
    rays = np.asarray(rows, f32)
    out = mesh.cast_rays(m, torch.from_numpy(rays).to(dev), index=idx)
    assert N_(out["code"]).tolist() == [mc.HIT] + [mc.NO_RAY] * 7 + [mc.HIT]
    want = mc.cast(rays, N_(m.vertices), N_(m.faces))
    for k in mc.KEYS:
        assert np.array_equal(bits(N_(out[k])), bits(want[k])), k
    none = mesh.cast_rays(m, torch.zeros((0, 8), device=dev), index=idx)
    assert all(v.shape[0] == 0 for v in none.values())
    empty = mesh.Mesh.from_arrays(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), device=dev)
    eidx = mesh.RayIndex(empty)
    assert eidx.res == (1, 1, 1) and eidx.records.shape[0] == 0
    img = mesh.raycast(empty, camera_of("pinhole"), torch.from_numpy(OUTSIDE), NEAR, FAR, index=eidx)
    assert bool((img["code"] == mc.MISSED).all()) and bool((img["face"] == -1).all()) and not bool(img["depth"].any())
    with pytest.raises(ValueError, match="mesh.raycast: index was built for a mesh of 0 vertices and 0 faces, this one has 8 and 12"):
        mesh.raycast(m, camera_of("pinhole"), torch.from_numpy(OUTSIDE), NEAR, FAR, index=eidx)


# ------------------------------------------------------------------------------------------------ 5: capture
def test_captured_cast_follows_the_ray_tensor(dev):
    m, V, F, _ = scene("sphere")
    idx = index_of("sphere", None)
    first = mc.rays_to((0.2, -0.1, -2.5), mc.edge_targets(V, F)[:1500], NEAR, FAR)
    second = mc.rays_to((-2.0, 0.4, 0.3), mc.edge_targets(V, F)[1500:3000], NEAR, FAR)
    rays = torch.from_numpy(first).to(dev)
    mesh.cast_rays(m, rays, index=idx)                               # warm call: module loading is not capturable
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = mesh.cast_rays(m, rays, index=idx)
    graph.replay()
    torch.cuda.synchronize()
    want = mc.cast(first, V, F)
    assert all(np.array_equal(bits(N_(out[k])), bits(want[k])) for k in mc.KEYS)
    rays.copy_(torch.from_numpy(second).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    eager = mesh.cast_rays(m, rays, index=idx)
    want = mc.cast(second, V, F)
    assert all(torch.equal(out[k].view(torch.uint8), eager[k].view(torch.uint8)) for k in out)
    assert all(np.array_equal(bits(N_(out[k])), bits(want[k])) for k in mc.KEYS)
    assert not np.array_equal(mc.cast(first, V, F)["depth"], want["depth"])


# ------------------------------------------------------------------------------------------------ 6: it closes loops
@pytest.mark.parametrize("model", ["pinhole", "fisheye", "equirect"])
def test_depth_metrics_of_the_box_view_against_room_depth(dev, model):
    cam, c2w = ir.cameras()[model], torch.from_numpy(INSIDE_ROOM)
    box = scene("box")[0]
    maps = mesh.raycast(box, cam, c2w, 0.0, 100.0)
    depth, normal = ir.room_maps(cam, INSIDE_ROOM)
    gt = torch.from_numpy(depth).to(dev)
    assert torch.equal(maps["valid"], gt > 0)
    ev = Evaluator()
    assert ev.evaluate_depth(maps, gt, valid=maps["valid"]) == "depth"
    got = ev.summarize()
    print("%s: abs_rel %.3e over %d pixels" % (model, got["depth_abs_rel"], got["depth_n"]))
    assert got["depth_n"] == int(maps["valid"].sum()) and got["depth_abs_rel"] <= REL_DEPTH_ERR
    rel = ((maps["depth"] - gt).abs() / gt.clamp(min=1e-9))[maps["valid"]]
    assert float(rel.max()) <= REL_DEPTH_ERR
    assert torch.equal(maps["normal"], torch.from_numpy(normal).to(dev))
    # the view lifts and reprojects like any other
    points, pix = pointcloud.lift((cam, c2w, maps))
    assert points.shape[0] == int(maps["valid"].sum())
    match = consistency.reproject((cam, c2w, maps), (cam, c2w, {"depth": gt}))
    assert int((match >= 0).sum()) > 0.9 * int(maps["valid"].sum())


@pytest.mark.parametrize("ln,mn", [("pinhole", "pinhole"), ("fisheye", "equirect"), ("equirect", "fisheye")])
def test_track_against_the_mesh_view(dev, ln, mn):
    """fusion.track of a room_depth frame from a perturbed pose against the mesh view of the room: the final pose lies within the
    bound tests/test_gpu_icp.py uses for the analytic model view of the same room (4 x the float64 restatement's own error +
    1e-5) -- the tighter of that file's two: its bound for the TSDF ray-cast view adds an eighth of a lattice cell, and a mesh
    has no lattice -- with every iteration ICP_OK as in that file's loop"""
    import test_gpu_icp as ti
    lcam, mcam = ir.cameras()[ln], ir.cameras(0.75)[mn]
    dl, _ = ir.room_maps(lcam, ti.TRUTH)
    dm, nm = ir.room_maps(mcam, ir.MODEL_POSE)
    pose_m = torch.as_tensor(np.asarray(ir.MODEL_POSE, f32))
    maps = mesh.raycast(scene("box")[0], mcam, pose_m, 0.0, 100.0)
    c2w, info = fusion.track((mcam, pose_m, maps), lcam, torch.as_tensor(dl).to(dev), torch.as_tensor(ti.GUESS.reshape(3, 4)), iters=10,
                             dist_max=ti.DIST_MAX, **ti.SOLVE_ARGS)
    torch.cuda.synchronize()
    hist = N_(info["history"])
    assert np.all(hist[:, 4] == fusion.ICP_OK), hist
    p64, _, _, _ = ir.track(ir.live_of(lcam), dl, ti.GUESS, ir.model_of(mcam, ir.MODEL_POSE), dm, nm, 10, ti.DIST_MAX, f=np.float64,
                            w2c=ti.w2c_of(ir.MODEL_POSE), **ti.SOLVE_ARGS)
    e, e64 = ir.pose_error(N_(c2w).reshape(12), ti.TRUTH), ir.pose_error(p64, ti.TRUTH)
    print("%s -> mesh view in %s: final error %s, the float64 restatement's on the analytic view %s" % (ln, mn, e, e64))
    assert e[0] <= 4.0 * e64[0] + 1e-5 and e[1] <= 4.0 * e64[1] + 1e-5


def test_vertex_attributes_arrive_in_the_image(dev):
    m, V, F, pose = scene("sphere")
    n = len(V)
    lab = torch.arange(n, device=dev, dtype=torch.int32) % 7
    inst = (torch.arange(n, device=dev, dtype=torch.int64) * 31) % 1000
    rgb = torch.stack([torch.arange(n, device=dev) % 251, torch.arange(n, device=dev) % 13, torch.arange(n, device=dev) % 101], 1).to(torch.uint8)
    lm = mesh.Mesh.from_arrays(m.vertices, m.faces, {"sem_label": lab, "inst_label": inst, "rgb": rgb})
    maps = mesh.raycast(lm, camera_of("pinhole"), torch.from_numpy(pose), NEAR, FAR, index=index_of("sphere", None))
    want = reference("sphere", "pinhole")
    valid, at = want["code"] == mc.HIT, np.maximum(want["vertex"], 0)
    assert valid.sum() > 300 and np.array_equal(N_(maps["vertex"]).reshape(-1), want["vertex"])
    assert maps["sem_label"].dtype == torch.int32 and maps["inst_label"].dtype == torch.int64 and maps["rgb"].dtype == torch.uint8
    assert np.array_equal(N_(maps["sem_label"]).reshape(-1), np.where(valid, N_(lab)[at], -1))
    assert np.array_equal(N_(maps["inst_label"]).reshape(-1), np.where(valid, N_(inst)[at], -1))
    assert np.array_equal(N_(maps["rgb"]).reshape(-1, 3), np.where(valid[:, None], N_(rgb)[at], 0))
    # the nearest corner is a corner of the face hit, and the one with the largest weight
    f, b = want["face"][valid], want["bary"][valid]
    assert (F[f, np.argmax(b, 1)] == want["vertex"][valid]).all()
    bare = mesh.raycast(lm, camera_of("pinhole"), torch.from_numpy(pose), NEAR, FAR, index=index_of("sphere", None), normals=False, attributes=False)
    assert sorted(bare) == sorted(k for k in mc.KEYS + ("valid",) if k != "normal")
