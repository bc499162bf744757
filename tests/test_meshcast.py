"""CPU tests of mesh ray casting's front ends: the entry points of include/pnr.h "mesh ray casting" refuse bad arguments with
PNR_EINVAL and a message that names the argument BEFORE any launch (non-null pointers that are never dereferenced), the ops and
mesh.raycast / cast_rays refuse in their own names before they ask for the stream (tests/_fake_gpu.py's tensors), empty inputs
are no-ops, and the host code -- Mesh.from_arrays, synthetic.icosphere / box_mesh, the default grid -- does what it says.
Nothing here touches a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from panopticnerf_amd import Pinhole, _lib, mesh, ops, synthetic

from _fake_gpu import cpu, z, zt

f32, i32, i8, u8 = torch.float32, torch.int32, torch.int8, torch.uint8
H, W = 12, 16
PIN = (50.0, 50.0, 8.0, 6.0)
EYE = torch.eye(4)[:3]
NV, NF, NE = 8, 12, 30
RES = (2, 3, 5)
CELLS = 30


# ------------------------------------------------------------------------------------------------ the C ABI
def _c(*v):
    return (ctypes.c_float * len(v))(*v)


one = ctypes.c_void_p(64)            # non-null, 16-byte aligned, never dereferenced: validation fails first
odd = ctypes.c_void_p(66)
null = ctypes.c_void_p(0)
LO, CELL, CAM, POSE = _c(0.0, 0.0, 0.0), _c(0.5, 0.5, 0.5), _c(*PIN), _c(*([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]))


def _raycast(**kw):
    a = dict(model=0, cam=CAM, c2w=POSE, width=W, height=H, near=0.1, far=5.0, vertices=one, nv=NV, faces=one, nf=NF, rx=2, ry=3, rz=5, lo=LO,
             cell=CELL, start=one, records=one, ne=NE, depth=one, face=one, code=one, bary=one, vertex=one, normal=one, side=one)
    a.update(kw)
    return _lib.load().pnr_mesh_raycast(a["model"], a["cam"], a["c2w"], a["width"], a["height"], a["near"], a["far"], a["vertices"], a["nv"],
                                        a["faces"], a["nf"], a["rx"], a["ry"], a["rz"], a["lo"], a["cell"], a["start"], a["records"], a["ne"],
                                        a["depth"], a["face"], a["code"], a["bary"], a["vertex"], a["normal"], a["side"], null)


def _cast_rays(**kw):
    a = dict(rays=one, n=4, vertices=one, nv=NV, faces=one, nf=NF, rx=2, ry=3, rz=5, lo=LO, cell=CELL, start=one, records=one, ne=NE, depth=one,
             face=one, code=one, bary=null, vertex=null, normal=null, side=null)
    a.update(kw)
    return _lib.load().pnr_mesh_cast_rays(a["rays"], a["n"], a["vertices"], a["nv"], a["faces"], a["nf"], a["rx"], a["ry"], a["rz"], a["lo"], a["cell"],
                                          a["start"], a["records"], a["ne"], a["depth"], a["face"], a["code"], a["bary"], a["vertex"], a["normal"],
                                          a["side"], null)


def _count(**kw):
    a = dict(vertices=one, nv=NV, faces=one, nf=NF, rx=2, ry=3, rz=5, lo=LO, cell=CELL, start=one, total=one, ws=one)
    a.update(kw)
    return _lib.load().pnr_mesh_grid_count(a["vertices"], a["nv"], a["faces"], a["nf"], a["rx"], a["ry"], a["rz"], a["lo"], a["cell"], a["start"],
                                           a["total"], a["ws"], null)


def _fill(**kw):
    a = dict(vertices=one, nv=NV, faces=one, nf=NF, rx=2, ry=3, rz=5, lo=LO, cell=CELL, start=one, ne=NE, records=one, ws=one)
    a.update(kw)
    return _lib.load().pnr_mesh_grid_fill(a["vertices"], a["nv"], a["faces"], a["nf"], a["rx"], a["ry"], a["rz"], a["lo"], a["cell"], a["start"],
                                          a["ne"], a["records"], a["ws"], null)


def _bounds(**kw):
    a = dict(vertices=one, nv=NV, faces=one, nf=NF, bounds=one, ws=one)
    a.update(kw)
    return _lib.load().pnr_mesh_grid_bounds(a["vertices"], a["nv"], a["faces"], a["nf"], a["bounds"], a["ws"], null)


INF, NAN, BIG = float("inf"), float("nan"), 2 ** 31

MESH_AND_GRID = [
    (dict(nv=-1), "n_vertices must be within 0 .. 2^31 - 1"),
    (dict(nv=BIG), "n_vertices must be within 0 .. 2^31 - 1"),
    (dict(nf=-1), "n_faces must be within 0 .. 2^31 - 1"),
    (dict(nf=BIG), "n_faces must be within 0 .. 2^31 - 1"),
    (dict(faces=null), "null faces"),
    (dict(vertices=null), "null vertices"),
    (dict(vertices=odd), "vertices and faces must be 4-byte aligned"),
    (dict(faces=odd), "vertices and faces must be 4-byte aligned"),
]
GRID = [
    (dict(rx=0), "bad grid 0 x 3 x 5 (every res within 1 .. 1024)"),
    (dict(rz=1025), "bad grid 2 x 3 x 1025 (every res within 1 .. 1024)"),
    (dict(lo=None), "null lo_host or cell_host"),
    (dict(cell=None), "null lo_host or cell_host"),
    (dict(lo=_c(0.0, NAN, 0.0)), "lo must be finite (axis 1)"),
    (dict(lo=_c(0.0, 0.0, -INF)), "lo must be finite (axis 2)"),
    (dict(cell=_c(0.0, 0.5, 0.5)), "cell must be positive and finite, with a finite inverse (axis 0"),
    (dict(cell=_c(0.5, INF, 0.5)), "cell must be positive and finite, with a finite inverse (axis 1"),
    (dict(cell=_c(0.5, 0.5, NAN)), "cell must be positive and finite, with a finite inverse (axis 2"),
    (dict(cell=_c(0.5, 1e-39, 0.5)), "cell must be positive and finite, with a finite inverse (axis 1"),
]
CAST = [
    (dict(ne=-1), "n_entries must be within 0 .. 2^31 - 1"),
    (dict(ne=BIG), "n_entries must be within 0 .. 2^31 - 1"),
    (dict(start=null), "null start"),
    (dict(records=null), "null records"),
    (dict(start=odd), "start must be 4-byte and records 16-byte aligned"),
    (dict(records=ctypes.c_void_p(72)), "start must be 4-byte and records 16-byte aligned"),
    (dict(depth=null), "null depth, face or code"),
    (dict(face=null), "null depth, face or code"),
    (dict(code=null), "null depth, face or code"),
    (dict(depth=odd), "misaligned array (depth, face, bary, vertex, normal: 4 bytes)"),
    (dict(normal=odd), "misaligned array (depth, face, bary, vertex, normal: 4 bytes)"),
]
IMAGE = [
    (dict(model=2), "unknown camera model 2"),
    (dict(model=7), "unknown camera model 7"),
    (dict(cam=None), "null camera or pose (cam_host, c2w12_host)"),
    (dict(c2w=None), "null camera or pose (cam_host, c2w12_host)"),
    (dict(width=0), "bad image 0 x 12"),
    (dict(width=65536, height=65536), "bad image 65536 x 65536"),
    (dict(cam=_c(0.0, 50.0, 8.0, 6.0)), "zero focal length or gamma"),
    (dict(model=3, cam=_c(0.0, 1.0, -0.5, 1.0 / 12)), "equirect longitudes span more than a full circle"),
    (dict(near=-0.5), "need 0 <= near < far"),
    (dict(near=NAN), "need 0 <= near < far"),
    (dict(far=0.1), "need 0 <= near < far"),
    (dict(far=NAN), "need 0 <= near < far"),
]
RAYS = [
    (dict(n=-1), "n_rays must be within 0 .. 2^31 - 1"),
    (dict(n=BIG), "n_rays must be within 0 .. 2^31 - 1"),
    (dict(rays=null), "rays must be non-null and 16-byte aligned"),
    (dict(rays=ctypes.c_void_p(68)), "rays must be non-null and 16-byte aligned"),
]


def _refused(call, who, cases):
    lib = _lib.load()
    for kw, msg in cases:
        assert call(**kw) == -1, (who, kw)
        err = lib.pnr_last_error().decode()
        assert err.startswith(who + ": ") and msg in err, (who, kw, err)


def test_entry_points_refuse_before_any_launch():
    _refused(_raycast, "pnr_mesh_raycast", IMAGE + MESH_AND_GRID + GRID + CAST)
    _refused(_cast_rays, "pnr_mesh_cast_rays", RAYS + MESH_AND_GRID + GRID + CAST)
    _refused(_count, "pnr_mesh_grid_count", MESH_AND_GRID + GRID + [
        (dict(start=null), "null start, total or workspace"), (dict(total=null), "null start, total or workspace"),
        (dict(ws=null), "null start, total or workspace"), (dict(total=ctypes.c_void_p(68)), "total and workspace 8-byte aligned")])
    _refused(_fill, "pnr_mesh_grid_fill", MESH_AND_GRID + GRID + [
        (dict(ne=-1), "n_entries must be within 0 .. 2^31 - 1 (got -1)"), (dict(ne=BIG), "n_entries must be within 0 .. 2^31 - 1 (got 2147483648)"),
        (dict(start=null), "null start, records or workspace"), (dict(records=null), "null start, records or workspace"),
        (dict(records=ctypes.c_void_p(72)), "records 16-byte and workspace 8-byte aligned")])
    _refused(_bounds, "pnr_mesh_grid_bounds", MESH_AND_GRID + [
        (dict(bounds=null), "null bounds or workspace"), (dict(ws=null), "null bounds or workspace"), (dict(ws=ctypes.c_void_p(68)), "workspace 8-byte aligned")])
    lib = _lib.load()
    assert lib.pnr_mesh_grid_workspace_bytes(0, 1, 1) == -1 and lib.pnr_mesh_grid_workspace_bytes(1, 1, 1025) == -1
    for res in ((1, 1, 1), (2, 3, 5), (37, 5, 11), (1024, 1024, 1)):
        cells = res[0] * res[1] * res[2]
        tiles = (cells + 1023) // 1024
        assert lib.pnr_mesh_grid_workspace_bytes(*res) == (32 + (tiles * 4 + 7) // 8 * 8 + cells * 4 + 7) // 8 * 8


def test_empty_inputs_are_no_ops_without_a_launch():
    assert _cast_rays(n=0, rays=null, depth=null, start=null) == 0          # zero rays: PNR_OK before the other checks
    assert _fill(ne=0, records=null) == 0 and _fill(nf=0, faces=null) == 0   # nothing to place
    assert _fill(ne=0, rx=0) == -1                                           # ... after the checks of the values


# ------------------------------------------------------------------------------------------------ the ops, behind the device check
@pytest.fixture()
def no_launch(monkeypatch):
    def stream():
        raise AssertionError("not refused: the op went on to its entry point")
    monkeypatch.setattr(ops, "_stream", stream)


def _outs(lead, **kw):
    out = {n: z(*(lead + tail), dtype=dt) for n, dt, tail in ops.MESHCAST_OUTPUTS}
    out.update(kw)
    return {k: v for k, v in out.items() if v is not None}


def _image_args(**kw):
    a = dict(camera_model="pinhole", cam=PIN, c2w=EYE, width=W, height=H, near=0.1, far=5.0, vertices=z(NV, 3), faces=z(NF, 3, dtype=i32), res=RES,
             lo=(0.0, 0.0, 0.0), cell=(0.5, 0.5, 0.5), start=z(CELLS + 1, dtype=i32), records=z(NE, 12), out=_outs((H, W)))
    a.update(kw)
    return a


def _list_args(**kw):
    a = dict(rays=z(9, 8), vertices=z(NV, 3), faces=z(NF, 3, dtype=i32), res=RES, lo=(0.0, 0.0, 0.0), cell=(0.5, 0.5, 0.5),
             start=z(CELLS + 1, dtype=i32), records=z(NE, 12), out=_outs((9,)))
    a.update(kw)
    return a


V_, T_ = ValueError, TypeError
SHARED = [
    (dict(vertices=z(NV, 4)), V_, "vertices must be (n, 3), got (8, 4)"),
    (dict(vertices=z(NV, 3, dtype=torch.float64)), T_, "vertices must be torch.float32, got torch.float64"),
    (dict(faces=z(NF, 3, dtype=torch.int64)), T_, "faces must be torch.int32, got torch.int64"),
    (dict(faces=[1, 2, 3]), V_, "faces must be a GPU tensor, got list"),
    (dict(res=(2, 3)), V_, "res must be three integers within 1 .. 1024, got (2, 3)"),
    (dict(res=(0, 3, 5)), V_, "res must be three integers within 1 .. 1024, got (0, 3, 5)"),
    (dict(res=(2, 3, 1025)), V_, "res must be three integers within 1 .. 1024, got (2, 3, 1025)"),
    (dict(lo=(0.0, float("nan"), 0.0)), V_, "lo must be finite (got [0.0, nan, 0.0])"),
    (dict(cell=(0.5, 0.0, 0.5)), V_, "cell must be positive and finite, with a finite inverse (got [0.5, 0.0, 0.5])"),
    (dict(cell=(0.5, 0.5, float("inf"))), V_, "cell must be positive and finite, with a finite inverse (got [0.5, 0.5, inf])"),
    (dict(start=z(CELLS, dtype=i32)), V_, "start must be (31,), got (30,)"),
    (dict(start=z(CELLS + 1)), T_, "start must be torch.int32, got torch.float32"),
    (dict(records=z(NE, 4)), V_, "records must be (n_entries, 12) with at most 2^31 - 1 entries, got (30, 4)"),
    (dict(records=z(NE, 12, dtype=torch.float64)), T_, "records must be torch.float32, got torch.float64"),
    (dict(out=None), V_, "out must be a dict of output tensors, got NoneType"),
    (dict(vertices=cpu(NV, 3)), RuntimeError, "vertices: expected a GPU tensor (the HIP path has no CPU fallback)"),
    (dict(records=z(NE, 12, device="cuda:1")), V_, "records is on cuda:1, not on cpu"),
    (dict(faces=zt(NF, 3, dtype=i32)), V_, "faces: tensor must be contiguous"),
]


def _out_cases(lead):
    full = lead + (3,)
    return [
        (dict(out=_outs(lead, depth=None)), V_, "depth must be a GPU tensor, got NoneType"),
        (dict(out=_outs(lead, code=z(*lead, dtype=i8))), T_, "code must be torch.uint8, got torch.int8"),
        (dict(out=_outs(lead, face=z(*lead, 1, dtype=i32))), V_, "face must be %s, got %s" % (lead, lead + (1,))),
        (dict(out=_outs(lead, bary=z(*lead))), V_, "bary must be %s, got %s" % (full, lead)),
        (dict(out=_outs(lead, side=z(*lead, dtype=u8))), T_, "side must be torch.int8, got torch.uint8"),
        (dict(out=_outs(lead, normal=z(*full, device="cuda:1"))), V_, "normal is on cuda:1, not on cpu"),
        (dict(out=_outs(lead, vertex=cpu(*lead, dtype=i32))), RuntimeError, "vertex: expected a GPU tensor (the HIP path has no CPU fallback)"),
        (dict(out=_outs(lead, colour=z(*lead))), V_, "unknown output 'colour' (known: depth, face, code, bary, vertex, normal, side)"),
    ]


IMAGE_OPS = [
    (dict(camera_model="orthographic"), V_, "camera_model must be 'pinhole', 'fisheye' or 'equirect', not 'orthographic'"),
    (dict(cam=(1.0, 2.0)), V_, "model 'pinhole' cam: expected 4 values, got 2"),
    (dict(width=0), V_, "bad image 0 x 12 (width, height >= 1, at most 2^31 - 1 pixels)"),
    (dict(near=-1.0), V_, "need 0 <= near < far (got -1.0, 5.0)"),
    (dict(far=0.05), V_, "need 0 <= near < far (got 0.1, 0.05)"),
    (dict(near=float("nan")), V_, "need 0 <= near < far (got nan, 5.0)"),
]
LIST_OPS = [
    (dict(rays=z(9, 7)), V_, "rays must be (R, 8), got (9, 7)"),
    (dict(rays=z(72)), V_, "rays must be (R, 8), got (72,)"),
    (dict(rays=z(9, 8, dtype=torch.float64)), T_, "rays must be torch.float32, got torch.float64"),
    (dict(rays=np.zeros((9, 8), np.float32)), V_, "rays must be a GPU tensor, got ndarray"),
]


@pytest.mark.parametrize("kw, exc, msg", IMAGE_OPS + SHARED + _out_cases((H, W)))
def test_mesh_raycast_refuses_by_name(no_launch, kw, exc, msg):
    with pytest.raises(exc) as e:
        ops.mesh_raycast.__wrapped__(**_image_args(**kw))
    assert str(e.value) == "mesh_raycast: " + msg


@pytest.mark.parametrize("kw, exc, msg", LIST_OPS + SHARED + _out_cases((9,)))
def test_mesh_cast_rays_refuses_by_name(no_launch, kw, exc, msg):
    with pytest.raises(exc) as e:
        ops.mesh_cast_rays.__wrapped__(**_list_args(**kw))
    assert str(e.value) == "mesh_cast_rays: " + msg


def test_zero_rays_reach_no_entry_point(no_launch):
    assert ops.mesh_cast_rays.__wrapped__(**_list_args(rays=z(0, 8), out=_outs((0,)))) is None


def test_public_functions_refuse_by_name(no_launch):
    box = synthetic.box_mesh((0, 0, 0), (1, 2, 3))
    cam = Pinhole(*PIN, W, H)
    idx = mesh.RayIndex.__new__(mesh.RayIndex)
    idx.n_vertices, idx.n_faces, idx.res = 8, 12, (1, 1, 1)
    other = mesh.RayIndex.__new__(mesh.RayIndex)
    other.n_vertices, other.n_faces = 162, 320
    with pytest.raises(ValueError, match="mesh.raycast: index was built for a mesh of 162 vertices and 320 faces, this one has 8 and 12"):
        mesh.raycast(box, cam, EYE, 0.1, 5.0, index=other)
    with pytest.raises(ValueError, match="mesh.cast_rays: index was built for a mesh of 162 vertices and 320 faces"):
        mesh.cast_rays(box, torch.zeros(4, 8), index=other)
    with pytest.raises(TypeError, match="mesh.raycast: index must be a mesh.RayIndex"):
        mesh.raycast(box, cam, EYE, 0.1, 5.0, index=(1, 1, 1))
    with pytest.raises(TypeError, match="mesh.raycast: mesh must be a mesh.Mesh"):
        mesh.raycast(box.vertices, cam, EYE, 0.1, 5.0, index=idx)
    with pytest.raises(TypeError, match="mesh.raycast: camera must be a camera.Pinhole"):
        mesh.raycast(box, "pinhole", EYE, 0.1, 5.0, index=idx)
    with pytest.raises(ValueError, match=r"mesh.raycast: need 0 <= near < far \(got 2.0, 1.0\)"):
        mesh.raycast(box, cam, EYE, 2.0, 1.0, index=idx)
    with pytest.raises(RuntimeError, match="mesh.raycast: the mesh must be on the GPU"):
        mesh.raycast(box, cam, EYE, 0.1, 5.0, index=idx)
    with pytest.raises(ValueError, match=r"mesh.cast_rays: rays must be an \(n, 8\) float32 tensor, got torch.float32 \(4, 7\)"):
        mesh.cast_rays(box, torch.zeros(4, 7), index=idx)
    with pytest.raises(RuntimeError, match="mesh.cast_rays: the mesh must be on the GPU"):
        mesh.cast_rays(box, torch.zeros(4, 8), index=idx)
    named = mesh.Mesh.from_arrays(box.vertices, box.faces, {"depth": torch.zeros(8), "label": torch.zeros(8, dtype=torch.int32)})
    with pytest.raises(ValueError, match="mesh.raycast: the attribute 'depth' has the name of one of the maps"):
        mesh.raycast(named, cam, EYE, 0.1, 5.0, index=idx)
    with pytest.raises(ValueError, match="mesh.cast_rays: the attribute 'depth' has the name of one of the maps"):
        mesh.cast_rays(named, torch.zeros(4, 8), index=idx)
    with pytest.raises(RuntimeError, match="mesh.raycast: the mesh must be on the GPU"):
        mesh.raycast(named, cam, EYE, 0.1, 5.0, index=idx, attributes=False)
    with pytest.raises(RuntimeError, match="mesh.RayIndex: the mesh must be on the GPU"):
        mesh.RayIndex(box)
    with pytest.raises(ValueError, match="mesh.RayIndex: res must be three integers within 1 .. 1024"):
        mesh.RayIndex(box, res=(4, 4, 2000))


# ------------------------------------------------------------------------------------------------ host code
def test_from_arrays_and_labels():
    v, f = np.zeros((4, 3), np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    m = mesh.Mesh.from_arrays(v, f, {"label": np.arange(4, dtype=np.int32), "rgb": torch.zeros(4, 3, dtype=torch.uint8)})
    assert (m.src, m.res, m.lo, m.step, m.level, m.grid) == (None,) * 6 and repr(m) == "Mesh(4 vertices, 2 faces)"
    assert m.vertices.dtype == f32 and m.faces.dtype == i32 and sorted(m.attributes) == ["label", "rgb"]
    with pytest.raises(ValueError, match="Mesh.labels: this mesh did not come from a lattice"):
        m.labels(torch.zeros(2, 2, 2))
    with pytest.raises(TypeError, match="Mesh.from_arrays: faces must be torch.int32, got torch.int64"):
        mesh.Mesh.from_arrays(v, f.astype(np.int64))
    with pytest.raises(ValueError, match=r"Mesh.from_arrays: vertices must be \(n, 3\), got \(4, 2\)"):
        mesh.Mesh.from_arrays(v[:, :2], f)
    with pytest.raises(ValueError, match=r"attributes\['label'\] must hold one row per vertex \(4\)"):
        mesh.Mesh.from_arrays(v, f, {"label": np.arange(5)})
    assert m.area() == 0.0


def test_synthetic_meshes_are_closed_and_wound_as_stated():
    for sub in (0, 1, 2):
        s = synthetic.icosphere(sub, radius=2.0, center=(1.0, -2.0, 0.5))
        V, F = s.vertices.numpy().astype(np.float64), s.faces.numpy()
        assert F.shape == (20 * 4 ** sub, 3) and len(V) == 10 * 4 ** sub + 2
        assert np.abs(np.linalg.norm(V - (1.0, -2.0, 0.5), axis=1) - 2.0).max() < 1e-6
        edges = {}
        for a, b, c in F:
            for e in ((a, b), (b, c), (c, a)):
                edges[e] = edges.get(e, 0) + 1
        assert all(n == 1 and edges.get((b, a)) == 1 for (a, b), n in edges.items())       # every edge once each way: closed, consistently wound
        n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
        assert ((n * (V[F].mean(1) - (1.0, -2.0, 0.5))).sum(1) > 0).all()                   # outwards
    assert 0.9 * 4 / 3 * np.pi < synthetic.icosphere(3).volume() < 4 / 3 * np.pi
    lo, hi = (-2.0, -1.5, -2.5), (2.5, 1.2, 3.0)
    b = synthetic.box_mesh(lo, hi)
    V, F = b.vertices.numpy().astype(np.float64), b.faces.numpy()
    assert V.shape == (8, 3) and F.shape == (12, 3) and abs(b.volume() + 4.5 * 2.7 * 5.5) < 1e-5 and abs(b.area() - 2 * (4.5 * 2.7 + 4.5 * 5.5 + 2.7 * 5.5)) < 1e-4
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    centre = (np.asarray(lo) + np.asarray(hi)) / 2
    assert ((n * (centre - V[F].mean(1))).sum(1) > 0).all()                                 # into the room
    assert ((n != 0).sum(1) == 1).all()                                                     # axis-aligned walls
    with pytest.raises(ValueError, match="box_mesh: lo and hi must be finite 3-vectors with lo < hi"):
        synthetic.box_mesh((0, 0, 0), (1, 0, 1))
    with pytest.raises(ValueError, match="icosphere: subdiv must be within 0 .. 7"):
        synthetic.icosphere(9)


def test_default_grid():
    f = np.float32
    # about two faces a cell, cubic cells, at most 1024 on an axis
    lo, cell, res = mesh.grid_box(np.array([-1, -1, -1, 1, 1, 1], f), 16000)
    assert res == (20, 20, 20) and (lo < -1).all() and (lo + cell * np.asarray(res, f) > 1).all()
    _, _, res = mesh.grid_box(np.array([0, 0, 0, 8, 1, 2], f), 2 * 128 * 16 * 32)
    assert all(abs(r - w) <= 1 for r, w in zip(res, (128, 16, 32)))
    _, _, res = mesh.grid_box(np.array([0, 0, 0, 1e4, 1, 1], f), 10 ** 7)
    assert res[0] == 1024 and max(res) <= 1024
    # a flat axis gets one cell, of positive size -- also far from the origin
    for off in (0.0, 3000.0, -1e5):
        lo, cell, res = mesh.grid_box(np.array([off, off, off, off + 2, off, off + 1], f), 800)
        assert res[1] == 1 and res[0] * res[2] in range(350, 450) and (cell > 0).all() and np.isfinite(cell).all()
        assert lo[1] < f(off) < lo[1] + cell[1]
    lo, cell, res = mesh.grid_box(np.array([5, 5, 5, 5, 5, 5], f), 3)                      # a single point
    assert res == (1, 1, 1) and (cell > 0).all() and (lo < 5).all()
    lo, cell, res = mesh.grid_box(np.array([np.inf] * 3 + [-np.inf] * 3, f), 0)            # no usable face
    assert res == (1, 1, 1) and np.array_equal(lo, np.zeros(3, f)) and np.array_equal(cell, np.ones(3, f))
    lo, cell, res = mesh.grid_box(np.array([-1, -1, -1, 1, 1, 1], f), 16000, res=(2, 3, 5))
    assert res == (2, 3, 5) and 1.0 < cell[0] < 1.01                                      # the coarsest axis sets the size
    # cubes that cover the box, the box centred, whatever the res
    for b, n, r in ((np.array([-1, -1, -1, 1, 1, 1], f), 16000, None), (np.array([0, 0, 0, 8, 1, 2], f), 70000, (5, 40, 3)),
                    (np.array([3000, 3000, 3000, 3002, 3000, 3001], f), 800, None), (np.array([-1, -1, -1, 1, 1, 1], f), 9, (1, 1, 1024))):
        lo, cell, res = mesh.grid_box(b, n, r)
        hi = lo + cell * np.asarray(res, f)
        assert cell[0] == cell[1] == cell[2] and (lo < b[:3]).all() and (hi > b[3:]).all()
        assert np.allclose((lo + hi) / 2, (b[:3] + b[3:]) / 2, atol=1e-3 * float(cell[0]) + 1e-3)
    with pytest.raises(ValueError, match="leave no finite float32 grid"):
        mesh.grid_box(np.array([-3e38, 0, 0, 3e38, 1, 1], f), 10)
