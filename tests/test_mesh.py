"""CPU tests of the mesh-extraction boundary: every refusal of mesh.*, ops.mesh_* and the three entry points happens before any
launch and names its argument; the workspace arithmetic; Mesh.save_ply read back; synthetic.sdf_grid against _mesh_ref."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import _mesh_ref as R
from panopticnerf_amd import _lib, mesh, ops, synthetic

LIMIT = (2 ** 31 - 1) // 12
NULL = ctypes.c_void_p(0)
PTR = ctypes.c_void_p(4096)             # non-null and aligned, never dereferenced: validation fails first
F3 = ctypes.c_float * 3


def refused(rc, *words):
    msg = _lib.load().pnr_last_error()
    return rc == -1 and all(w.encode() in msg for w in words)


# ---------------------------------------------------------------- the entry points
def test_workspace_bytes():
    ws = _lib.load().pnr_mesh_workspace_bytes
    assert ops.MESH_MAX_POINTS == R.MAX_POINTS == LIMIT == 178956970
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (LIMIT + 1, 1, 1), (1 << 16, 1 << 16, 1 << 16), (564, 564, 564), (2 ** 31 - 1,) * 3):
        assert refused(ws(*bad), "pnr_mesh_workspace_bytes"), bad
    assert ws(LIMIT, 1, 1) > 0 and ws(563, 563, 563) > 0 and ws(1, 1, 1) > 0
    # monotone in the lattice size, and a whole number of 1024-point chunks of 14 bytes a point + 8 a chunk
    last = 0
    for n in (1, 2, 1023, 1024, 1025, 4096, 10 ** 6, 10 ** 8, LIMIT):
        b = ws(n, 1, 1)
        chunks = (n + 1023) // 1024
        assert b == chunks * (14 * 1024 + 8) and b >= last
        last = b
    for rx, ry, rz in ((2, 3, 5), (31, 33, 65), (256, 256, 256)):
        assert ws(rx, ry, rz) == ws(rx * ry * rz, 1, 1) == ws(rz, rx, ry)
    with pytest.raises(RuntimeError, match="pnr_mesh_workspace_bytes"):
        ops.mesh_workspace_bytes(0, 1, 1)


def test_count_refuses_before_any_launch():
    count = _lib.load().pnr_mesh_count
    assert refused(count(PTR, 0, 4, 4, 0.0, PTR, PTR, NULL), "pnr_mesh_count", "lattice")
    assert refused(count(PTR, 4, 4, -3, 0.0, PTR, PTR, NULL), "pnr_mesh_count", "lattice")
    assert refused(count(PTR, 564, 564, 564, 0.0, PTR, PTR, NULL), "pnr_mesh_count", "lattice")
    for level in (float("nan"), float("inf"), -float("inf")):
        assert refused(count(PTR, 4, 4, 4, level, PTR, PTR, NULL), "pnr_mesh_count", "level")
    for args in ((NULL, PTR, PTR), (PTR, NULL, PTR), (PTR, PTR, NULL)):
        assert refused(count(args[0], 4, 4, 4, 0.0, args[1], args[2], NULL), "pnr_mesh_count", "null")
    for args in ((4098, 4096, 4096), (4096, 4104, 4096), (4096, 4096, 4100)):
        assert refused(count(ctypes.c_void_p(args[0]), 4, 4, 4, 0.0, ctypes.c_void_p(args[1]), ctypes.c_void_p(args[2]), NULL),
                       "pnr_mesh_count", "misaligned")


def test_emit_refuses_before_any_launch():
    emit = _lib.load().pnr_mesh_emit
    lo, step = F3(0.0, 0.0, 0.0), F3(1.0, 1.0, 1.0)
    assert refused(emit(PTR, 4, 0, 4, 0.0, lo, step, PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "lattice")
    assert refused(emit(PTR, 1000, 1000, 1000, 0.0, lo, step, PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "lattice")
    assert refused(emit(PTR, 4, 4, 4, float("nan"), lo, step, PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "level")
    assert refused(emit(PTR, 4, 4, 4, 0.0, None, step, PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "null lo or step")
    assert refused(emit(PTR, 4, 4, 4, 0.0, lo, None, PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "null lo or step")
    for bad in (float("nan"), float("inf")):
        for axis in range(3):
            v = [0.5, 0.5, 0.5]
            v[axis] = bad
            assert refused(emit(PTR, 4, 4, 4, 0.0, F3(*v), step, PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "finite", "axis %d" % axis)
            assert refused(emit(PTR, 4, 4, 4, 0.0, lo, F3(*v), PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "finite", "axis %d" % axis)
    assert refused(emit(NULL, 4, 4, 4, 0.0, lo, step, PTR, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "null field")
    assert refused(emit(PTR, 4, 4, 4, 0.0, lo, step, NULL, PTR, PTR, PTR, NULL), "pnr_mesh_emit", "null field or workspace")
    for k in range(5):                      # field, workspace, vertices, faces, src
        p = [4096] * 5
        p[k] += (2, 8, 2, 2, 4)[k]
        p = [ctypes.c_void_p(v) for v in p]
        assert refused(emit(p[0], 4, 4, 4, 0.0, lo, step, p[1], p[2], p[3], p[4], NULL), "pnr_mesh_emit", "misaligned"), k


# ---------------------------------------------------------------- ops and mesh
def test_ops_refuse_by_name():
    f = torch.zeros(3, 4, 5)
    with pytest.raises(RuntimeError, match="mesh_count: field.*no CPU fallback"):
        ops.mesh_count(f, 0.0)
    with pytest.raises(ValueError, match="mesh_count: field must be a GPU tensor"):
        ops.mesh_count(np.zeros((3, 4, 5), np.float32), 0.0)
    with pytest.raises(ValueError, match="mesh_count: field must be float32"):
        ops.mesh_count(f.double(), 0.0)
    for bad in (torch.zeros(4, 5), torch.zeros(0, 4, 5), torch.zeros(2, 3, 4, 5)):
        with pytest.raises(ValueError, match=r"mesh_count: field must be \(res_z, res_y, res_x\)"):
            ops.mesh_count(bad, 0.0)
    for level in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mesh_count: level must be finite"):
            ops.mesh_count(f, level)
    with pytest.raises(ValueError, match="mesh_count: workspace"):
        ops.mesh_count(f, 0.0, workspace=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mesh_count: totals"):
        ops.mesh_count(f, 0.0, totals=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="more than the limit"):
        ops.mesh_count(torch.zeros(1).expand(564, 564, 564), 0.0)
    ws = torch.zeros(ops.mesh_workspace_bytes(5, 4, 3), dtype=torch.uint8)
    v, t, s = torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="mesh_emit: field.*no CPU fallback"):
        ops.mesh_emit(f, 0.0, (0, 0, 0), (1, 1, 1), ws, v, t, s)
    with pytest.raises(ValueError, match="mesh_emit: lo"):
        ops.mesh_emit(f, 0.0, (0, 0), (1, 1, 1), ws, v, t, s)
    with pytest.raises(ValueError, match="mesh_emit: step must be finite"):
        ops.mesh_emit(f, 0.0, (0, 0, 0), (1, float("nan"), 1), ws, v, t, s)
    with pytest.raises(ValueError, match="mesh_emit: lo must be finite"):
        ops.mesh_emit(f, 0.0, (float("inf"), 0, 0), (1, 1, 1), ws, v, t, s)
    with pytest.raises(ValueError, match="mesh_emit: workspace"):
        ops.mesh_emit(f, 0.0, (0, 0, 0), (1, 1, 1), ws[:100], v, t, s)
    with pytest.raises(ValueError, match="mesh_emit: vertices"):
        ops.mesh_emit(f, 0.0, (0, 0, 0), (1, 1, 1), ws, v.double(), t, s)
    with pytest.raises(ValueError, match="mesh_emit: faces"):
        ops.mesh_emit(f, 0.0, (0, 0, 0), (1, 1, 1), ws, v, t.long(), s)
    with pytest.raises(ValueError, match="mesh_emit: src"):
        ops.mesh_emit(f, 0.0, (0, 0, 0), (1, 1, 1), ws, v, t, s.int())
    with pytest.raises(ValueError, match="mesh_emit: src holds"):
        ops.mesh_emit(f, 0.0, (0, 0, 0), (1, 1, 1), ws, v, t, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="mesh_emit: level must be finite"):
        ops.mesh_emit(f, float("nan"), (0, 0, 0), (1, 1, 1), ws, v, t, s)


def test_mesh_refuses_by_name():
    f = torch.zeros(3, 4, 5)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="mesh.extract: field must be a GPU tensor.*no CPU fallback"):
        mesh.extract(f, lo, hi, 0.0)
    with pytest.raises(ValueError, match="mesh.extract: field must be a GPU tensor"):
        mesh.extract([[0.0]], lo, hi, 0.0)
    with pytest.raises(ValueError, match="mesh.extract: field must be float32"):
        mesh.extract(f.half(), lo, hi, 0.0)
    with pytest.raises(ValueError, match="mesh.extract: field must be"):
        mesh.extract(f[0], lo, hi, 0.0)
    with pytest.raises(ValueError, match="mesh.extract: level must be finite"):
        mesh.extract(f, lo, hi, float("-inf"))
    with pytest.raises(ValueError, match="mesh: lo must be three numbers"):
        mesh.extract(f, (0.0, 1.0), hi, 0.0)
    with pytest.raises(ValueError, match="mesh: hi must be finite"):
        mesh.extract(f, lo, (1.0, float("nan"), 1.0), 0.0)
    with pytest.raises(ValueError, match="mesh: lo must be three numbers"):
        mesh.extract(f, "abc", hi, 0.0)
    with pytest.raises(ValueError, match="overflows float32"):
        mesh.extract(f, (-3e38,) * 3, (3e38,) * 3, 0.0)
    with pytest.raises(ValueError, match="from_network: level must be finite"):
        mesh.from_network(None, lo, hi, 4, float("nan"))
    with pytest.raises(ValueError, match="mesh: lo must be finite"):
        mesh.from_network(None, (float("inf"), 0, 0), hi, 4, 0.0)
    m = mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), (5, 4, 3), None, None, 0.0)
    with pytest.raises(ValueError, match=r"Mesh.labels: grid must be a \(3, 4, 5\) tensor"):
        m.labels(torch.zeros(5, 4, 3))
    with pytest.raises(ValueError, match="Mesh.labels: grid"):
        m.labels(np.zeros((3, 4, 5)))
    assert m.labels(torch.zeros(3, 4, 5)).shape == (0,) and m.area() == 0.0 and m.volume() == 0.0
    lo32, step = mesh.lattice((-1, 0, 1), (1, 3, 2), (8, 5, 3))
    rlo, rstep = R.lattice((-1, 0, 1), (1, 3, 2), (8, 5, 3))
    assert np.array_equal(lo32, rlo) and np.array_equal(step, rstep) and step.dtype == np.float32


# ---------------------------------------------------------------- Mesh: host code on any device
def read_ply(path):
    """a ten-line parser of the binary little-endian PLY this package writes"""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    n_f = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    props = [ln.split()[1:] for ln in lines[:[i for i, ln in enumerate(lines) if ln.startswith("element face")][0]] if ln.startswith("property")]
    fmt = "<" + "".join({"float": "f", "uchar": "B", "int": "i"}[t] for t, _ in props)
    rows = [struct.unpack_from(fmt, body, i * struct.calcsize(fmt)) for i in range(n_v)]
    off = n_v * struct.calcsize(fmt)
    faces = [struct.unpack_from("<Biii", body, off + 13 * i) for i in range(n_f)]
    assert off + 13 * n_f == len(body)
    return [name for _, name in props], rows, faces


def test_save_ply_round_trip(tmp_path):
    f, (lo, hi) = np.zeros((3, 3, 3), np.float32), ((-0.5,) * 3, (2.5,) * 3)
    f[1, 1, 1] = 1.0
    v, t, s = R.extract(f, lo, hi, 0.5)
    m = mesh.Mesh(torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(s), (3, 3, 3), None, None, 0.5)
    assert abs(m.volume() - 0.5) < 1e-6 and abs(m.volume() - R.volume(v, t)) < 1e-12 and abs(m.area() - R.area(v, t)) < 1e-12
    assert torch.equal(m.labels(torch.arange(27).reshape(3, 3, 3)), torch.full((14,), 13))
    colors = torch.arange(14 * 3, dtype=torch.uint8).reshape(14, 3)
    labels = torch.arange(14, dtype=torch.int32) * 1000 - 5
    for kw in ({}, {"colors": colors}, {"labels": labels}, {"colors": colors, "labels": labels.long()}):
        path = str(tmp_path / "m.ply")
        m.save_ply(path, **kw)
        names, rows, faces = read_ply(path)
        assert names == ["x", "y", "z"] + (["red", "green", "blue"] if "colors" in kw else []) + (["label"] if "labels" in kw else [])
        assert len(rows) == 14 and len(faces) == 24
        assert np.array_equal(np.array([r[:3] for r in rows], np.float32), v)
        assert all(fc[0] == 3 for fc in faces) and np.array_equal(np.array([fc[1:] for fc in faces], np.int32), t)
        if "colors" in kw:
            assert np.array_equal(np.array([r[3:6] for r in rows], np.uint8), colors.numpy())
        if "labels" in kw:
            assert [r[-1] for r in rows] == labels.tolist()
    with pytest.raises(ValueError, match="save_ply: colors"):
        m.save_ply(str(tmp_path / "x.ply"), colors=colors[:3])
    with pytest.raises(ValueError, match="save_ply: labels"):
        m.save_ply(str(tmp_path / "x.ply"), labels=torch.zeros(14))
    empty = mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), (3, 3, 3), None, None, 0.0)
    empty.save_ply(str(tmp_path / "e.ply"))
    assert read_ply(str(tmp_path / "e.ply")) == (["x", "y", "z"], [], [])


# ---------------------------------------------------------------- synthetic.sdf_grid
def test_sdf_grid():
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    x, y, z = R.positions(lo, hi, (9, 8, 7))
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    f = synthetic.sdf_grid("sphere", lo, hi, (9, 8, 7), radius=0.7)
    assert f.shape == (7, 8, 9) and f.dtype == torch.float32
    assert np.array_equal(f.numpy(), (np.float32(0.7) - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32))
    p = synthetic.sdf_grid("plane", lo, hi, (9, 8, 7), axis=1, offset=0.25)
    assert np.array_equal(p.numpy(), (Y - np.float32(0.25)).astype(np.float32))
    # positive inside, and the level-0 surfaces have the right topology
    for kind, chi, kw in (("sphere", 2, {}), ("torus", 0, {"radius": 0.6, "minor": 0.25}), ("box", 2, {"half": (0.5, 0.4, 0.3)})):
        g = synthetic.sdf_grid(kind, lo, hi, 16, **kw).numpy()
        v, t, s = R.extract(g, lo, hi, 0.0)
        assert R.is_closed_oriented(t, len(v)) and R.euler(t) == chi and R.volume(v, t) > 0, kind
    box = synthetic.sdf_grid("box", lo, hi, 32, half=(0.5, 0.4, 0.3)).numpy()
    v, t, s = R.extract(box, lo, hi, 0.0)
    assert abs(R.volume(v, t) - 1.0 * 0.8 * 0.6) < 0.02
    with pytest.raises(ValueError, match="sdf_grid: unknown kind"):
        synthetic.sdf_grid("cone", lo, hi, 4)
    with pytest.raises(ValueError, match="sdf_grid: res"):
        synthetic.sdf_grid("sphere", lo, hi, (4, 0, 4))
    with pytest.raises(ValueError, match="sdf_grid: lo and hi"):
        synthetic.sdf_grid("sphere", (0, 0), hi, 4)
    with pytest.raises(ValueError, match="sdf_grid: axis"):
        synthetic.sdf_grid("plane", lo, hi, 4, axis=3)
