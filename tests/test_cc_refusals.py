"""CPU tests of the refusals of the connected-components ops (ops.cc_label / cc_mesh / cc_stats / cc_workspace_bytes), of the
wrappers above them (components.label, depth.despeckle, stereo.despeckle, Mesh.select) and of the C entry points behind them,
after the pattern of test_ops_refusals.py: _fake_gpu tensors passed to the op behind `_on_device` (`op.__wrapped__`), asking
for the stream fails the test, and every case names the exception type and the WHOLE message.  The C-ABI refusals go through
ctypes as test_abi.py's do: PNR_EINVAL and a message before any launch.  Nothing here touches a GPU."""
import ctypes

import pytest
import torch

from panopticnerf_amd import _lib, components, depth, mesh, ops, stereo

from _fake_gpu import _fake, cpu, z, zt

RZ, RY, RX = 3, 4, 5
NV, NF, NC = 9, 6, 4
NO_GPU = " (the HIP path has no CPU fallback)"
CONTIG = ": tensor must be contiguous"
f32, i16, i32, i64 = torch.float32, torch.int16, torch.int32, torch.int64
V, T = ValueError, TypeError
WORDS = lambda n: ops.cc_workspace_bytes(n) // 8
LATTICE = "must be an image (height, width) or a lattice (res_z, res_y, res_x)"


@pytest.fixture(autouse=True)
def _no_launch(monkeypatch):
    def stream():
        raise AssertionError("not refused: the op went on to its entry point")
    monkeypatch.setattr(ops, "_stream", stream)


BASE = {
    "cc_label": lambda: dict(data=z(RZ, RY, RX, dtype=i32), full=True, labels=z(RZ, RY, RX, dtype=i32), size=z(RZ, RY, RX, dtype=i32),
                             count=z(1, dtype=i64), workspace=z(WORDS(RZ * RY * RX), dtype=i64)),
    "cc_mesh": lambda: dict(faces=z(NF, 3, dtype=i32), n_vertices=NV, vertex_label=z(NV, dtype=i32), face_label=z(NF, dtype=i32),
                            face_size=z(NF, dtype=i32), count=z(1, dtype=i64), workspace=z(WORDS(NV), dtype=i64)),
    "cc_stats": lambda: dict(labels=z(RZ, RY, RX, dtype=i32), size=z(RZ, RY, RX, dtype=i32), n_components=NC, sizes=z(NC, dtype=i32),
                             boxes=z(NC, 6, dtype=i32)),
}
_D = z(RZ, RY, RX, dtype=i32)

CASES = [
    # ------------------------------------------------------------------------------------------------------------ cc_label
    ("cc_label", dict(data=[1]), V, "cc_label: data must be a GPU tensor, got list"),
    ("cc_label", dict(data=z(RZ, RY, RX, dtype=i64)), T, "cc_label: data must be torch.int32 (keys) or torch.float32 (values), got torch.int64"),
    ("cc_label", dict(data=z(RX, dtype=i64)), T, "cc_label: data must be torch.int32 (keys) or torch.float32 (values), got torch.int64"),     # dtype, then rank
    ("cc_label", dict(data=z(RX, dtype=i32)), V, "cc_label: data %s, got (5,)" % LATTICE),
    ("cc_label", dict(data=z(2, 2, 2, 2, dtype=i32)), V, "cc_label: data %s, got (2, 2, 2, 2)" % LATTICE),
    ("cc_label", dict(data=z(0, RY, RX, dtype=i32)), V, "cc_label: data must be (res_z, res_y, res_x) with every res >= 1, got (0, 4, 5)"),
    ("cc_label", dict(data=_fake(torch.zeros(1, dtype=i32).expand(2, 2 ** 15, 2 ** 15))), V,
     "cc_label: data holds 2147483648 points, more than the limit of 2^31 - 2"),
    ("cc_label", dict(full=2), V, "cc_label: full must be False or True (got 2)"),
    ("cc_label", dict(tol=0.5), V, "cc_label: tol goes with float32 data; int32 keys are linked where they are equal"),
    ("cc_label", dict(data=z(RZ, RY, RX)), V, "cc_label: float32 data are values and need tol"),
    ("cc_label", dict(data=z(RZ, RY, RX), tol=-1.0), V, "cc_label: tol must be >= 0 and not NaN (got -1.0)"),
    ("cc_label", dict(data=z(RZ, RY, RX), tol=float("nan")), V, "cc_label: tol must be >= 0 and not NaN (got nan)"),
    ("cc_label", dict(data=z(RZ, RY, RX), tol="x"), V, "cc_label: tol must be a number >= 0 (got 'x')"),
    ("cc_label", dict(size="yes"), V, "cc_label: size must be True, False or an int32 tensor of the data's shape (got str)"),
    ("cc_label", dict(labels=z(RZ, RY, RX)), T, "cc_label: labels must be torch.int32, got torch.float32"),
    ("cc_label", dict(labels=z(RZ, RY, dtype=i32)), V, "cc_label: labels must be (3, 4, 5), got (3, 4)"),
    ("cc_label", dict(size=z(RZ, RY, RX + 1, dtype=i32)), V, "cc_label: size must be (3, 4, 5), got (3, 4, 6)"),
    ("cc_label", dict(count=z(2, dtype=i64)), V, "cc_label: count must be (1,), got (2,)"),
    ("cc_label", dict(count=z(1, dtype=i32)), T, "cc_label: count must be torch.int64, got torch.int32"),
    ("cc_label", dict(data=cpu(RZ, RY, RX, dtype=i32)), RuntimeError, "cc_label: data: expected a GPU tensor" + NO_GPU),
    ("cc_label", dict(data=zt(RZ, RY, RX, dtype=i32)), V, "cc_label: data" + CONTIG),
    ("cc_label", dict(labels=zt(RZ, RY, RX, dtype=i32)), V, "cc_label: labels" + CONTIG),
    ("cc_label", dict(labels=z(RZ, RY, RX, dtype=i32, device="cuda:1")), V, "cc_label: labels is on cuda:1, not on cpu"),
    ("cc_label", dict(count=z(1, dtype=i64, device="cuda:1")), V, "cc_label: count is on cuda:1, not on cpu"),
    ("cc_label", dict(data=_D, labels=_D), V, "cc_label: labels may not alias data"),
    ("cc_label", dict(data=_D, size=_D), V, "cc_label: size may not alias data"),
    ("cc_label", dict(workspace=z(1, dtype=i64)), V, "cc_label: workspace must be an int64 tensor of at least %d words" % WORDS(RZ * RY * RX)),
    ("cc_label", dict(workspace=z(1000, dtype=i32)), V, "cc_label: workspace must be an int64 tensor of at least %d words" % WORDS(RZ * RY * RX)),
    ("cc_label", dict(labels=z(RZ, RY, RX), count=z(1, dtype=i64, device="cuda:1")), T, "cc_label: labels must be torch.int32, got torch.float32"),
    # ------------------------------------------------------------------------------------------------------------- cc_mesh
    ("cc_mesh", dict(faces="faces"), V, "cc_mesh: faces must be a GPU tensor, got str"),
    ("cc_mesh", dict(faces=z(NF, 3)), T, "cc_mesh: faces must be torch.int32, got torch.float32"),
    ("cc_mesh", dict(faces=z(NF, 4, dtype=i32)), V, "cc_mesh: faces must be (n, 3), got (6, 4)"),
    ("cc_mesh", dict(n_vertices=-1), V, "cc_mesh: n_vertices must be an integer in 0 .. 2^31 - 2 (got -1)"),
    ("cc_mesh", dict(n_vertices=2 ** 31 - 1), V, "cc_mesh: n_vertices must be an integer in 0 .. 2^31 - 2 (got 2147483647)"),
    ("cc_mesh", dict(n_vertices=9.0), V, "cc_mesh: n_vertices must be an integer in 0 .. 2^31 - 2 (got 9.0)"),
    ("cc_mesh", dict(face_size=3), V, "cc_mesh: face_size must be True, False or an (F,) int32 tensor (got int)"),
    ("cc_mesh", dict(vertex_label=z(NV - 1, dtype=i32)), V, "cc_mesh: vertex_label must be (9,), got (8,)"),
    ("cc_mesh", dict(face_label=z(NF, dtype=i64)), T, "cc_mesh: face_label must be torch.int32, got torch.int64"),
    ("cc_mesh", dict(faces=cpu(NF, 3, dtype=i32)), RuntimeError, "cc_mesh: faces: expected a GPU tensor" + NO_GPU),
    ("cc_mesh", dict(faces=zt(NF, 3, dtype=i32)), V, "cc_mesh: faces" + CONTIG),
    ("cc_mesh", dict(face_size=zt(NF, dtype=i32)), V, "cc_mesh: face_size" + CONTIG),
    ("cc_mesh", dict(face_label=z(NF, dtype=i32, device="cuda:1")), V, "cc_mesh: face_label is on cuda:1, not on cpu"),
    ("cc_mesh", dict(workspace=z(1, dtype=i64)), V, "cc_mesh: workspace must be an int64 tensor of at least %d words" % WORDS(NV)),
    # ------------------------------------------------------------------------------------------------------------ cc_stats
    ("cc_stats", dict(labels=None), V, "cc_stats: labels must be a GPU tensor, got NoneType"),
    ("cc_stats", dict(labels=z(RZ, RY, RX)), T, "cc_stats: labels must be torch.int32, got torch.float32"),
    ("cc_stats", dict(labels=z(2, 2, 2, 2, dtype=i32)), V, "cc_stats: labels %s, got (2, 2, 2, 2)" % LATTICE),
    ("cc_stats", dict(size=z(RZ, RY, RX)), T, "cc_stats: size must be torch.int32, got torch.float32"),
    ("cc_stats", dict(size=z(RZ, RY, RX + 1, dtype=i32)), V, "cc_stats: size must be (3, 4, 5), got (3, 4, 6)"),
    ("cc_stats", dict(n_components=-1), V, "cc_stats: n_components must be an integer in 0 .. 2^31 - 2 (got -1)"),
    ("cc_stats", dict(n_components=True), V, "cc_stats: n_components must be an integer in 0 .. 2^31 - 2 (got True)"),
    ("cc_stats", dict(sizes=z(NC + 1, dtype=i32)), V, "cc_stats: sizes must be (4,), got (5,)"),
    ("cc_stats", dict(boxes=z(NC, 5, dtype=i32)), V, "cc_stats: boxes must be (4, 6), got (4, 5)"),
    ("cc_stats", dict(boxes="all"), V, "cc_stats: boxes must be True, False or an (n, 6) int32 tensor (got str)"),
    ("cc_stats", dict(labels=cpu(RZ, RY, RX, dtype=i32)), RuntimeError, "cc_stats: labels: expected a GPU tensor" + NO_GPU),
    ("cc_stats", dict(labels=zt(RZ, RY, RX, dtype=i32)), V, "cc_stats: labels" + CONTIG),
    ("cc_stats", dict(sizes=z(NC, dtype=i32, device="cuda:1")), V, "cc_stats: sizes is on cuda:1, not on cpu"),
]


@pytest.mark.parametrize("op,over,exc,message", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_by_type_and_whole_message(op, over, exc, message):
    args = BASE[op]()
    args.update(over)
    with pytest.raises(Exception) as e:
        getattr(ops, op).__wrapped__(**args)
    assert type(e.value) is exc and str(e.value) == message, "%s: %s" % (type(e.value).__name__, e.value)


def test_every_op_is_covered_and_its_base_arguments_reach_the_launch():
    assert {c[0] for c in CASES} == set(BASE)
    for op, base in BASE.items():
        with pytest.raises(AssertionError, match="not refused: the op went on to its entry point"):
            getattr(ops, op).__wrapped__(**base())
    # an image, float32 values with tol, size=False, and a mesh's faces as a 1 x 1 x F lattice reach it too
    for op, args in (("cc_label", dict(data=z(RY, RX), tol=float("inf"), size=False)), ("cc_label", dict(data=z(RY, RX, dtype=i32))),
                     ("cc_mesh", dict(faces=z(NF, 3, dtype=i32), n_vertices=NV, face_size=False)),
                     ("cc_stats", dict(labels=z(NF, dtype=i32), size=z(NF, dtype=i32), n_components=2, boxes=False))):
        with pytest.raises(AssertionError, match="not refused: the op went on to its entry point"):
            getattr(ops, op).__wrapped__(**args)


def test_workspace_bytes_is_host_arithmetic():
    tile = 4 * 256                                              # the scan's tile: one int32 sum each
    for n in (0, 1, 7, tile, tile + 1, 10 ** 6):
        r8 = lambda b: (b + 7) // 8 * 8
        assert ops.cc_workspace_bytes(n) == r8(4 * (n + 1)) + r8(4 * n) + r8(4 * ((n + tile - 1) // tile))
    assert ops.cc_workspace_bytes(2 ** 31 - 2) > 0
    for n in (-1, 2 ** 31 - 1):
        with pytest.raises(RuntimeError, match="pnr_cc_workspace_bytes"):
            ops.cc_workspace_bytes(n)


WRAPPERS = [
    (lambda: components.label([0, 1]), V, "components.label: x must be a GPU tensor, got list"),
    (lambda: components.label(z(5, dtype=i32)), V, "components.label: x must be 2-D (an image) or 3-D (res_z, res_y, res_x), got (5,)"),
    (lambda: components.label(z(4, 5, dtype=i32), connectivity=6), V, "components.label: connectivity must be 4 or 8 for a 2-D tensor (got 6)"),
    (lambda: components.label(z(3, 4, 5, dtype=i32), connectivity=8), V, "components.label: connectivity must be 6 or 26 for a 3-D tensor (got 8)"),
    (lambda: components.label(z(3, 4, 5, dtype=i32), connectivity=True), V, "components.label: connectivity must be 6 or 26 for a 3-D tensor (got True)"),
    (lambda: components.label(z(4, 5, dtype=i64)), T,
     "components.label: int64 keys are not taken (a key beyond int32 could not be told without reading back): cast to int32"),
    (lambda: components.label(z(4, 5, dtype=torch.float64)), T,
     "components.label: x must be bool, uint8, int16 or int32 (keys) or float32 (values), got torch.float64"),
    (lambda: components.label(cpu(4, 5, dtype=i32)), RuntimeError, "components.label: x must be a GPU tensor" + NO_GPU),
    (lambda: components.label(z(4, 5)), V, "components.label: float32 x are values and need tol"),
    (lambda: components.label(z(4, 5), tol=-0.5), V, "components.label: tol must be >= 0 and not NaN (got -0.5)"),
    (lambda: components.label(z(4, 5, dtype=i16), tol=1.0), V,
     "components.label: tol goes with float32 values; integer keys are linked where they are equal"),
    (lambda: components.label_mesh("mesh"), T, "components.label_mesh: mesh must be a mesh.Mesh"),
    (lambda: depth.despeckle(z(4, 5), 0.1, 5, connectivity=6), V, "depth.despeckle: connectivity must be 4 or 8 (got 6)"),
    (lambda: depth.despeckle(z(4, 5), -0.1, 5), V, "depth.despeckle: tol must be >= 0 and not NaN (got -0.1)"),
    (lambda: depth.despeckle(z(4, 5), 0.1, 2.5), V, "depth.despeckle: min_size must be an integer >= 0 (got 2.5)"),
    (lambda: depth.despeckle(z(4, 5, dtype=i32), 0.1, 5), V,
     "depth.despeckle: depth must be a float32 tensor of shape (height, width), got torch.int32 (4, 5)"),
    (lambda: depth.despeckle(zt(4, 5), 0.1, 5), V,
     "depth.despeckle: depth must be contiguous (a transposed or strided view is not taken; call .contiguous())"),
    (lambda: stereo.despeckle([1]), T, "stereo.despeckle: result must be the dict stereo.sgm returns"),
    (lambda: stereo.despeckle({"d16": z(4, 5, dtype=i16)}, max_diff=float("inf")), V,
     "stereo.despeckle: max_diff must be finite and >= 0 pixels (got inf)"),
    (lambda: stereo.despeckle({"d16": z(4, 5, dtype=i16)}, min_size=-1), V, "stereo.despeckle: min_size must be an integer >= 0 (got -1)"),
    (lambda: stereo.despeckle({"d16": z(4, 5)}), V, "stereo.despeckle: result['d16'] must be an (H, W) int16 tensor"),
    (lambda: stereo.depth_from_pair(None, None, __import__("panopticnerf_amd").Pinhole(50.0, 50.0, 2.0, 2.0, 5, 4), 0.5, speckle=3), V,
     "stereo.depth_from_pair: speckle must be None or (max_diff, min_size)"),
    (lambda: mesh.from_network(None, (0, 0, 0), (1, 1, 1), 4, 0.5, min_faces=-2), V, "mesh.from_network: min_faces must be an integer >= 0 (got -2)"),
    (lambda: mesh.Mesh.from_arrays(torch.zeros(4, 3), torch.zeros((2, 3), dtype=i32)).select(torch.ones(3, dtype=torch.bool)), V,
     "Mesh.select: face_mask must be a (2,) bool tensor, got torch.bool (3,)"),
]


@pytest.mark.parametrize("call,exc,message", WRAPPERS, ids=[str(i) for i in range(len(WRAPPERS))])
def test_wrappers_refuse_by_name(call, exc, message):
    with pytest.raises(Exception) as e:
        call()
    assert type(e.value) is exc and str(e.value) == message, "%s: %s" % (type(e.value).__name__, e.value)


def test_select_on_the_cpu_is_torch_indexing():
    """Mesh.select launches nothing: it runs wherever the mesh is"""
    m = mesh.Mesh.from_arrays(torch.arange(15, dtype=f32).reshape(5, 3), torch.tensor([[0, 1, 2], [2, 3, 4], [0, 9, 1]], dtype=i32),
                              attributes={"tag": torch.arange(5)})
    s = m.select(torch.tensor([False, True, True]))
    assert s.faces.tolist() == [[0, 1, 2]] and s.attributes["tag"].tolist() == [2, 3, 4] and s.src is None and s.faces.dtype == i32


# ---------------------------------------------------------------------------------------------------------------- the C ABI

def _err(lib):
    return lib.pnr_last_error().decode()


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    null, a, b, c, w = (ctypes.c_void_p(v) for v in (0, 4096, 8192, 16384, 32768))
    odd = ctypes.c_void_p(4098)
    lab = lambda data=a, mode=0, tol=0.0, rx=5, ry=4, rz=3, full=0, labels=b, size=null, count=c, ws=w: \
        lib.pnr_cc_label(data, mode, tol, rx, ry, rz, full, labels, size, count, ws, null)
    for call, words in ((lambda: lab(mode=2), "unknown mode 2"), (lambda: lab(full=2), "full must be 0 or 1 (got 2)"),
                      (lambda: lab(mode=1, tol=-1.0), "tol must be >= 0 and not NaN (got -1)"), (lambda: lab(mode=1, tol=float("nan")), "tol must be >= 0 and not NaN"),
                      (lambda: lab(count=null), "count must be non-null and 8-byte aligned"), (lambda: lab(count=ctypes.c_void_p(16388)), "count must be non-null and 8-byte aligned"),
                      (lambda: lab(rx=-1), "bad lattice -1 x 4 x 3"), (lambda: lab(rx=2 ** 16, ry=2 ** 15, rz=1), "at most 2147483646 points"),
                      (lambda: lab(data=null), "null data, labels or workspace"), (lambda: lab(labels=null), "null data, labels or workspace"),
                      (lambda: lab(ws=null), "null data, labels or workspace"), (lambda: lab(labels=odd), "must be 4-byte aligned"),
                      (lambda: lab(size=odd), "must be 4-byte aligned"), (lambda: lab(ws=ctypes.c_void_p(32772)), "workspace must be 8-byte aligned"),
                      (lambda: lab(labels=a), "may not overlap"), (lambda: lab(labels=ctypes.c_void_p(4096 + 4 * 59)), "may not overlap"),
                      (lambda: lab(size=ctypes.c_void_p(8192 + 4 * 10)), "may not overlap")):
        rc = call()
        assert rc == -1 and words in _err(lib), (rc, words, _err(lib))
    msh = lambda faces=a, nf=6, nv=9, vl=b, fl=c, fs=null, count=w, ws=ctypes.c_void_p(65536): \
        lib.pnr_cc_mesh(faces, nf, nv, vl, fl, fs, count, ws, null)
    for call, words in ((lambda: msh(nf=-1), "n_faces must be within 0 .. 2^31 - 1"), (lambda: msh(nv=2 ** 31 - 1), "n_vertices must be within 0 .. 2^31 - 2"),
                      (lambda: msh(faces=null), "null faces"), (lambda: msh(count=null), "count must be non-null"), (lambda: msh(vl=null), "null vertex_label or face_label"),
                      (lambda: msh(fl=null), "null vertex_label or face_label"), (lambda: msh(fs=odd), "must be 4-byte aligned"),
                      (lambda: msh(fl=ctypes.c_void_p(4096 + 12 * 5)), "may not overlap faces"), (lambda: msh(ws=null), "workspace must be non-null and 8-byte aligned")):
        rc = call()
        assert rc == -1 and words in _err(lib), (rc, words, _err(lib))
    st = lambda labels=a, size=b, rx=5, ry=4, rz=3, n=4, sizes=c, boxes=null: lib.pnr_cc_stats(labels, size, rx, ry, rz, n, sizes, boxes, null)
    for call, words in ((lambda: st(rz=0), "bad lattice 5 x 4 x 0"), (lambda: st(n=-1), "n_components must be within 0 .. 2^31 - 2"), (lambda: st(labels=null), "null labels, size or sizes"),
                      (lambda: st(size=null), "null labels, size or sizes"), (lambda: st(sizes=null), "null labels, size or sizes"), (lambda: st(boxes=odd), "must be 4-byte aligned")):
        rc = call()
        assert rc == -1 and words in _err(lib), (rc, words, _err(lib))
    assert st(n=0, labels=null, size=null, sizes=null) == 0                   # no components: a no-op
    assert lib.pnr_cc_workspace_bytes(-1) == -1 and lib.pnr_cc_workspace_bytes(2 ** 31 - 1) == -1 and lib.pnr_cc_workspace_bytes(0) == 8
