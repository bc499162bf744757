"""GPU parity of the mesh extractor (csrc/pnr_mesh.hip) with tests/_mesh_ref.py.  The rule fixes every operation and the numbering
of vertices and triangles, so totals, vertices, faces and src are compared with torch.equal (the vertices on their bit
patterns) -- no tolerance anywhere.  Every caller-owned buffer, the workspace included, sits between canaries."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _mesh_ref as R
from panopticnerf_amd import Pinhole, make_network, mesh, ops, pointcloud, synthetic

pytestmark = pytest.mark.gpu

PAD = 64                # canary elements on each side (at least 64 bytes: the workspace inside stays 16-byte aligned)
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
ANISO = ((-3.0, 0.5, 10.0), (2.0, 0.75, 47.0))
# launch constants of csrc/pnr_mesh.hip
MESH_CHUNK = 1024               # PNR_MESH_CHUNK: points per block trip, and per entry of the chunk-sum level
MESH_BLOCKS_PER_CU = 8          # PNR_MESH_BLOCKS_PER_CU: the per-point kernels' grid is min(chunks, this x compute units)
MESH_SCAN_TILE = 256 * 4        # PNR_MESH_BLOCK x PNR_MESH_SCAN_ITEMS: chunk sums per trip of the one-block scan


class Guarded:
    """a caller-owned output inside a larger buffer of a known value"""

    def __init__(self, shape, dtype, dev, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
        self.fill = fill
        self.t = self.buf[PAD:PAD + n].view(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == self.fill).all()) and bool((self.buf[-PAD:] == self.fill).all())


def gpu_extract(field, lo, hi, level, dev, want_src=True):
    """count and emit through ops with every buffer guarded; returns (vertices, faces, src, totals) as they lie on the device"""
    f = field if isinstance(field, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(field)).to(dev)
    rz, ry, rx = f.shape
    ws = Guarded((ops.mesh_workspace_bytes(rx, ry, rz),), torch.uint8, dev, 0xA5)
    tot = Guarded((2,), torch.int64, dev, -77)
    totals, workspace = ops.mesh_count(f, level, workspace=ws.t, totals=tot.t)
    assert totals.data_ptr() == tot.t.data_ptr() and workspace.data_ptr() == ws.t.data_ptr()
    n_v, n_t = totals.tolist()
    assert ws.intact() and tot.intact()
    v = Guarded((n_v, 3), torch.float32, dev, 12345.0)
    t = Guarded((n_t, 3), torch.int32, dev, -99)
    s = Guarded((n_v,), torch.int64, dev, -98) if want_src else None
    lo32, step = mesh.lattice(lo, hi, (rx, ry, rz))
    ops.mesh_emit(f, level, lo32, step, ws.t, v.t, t.t, None if s is None else s.t)
    torch.cuda.synchronize()
    assert v.intact() and t.intact() and ws.intact() and tot.intact() and (s is None or s.intact())
    return v.t, t.t, None if s is None else s.t, (n_v, n_t)


def same_bits(got, want, dev):
    v, t, s = got[:3]
    wv, wt, ws = (torch.from_numpy(a).to(dev) for a in want)
    return (v.shape == wv.shape and torch.equal(v.view(torch.int32), wv.view(torch.int32)) and t.shape == wt.shape and torch.equal(t, wt)
            and (s is None or torch.equal(s, ws)))


def check(dev, field, lo, hi, level):
    want = R.extract(field, lo, hi, level)
    got = gpu_extract(field, lo, hi, level, dev)
    assert got[3] == (len(want[0]), len(want[1])), (field.shape, level, got[3])
    assert same_bits(got, want, dev), (field.shape, level)
    return got, want


# ---------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("level", [0.0, 0.7])
@pytest.mark.parametrize("shape", [(2, 2, 2), (1, 5, 5), (2, 3, 2), (3, 3, 3), (5, 9, 17), (31, 33, 65), (63, 64, 65)])
def test_noise_equals_the_reference(dev, shape, level):
    """Gaussian noise meets all 16 cases of all six tetrahedra (tests/test_mesh_ref.py checks that it does)"""
    f = np.random.default_rng(sum(shape) + shape[2]).standard_normal(shape).astype(np.float32)
    (v, t, s, (n_v, n_t)), _ = check(dev, f, *UNIT, level)
    if min(shape) < 2:
        assert (n_v, n_t) == (0, 0)
    else:
        assert n_v > 0 and n_t > 0


def test_sphere_and_torus_equal_the_reference(dev):
    for res in (8, 16, 32):
        check(dev, synthetic.sdf_grid("sphere", *UNIT, res, radius=0.7).numpy(), *UNIT, 0.0)
    check(dev, synthetic.sdf_grid("torus", *UNIT, 16, radius=0.6, minor=0.25).numpy(), *UNIT, 0.0)
    check(dev, synthetic.sdf_grid("box", *UNIT, (13, 16, 11), half=(0.5, 0.4, 0.3)).numpy(), *UNIT, 0.0)
    for c in (0.1, -0.37, 0.125):               # the plane x = c: every vertex has x == c to one rounding, on the device's output
        (v, t, s, _), _ = check(dev, synthetic.sdf_grid("plane", *UNIT, (8, 5, 6), offset=c).numpy(), *UNIT, 0.0)
        assert v.shape[0] > 0 and float((v[:, 0].double() - float(np.float32(c))).abs().max()) <= float(np.spacing(np.float32(abs(c))))


@pytest.mark.parametrize("const", [1.0, -1.0, 0.25, float("nan"), float("inf"), float("-inf")])
def test_constant_lattices_give_zero_rows(dev, const):
    """all inside, all outside, all equal to the level, all NaN: zero-row outputs, NULL pointers into the entry point"""
    f = np.full((7, 6, 37), const, np.float32)
    (v, t, s, totals), _ = check(dev, f, *UNIT, 0.25)
    assert totals == (0, 0) and v.shape == (0, 3) and t.shape == (0, 3) and s.shape == (0,)


@pytest.mark.parametrize("shape", [(4, 5, 6), (9, 17, 33)])
def test_non_finite_and_equal_values(dev, shape):
    rng = np.random.default_rng(shape[0])
    f = rng.standard_normal(shape).astype(np.float32)
    flat = f.reshape(-1)
    n = flat.size // 4
    flat[rng.choice(flat.size, n, replace=False)] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.25, 0.25], np.float32), n)
    for level in (0.25, 0.0):
        (v, t, s, _), want = check(dev, f, *ANISO, level)
        assert bool(torch.isfinite(v).all())
    # the hand cases of the rule: (owner value, far value) -> t
    for fa, fb, t_want in ((-np.inf, 1.0, 0.5), (0.0, np.inf, 0.0), (np.inf, 0.0, 0.5), (1.0, -np.inf, 0.0), (np.nan, 1.0, 0.5), (1.0, np.nan, 0.5),
                           (0.5, 1.0, 0.0), (1.0, 0.5, 1.0)):
        g = np.full((2, 2, 2), fa, np.float32)
        g[:, :, 1] = fb
        (v, t, s, totals), _ = check(dev, g, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0), 0.5)
        assert totals[0] == 9 and v[:, 0].tolist() == [0.5 + t_want] * 9, (fa, fb)


@pytest.mark.parametrize("lo,hi", [ANISO, ((1e-3, 1e3, -7.0), (2e-3, 1e3 + 1, 9.0)), ((1.0, 1.0, 1.0), (-1.0, -2.0, 0.0))])
def test_anisotropic_boxes(dev, lo, hi):
    """unequal steps, a box far from the origin next to a thin one, and a box given upside down (negative steps)"""
    f = np.random.default_rng(8).standard_normal((6, 11, 21)).astype(np.float32)
    check(dev, f, lo, hi, 0.1)
    got = gpu_extract(f, lo, hi, 0.1, dev, want_src=False)          # src is optional
    assert same_bits(got, R.extract(f, lo, hi, 0.1), dev)


def test_one_larger_lattice(dev):
    """A lattice sized from the kernels' launch constants (at the top of this file) so that the per-point kernels' capped grid
    -- MESH_BLOCKS_PER_CU blocks a compute unit, MESH_CHUNK points a block trip -- walks every grid-stride loop at least three
    times, and the chunk-sum level has more than two tiles of the one-block scan (far more than three entries): a rough sphere."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    need = MESH_CHUNK * max(2 * MESH_BLOCKS_PER_CU * cus, 2 * MESH_SCAN_TILE) + 1
    side = int(round(need ** (1.0 / 3.0)))
    while side ** 3 < need:
        side += 1
    res = (side, side + 2, side - 1)
    while res[0] * res[1] * res[2] < need:
        res = (res[0] + 1, res[1], res[2])
    n = res[0] * res[1] * res[2]
    chunks = -(-n // MESH_CHUNK)
    assert -(-chunks // min(chunks, MESH_BLOCKS_PER_CU * cus)) >= 3 and -(-chunks // MESH_SCAN_TILE) >= 3 and chunks >= 3
    f = synthetic.sdf_grid("sphere", *UNIT, res, radius=0.8).numpy()
    f += 0.02 * np.random.default_rng(1).standard_normal(f.shape).astype(np.float32)
    (v, t, s, totals), want = check(dev, f, *UNIT, 0.0)
    assert totals[0] > 100000 and totals[1] > 200000
    own = want[2] // (res[0] * res[1])
    assert own.min() < res[2] // 4 and own.max() > 3 * res[2] // 4          # the surface spans the chunks


# ---------------------------------------------------------------- repeatability
def test_a_second_call_gives_the_same_bits(dev):
    f = np.random.default_rng(4).standard_normal((33, 31, 29)).astype(np.float32)
    a = gpu_extract(f, *ANISO, 0.3, dev)
    b = gpu_extract(f, *ANISO, 0.3, dev)
    assert a[3] == b[3] and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_count_and_emit_in_a_captured_graph_follow_the_field(dev):
    rng = np.random.default_rng(6)
    f0 = rng.standard_normal((17, 18, 19)).astype(np.float32)
    f1 = np.where(f0 > 0, f0 * np.float32(3.0), f0).astype(np.float32)          # the same inside set, so the same totals; other positions
    want0, want1 = R.extract(f0, *ANISO, 0.0), R.extract(f1, *ANISO, 0.0)
    assert len(want0[0]) == len(want1[0]) and np.array_equal(want0[1], want1[1]) and not np.array_equal(want0[0], want1[0])
    field = torch.from_numpy(f0).to(dev)
    lo32, step = mesh.lattice(*ANISO, (19, 18, 17))
    totals, ws = ops.mesh_count(field, 0.0)                      # warm call: module loading is not capturable
    n_v, n_t = totals.tolist()
    v = Guarded((n_v, 3), torch.float32, dev, 5.0)
    t = Guarded((n_t, 3), torch.int32, dev, -9)
    s = Guarded((n_v,), torch.int64, dev, -8)
    ops.mesh_emit(field, 0.0, lo32, step, ws, v.t, t.t, s.t)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.mesh_count(field, 0.0, workspace=ws, totals=totals)
        ops.mesh_emit(field, 0.0, lo32, step, ws, v.t, t.t, s.t)
    for f, want in ((f0, want0), (f1, want1), (f0, want0)):
        field.copy_(torch.from_numpy(f))
        v.t.fill_(5.0)
        totals.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert totals.tolist() == [n_v, n_t] and v.intact() and t.intact() and s.intact()
        assert same_bits((v.t, t.t, s.t), want, dev)


# ---------------------------------------------------------------- the whole path
def test_extract_on_the_sphere_passes_the_closed_forms(dev):
    exact = 4.0 / 3.0 * np.pi * 0.7 ** 3
    errs = []
    for res in (8, 16, 32):
        f = synthetic.sdf_grid("sphere", *UNIT, res, radius=0.7, device=dev)
        m = mesh.extract(f, *UNIT, 0.0)
        assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.src.dtype == torch.int64
        assert m.vertices.is_cuda and m.faces.is_cuda and m.src.is_cuda and m.res == (res, res, res)
        v, t = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
        assert R.is_closed_oriented(t, len(v)) and R.euler(t) == 2
        vol = m.volume()
        assert vol > 0 and abs(vol - R.volume(v, t)) <= 1e-12
        errs.append((vol - exact) / exact)
        h = 2.0 / res
        assert float((m.vertices.double().norm(dim=1) - 0.7).abs().max()) <= h * h
        assert bool((m.labels(f) > 0).all()) and torch.equal(m.labels(f), f.reshape(-1)[m.src])
        assert abs(m.area() - R.area(v, t)) <= 1e-9
    assert 3.0 < errs[0] / errs[1] < 5.0 and 3.0 < errs[1] / errs[2] < 5.0
    # one inside point: 14 vertices, 24 triangles, volume 0.5
    f = torch.zeros(3, 3, 3, device=dev)
    f[1, 1, 1] = 1.0
    m = mesh.extract(f, (-0.5,) * 3, (2.5,) * 3, 0.5)
    assert (m.vertices.shape[0], m.faces.shape[0]) == (14, 24) and abs(m.volume() - 0.5) < 1e-6 and set(m.src.tolist()) == {13}
    # no cube: an empty mesh, not an error
    m = mesh.extract(torch.randn(1, 5, 5, device=dev), *UNIT, 0.0)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.src.shape == (0,) and m.volume() == 0.0


def test_from_network_labels_and_splat(dev):
    torch.manual_seed(3)
    net = make_network(NS(D=2, W=128, skips=[], N_importance=0, num_classes=5, num_instances=3)).to(dev).eval()
    lo, hi, res = (-1.0, -0.5, 2.0), (1.0, 1.5, 4.0), (12, 10, 9)
    grid = net.query_grid(lo, hi, res, want=("sigma", "labels", "panoptic"))
    level = float(grid["sigma"].median())
    m = mesh.from_network(net, lo, hi, res, level)
    assert m.vertices.shape[0] > 0 and m.faces.shape[0] > 0
    assert set(m.attributes) == {"sigma", "sem_label", "inst_label", "panoptic"}
    for k in ("sigma", "sem_label", "inst_label", "panoptic"):
        assert torch.equal(m.grid[k], grid[k])
        assert torch.equal(m.attributes[k], grid[k].reshape(-1)[m.src]) and torch.equal(m.attributes[k], m.labels(grid[k]))
    assert bool((m.attributes["sigma"] > level).all())
    assert same_bits((m.vertices, m.faces, m.src), R.extract(grid["sigma"].cpu().numpy(), lo, hi, level), dev)
    # the vertices as a cloud into a pinhole view looking down +z from the origin
    cam = Pinhole(40.0, 40.0, 31.5, 23.5, 64, 48)
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    view = pointcloud.splat(cam, c2w, m.vertices, labels=m.attributes["sem_label"])
    assert int(view["valid"].sum()) > 0
    seen = view["valid"]
    assert bool((view["depth"][seen] >= 2.0).all()) and bool((view["depth"][seen] <= 4.0).all())
    assert torch.equal(view["label"][seen], m.attributes["sem_label"][view["index"][seen].long()])
