"""CPU tests that pin tests/_cc_ref.py, the restatement of include/pnr.h "connected components", against two independent
implementations: scipy.ndimage.label (binary keys: labels == scipy - 1 exactly, numbering included) and
scipy.sparse.csgraph.connected_components over an explicit edge list built with numpy (multi-key lattices, the values mode and
meshes; compared after renumbering by lowest member), and against the closed forms of synthetic.blobs and of the patterns.
Nothing here touches a GPU."""
import numpy as np
import pytest
import scipy.ndimage as ndi
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import _cc_ref as cr
from panopticnerf_amd import synthetic

TILE_2D, TILE_3D = (8, 4), (4, 4, 2)            # small stand-ins: the GPU tests take the library's own
SHAPES = [(7, 9), (1, 13), (12, 1), (9, 17)] + [(3, 5, 4), (1, 1, 11), (5, 9, 9)]


def _graph_labels(data, mode, tol, full):
    """labels by scipy's graph components over the explicit list of links, renumbered by lowest member"""
    data = np.asarray(data)
    d3 = data.reshape((1,) * (3 - data.ndim) + data.shape)
    fg = cr.foreground(d3, mode)
    idx = np.arange(d3.size).reshape(d3.shape)
    rows, cols = [], []
    for dz, dy, dx in cr.offsets(data.ndim, full):
        src = tuple(slice(max(-d, 0), s - max(d, 0)) for d, s in zip((dz, dy, dx), d3.shape))
        dst = tuple(slice(max(d, 0), s - max(-d, 0)) for d, s in zip((dz, dy, dx), d3.shape))
        a, b = d3[src], d3[dst]
        with np.errstate(invalid="ignore", over="ignore"):
            test = (a == b) if mode == cr.KEYS else (np.abs(a.astype(np.float32) - b.astype(np.float32)) <= np.float32(tol))
        on = fg[src] & fg[dst] & test
        rows.append(idx[src][on])
        cols.append(idx[dst][on])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(d3.size, d3.size))
    _, comp = connected_components(g, directed=False)
    lab, count = cr.renumber(comp, fg.reshape(-1))
    return lab.reshape(data.shape), count


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("full", [False, True])
def test_binary_patterns_equal_scipy_ndimage_label(shape, full):
    rank = len(shape)
    for name, keys in cr.key_patterns(shape, TILE_2D if rank == 2 else TILE_3D).items():
        binary = np.where(keys >= 0, 0, -1).astype(np.int32)
        lab, count, size = cr.label(binary, cr.KEYS, 0.0, full)
        want, n = ndi.label(binary >= 0, ndi.generate_binary_structure(rank, rank if full else 1))
        assert count == n, name
        assert np.array_equal(lab, want.astype(np.int32) - 1), name
        assert np.array_equal(size, np.where(lab >= 0, np.bincount(lab[lab >= 0], minlength=max(count, 1))[np.maximum(lab, 0)], 0)), name


def test_scipy_numbers_components_in_raster_order_of_their_first_element():
    """the claim the numbering rests on, on 32 random masks of both ranks and connectivities"""
    g = np.random.default_rng(5)
    for k in range(32):
        rank = 2 + k % 2
        shape = tuple(int(v) for v in g.integers(3, 9, size=rank))
        mask = g.random(shape) < g.choice([0.3, 0.5, 0.7])
        full = bool((k // 2) % 2)
        want, n = ndi.label(mask, ndi.generate_binary_structure(rank, rank if full else 1))
        first = [int(np.flatnonzero(want.reshape(-1) == c + 1)[0]) for c in range(n)]
        assert first == sorted(first)
        assert np.array_equal(cr.label(np.where(mask, 0, -1), cr.KEYS, 0.0, full)[0], want - 1)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("full", [False, True])
def test_keys_and_values_equal_graph_components(shape, full):
    rank = len(shape)
    for name, keys in cr.key_patterns(shape, TILE_2D if rank == 2 else TILE_3D).items():
        lab, count, _ = cr.label(keys, cr.KEYS, 0.0, full)
        want, n = _graph_labels(keys, cr.KEYS, 0.0, full)
        assert count == n and np.array_equal(lab, want), name
    for name, (values, tol) in cr.value_cases(shape).items():
        lab, count, _ = cr.label(values, cr.VALUES, tol, full)
        want, n = _graph_labels(values, cr.VALUES, tol, full)
        assert count == n and np.array_equal(lab, want), name


def test_closed_forms_of_the_patterns():
    for shape in ((9, 17), (5, 9, 9)):
        rank = len(shape)
        n = int(np.prod(shape))
        for full in (False, True):
            lab = lambda keys: cr.label(keys, cr.KEYS, 0.0, full)
            assert lab(np.full(shape, -1, np.int32))[1] == 0
            l, c, s = lab(np.zeros(shape, np.int32))
            assert c == 1 and (l == 0).all() and (s == n).all()
            assert lab(cr.serpentine(shape))[1] == 1 and lab(cr.spiral(shape))[1] == 1
            assert lab(cr.comb(shape))[1] == 1 and lab(cr.u_shape(shape))[1] == 1
            assert lab(cr.checkerboard(shape))[1] == (1 if full else (n + 1) // 2)
            corner = cr.corner_pair(shape, TILE_2D if rank == 2 else TILE_3D)
            assert lab(corner)[1] == (1 if full else 2)
        # the comb and the U are one piece only through their last row
        for make in (cr.comb, cr.u_shape):
            cut = make(shape)
            cut[..., -1, :] = -1
            assert cr.label(cut, cr.KEYS, 0.0, False)[1] > 1


def test_values_mode_rules():
    cases = cr.value_cases((1, 24))
    for full in (False, True):
        ramp, tol = cases["ramp_at_tol"]
        assert cr.label(ramp, cr.VALUES, tol, full)[1] == 1                  # a step of exactly tol links
        steep, tol = cases["ramp_above_tol"]
        assert cr.label(steep, cr.VALUES, tol, full)[1] == 24                # the next float32 above tol does not
        chain, tol = cases["chain"]
        lab, count, _ = cr.label(chain, cr.VALUES, tol, full)
        assert count == 1 and list(lab[0, :4]) == [0, 0, 0, -1]              # a ~ b ~ c although |a - c| > tol
        holes, _ = cases["holes"]
        lab = cr.label(holes, cr.VALUES, np.float32(np.inf), full)[0]
        assert ((lab >= 0) == (np.isfinite(holes) & (holes > 0))).all() and (lab < 0).sum() >= 6
    quant, _ = cases["tol_zero"]
    assert np.array_equal(cr.label(quant, cr.VALUES, 0.0)[0], cr.label(quant.astype(np.int32), cr.KEYS)[0])


@pytest.mark.parametrize("shape", [(40, 50), (20, 19, 18)])
def test_blobs_have_the_count_and_sizes_they_state(shape):
    for seed in range(4):
        mask, count, sizes = synthetic.blobs(shape, seed)
        assert count >= 2
        keys = np.where(mask.numpy(), 0, -1).astype(np.int32)
        for full in (False, True):
            lab, n, _ = cr.label(keys, cr.KEYS, 0.0, full)
            assert n == count and np.array_equal(cr.stats(lab, n)[0], sizes)


def _mesh_graph(faces, V):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < V)).all(axis=1) if len(faces) else np.zeros(0, bool)
    f = faces[ok]
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V))
    _, comp = connected_components(g, directed=False)
    used = np.zeros(V, bool)
    used[f.reshape(-1)] = True
    return cr.renumber(comp, used), ok


def test_meshes_equal_graph_components():
    g = np.random.default_rng(2)
    ico, box = synthetic.icosphere(1), synthetic.box_mesh((2, 2, 2), (3, 3, 3))
    faces = np.concatenate([ico.faces.numpy(), box.faces.numpy() + ico.vertices.shape[0]])
    V = ico.vertices.shape[0] + 8
    cases = [(faces, V), (faces[g.permutation(len(faces))], V), (g.permutation(V).astype(np.int32)[faces], V), (faces, V + 5),
             (np.concatenate([faces, [[0, 1, V], [-1, 2, 3]]]).astype(np.int32), V), (np.zeros((0, 3), np.int32), 4),
             (g.integers(0, 60, size=(25, 3)).astype(np.int32), 60)]
    for f, v in cases:
        vlab, flab, fsize, count = cr.label_mesh(f, v)
        (want, n), ok = _mesh_graph(f, v)
        assert count == n and np.array_equal(vlab, want)
        assert np.array_equal(flab, np.where(ok, want[np.clip(np.asarray(f).reshape(-1, 3)[:, 0], 0, v - 1)], -1))
        assert np.array_equal(fsize, np.where(flab >= 0, np.bincount(flab[flab >= 0], minlength=max(count, 1))[np.maximum(flab, 0)], 0))
    vlab, flab, fsize, count = cr.label_mesh(faces, V)
    assert count == 2 and set(fsize[:80]) == {80} and set(fsize[80:]) == {12}           # 20 * 4 faces and 12, in closed form
