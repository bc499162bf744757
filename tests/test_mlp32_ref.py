"""CPU pins of the float64 reference of the fp32 parity mode (tests/_mlp32_ref.py): it agrees with float64 autograd through the
independent torch oracle; the numpy float32 restatement of the kernels' GEMM order passes every check at a quarter of its bound;
seven corrupted variants of that restatement fail; and the two size functions of the library -- host code, no GPU -- equal the
ledgers restated here from the network's shape (include/pnr.h: the acts layout, the backward's workspace)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _mlp32_ref as m32
from oracle import c_oracle as co
from oracle import torch_oracle as to
from panopticnerf_amd import _lib, ops


def _rays(rng, R, near=0.5, far=8.0):
    o = rng.normal(0, 1, (R, 3)) + np.array([0, 1.5, 0])
    d = rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])
    return np.concatenate([o, d, np.full((R, 1), near), np.full((R, 1), far)], 1).astype(np.float32)


GEOMS = {  # D, W, skip, xyz_L, dir_L, C, K, tap, depth
    "skip": (3, 128, 0, 10, 4, 5, 3, "trunk", 2),          # ex = 63: three full k-tiles and one of 15
    "depth1": (2, 128, -1, 4, 0, 3, 0, "feature", 1),
}


def _case(geom, R, N, seed=0):
    D, W, skip, Lx, Ld, C, K, tap, depth = geom
    cfg = to.mlp_config(D=D, W=W, skips=(skip,) if skip >= 0 else (), xyz_L=Lx, dir_L=Ld, n_sem=C, n_inst=K, head_W=W // 2,
                        head_tap=tap, head_depth=depth)
    params = to.init_params(cfg, seed=seed)
    desc = ops.make_desc(D, W, skip, Lx, Ld, C, K, W // 2, "fp32", tap, depth)
    rng = np.random.default_rng(seed + 11)
    rays = _rays(rng, R)
    z = co.stratified(rays, N, t_rand=rng.random((R, N)).astype(np.float32))
    d_raw = torch.from_numpy(rng.normal(size=(R * N, 4 + C + K)).astype(np.float32))
    return dict(cfg=cfg, params=params, desc=desc, rays=torch.from_numpy(rays), z=torch.from_numpy(z), d_raw=d_raw, S=R * N)


def _honest(c):
    raw, acts = m32.forward32(c["desc"], c["params"], c["rays"].numpy(), c["z"].numpy())
    c["raw"], c["acts"] = torch.from_numpy(raw), torch.from_numpy(acts)
    return c


@pytest.fixture(scope="module")
def skip_case():
    return _honest(_case(GEOMS["skip"], 7, 41))


@pytest.fixture(scope="module")
def slab_case():
    return _honest(_case(GEOMS["depth1"], 14, 151))        # S = 2114: a second slab of one full 64-row tile and two samples


def _fwd(c, raw=None, acts=None):
    return m32.check_forward(m32.Report(), c["desc"], c["params"], c["rays"], c["z"], c["raw"] if raw is None else raw,
                             c["acts"] if acts is None else acts)


def _bwd(c, grads, d_raw=None):
    g = {k: torch.from_numpy(v) for k, v in grads.items()}
    return m32.check_backward(m32.Report(), c["desc"], c["params"], c["acts"], c["d_raw"] if d_raw is None else d_raw, g, c["S"])


def _failed(rep, *regions):
    return any(f.startswith(r + ":") for f in rep.fails for r in regions)


# ------------------------------------------------------------------------------------------- the reference is a reference
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_reference_agrees_with_float64_autograd(geom):
    """chain64 + backward64 against torch_oracle.run_network and its autograd, everything float64: raw and every gradient to
    1e-12 of the tensor's scale"""
    c = _case(GEOMS[geom], 5, 13, seed=3)
    p64 = {k: v.double().requires_grad_(True) for k, v in c["params"].items()}
    raw_ref = to.run_network(p64, c["cfg"], c["rays"].double(), c["z"].double())
    (raw_ref * c["d_raw"].double().reshape(raw_ref.shape)).sum().backward()
    X, raw = m32.chain64(c["desc"], c["params"], c["rays"], c["z"])
    assert (raw - raw_ref.detach().reshape(raw.shape)).abs().max() <= 1e-12 * raw_ref.abs().max()
    ref = m32.backward64(c["desc"], m32.Net(c["desc"], c["params"], "cpu"), X, c["d_raw"].double())
    assert set(ref) == set(p64)
    for k, (r, A) in ref.items():
        assert (r - p64[k].grad).abs().max() <= 1e-12 * p64[k].grad.abs().max(), k
        assert (r.abs() <= A * (1 + 1e-12)).all(), k           # A bounds the value it is the condition of


def test_path_lengths_from_the_descriptor():
    """P by hand for the two geometries (W = 128, H = 64)"""
    P = m32.path_lengths(_case(GEOMS["skip"], 1, 1)["desc"])          # deep heads of 5 and 3 on the trunk output
    assert P["views_linears.0"] == 3 and P["semantic_linears.0"] == 5 and P["instance_linears.0"] == 3
    assert P["feature_linear"] == 3 + 64                             # rgb (3) -> views (64), nothing accumulated into d F
    # d h: heads (5 + 64, 3 + 64), feature (67 + 128), alpha (1): four launches, three of them accumulate
    assert P["pts_linears.2"] == 67 + 128 + 3 and P["pts_linears.1"] == P["pts_linears.2"] + 128 and P["pts_linears.0"] == P["pts_linears.2"] + 256
    assert all(P[k] == 0 for k in ("rgb_linear", "alpha_linear", "semantic_linears.1", "instance_linears.1"))
    P = m32.path_lengths(_case(GEOMS["depth1"], 1, 1)["desc"])        # one Linear 128 -> 3 on the feature
    assert P["semantic_linears.0"] == 0 and P["feature_linear"] == 67 + 1 and P["pts_linears.1"] == 68 + 128 + 1


# --------------------------------------------------------------------------------------- the float32 restatement passes
def _quarter(rep):
    rep.check()
    worst = {k: v for k, v in rep.worst.items() if k != "trig abs"}
    assert worst and max(worst.values()) <= 0.25, worst


def test_float32_restatement_passes_at_a_quarter_of_every_bound(skip_case, slab_case):
    for c in (skip_case, slab_case):
        _quarter(_fwd(c))
        grads = m32.backward32(c["desc"], c["params"], c["acts"].numpy(), c["d_raw"].numpy())
        assert set(grads) == set(c["params"])
        _quarter(_bwd(c, grads))


# ------------------------------------------------------------------------------------------ corrupted variants must fail
@pytest.mark.parametrize("corrupt,region", [("ktile", "X1"), ("skip_bias", "X2"), ("skip_order", "X2")])
def test_corrupted_forward_fails(skip_case, corrupt, region):
    """the last k-tile of the 63-wide reduction dropped; the bias left out of the skip layer's second launch; the skip concat in the
    wrong order.  Layer-local: the layers behind the wrong one read its (wrong) output and still pass."""
    c = skip_case
    raw, acts = m32.forward32(c["desc"], c["params"], c["rays"].numpy(), c["z"].numpy(), corrupt=corrupt)
    rep = _fwd(c, torch.from_numpy(raw), torch.from_numpy(acts))
    assert _failed(rep, region) and all(f.startswith(region + ":") for f in rep.fails), rep.fails


def test_corrupted_gate_fails(skip_case):
    """the top trunk dY gated by X_{D-1} instead of X_D"""
    c = skip_case
    rep = _bwd(c, m32.backward32(c["desc"], c["params"], c["acts"].numpy(), c["d_raw"].numpy(), corrupt="gate"))
    assert _failed(rep, "pts_linears.2.weight") and _failed(rep, "pts_linears.0.bias")
    assert not _failed(rep, "feature_linear.weight", "views_linears.0.weight", "rgb_linear.weight")


def test_one_wrong_row_of_the_direction_columns_fails(skip_case):
    c = skip_case
    rep = _bwd(c, m32.backward32(c["desc"], c["params"], c["acts"].numpy(), c["d_raw"].numpy(), corrupt="views_row"))
    assert len(rep.fails) == 1 and _failed(rep, "views_linears.0.weight"), rep.fails
    assert " of %d fp32 values off" % (64 * (128 + 27)) in rep.fails[0] and int(rep.fails[0].split()[1]) <= 27


@pytest.mark.parametrize("corrupt,kind", [("drop_sample", "tile"), ("slab_twice", "slab")])
def test_corrupted_tail_slab_fails_under_the_localised_d_raw(slab_case, corrupt, kind):
    """one sample dropped from the last slab; the last slab counted twice.  With d_raw zero outside the tail the honest
    restatement still passes at a quarter of the bounds and every gradient tensor of the corrupted one fails."""
    c = slab_case
    d_raw = m32.localise(c["d_raw"], kind)
    assert int((d_raw != 0).any(1).sum()) == {"tile": 2, "slab": 66}[kind]
    _quarter(_bwd(c, m32.backward32(c["desc"], c["params"], c["acts"].numpy(), d_raw.numpy()), d_raw))
    rep = _bwd(c, m32.backward32(c["desc"], c["params"], c["acts"].numpy(), d_raw.numpy(), corrupt=corrupt), d_raw)
    assert all(_failed(rep, k) for k in c["params"] if k.endswith(".bias")), rep.fails
    assert _failed(rep, "pts_linears.0.weight", "rgb_linear.weight")


# ------------------------------------------------------------------------------------------------------------- ledgers
HEADS = (0, 1, 64, 65, 131, 132, 190, 191, 192, 256)
SAMPLES = (1, 2048, 2049, 4101)


def _descs():
    for W, Lx, Ld, depth, tap in itertools.product((128, 256), (0, 4, 10), (0, 4), (1, 2), ("trunk", "feature")):
        for C, K in itertools.product(HEADS, HEADS):
            yield ops.make_desc(3, W, 1, Lx, Ld, C, K, W // 2, "fp32", tap, depth)
    for D, skip in ((2, -1), (2, 0), (8, 4), (16, -1)):
        for C in (0, 200):
            yield ops.make_desc(D, 128, skip, 10, 4, C, 0, 64, "fp32", "trunk", 1)


def test_workspace_and_acts_sizes_equal_their_ledgers():
    """pnr_mlp_backward_fp32_workspace_bytes == 4 (S (3 W + 2 H) + n_slab max over the weight-gradient launches of (n_out k +
    [bias] n_out)), and the last region of the documented acts layout ends at pnr_mlp_fp32_acts_floats.  Until the head_depth-1
    Linears (n_out = n_sem or n_inst, k = W) were counted, the library returned less than the launches write at W = 128 from
    n = 132 (xyz_L = dir_L = 0), 155 (a widest embedding of 27 columns) and 191 (xyz_L = 10) upward: 2968 of the shapes below, by
    up to 189 KiB (n = 256, three slabs)."""
    lib = _lib.load()
    short, wrong, acts_wrong, n = [], [], [], 0
    for desc in _descs():
        for S in SAMPLES:
            n += 1
            key = (desc.W, desc.xyz_L, desc.dir_L, desc.head_depth, desc.head_tap, desc.n_sem, desc.n_inst, S)
            got, need = int(lib.pnr_mlp_backward_fp32_workspace_bytes(ctypes.byref(desc), S)), m32.workspace_bytes(desc, S)
            if got < need:
                short.append((key, got, need))
            elif got != need:
                wrong.append((key, got, need))
            if int(lib.pnr_mlp_fp32_acts_floats(ctypes.byref(desc), S)) != m32.acts_regions(desc, S)[1]:
                acts_wrong.append(key)
    assert n > 19000
    assert not short, "%d descriptors whose workspace is SMALLER than one launch's partials, first %s" % (len(short), short[:3])
    assert not wrong, "%d descriptors off the ledger, first %s" % (len(wrong), wrong[:3])
    assert not acts_wrong, acts_wrong[:3]


def test_ledger_launches_by_hand():
    """the launch list for one network written out by hand: D = 3, W = 128, skip 1, ex = 63, ed = 27, one Linear 128 -> 200"""
    desc = ops.make_desc(3, 128, 1, 10, 4, 200, 0, 64, "fp32", "trunk", 1)
    assert sorted(m32.wgrad_launches(desc)) == sorted([
        (128, 63, True), (128, 128, True), (128, 63, False), (128, 128, True),       # pts 0, 1, 2 = [gamma(x) | X_2]
        (1, 128, True), (128, 128, True), (64, 128, True), (64, 27, False), (3, 64, True), (200, 128, True)])
    assert m32.workspace_bytes(desc, 4101) == 4 * (4101 * (384 + 128) + 3 * 200 * 129)
    assert m32.workspace_bytes(desc, 4101) > m32.parent_workspace_bytes(desc, 4101)
    reg, total = m32.acts_regions(desc, 10)
    assert list(reg) == ["EX", "ED", "X1", "X2", "X3", "F", "G"] and total == 10 * (63 + 27 + 4 * 128 + 64)
    reg, total = m32.acts_regions(ops.make_desc(2, 256, -1, 0, 0, 0, 7, 128, "fp32", "feature", 2), 3)
    assert reg["SH_inst"] == (3 * (3 + 3 + 3 * 256 + 128), 128) and "SH_sem" not in reg and total == 3 * (6 + 768 + 256)
