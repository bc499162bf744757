"""CPU pins of the probe networks of tests/_mlp_probe.py, with launch = _mlp32_ref.forward32 (the numpy float32 restatement, NOT
the inference kernel: this validates the probe weights and the checker, the GPU sweep validates the kernel):
  * every probe returns the region of forward32's own acts bit for bit, at all 14 geometries of the fp32 training sweep, S = 35;
  * the whole checker passes on forward32, with and without the G readout;
  * the checker fails, naming the region, for six corrupted launchers;
  * the two-step rgb bound (no G readout) against the old bar 1e-4 max(1, |rgb|): 0.97 on the case below (asserted below 1), but
    1.3 ... 4.5 at other geometries of the sweep (its rgb row measures 7e-4 of it): it is not tighter than the old bar everywhere,
    so the GPU sweep reads G out at EVERY geometry and keeps the two-step bound only where it varies sizes and edge inputs;
  * fma32 is a single-rounding fused multiply-add, and kernel_order visits every column of a segment once."""
import math

import numpy as np
import pytest
import torch

import _mlp32_ref as m32
import _mlp_probe as mp
from test_gpu_mlp_fp32_sweep import GEOMS, _ID, make_case

R, N = 5, 7                                      # S = 35: a full 32-sample tile and a second one of three samples
SKIP = (3, 128, 0, 10, 4, 5, 3, "trunk", 2)      # test_mlp32_ref.py's skip case: ex = 63, the skip layer right behind layer 0


def launch32(desc, params, rays, z, corrupt=None):
    return torch.from_numpy(m32.forward32(desc, params, rays.numpy(), z.numpy(), corrupt=corrupt)[0])


@pytest.mark.parametrize("geom", GEOMS, ids=_ID)
def test_every_probe_returns_the_region_bit_for_bit(geom):
    c = make_case(geom, R, N, seed=GEOMS.index(geom))
    desc, S = c["desc"], c["S"]
    mp.assert_normal(desc, c["params"], c["rays"], c["z"])
    raw, acts = m32.forward32(desc, c["params"], c["rays"].numpy(), c["z"].numpy())
    want = m32.read_acts(desc, S, torch.from_numpy(acts))
    X = mp.read_out(launch32, mp.probes(desc, c["params"], full_G=True), c["rays"], c["z"], real=torch.from_numpy(raw))
    assert set(X) == set(want)
    for nm in want:
        assert X[nm].shape == want[nm].shape and torch.equal(X[nm], want[nm]), nm
    assert torch.equal(mp.assemble_acts(desc, S, X), torch.from_numpy(acts))


@pytest.fixture(scope="module")
def skip_case():
    return make_case(SKIP, R, N, seed=0)


def _check(c, launch, **kw):
    rep = m32.Report()
    mp.check(rep, launch, c["desc"], c["params"], c["rays"], c["z"], **kw)
    return rep


def _regions(rep):
    return {f.split(":")[0] for f in rep.fails}


@pytest.mark.parametrize("full_G", [False, True])
def test_checker_passes_on_the_restatement(skip_case, full_G):
    rep = _check(skip_case, launch32, full_G=full_G)
    rep.check()
    worst = {k: v for k, v in rep.worst.items() if k not in ("trig abs", "two-step rgb bound / (1e-4 max(1, |rgb|))")}
    assert worst and max(worst.values()) <= 0.25, worst
    if not full_G:
        assert rep.worst["two-step rgb bound / (1e-4 max(1, |rgb|))"] < 1.0, rep.worst


def test_checker_on_the_heads_alone_reads_only_their_regions(skip_case):
    c, seen = skip_case, []

    def launch(desc, params, rays, z):
        seen.append((desc.D, desc.n_sem, desc.n_inst, desc.head_depth))
        return launch32(desc, params, rays, z)
    only = {"semantic_linears.0", "semantic_linears.1", "instance_linears.0", "instance_linears.1"}
    assert mp.regions_of(c["desc"], only) == {"X3", "SH_sem", "SH_inst"}
    _check(c, launch, only=only).check()
    assert seen == [(3, 5, 3, 2), (3, 128, 0, 1), (3, 64, 64, 2)]


def _off_by_one_head(desc, params, rays, z):
    """store_raw_block's `lim` off for a last block that is not full: the rows of a head whose width is no multiple of 32 land one
    channel late (the probes' heads are W or W / 2 wide: full blocks)"""
    raw = launch32(desc, params, rays, z)
    if desc.n_sem % 32:
        raw[:, 5:4 + desc.n_sem] = raw[:, 4:3 + desc.n_sem].clone()
    return raw


def _neighbour_sample(desc, params, rays, z):
    """sample 33 -- the second tile -- evaluated at sample 34's inputs, in every launch"""
    raw = launch32(desc, params, rays, z)
    raw[33] = raw[34]
    return raw


CORRUPT = {
    # pts_linears.0 IS the EX probe's layer: the dropped columns read as 0, and the skip layer, which sees them, disagrees too
    "ktile": (lambda *a: launch32(*a, corrupt="ktile"), {"EX"}, {"EX", "X1", "X2"}),
    "skip_bias": (lambda *a: launch32(*a, corrupt="skip_bias"), {"X2"}, {"X2"}),
    "skip_order": (lambda *a: launch32(*a, corrupt="skip_order"), {"X2"}, {"X2"}),
    "head_row_one_off": (_off_by_one_head, {"raw[semantic_linears.1]"}, {"raw[semantic_linears.1]", "raw[instance_linears.1]"}),
    "band_swap": (lambda *a: launch32(*a, corrupt="band_swap"), {"EX"}, {"EX"}),
    "neighbour_sample": (_neighbour_sample, {"EX"}, {"EX"}),
}


@pytest.mark.parametrize("what", sorted(CORRUPT))
def test_corrupted_launcher_fails_by_name(skip_case, what):
    """layer-local: the layers behind the wrong one read its (wrong) output and still pass"""
    launch, must, may = CORRUPT[what]
    rep = _check(skip_case, launch)
    assert must <= _regions(rep) <= may, rep.fails


def test_fma32_rounds_once():
    """a b + c on a float32 midpoint in float64 arithmetic: the exact sum is just beyond it"""
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)          # a b = 1 + 2^-11 + 2^-24
    c = np.float32(2.0 ** -60)
    got = mp.fma32(np.array([a, a]), np.array([b, b]), np.array([c, -c]))
    lo = np.float32(1 + 2.0 ** -11)
    assert got[0] == np.nextafter(lo, np.float32(2)) and got[1] == lo
    assert (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32) == lo      # plain double rounding ties to even
    rng = np.random.default_rng(0)
    x, y, z = (rng.normal(size=4096).astype(np.float32) for _ in range(3))
    if hasattr(math, "fma"):
        ref = np.array([np.float32(math.fma(float(p), float(q), float(r))) for p, q, r in zip(x, y, z)])     # (one more rounding: ties only)
        assert (mp.fma32(x, y, z) != ref).sum() <= 1


@pytest.mark.parametrize("kind,L,width,n", [("gx", 10, 0, 63), ("gx", 4, 0, 27), ("gx", 0, 0, 3), ("gd", 4, 0, 27), ("gd", 0, 0, 3),
                                            ("feat", 0, 128, 128), ("feat", 0, 256, 256)])
def test_kernel_order_visits_every_column_once(kind, L, width, n):
    order = mp.kernel_order(kind, L, width)
    assert sorted(order) == list(range(n))
    if kind == "feat":
        assert order[:4] == [0, 4, 1, 5]             # slot v of the two half-waves: rows row(v, 0), row(v, 1) = row(v, 0) + 4


def test_layer32_equals_the_plain_chain_up_to_order(skip_case):
    """the kernel-order restatement of pts_linears.0 is inside check_linear's bound of float64 and differs from the ascending-k chain
    only by rounding"""
    c = skip_case
    raw, acts = m32.forward32(c["desc"], c["params"], c["rays"].numpy(), c["z"].numpy())
    X = m32.read_acts(c["desc"], c["S"], torch.from_numpy(acts))
    w, b = c["params"]["pts_linears.0.weight"].numpy(), c["params"]["pts_linears.0.bias"].numpy()
    got = mp.layer32([(X["EX"].numpy(), mp.kernel_order("gx", 10))], w, b)
    r64 = np.maximum(X["EX"].numpy().astype(np.float64) @ w.astype(np.float64).T + b, 0)
    m = np.abs(X["EX"].numpy()).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(b)
    assert (np.abs(got - r64) <= m32.C_ACC * 65 * m32.U * m + 2.0 ** -24 * np.maximum(np.abs(r64), 2.0 ** -100)).all()
    assert np.abs(got - X["X1"].numpy()).max() < 1e-5
