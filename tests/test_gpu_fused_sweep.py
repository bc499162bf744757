"""The fused inference pass (pnr_mlp_forward_composite: the MLP epilogue of csrc/pnr_mlp_fuse.h / csrc/asm/gen_mlp_tt.py, then
k_composite_combine) against the float64 reference of tests/_fused_ref.py, at every sample count it takes, on every plan, in both
compositing modes.  SURVEY.md 8a rows a5 + a6.

The reference input is the kernels' own fp32 raw: ops.mlp_forward on the plan-0 image of the same network (the inference kernels'
raw is checked layer by layer against float64 in tests/test_gpu_mlp_bf16_infer_sweep.py, the training forward's in
tests/test_gpu_mlp_sweep.py), in float64.  Three layers:
  A  the epilogue records (pnr_mlp_forward_tiles): Q, lw and the logit sums S against tiles64; the quadruples' r, g, b must be
     raw's colour channels BIT FOR BIT (the fused kernels and mlp_forward run the same MLP arithmetic);
  B  k_composite_combine (pnr_composite_combine) on records and quadruples written by hand -- Q = 0, subnormal, 1 - 2^-24, local
     weights summing to 1 - Q, logit sums of +-1e4, C + K = 128, ignored labels, R = 1 -- against combine64;
  C  every map of ops.mlp_forward_composite against forward64.

Error = max |kernel - ref64| per ray, over the ray's scale: max(1, max |ref64[ray]|), the ray's far for depth.  Each (kernel path,
quantity) has one bound on error / scale: 4x the worst value measured on an MI355X over this whole file (`worst`), floored at 1e-6,
and capped ("cap") where that would be looser than what the older tests imply at some N.  They bound the fused maps at 2e-6 (4e-6
for fix_* and softmax fields) x N / 32 of the map's GLOBAL scale against the two-kernel path, whose own bound against float64 is
tests/test_gpu_composite_sweep.py's: k_composite at N = 32, k_composite2 at N = 64.  For the weights that is 2e-6 + 4.0e-6 at
N = 32 and 4e-6 + 1.2e-6 = 5.2e-6 at N = 64; every other C bound below is already under its smallest implied value.
PNR_SWEEP_REPORT=<file.json> makes a run write the worst errors it saw, which is how this table was made.

Measured on an MI355X (ROCm 7.0), error / scale:

  path                  quantity      worst      bound
  A plan 0              Q             5.11e-07   2.1e-06
  A plan 0              S             3.83e-07   1.6e-06
  A plan 0              lw            4.43e-07   1.8e-06
  A plan 1              Q             5.77e-07   2.4e-06
  A plan 1              S             1.18e-06   4.8e-06
  A plan 1              lw            4.35e-07   1.8e-06
  A plan 1 softmax      Q             5.77e-07   2.4e-06
  A plan 1 softmax      S             3.55e-07   1.5e-06
  A plan 1 softmax      lw            4.35e-07   1.8e-06
  A plan 2              Q             5.21e-07   2.1e-06
  A plan 2              S             1.18e-06   4.8e-06
  A plan 2              lw            3.62e-07   1.5e-06
  A plan 2 softmax      Q             5.21e-07   2.1e-06
  A plan 2 softmax      S             3.55e-07   1.5e-06
  A plan 2 softmax      lw            3.62e-07   1.5e-06
  B k_composite_combine acc           1.36e-07   1.0e-06 (floor)
  B k_composite_combine depth         1.01e-07   1.0e-06 (floor)
  B k_composite_combine fix_instance  2.25e-08   1.0e-06 (floor)
  B k_composite_combine fix_semantic  2.21e-08   1.0e-06 (floor)
  B k_composite_combine instance      1.57e-07   1.0e-06 (floor)
  B k_composite_combine rgb           1.65e-07   1.0e-06 (floor)
  B k_composite_combine semantic      1.46e-07   1.0e-06 (floor)
  B k_composite_combine weights       1.47e-08   1.0e-06 (floor)
  C plan 0              acc           9.32e-07   3.8e-06
  C plan 0              depth         8.55e-07   3.5e-06
  C plan 0              fix_instance  1.15e-06   4.7e-06
  C plan 0              fix_semantic  1.28e-06   5.2e-06
  C plan 0              instance      3.95e-07   1.6e-06
  C plan 0              rgb           4.61e-07   1.9e-06
  C plan 0              semantic      4.02e-07   1.7e-06
  C plan 0              weights       1.28e-06   5.2e-06
  C plan 1              acc           8.34e-07   3.4e-06
  C plan 1              depth         1.20e-06   4.9e-06
  C plan 1              fix_instance  8.39e-07   3.4e-06
  C plan 1              fix_semantic  8.37e-07   3.4e-06
  C plan 1              instance      7.99e-07   3.2e-06
  C plan 1              rgb           4.90e-07   2.0e-06
  C plan 1              semantic      7.58e-07   3.1e-06
  C plan 1              weights       1.92e-06   5.2e-06 (cap)
  C plan 1 softmax      acc           8.34e-07   3.4e-06
  C plan 1 softmax      depth         1.20e-06   4.9e-06
  C plan 1 softmax      fix_instance  8.39e-07   3.4e-06
  C plan 1 softmax      fix_semantic  8.37e-07   3.4e-06
  C plan 1 softmax      instance      6.10e-07   2.5e-06
  C plan 1 softmax      rgb           4.90e-07   2.0e-06
  C plan 1 softmax      semantic      6.10e-07   2.5e-06
  C plan 1 softmax      weights       1.92e-06   5.2e-06 (cap)
  C plan 2              acc           7.20e-07   2.9e-06
  C plan 2              depth         7.58e-07   3.1e-06
  C plan 2              fix_instance  6.94e-07   2.8e-06
  C plan 2              fix_semantic  7.12e-07   2.9e-06
  C plan 2              instance      7.99e-07   3.2e-06
  C plan 2              rgb           4.90e-07   2.0e-06
  C plan 2              semantic      7.58e-07   3.1e-06
  C plan 2              weights       9.36e-07   3.8e-06
  C plan 2 softmax      acc           7.20e-07   2.9e-06
  C plan 2 softmax      depth         7.58e-07   3.1e-06
  C plan 2 softmax      fix_instance  6.94e-07   2.8e-06
  C plan 2 softmax      fix_semantic  7.12e-07   2.9e-06
  C plan 2 softmax      instance      6.10e-07   2.5e-06
  C plan 2 softmax      rgb           4.90e-07   2.0e-06
  C plan 2 softmax      semantic      6.10e-07   2.5e-06
  C plan 2 softmax      weights       9.36e-07   3.8e-06
"""
import json
import os

import numpy as np
import pytest
import torch
from types import SimpleNamespace as NS

import _composite_ref as cref
import _fused_io as fio
import _fused_ref as fref
from panopticnerf_amd import make_network, ops, synthetic

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

ALL_N = list(range(32, 257, 32))
R_SWEEP = 157               # ragged: R * N is not a multiple of the 256-sample group for odd N / 32

# (C, K, cfg extras, plan of the fused image).  Plan 2 = k_mlp_tt (the benched kernel), 1 = k_mlp_pp on the merged logit chunk (an
# 8 x 256 geometry capped at plan 1, as PNR_FUSED_PLAN=1 does), 0 = k_mlp_pp on the classic chunk order (geometries without a
# better kernel: an instance head alone, more than 2 + 1 logit blocks, W = 128)
NETS = {
    "s45i32": (45, 32, {}, 2), "s19i8": (19, 8, {}, 2), "s64i1": (64, 1, {}, 2), "s45i0": (45, 0, {}, 2), "s0i0": (0, 0, {}, 2),
    "s70i0": (70, 0, {}, 2), "s19i8-feature": (19, 8, {"head_tap": "feature"}, 2), "s19i8-depth1": (19, 8, {"head_depth": 1}, 2),
    "s45i32-plan1": (45, 32, {}, 1), "s19i8-plan1": (19, 8, {}, 1), "s40i0-plan1": (40, 0, {}, 1),
    "s0i32": (0, 32, {}, 0), "s100i0": (100, 0, {}, 0), "s19i40": (19, 40, {}, 0), "W128-s19i8": (19, 8, {"D": 4, "W": 128}, 0),
}

BOUND = {   # (path, quantity) -> bound on error / scale: the table above
    ("A plan 0", "Q"): 2.1e-06, ("A plan 0", "S"): 1.6e-06, ("A plan 0", "lw"): 1.8e-06, ("A plan 1", "Q"): 2.4e-06,
    ("A plan 1", "S"): 4.8e-06, ("A plan 1", "lw"): 1.8e-06, ("A plan 1 softmax", "Q"): 2.4e-06,
    ("A plan 1 softmax", "S"): 1.5e-06, ("A plan 1 softmax", "lw"): 1.8e-06, ("A plan 2", "Q"): 2.1e-06,
    ("A plan 2", "S"): 4.8e-06, ("A plan 2", "lw"): 1.5e-06, ("A plan 2 softmax", "Q"): 2.1e-06,
    ("A plan 2 softmax", "S"): 1.5e-06, ("A plan 2 softmax", "lw"): 1.5e-06, ("B k_composite_combine", "acc"): 1.0e-06,
    ("B k_composite_combine", "depth"): 1.0e-06, ("B k_composite_combine", "fix_instance"): 1.0e-06,
    ("B k_composite_combine", "fix_semantic"): 1.0e-06, ("B k_composite_combine", "instance"): 1.0e-06,
    ("B k_composite_combine", "rgb"): 1.0e-06, ("B k_composite_combine", "semantic"): 1.0e-06,
    ("B k_composite_combine", "weights"): 1.0e-06, ("C plan 0", "acc"): 3.8e-06, ("C plan 0", "depth"): 3.5e-06,
    ("C plan 0", "fix_instance"): 4.7e-06, ("C plan 0", "fix_semantic"): 5.2e-06, ("C plan 0", "instance"): 1.6e-06,
    ("C plan 0", "rgb"): 1.9e-06, ("C plan 0", "semantic"): 1.7e-06, ("C plan 0", "weights"): 5.2e-06,
    ("C plan 1", "acc"): 3.4e-06, ("C plan 1", "depth"): 4.9e-06, ("C plan 1", "fix_instance"): 3.4e-06,
    ("C plan 1", "fix_semantic"): 3.4e-06, ("C plan 1", "instance"): 3.2e-06, ("C plan 1", "rgb"): 2.0e-06,
    ("C plan 1", "semantic"): 3.1e-06, ("C plan 1", "weights"): 5.2e-06, ("C plan 1 softmax", "acc"): 3.4e-06,
    ("C plan 1 softmax", "depth"): 4.9e-06, ("C plan 1 softmax", "fix_instance"): 3.4e-06,
    ("C plan 1 softmax", "fix_semantic"): 3.4e-06, ("C plan 1 softmax", "instance"): 2.5e-06,
    ("C plan 1 softmax", "rgb"): 2.0e-06, ("C plan 1 softmax", "semantic"): 2.5e-06, ("C plan 1 softmax", "weights"): 5.2e-06,
    ("C plan 2", "acc"): 2.9e-06, ("C plan 2", "depth"): 3.1e-06, ("C plan 2", "fix_instance"): 2.8e-06,
    ("C plan 2", "fix_semantic"): 2.9e-06, ("C plan 2", "instance"): 3.2e-06, ("C plan 2", "rgb"): 2.0e-06,
    ("C plan 2", "semantic"): 3.1e-06, ("C plan 2", "weights"): 3.8e-06, ("C plan 2 softmax", "acc"): 2.9e-06,
    ("C plan 2 softmax", "depth"): 3.1e-06, ("C plan 2 softmax", "fix_instance"): 2.8e-06,
    ("C plan 2 softmax", "fix_semantic"): 2.9e-06, ("C plan 2 softmax", "instance"): 2.5e-06,
    ("C plan 2 softmax", "rgb"): 2.0e-06, ("C plan 2 softmax", "semantic"): 2.5e-06, ("C plan 2 softmax", "weights"): 3.8e-06,
}
_REPORT = os.environ.get("PNR_SWEEP_REPORT")
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _REPORT:
        rows = [{"path": p, "quantity": q, "worst": w, "bound": BOUND.get((p, q))} for (p, q), w in sorted(_WORST.items())]
        with open(_REPORT, "w") as f:
            json.dump(rows, f, indent=1)


def _check(path, q, e, what):
    _WORST[(path, q)] = max(_WORST.get((path, q), 0.0), e)
    assert e <= BOUND[(path, q)], (what, path, q, e, BOUND[(path, q)])


def _ray_err(got, want, scale=None):
    """max over rays of |got - want| / the ray's scale (default max(1, max |want[ray]|))"""
    R = want.shape[0]
    g, w = got.detach().cpu().double().reshape(R, -1), want.reshape(R, -1)
    if w.shape[1] == 0:
        return 0.0
    s = w.abs().amax(1).clamp(min=1.0) if scale is None else scale
    return float(((g - w).abs().amax(1) / s).max())


def check_maps(path, out, ref, rays, what):
    assert set(out) == set(ref), (what, sorted(out), sorted(ref))
    far = (rays.detach().cpu() if isinstance(rays, torch.Tensor) else torch.as_tensor(rays))[:, 7].double()
    for k in ref:
        _check(path, k, _ray_err(out[k], ref[k], far if k == "depth" else None), what)


def _path(plan, sem_mode, layer):
    return "%s plan %d%s" % (layer, plan, " softmax" if sem_mode else "")


# ------------------------------------------------------------------------------------------------------------------ networks
def _net(dev, name, seed=0, edit=None):
    C, K, extra, plan = NETS[name]
    torch.manual_seed(seed)
    net = make_network(NS(N_importance=128, num_classes=C, num_instances=K, **extra)).to(dev).eval()
    synthetic.trained_like_(net, 0.05)
    if edit is not None:
        with torch.no_grad():
            edit(net.nerf_1)
    return net, C, K, plan


def _raw64(d0, i0, rays, z):
    """the kernels' own fp32 raw (plan-0 image, ops.mlp_forward) as (R, N, ch): float32 on the device and float64 on the CPU"""
    R, N = z.shape
    raw = ops.mlp_forward(d0, i0, rays, z, channel_major=True)
    sm = raw.T.reshape(R, N, -1)
    return sm, sm.cpu().double()


def check_tiles(path, desc, img, rays, z, raw, raw64, C, K, sem_mode, what):
    """layer A: the epilogue's records and quadruples against tiles64"""
    R, N = z.shape
    rec, ps = fio.tiles_workspace(ops.desc_for_mode(desc, sem_mode), img, rays, z)
    ps = ps.reshape(R, N, 4)
    assert torch.equal(ps[..., 1:].contiguous().view(torch.int32), raw[..., :3].contiguous().view(torch.int32)), \
        (what, "the quadruples' r, g, b are not mlp_forward's raw bits", int((ps[..., 1:] != raw[..., :3]).sum()))
    r64, q64 = fref.tiles64(raw64, z, rays, C, K, sem_mode)
    rec = rec.reshape(R, N // 32, 1 + C + K)
    _check(path, "Q", _ray_err(rec[..., 0], r64[..., 0]), what)
    _check(path, "lw", _ray_err(ps[..., 0], q64[..., 0]), what)
    if C + K:
        _check(path, "S", _ray_err(rec[..., 1:], r64[..., 1:]), what)


def run_case(dev, net, C, K, plan, rays, z, ls, li, white, sem_modes, what, tiles=True, level=1):
    """layers A and C for one (network, rays, z) in the given compositing modes; returns the maps of the last mode"""
    d0, i0 = net.packed(level, dev, "bf16")
    raw, raw64 = _raw64(d0, i0, rays, z)
    N = z.shape[1]
    out = None
    for sm in sem_modes:
        desc, img = _image(net, dev, plan, sm, level)
        assert desc.plan == plan, (what, desc.plan, plan)
        assert ops.fused_supported(desc, N, sm), what
        if tiles:
            check_tiles(_path(plan, sm, "A"), desc, img, rays, z, raw, raw64, C, K, sm, f"{what} sm={sm}")
        out = ops.mlp_forward_composite(desc, img, rays, z, ls, li, white, True, sem_mode=sm)
        ref = cref.forward64(raw64, z, rays, C, K, None, ls, li, sm, white)
        check_maps(_path(plan, sm, "C"), out, ref, rays, f"{what} sm={sm} wb={white}")
    return out


def _image(net, dev, plan, sem_mode, level=1):
    """(desc, image) of the fused pass on the given plan: the best image for the mode (plan 2), or the image capped at the plan"""
    if plan == 2:
        return net.packed(level, dev, "bf16", fused=ops.fused_image(sem_mode))
    return net.packed(level, dev, "bf16", fused=plan)


def _modes(net, C, K, N, dev, plan, level=1):
    """softmax compositing (sem_mode 1) where the plan has a softmax kernel: plans 2 and 1 of a geometry with heads"""
    d0, _ = net.packed(level, dev, "bf16")
    return (0, 1) if (C + K and plan >= 1 and ops.fused_supported(d0, N, 1)) else (0,)


def _dev_inputs(dev, seed, R, N, C, K, labels, edge=True):
    rays, z = fio.rays_z(seed, R, N, edge=edge)
    ls = torch.tensor(fio.labels(seed, R, N, C)).to(dev) if labels and C else None
    li = torch.tensor(fio.labels(seed + 1, R, N, K)).to(dev) if labels and K else None
    return torch.tensor(rays).to(dev), torch.tensor(z).to(dev), ls, li


# ------------------------------------------------------------------------------------------------------------------ A + C: every net, every N
def test_plan_of_every_network(dev):
    """what the sweep assumes about pnr_mlp_fused_plan, and that softmax compositing exists where the sweep runs it"""
    for name, (C, K, extra, plan) in NETS.items():
        net, *_ = _net(dev, name)
        d0, _ = net.packed(1, dev, "bf16")
        assert ops.fused_plan(d0) == (plan if plan != 1 else 2), name
        for sm in _modes(net, C, K, 64, dev, plan):
            assert _image(net, dev, plan, sm)[0].plan == plan, (name, sm)
        if plan == 0 and C + K:
            assert not ops.fused_supported(d0, 64, 1), name


@pytest.mark.parametrize("name", list(NETS))
def test_every_N(dev, name):
    """every N in 32 .. 256, both compositing modes where the geometry has a softmax kernel, white background and labels on for
    one half of the N and off for the other, the edge rays of _fused_io.rays_z; and one ray alone"""
    net, C, K, plan = _net(dev, name, seed=len(name))
    for j, N in enumerate(ALL_N):
        rays, z, ls, li = _dev_inputs(dev, 100 * j + len(name), R_SWEEP, N, C, K, labels=j % 2 == 0)
        run_case(dev, net, C, K, plan, rays, z, ls, li, j % 4 in (1, 2), _modes(net, C, K, N, dev, plan), f"{name} N={N}")
    rays, z, ls, li = _dev_inputs(dev, 7, 1, 160, C, K, labels=True)
    run_case(dev, net, C, K, plan, rays, z, ls, li, True, _modes(net, C, K, 160, dev, plan), f"{name} R=1")


# ------------------------------------------------------------------------------------------------------------------ edge networks
def _bias(name, v):
    def f(n):
        getattr(n, name).bias.fill_(v)
    return f


def _logits(scale, shift):
    def f(n):
        for head in (n.semantic_linears, n.instance_linears):
            head[-1].weight.mul_(scale)
            head[-1].bias.copy_(torch.linspace(-shift, shift, head[-1].bias.numel()))
    return f


EDGES = {"opaque": _bias("alpha_linear", 30.0), "empty": _bias("alpha_linear", -30.0), "rgb+30": _bias("rgb_linear", 30.0),
         "rgb-30": _bias("rgb_linear", -30.0), "logits80": _logits(40.0, 80.0), "logits1e4": _logits(3000.0, 1e4)}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("name", ["s19i8", "s19i8-plan1", "s19i40"])
def test_edge_networks(dev, name, edge):
    net, C, K, plan = _net(dev, name, seed=3, edit=EDGES[edge])
    for j, N in enumerate((32, 128, 224, 256)):
        rays, z, ls, li = _dev_inputs(dev, 10 * j + 5, R_SWEEP, N, C, K, labels=True)
        white = edge == "empty" or j % 2 == 1
        out = run_case(dev, net, C, K, plan, rays, z, ls, li, white, _modes(net, C, K, N, dev, plan), f"{name} {edge} N={N}")
        if edge == "empty":
            assert float(out["acc"].abs().max()) == 0.0 and bool((out["rgb"] == 1.0).all()), (name, N)
        if edge == "opaque":                     # opaque within the first tile
            w = torch.cat([out["weights"][:1], out["weights"][2:]])       # ray 1: every z equal, only the last interval is open
            assert float((out["acc"] - 1).abs().max()) < 1e-5, (name, N)
            assert N == 32 or float(w[:, 32:].abs().max()) < 1e-6, (name, N)


def test_near_zero_last_density_at_the_bench_geometry(dev):
    """the rays whose last density is near zero (alpha of the 1e10 interval is a step function of its sign; the frame-scale oracle
    test has to exclude them) are compared like every other ray here.  The geometry is that test's: BASELINE config 5 with the
    parameters of tests/golden/make_golden.py::config_case(5), 4136 rays strided over the camera's frame, and the coarse level
    (N = 64: the renderer's z at perturb 0 is ops.stratified), which the renderer composites through the fused pass."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden import config_case
    c, _, params, _, _, _ = config_case(5)
    C, K, plan = c["num_classes"], c["num_instances"], 2
    net = make_network(synthetic.baseline_cfg(5, precision="bf16")).eval()
    net.nerf_0.load_state_dict(params["coarse"])
    net.nerf_1.load_state_dict(params["fine"])
    net = net.to(dev)
    rays = synthetic.camera_rays()[3::128].contiguous().to(dev)
    z = ops.stratified(rays, c["N_samples"])
    assert z.shape == (4136, 64)
    d0, i0 = net.packed(0, dev, "bf16")
    raw, _ = _raw64(d0, i0, rays, z)
    n0 = int((raw[:, -1, 3].abs() <= 2e-2).sum())
    print(f"bench geometry: {n0} of {rays.shape[0]} rays have |sigma_last| <= 2e-2")
    assert n0 > 0
    run_case(dev, net, C, K, plan, rays, z, None, None, False, _modes(net, C, K, 64, dev, plan, level=0), "bench geometry", level=0)


# ------------------------------------------------------------------------------------------------------------------ several passes
def test_several_passes_of_the_persistent_kernel(dev):
    """4096 x 192 on the benched network: k_mlp_tt launches min(groups, CUs) workgroups (pnr_mlp_tt_launch) over 256-sample groups,
    so each workgroup loops over several groups; slices and wg_cap launches equal the full launch bit for bit, and a strided
    subset of rays matches float64"""
    R, N = 4096, 192
    net, C, K, plan = _net(dev, "s45i32", seed=5)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    groups = (R * N + 255) // 256
    passes = -(-groups // min(groups, cus))
    assert passes >= 3, passes
    rays, z, ls, li = _dev_inputs(dev, 9, R, N, C, K, labels=True)
    desc, img = net.packed(1, dev, "bf16", fused=True)
    full = ops.mlp_forward_composite(desc, img, rays, z, ls, li, False, True)
    for cap in (64, 192):
        out = ops.mlp_forward_composite(desc, img, rays, z, ls, li, False, True, wg_cap=cap)
        for k in full:
            assert torch.equal(full[k], out[k]), (cap, k)
    for a, b in ((0, 777), (R // 2 - 301, R // 2 + 476), (R - 777, R)):
        part = ops.mlp_forward_composite(desc, img, rays[a:b].contiguous(), z[a:b].contiguous(), ls[a:b].contiguous(),
                                         li[a:b].contiguous(), False, True)
        for k in full:
            assert torch.equal(full[k][a:b], part[k]), ((a, b), k)
    idx = torch.arange(3, R, 8, device=dev)
    d0, i0 = net.packed(1, dev, "bf16")
    _, raw64 = _raw64(d0, i0, rays[idx].contiguous(), z[idx].contiguous())
    ref = cref.forward64(raw64, z[idx], rays[idx], C, K, None, ls[idx], li[idx], 0, False)
    check_maps(_path(plan, 0, "C"), {k: v[idx] for k, v in full.items()}, ref, rays[idx], f"{passes} passes")


# ------------------------------------------------------------------------------------------------------------------ B: crafted records
def _crafted(seed, R, N, C, K):
    """float32 records (R, T, 1 + C + K) and quadruples (R, N, 4) no network produces: per tile Q from {0, 1e-40 (subnormal),
    1 - 2^-24, 1, uniform}, the local weights a random split of exactly 1 - Q (in float64, then rounded), logit sums of +-1e4 in
    every 4th ray, raw colours of +-30"""
    rng = np.random.default_rng(seed)
    T = N // 32
    Q = rng.uniform(0, 1, (R, T))
    pick = rng.integers(0, 5, (R, T))
    Q = np.where(pick == 0, 0.0, np.where(pick == 1, 1e-40, np.where(pick == 2, 1 - 2.0 ** -24, np.where(pick == 3, 1.0, Q))))
    share = rng.dirichlet(np.ones(32), (R, T))
    lw = (share * (1.0 - Q)[..., None]).reshape(R, N)
    S = rng.normal(0, 3, (R, T, C + K))
    S[::4] = rng.choice([-1e4, 1e4], S[::4].shape)
    rec = np.concatenate([Q[..., None], S], -1).astype(np.float32)
    rgb = rng.normal(0, 2, (R, N, 3))
    rgb[1::3] = rng.choice([-30.0, 30.0], rgb[1::3].shape)
    qd = np.concatenate([lw[..., None], rgb], -1).astype(np.float32)
    return rec, qd


@pytest.mark.parametrize("C,K", [(100, 28), (45, 32), (19, 0), (0, 5), (0, 0)])
def test_combine_on_crafted_records(dev, C, K):
    desc = ops.make_desc(n_sem=C, n_inst=K)
    for j, (R, N) in enumerate(((157, 256), (1, 32), (1, 256), (61, 96), (300, 160), (33, 224))):
        rays, z = fio.rays_z(j, R, N)
        rec, qd = _crafted(17 * j + C, R, N, C, K)
        ls = fio.labels(j, R, N, C) if C else None
        li = fio.labels(j + 1, R, N, K) if K else None
        g = lambda a: None if a is None else torch.tensor(a).to(dev)    # noqa: E731
        for white in (False, True):
            out = fio.combine(desc, g(rec), g(qd), g(z), g(ls), g(li), white)
            ref = fref.combine64(rec, qd, z, C, K, ls, li, white)
            check_maps("B k_composite_combine", out, ref, rays, f"C={C} K={K} R={R} N={N} wb={white}")
