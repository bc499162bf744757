"""Network.query / ops.mlp_query on an MI355X: density and panoptic labels at 3D points (k_mlp_pp_field on the plan-4 image).

The yardstick is the classic pass, which the oracle tests already cover: ops.mlp_forward on the plan-0 image with rays
(o, d, near, far) and samples z, against the query on points = ops.points(rays, z) -- pnr_points computes o + d * z as a separate
multiply and add, as the MLP kernels do, so the two passes see the same fp32 positions.  sigma must be raw row 3 and the logits
raw rows 4.., 4 + n_sem.. BIT FOR BIT (torch.equal) in every case, head_depth 1 included: the field kernel multiplies plan 0's
fragments in plan 0's order in the classic pass's own (untransposed) accumulator layout, so no case needs a tolerance.  Labels are
then decided: they must equal ops.panoptic_labels on the transposed classic logits, no exclusions.

Which bit-for-bit cases run (test_bits_*): the benched trunk (8 x 256, skip 4) crossed fully with the heads {0+0, 45+32, 45+0,
0+32, 19+8, 96+0, 33+33} x head_tap x head_depth at the ragged P = 2051; every other trunk (8 x 256 with the skip into the last
trunk layer, 4 x 128 without a skip, 3 x 128 skip 1) with two or three head / tap / depth combinations; every P of {1, 31, 32, 33,
255} on two networks; one P of >= 3 grid-stride passes on a 256-CU part on two networks; and 130 + 0 logits through
Network.query (the kernel takes it: heads are run-time loops over 32-row blocks)."""
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import torch_oracle as to
from panopticnerf_amd import make_network, make_renderer, ops, synthetic

pytestmark = pytest.mark.gpu

BENCHED = (8, 256, (4,))
TRUNKS = [BENCHED, (8, 256, (6,)), (4, 128, ()), (3, 128, (1,))]          # (8, 256, (6,)): the skip feeds the LAST trunk layer
HEADS = [(0, 0), (45, 32), (45, 0), (0, 32), (19, 8), (96, 0), (33, 33)]
# a 256-CU part runs 256 workgroups of 256 samples per pass: three full passes and a ragged fourth
P_LARGE = 3 * 256 * 256 + 77
_NETS = {}


def _net(dev, C, K, tap="trunk", depth=2, trunk=BENCHED, precision="bf16", fine=False):
    D, W, skips = trunk
    key = (C, K, tap, depth, trunk, precision, fine, str(dev))
    if key not in _NETS:
        torch.manual_seed(C * 7 + K + depth + D + W + sum(skips))
        net = make_network(NS(D=D, W=W, skips=list(skips), N_importance=64 if fine else 0, num_classes=C, num_instances=K,
                              head_tap=tap, head_depth=depth, precision=precision)).to(dev).eval()
        synthetic.trained_like_(net, 0.05)
        _NETS[key] = net
    return _NETS[key]


def _rays_z(dev, R, N, seed=0):
    """Rays with origins from a continuous distribution (no -0.0 component), |d| in 0.5 .. 2, sorted z in [0.5, 60]."""
    g = torch.Generator().manual_seed(1000 + seed)
    o = torch.randn(R, 3, generator=g) * 3 + torch.tensor([0.0, 1.5, 0.0])
    d = (torch.randn(R, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 1.0])) * (0.5 + 1.5 * torch.rand(R, 1, generator=g))
    z = 0.5 + 59.5 * (torch.arange(N) + torch.rand(R, N, generator=g)) / N
    rays = torch.cat([o, d, torch.full((R, 1), 0.5), torch.full((R, 1), 60.0)], 1).float().contiguous()
    return rays.to(dev), z.float().contiguous().to(dev)


def _split(P):
    """(R, N) with R * N == P and a sample count that is not a round number where P allows it"""
    for N in (293, 51, 11, 5, 3):
        if P % N == 0 and P > N:
            return P // N, N
    return 1, P


def _classic(net, rays, z, level=0):
    """raw (ch, S) of the classic pass, and the points it evaluated"""
    desc, img = net.packed(level, rays.device)
    assert desc.plan == 0
    return ops.mlp_forward(desc, img, rays, z), ops.points(rays, z).reshape(-1, 3)


def _assert_bits(net, out, raw, C, K):
    assert torch.equal(out["sigma"], raw[3])
    assert ("sem_logits" in out) == bool(C) and ("inst_logits" in out) == bool(K)
    if C:
        assert torch.equal(out["sem_logits"], raw[4:4 + C])
    if K:
        assert torch.equal(out["inst_logits"], raw[4 + C:4 + C + K])


def _first_max(l):
    """lowest index attaining the column maximum (torch.argmax does not promise which of equal entries it returns)"""
    n = l.shape[0]
    idx = torch.arange(n, device=l.device, dtype=torch.int32)[:, None].expand_as(l)
    return torch.where(l == l.max(0).values, idx, torch.full_like(idx, n)).min(0).values.to(torch.int32)


def _assert_labels(out, raw, C, K, is_thing):
    sem, inst = raw[4:4 + C], raw[4 + C:4 + C + K]
    if C:
        want = ops.panoptic_labels(sem.t().contiguous(), inst.t().contiguous() if K else None, is_thing)
        assert torch.equal(out["sem_label"], want[0])
        assert torch.equal(out["sem_label"], _first_max(sem))
        assert torch.equal(out["panoptic"], want[2])
        if K:
            assert torch.equal(out["inst_label"], want[1])
    else:
        assert "sem_label" not in out and "panoptic" not in out
        if K:
            assert torch.equal(out["inst_label"], _first_max(inst))
    assert ("inst_label" in out) == bool(K)


def _things(dev, C):
    return (torch.arange(C, device=dev, dtype=torch.int32) % 3 != 0).to(torch.int32).contiguous() if C else None


ALL = ("sigma", "labels", "panoptic", "logits")


def _run_case(dev, C, K, tap, depth, trunk, P, seed=0):
    net = _net(dev, C, K, tap, depth, trunk)
    assert ops.field_query_supported(net.nerf_0.desc("bf16"))
    rays, z = _rays_z(dev, *_split(P), seed=seed)
    raw, pts = _classic(net, rays, z)
    assert pts.shape[0] == P
    for it in (None, _things(dev, C)) if C else (None,):
        out = net.query(pts, want=ALL, is_thing=it, fast=True)
        assert all(v.shape[-1] == P for v in out.values())
        _assert_bits(net, out, raw, C, K)
        _assert_labels(out, raw, C, K, it)
    return net, pts, raw


# ------------------------------------------------------------------------------------------------- 1 + 2: bits and labels
@pytest.mark.parametrize("depth", [2, 1])
@pytest.mark.parametrize("tap", ["trunk", "feature"])
@pytest.mark.parametrize("heads", HEADS)
def test_bits_benched_trunk_every_head(dev, heads, tap, depth):
    _run_case(dev, *heads, tap, depth, BENCHED, 2051)


@pytest.mark.parametrize("trunk,heads,tap,depth", [
    (TRUNKS[1], (45, 32), "trunk", 2), (TRUNKS[1], (19, 8), "feature", 1), (TRUNKS[1], (0, 0), "trunk", 2),
    (TRUNKS[2], (45, 32), "feature", 2), (TRUNKS[2], (0, 32), "trunk", 1), (TRUNKS[2], (0, 0), "trunk", 2),
    (TRUNKS[3], (33, 33), "trunk", 2), (TRUNKS[3], (96, 0), "feature", 1), (TRUNKS[3], (45, 0), "feature", 2)])
def test_bits_other_trunks(dev, trunk, heads, tap, depth):
    _run_case(dev, *heads, tap, depth, trunk, 2051, seed=1)


@pytest.mark.parametrize("P", [1, 31, 32, 33, 255])
@pytest.mark.parametrize("which", [((45, 32), "trunk", 2, BENCHED), ((19, 8), "feature", 1, TRUNKS[3])])
def test_bits_small_and_ragged_sizes(dev, which, P):
    heads, tap, depth, trunk = which
    _run_case(dev, *heads, tap, depth, trunk, P, seed=2)


@pytest.mark.parametrize("which", [((45, 32), "trunk", 2, BENCHED), ((33, 33), "feature", 2, TRUNKS[2])])
def test_bits_several_grid_stride_passes(dev, which):
    heads, tap, depth, trunk = which
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert (P_LARGE + 255) // 256 >= 3 * cus, "the launch is one 256-sample workgroup per CU: raise P_LARGE for this part"
    _run_case(dev, *heads, tap, depth, trunk, P_LARGE, seed=3)


def test_bits_more_than_128_logits(dev):
    """130 + 0: wider than the fused inference pass takes.  Network.query answers either way; here the kernel does (a head is a
    run-time loop over 32-row blocks)."""
    net = _net(dev, 130, 0)
    rays, z = _rays_z(dev, 7, 293, seed=4)
    raw, pts = _classic(net, rays, z)
    out = net.query(pts, want=ALL)
    _assert_bits(net, out, raw, 130, 0)
    _assert_labels(out, raw, 130, 0, None)
    if ops.field_query_supported(net.nerf_0.desc("bf16")):
        assert all(torch.equal(v, net.query(pts, want=ALL, fast=False)[k]) for k, v in out.items())


def _tie_net(dev, C, K, edit):
    torch.manual_seed(5)
    net = make_network(NS(N_importance=0, num_classes=C, num_instances=K)).to(dev).eval()
    with torch.no_grad():
        edit(net.nerf_0)
    return net


def _dup(lin, i, j, lift=0.5):
    """rows i < j of a Linear made identical, and lifted so that they win often"""
    lin.weight[j].copy_(lin.weight[i])
    lin.bias[i] += lift
    lin.bias[j].copy_(lin.bias[i])


@pytest.mark.parametrize("C,K,pairs", [(45, 32, [("semantic_linears", 3, 17), ("instance_linears", 2, 30)]),
                                       (96, 0, [("semantic_linears", 3, 40), ("semantic_linears", 5, 70)])])
def test_ties_go_to_the_lowest_index(dev, C, K, pairs):
    """Two identical output rows (40 and 70 sit in other 32-row blocks than 3 and 5: the step across blocks and across the
    half-waves): the lower index wherever either wins."""
    def edit(n):
        for name, i, j in pairs:
            _dup(getattr(n, name)[1], i, j)
    net = _tie_net(dev, C, K, edit)
    rays, z = _rays_z(dev, 7, 293, seed=6)
    raw, pts = _classic(net, rays, z)
    out = net.query(pts, want=ALL)
    _assert_bits(net, out, raw, C, K)
    _assert_labels(out, raw, C, K, None)
    won = 0
    for name, i, j in pairs:
        lab = out["sem_label" if name == "semantic_linears" else "inst_label"]
        rows = raw[4:4 + C] if name == "semantic_linears" else raw[4 + C:]
        assert torch.equal(rows[i], rows[j])
        assert not (lab == j).any()
        won += int((lab == i).sum())
    assert won > 0, "the duplicated rows never win: the test has no teeth"


def test_all_equal_logits_answer_zero(dev):
    def edit(n):
        for name in ("semantic_linears", "instance_linears"):
            getattr(n, name)[1].weight.zero_()
            getattr(n, name)[1].bias.fill_(0.25)
    net = _tie_net(dev, 45, 32, edit)
    _, pts = _classic(net, *_rays_z(dev, 7, 293, seed=7))
    out = net.query(pts, want=ALL)
    assert (out["sem_logits"] == 0.25).all() and (out["inst_logits"] == 0.25).all()
    for k in ("sem_label", "inst_label", "panoptic"):
        assert not out[k].any(), k


# ------------------------------------------------------------------------------------------------- 3: every subset of `want`
F_CANARY, I_CANARY, GUARD = -12345.678, -777, 37


@pytest.mark.parametrize("heads", [(45, 32), (0, 32), (0, 0)])
def test_every_want_subset_same_bits_and_nothing_else_written(dev, heads):
    C, K = heads
    net = _net(dev, C, K)
    desc, img = net.packed(0, dev, fused="field")
    assert desc.plan == 4
    P = 2051
    _, pts = _classic(net, *_rays_z(dev, *_split(P), seed=8))
    it = _things(dev, C)
    full = ops.mlp_query(desc, img, pts, ALL, it)
    stride = P + 29
    for r in range(1, 5):
        for want in itertools.combinations(ALL, r):
            try:
                keys = ops.query_keys(desc, want)
            except ValueError:
                continue                    # nothing this network has (e.g. labels of a network without heads)
            bufs, views = {}, {}
            for k in keys:
                if k.endswith("_logits"):
                    n = C if k == "sem_logits" else K
                    bufs[k] = torch.full((2 * GUARD + n * stride,), F_CANARY, device=dev)
                    views[k] = bufs[k][GUARD:GUARD + n * stride].view(n, stride)[:, :P]
                else:
                    f = k == "sigma"
                    bufs[k] = torch.full((2 * GUARD + P,), F_CANARY if f else I_CANARY, device=dev,
                                         dtype=torch.float32 if f else torch.int32)
                    views[k] = bufs[k][GUARD:GUARD + P]
            got = ops.mlp_query(desc, img, pts, want, it, out=views)
            assert sorted(got) == sorted(keys)
            for k in keys:
                assert got[k].data_ptr() == views[k].data_ptr()
                assert torch.equal(got[k], full[k]), (want, k)
                can = F_CANARY if bufs[k].dtype == torch.float32 else I_CANARY
                assert (bufs[k][:GUARD] == can).all() and (bufs[k][-GUARD:] == can).all(), (want, k)
                if k.endswith("_logits"):
                    pad = bufs[k][GUARD:-GUARD].view(-1, stride)[:, P:]
                    assert (pad == can).all(), (want, k)


# ------------------------------------------------------------------------------------------------- 4: against the oracle itself
@pytest.mark.parametrize("geom", [(8, 256, (4,), 45, 32), (3, 128, (1,), 7, 0)])
def test_query_matches_the_bf16_oracle(dev, geom):
    """The bounds of tests/test_gpu_stages.py::test_mlp_bf16_matches_bf16_oracle for the same comparison."""
    D, W, skips, C, K = geom
    net = _net(dev, C, K, trunk=(D, W, skips))
    _, pts = _classic(net, *_rays_z(dev, 7, 293, seed=9))
    out = net.query(pts, want=("sigma", "logits"))
    got = torch.cat([out["sigma"][None]] + [out[k] for k in ("sem_logits", "inst_logits") if k in out], 0).t().cpu().numpy()
    cfg = to.mlp_config(D=D, W=W, skips=skips, n_sem=C, n_inst=K, head_W=W // 2)
    p = {k: v.detach().cpu() for k, v in net.nerf_0.state_dict().items()}
    dirs = torch.nn.functional.normalize(torch.randn(pts.shape[0], 3, generator=torch.Generator().manual_seed(0)), dim=-1)
    refbf = to.mlp_forward(p, cfg, pts.cpu(), dirs, emulate_bf16=True)[:, 3:].numpy()
    ref32 = to.mlp_forward(p, cfg, pts.cpu(), dirs)[:, 3:].numpy()
    err = np.abs(got - refbf)
    assert err.max() < 1e-2, f"max {err.max()}"
    assert np.median(err) < 5e-4
    assert np.abs(got - ref32).max() < 6e-2


# ------------------------------------------------------------------------------------------------- 5: the fallback
def test_fp32_network_answers_through_the_classic_pass(dev):
    C, K = 19, 8
    net32 = _net(dev, C, K, precision="fp32")
    assert not ops.field_query_supported(net32.nerf_0.desc("fp32"))
    _, pts = _classic(_net(dev, C, K), *_rays_z(dev, 7, 293, seed=10))
    it = _things(dev, C)
    out = net32.query(pts, want=ALL, is_thing=it)
    with pytest.raises(RuntimeError, match="fast=True"):
        net32.query(pts, fast=True)
    fast = _net(dev, C, K).query(pts, want=ALL, is_thing=it)
    assert list(out) == list(fast)
    for k in out:
        assert out[k].shape == fast[k].shape and out[k].dtype == fast[k].dtype, k
    cfg = to.mlp_config(n_sem=C, n_inst=K)
    p = {k: v.detach().cpu() for k, v in net32.nerf_0.state_dict().items()}
    ref = to.mlp_forward(p, cfg, pts.cpu(), torch.tensor([[0.0, 0.0, 1.0]]).expand(pts.shape[0], 3))[:, 3:].numpy()
    got = torch.cat([out["sigma"][None], out["sem_logits"], out["inst_logits"]], 0).t().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=1e-4, rtol=0)          # test_mlp_fp32_matches_oracle's bound
    raw = torch.cat([torch.zeros(3, pts.shape[0], device=dev), out["sigma"][None], out["sem_logits"], out["inst_logits"]], 0)
    _assert_labels(out, raw, C, K, it)


@pytest.mark.parametrize("heads", [(45, 32), (0, 32), (0, 0)])
def test_fallback_of_a_bf16_network_gives_the_same_bits(dev, heads):
    C, K = heads
    net = _net(dev, C, K, "feature", 1)
    _, pts = _classic(net, *_rays_z(dev, 7, 293, seed=11))
    pts = pts.clone()
    pts[5, 0] = -0.0                 # the classic pass turns -0.0 into +0.0 (o + d * 0); the kernel must see the same position
    pts[9] = 0.0
    pts[11, 2] = -0.0
    it = _things(dev, C)
    want = [w for w in ALL if C or K or w == "sigma"]
    a = net.query(pts, want=want, is_thing=it, fast=True)
    b = net.query(pts, want=want, is_thing=it, fast=False)
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------- 6: position independence, chunks
def test_rows_do_not_depend_on_their_neighbours_or_the_chunking(dev):
    C, K = 45, 32
    net = _net(dev, C, K)
    _, pts = _classic(net, *_rays_z(dev, 19, 293, seed=12))
    P = pts.shape[0]
    it = _things(dev, C)
    full = net.query(pts, want=ALL, is_thing=it)
    for a, b in ((0, 1), (3, 1000), (257, 2051), (1031, P), (P - 1, P)):
        part = net.query(pts[a:b], want=ALL, is_thing=it)
        for k in full:
            assert torch.equal(part[k], full[k][..., a:b]), (k, a, b)
    for chunk in (1000, 4096, P):
        got = net.query(pts, want=ALL, is_thing=it, chunk=chunk)
        for k in full:
            assert torch.equal(got[k], full[k]), (k, chunk)
    shaped = net.query(pts[:7 * 11].reshape(7, 11, 3), want=ALL, is_thing=it)
    for k in full:
        lead = (C,) if k == "sem_logits" else (K,) if k == "inst_logits" else ()
        assert shaped[k].shape == lead + (7, 11)
        assert torch.equal(shaped[k].reshape(lead + (77,)), full[k][..., :77]), k
    # inference only: no autograd history, whatever requires_grad says
    out = net.query(pts[:64].clone().requires_grad_(True), want=("sigma", "logits"))
    assert all(not v.requires_grad and v.grad_fn is None for v in out.values())
    assert net.query(pts[:0], want=ALL)["sigma"].shape == (0,)


# ------------------------------------------------------------------------------------------------- 7: query_grid
@pytest.mark.parametrize("lo,hi,res,chunk", [((-3.0, -1.0, 2.0), (5.0, 2.5, 40.0), (13, 7, 29), None),
                                             ((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0), 19, 1000),
                                             ((0.1, 0.2, 0.3), (0.7, 1.9, 3.3), (5, 3, 2), 7)])
def test_query_grid_is_query_on_the_documented_points(dev, lo, hi, res, chunk):
    C, K = 19, 8
    net = _net(dev, C, K)
    rx, ry, rz = (res,) * 3 if isinstance(res, int) else res
    lo32, hi32 = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
    step = (hi32 - lo32) / torch.tensor([rx, ry, rz], device=dev, dtype=torch.float32)
    iz, iy, ix = torch.meshgrid(torch.arange(rz, device=dev), torch.arange(ry, device=dev), torch.arange(rx, device=dev), indexing="ij")
    i = torch.stack((ix, iy, iz), -1).float()
    pts = (i + 0.5) * step
    pts = pts + lo32                                  # a multiply, then an add (never addcmul)
    want = net.query(pts, want=ALL)
    got = net.query_grid(lo, hi, res, want=ALL, chunk=chunk)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].shape[-3:] == (rz, ry, rx)
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------- 8: levels and the cache
def test_levels_and_cache_invalidation(dev):
    C, K = 19, 8
    net = _net(dev, C, K, fine=True)
    assert net.nerf_1 is not None
    rays, z = _rays_z(dev, 7, 293, seed=13)
    raw0, pts = _classic(net, rays, z, 0)
    raw1, _ = _classic(net, rays, z, 1)
    assert not torch.equal(raw0[3], raw1[3])
    _assert_bits(net, net.query(pts, level=0, want=("sigma", "logits")), raw0, C, K)
    _assert_bits(net, net.query(pts, level=1, want=("sigma", "logits")), raw1, C, K)
    _assert_bits(net, net.query(pts, want=("sigma", "logits")), raw1, C, K)          # None: the fine NeRF when there is one
    with torch.no_grad():
        net.nerf_1.semantic_linears[1].weight.data.mul_(-1.5)                        # .data: invisible to tensor versions
        net.nerf_1.alpha_linear.bias.data.add_(0.1)
    net.invalidate_packed()
    raw1b, _ = _classic(net, rays, z, 1)
    assert not torch.equal(raw1b[3], raw1[3])
    _assert_bits(net, net.query(pts, want=("sigma", "logits")), raw1b, C, K)
    coarse_only = _net(dev, C, K)
    rawc, _ = _classic(coarse_only, rays, z, 0)
    _assert_bits(coarse_only, coarse_only.query(pts, want=("sigma", "logits")), rawc, C, K)      # None: the coarse one otherwise
    torch.manual_seed(3)
    shared = make_network(NS(N_importance=64, share_coarse_fine=True, num_classes=C, num_instances=K)).to(dev).eval()
    raws, _ = _classic(shared, rays, z, 0)
    for level in (None, 0, 1):
        _assert_bits(shared, shared.query(pts, level=level, want=("sigma", "logits")), raws, C, K)


# ------------------------------------------------------------------------------------------------- 9: stream capture
def test_query_is_graph_capturable(dev):
    C, K = 45, 32
    net = _net(dev, C, K)
    desc, img = net.packed(0, dev, fused="field")
    _, pa = _classic(net, *_rays_z(dev, 7, 293, seed=14))
    _, pb = _classic(net, *_rays_z(dev, 7, 293, seed=15))
    it = _things(dev, C)
    static_in = pa.clone()
    ops.mlp_query(desc, img, static_in, ALL, it)                 # warm call (the kernel's attribute is set on first use)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        static_out = ops.mlp_query(desc, img, static_in, ALL, it)
    static_in.copy_(pb)
    g.replay()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in static_out.items()}
    ref = ops.mlp_query(desc, img, pb, ALL, it)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    assert not torch.equal(got["sigma"], ops.mlp_query(desc, img, pa, ("sigma",))["sigma"])


# ------------------------------------------------------------------------------------------------- 10: the field that was rendered
def test_query_returns_the_field_the_renderer_composited(dev):
    C, K = 19, 8
    cfg = NS(N_samples=64, N_importance=128, num_classes=C, num_instances=K, precision="bf16")
    torch.manual_seed(0)
    net = make_network(cfg).to(dev).eval()
    synthetic.trained_like_(net)
    rays = synthetic.camera_rays()[::8273][:64].contiguous().to(dev)
    assert rays.shape[0] == 64
    with torch.no_grad():
        out = make_renderer(cfg, net).render({"rays": rays[None]})
    z = out["z_vals_1"][0].contiguous()
    raw, pts = _classic(net, rays, z, 1)
    assert (raw[3] > 0).any() and (raw[3] < 0).any()
    got = net.query(pts.reshape(64, -1, 3), want=("sigma", "logits"))
    assert got["sigma"].shape == z.shape
    assert torch.equal(got["sigma"].reshape(-1), raw[3])
    assert torch.equal(got["sem_logits"].reshape(C, -1), raw[4:4 + C])
    assert torch.equal(got["inst_logits"].reshape(K, -1), raw[4 + C:])


# ------------------------------------------------------------------------------------------------- 11: non-finite and far points
def test_non_finite_and_far_points_leave_the_other_rows_alone(dev):
    """No address in k_mlp_pp_field depends on a point's value (positions enter arithmetic only; stores are indexed by the point's
    number; the is_thing lookup by a label that is in [0, n_sem) by construction): this checks that rows are isolated from one
    another.  The values in the odd rows themselves are unspecified."""
    C, K = 45, 32
    net = _net(dev, C, K)
    _, pts = _classic(net, *_rays_z(dev, 7, 293, seed=16))
    it = _things(dev, C)
    clean = net.query(pts, want=ALL, is_thing=it)
    odd = pts.clone()
    rows = torch.tensor([0, 31, 32, 500, 1027, 2050], device=dev)
    odd[rows[0]] = 1e6
    odd[rows[1]] = torch.tensor([float("inf"), 0.0, 1.0], device=dev)
    odd[rows[2]] = float("nan")
    odd[rows[3]] = torch.tensor([-1e6, float("-inf"), float("nan")], device=dev)
    odd[rows[4], 1] = float("nan")
    odd[rows[5]] = -1e6
    got = net.query(odd, want=ALL, is_thing=it)
    torch.cuda.synchronize()
    keep = torch.ones(pts.shape[0], dtype=torch.bool, device=dev)
    keep[rows] = False
    for k in clean:
        assert torch.equal(got[k][..., keep], clean[k][..., keep]), k
    for k in ("sem_label", "inst_label"):
        n = C if k == "sem_label" else K
        assert ((got[k] >= -1) & (got[k] < n)).all(), k
