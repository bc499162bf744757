"""Test support: the probe networks of tests/_mlp_probe.py for the bf16 inference kernels (k_mlp_pp<W, false> behind
pnr_mlp_forward, and the lock-step k_mlp_fused<bf16> under desc.schedule = 1), and the layer-local float64 check of
tests/_mlp_ref.py run on what they return.  Not part of the product package.

Why the probes carry over: identity and +-1 selector rows are exact in bf16; a bf16 activation times 1 plus zeros is exact in the
fp32 accumulator in any order; RNE of a bf16 value is itself.  So the fp32 raw row of a probe IS the kernel's internal bf16
activation, bit for bit, as long as that value is a normal number or 0 (whether a bf16 MFMA keeps subnormal operands is not
documented: assert_normal).  The regions and stores are _mlp_probe.probes' own, with bf16 descriptors:

  X_l, X_D, F, SH_*, G   what the next Linear reads: RNE to bf16 of the fp32 accumulator (ReLU applied, except F)
  EX, ED                 RNE to bf16 of the kernel's fp32 gamma(x), gamma(d), in canonical column order, the bands the weights see

check(): _mlp_ref.check_forward -- the forward half of the training check -- on the read-out: the identity columns of EX are bf16 of
c_oracle.points bit for bit, the bands inside the E_j of _mlp_ref.py's header, ED with the 8 u direction term, every X_l, G, SH_*
(ReLU) and F inside [RNE(r64 - delta), RNE(r64 + delta)], delta = C_ACC K u m, every raw row inside C_ACC K u m + ulp of float64 on
the kernel's own input region.  No measured number enters.

Every probe descriptor must be one the ping-pong launcher takes (assert_pp_takes: at least four chunks in the weight stream, three
LDS slots of the largest chunk within 160 KiB); the smallest are the D = 2 carriers of EX, ED and X_1."""
import numpy as np
import torch

import _mlp32_ref as m32
import _mlp_probe as mp
import _mlp_ref as mr
from oracle import c_oracle as co
from oracle import torch_oracle as to
from panopticnerf_amd import ops

TINY = 2.0 ** -126              # bf16 has fp32's exponent range
FRAG_BYTES = 1024               # PNR_FRAG_BYTES (pnr_mlp_layout.h)
GEOM_ID = "D%d_W%d_s%d_C%d_K%d_%s%d_L%d_%d"


def rays_of(rng, R, near=0.5, far=8.0):
    o = rng.normal(0, 1, (R, 3)) + np.array([0, 1.5, 0])
    d = rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])
    return np.concatenate([o, d, np.full((R, 1), near), np.full((R, 1), far)], 1).astype(np.float32)


def cfg_of(geom):
    D, W, skip, C, K, tap, depth, Lx, Ld = geom
    return to.mlp_config(D=D, W=W, skips=(skip,) if skip >= 0 else (), xyz_L=Lx, dir_L=Ld, n_sem=C, n_inst=K, head_W=W // 2,
                         head_tap=tap, head_depth=depth)


def desc_of(geom, schedule=0):
    D, W, skip, C, K, tap, depth, Lx, Ld = geom
    return ops.make_desc(D, W, skip, Lx, Ld, C, K, W // 2, "bf16", tap, depth, schedule=schedule)


def geom_of(desc):
    return (desc.D, desc.W, desc.skip, desc.n_sem, desc.n_inst, "feature" if desc.head_tap else "trunk",
            1 if desc.head_depth == 1 else 2, desc.xyz_L, desc.dir_L)


def make_case(geom, R, N, seed=0, near=0.5, far=8.0, params_fn=None, rays_z=None, params=None):
    """geom = (D, W, skip, n_sem, n_inst, head_tap, head_depth, xyz_L, dir_L), the order of test_gpu_mlp_sweep.GEOMS"""
    params = to.init_params(cfg_of(geom), seed=seed) if params is None else params
    if params_fn:
        params_fn(params)
    if rays_z is None:
        rng = np.random.default_rng(seed + 11)
        rays = rays_of(rng, R, near=near, far=far)
        z = co.stratified(rays, N, t_rand=rng.random((R, N)).astype(np.float32))
    else:
        rays, z = rays_z
    return dict(geom=geom, desc=desc_of(geom), params=params, rays=torch.from_numpy(rays), z=torch.from_numpy(z),
                S=z.size, R=z.shape[0], N=z.shape[1])


def probes(desc, params, need=None):
    return mp.probes(desc, params, full_G=True, need=need, prec="bf16")


def assert_pp_takes(img, what=""):
    """the packed image's header: launch_mlp_pp refuses fewer than four chunks, and three slots of the largest chunk beyond 160 KiB"""
    h = img[:16].cpu().numpy().view(np.uint32)
    n_chunks, max_frags = int(h[2]), int(h[3])
    assert n_chunks >= 4 and 3 * max_frags * FRAG_BYTES <= 160 * 1024, (what, n_chunks, max_frags)


def points_dirs(rays, z):
    """(c_oracle.points (S, 3) fp32 -- k_points' separate multiply and add --, float64 unit view directions (S, 3)), CPU"""
    rays, z = rays.cpu(), z.cpu()
    pts = torch.from_numpy(co.points(rays.numpy(), z.numpy()).reshape(-1, 3))
    return pts, mr.unit_dirs64(rays).repeat_interleave(z.shape[1], 0)


def chain_bf16(desc, params, rays, z):
    """the bf16-emulating forward in float64 (bf16 weights, every activation RNE to bf16, exact sums): (X regions, raw (S, ch))"""
    net = mr.Net(desc, params, "cpu")
    pts, vd = points_dirs(rays, z)
    rne = lambda r: mr.bf16_neighbours(r)[0]                                         # noqa: E731
    emb = lambda x, L: torch.cat([x] + [f(x * 2.0 ** k) for k in range(L) for f in (torch.sin, torch.cos)], 1)   # noqa: E731
    X = {"EX": rne(emb(pts.double(), desc.xyz_L)), "ED": rne(emb(vd, desc.dir_L))}
    raw = torch.zeros((pts.shape[0], 4 + desc.n_sem + desc.n_inst), dtype=torch.float64)
    for name, src, dst, relu in m32.linears(desc):
        y = torch.cat([X[s] for s in src], 1) @ net.w[name].t() + net.b[name]
        y = y.clamp(min=0) if relu else y
        if isinstance(dst, str):
            X[dst] = rne(y)
        else:
            raw[:, dst[1]: dst[1] + dst[2]] = y
    return X, raw


def assert_normal(desc, params, rays, z):
    """read-outs are exact for normal numbers: no activation of the bf16-emulating float64 chain may lie in (0, 2^-126)"""
    X, raw = chain_bf16(desc, params, rays, z)
    for nm, x in list(X.items()) + [("raw", raw)]:
        a = x.abs()
        assert not ((a > 0) & (a < TINY)).any(), "%s: a subnormal activation (choose another seed)" % nm


def read_out(launch, desc, params, rays, z, need=None, real=None, probe_list=None):
    """-> (region -> (S, width) fp32 as the launches return it, the [rgb, sigma] columns of a launch that keeps the whole case).
    real: the case's own raw, whose first four channels those launches must reproduce bit for bit; every value read must be
    bf16-representable.  probe_list: probes(desc, params, need) built earlier (a launcher that caches packed images by parameter
    tensor then packs each probe once, however many inputs it is run on)."""
    X, rgbs = {}, None
    for pr in probes(desc, params, need) if probe_list is None else probe_list:
        raw = launch(pr.desc, pr.params, rays, z)
        pr.store(X, raw)
        if pr.same_rgbs or pr.region == "SH":
            rgbs = raw[:, :4].clone()
            assert real is None or torch.equal(rgbs, real[:, :4]), "%s probe: rgb / sigma differ from the real launch" % pr.region
    for nm, x in X.items():
        assert torch.equal(x, x.to(torch.bfloat16).float()), "%s: the read-out is not bf16-representable" % nm
    return X, rgbs


def check_regions(rep, desc, params, rays, z, X, raw, regions=None, parts=None, net=None):
    """_mlp_ref.check_forward on a read-out X (fp32 tensors on raw's device); EX / ED are checked where X holds them"""
    dev = raw.device
    net = mr.Net(desc, params, dev) if net is None else net
    pts = vd = None
    if "EX" in X or "ED" in X:
        pts, vd = (t.to(dev) for t in points_dirs(rays, z))
    mr.check_forward(rep, net, {k: v.double() for k, v in X.items()}, raw, pts if "EX" in X else None, vd if "ED" in X else None,
                     regions=regions, parts=parts)


def check(rep, launch, desc, params, rays, z, real=None):
    """every region of one case through `launch`: the case's own raw, every probe read out, every region and every raw row checked.
    Returns (X, real)."""
    assert_normal(desc, params, rays, z)
    real = launch(desc, params, rays, z) if real is None else real
    X, _ = read_out(launch, desc, params, rays, z, real=real)
    check_regions(rep, desc, params, rays, z, X, real)
    return X, real
