"""The staged reference render of tests/test_gpu_render_matrix.py: the whole batch as ONE chunk on the current stream, built from
the single-purpose ops only -- bbox_hits / convex_hits, restrict_rays, stratified, sample_labels, the level, sample_pdf,
sample_labels, the level -- with explicit t_rand / u / noise tensors.  Never ops.ray_setup or ops.sample_pdf_labels, no out=, no side
stream, no wg_cap.  The level kernel is NAMED by the case's route record (_render_cases.route), not looked up: a fused level runs
ops.mlp_forward_composite on the classic plan-0 image (softmax compositing: the plan-1 image, the plan-0 image refuses the flag),
a sigma-only level the same call with rgb / semantic / instance removed, a two-kernel level ops.mlp_forward + ops.composite, a
training level train.level_train on a plain renderer.  The suite documents each equality this rests on as bit for bit (ray_setup ==
the four kernels, sample_pdf_labels == the two, "weights" == "all", overlapped == serial, chunked == one chunk, plan 2 == plan 1 ==
plan 0, device draws == materialised draws), so Renderer.render has to return these bits."""
from types import SimpleNamespace as NS

import torch

import _render_cases as rc

DROPS = ("rgb", "semantic", "instance")


def max_hits(case):
    return 33 if case["prior"] == "box33" else 8


def materialised_draws(call, case, R):
    """(t_rand, u, [noise of level 0, of level 1]) of a render whose pnr_rng_begin copies `call`: tags 1, 2 and 3 + level, ray base 0"""
    from panopticnerf_amd import ops
    Nc, Nf = case["samples"]
    t_rand = ops.rng_fill(call, 1, 0, R, Nc)
    u = ops.rng_fill(call, 2, 0, R, Nf) if Nf > 0 else None
    noise = [ops.rng_fill(call, 3 + lv, 0, R, N, normal=True, std=1.0) for lv, N in enumerate(rc.level_samples(case))]
    return t_rand, u, noise


def staged_render(case, net, batch, t_rand=None, u=None, noise=(None, None)):
    """batch: the render's batch (rays (1, R, 8), the prior's keys).  t_rand (R, Nc), u (R, Nf), noise[lv] (R, N_lv) or None."""
    from panopticnerf_amd import ops, train
    from panopticnerf_amd.renderer import Renderer
    r = rc.route(case)
    rays = batch["rays"].reshape(-1, 8).float().contiguous()
    dev, R = rays.device, rays.shape[0]
    Nc, Nf = case["samples"]
    C, K = case["heads"]
    sem = 1 if case["semantic_activation"] == "softmax" else 0
    white = case["white_bkgd"]
    hits = ids = None
    if case["prior"] == "prim8":
        hits = ops.convex_hits(rays, batch["prim_planes"], batch["prim_offsets"], max_hits(case))
        ids = batch["prim_ids"]
    elif case["prior"] != "none":
        hits = ops.bbox_hits(rays, batch["bbox"], max_hits(case))
        ids = batch["bbox_ids"]
    plain = Renderer(net, NS(semantic_activation=case["semantic_activation"], white_bkgd=white))      # what level_train reads of it

    def labels(z):
        return ops.sample_labels(z, hits[0], hits[1], hits[2], ids) if hits is not None else (None, None)

    def level(lv, z, nz):
        kernel = r.levels[lv]
        ls, li = labels(z)
        nlv = 0 if case["share_coarse_fine"] else lv                # share_coarse_fine: level 0's network twice
        if kernel == "train":
            return train.level_train(plain, nlv, rays, z, ls, li, nz)
        if kernel in ("fused", "sigma"):
            assert nz is None
            s = sem if C + K else 0                                 # no learned field: nothing to take a softmax of
            desc, img = net.packed(nlv, dev, "bf16", fused=1 if s else 0)
            assert desc.plan == (1 if s else 0)
            res = ops.mlp_forward_composite(desc, img, rays, z, ls, li, white, True, sem_mode=s)
            return {k: v for k, v in res.items() if not (kernel == "sigma" and k in DROPS)}
        assert kernel == "two_kernel"
        desc, img = net.packed(nlv, dev)
        raw = ops.mlp_forward(desc, img, rays, z, channel_major=True)
        res = ops.composite(raw, z, rays, C, K, True, nz, ls, li, sem, white, True)
        weights_only = lv == 0 and case["coarse_outputs"] == "weights"
        return {k: v for k, v in res.items() if not (weights_only and k in DROPS)}

    rays_s = ops.restrict_rays(rays, hits[0], hits[2]) if (hits is not None and case["bbox_sampling"] == "hull") else rays
    z0 = ops.stratified(rays_s, Nc, case["lindisp"], t_rand)
    o0 = level(0, z0, noise[0])
    ret = {**{k + "_0": v for k, v in o0.items()}, "z_vals_0": z0}
    if Nf > 0:
        z1 = ops.sample_pdf(z0, o0["weights"].detach().contiguous(), Nf, u)[0]
        o1 = level(1, z1, noise[1])
        ret.update({**{k + "_1": v for k, v in o1.items()}, "z_vals_1": z1})
    # the render's key rule (keep_weights) drops maps, it does not change any: every expected key has to be here
    assert r.keys <= set(ret), sorted(r.keys - set(ret))
    return {k: v if v.dim() == 0 else v.reshape(1, R, *v.shape[1:]) for k, v in ret.items() if k in r.keys}
