"""CPU tests of the NeRF core ops' refusals: a tensor whose element count is not what the kernel will index (too short: the
out-of-bounds case), a tensor on another device, a wrong dtype, and double faults that fix the order.  Built like
test_ops_refusals.py: _fake_gpu's tensors, the op behind `_on_device` (`op.__wrapped__`), every case named by exception type and
WHOLE message, and asking for the stream -- the last thing before the entry point -- fails the test, so nothing here is launched.
The sizes the library computes (image bytes, the training layout) come from libpnr.so, which loads without a GPU.
Nothing here touches a GPU."""
import ctypes

import pytest
import torch

from panopticnerf_amd import _lib, ops

import _pack_cases
from _fake_gpu import cpu, z, zt

R, N, NF, M, MH = 4, 32, 8, 3, 2                    # rays, samples (the fused path's minimum), fine samples, boxes, kept hits
S, C, K, CH = R * N, 3, 2, 9                        # samples, classes, instances, channels of raw
GEOM = dict(D=2, W=128, skip=-1, xyz_L=1, dir_L=1, n_sem=C, n_inst=K)
D2, D1, D32 = ops.make_desc(**GEOM), ops.make_desc(**GEOM, head_depth=1), ops.make_desc(**GEOM, precision="fp32")
D3, D4 = ops._desc_with(D2, plan=3), ops._desc_with(D2, plan=4)
D65 = ops.make_desc(**dict(GEOM, n_sem=65))         # pnr_mlp_backward has no image for it and says so itself
f32, f64, bf16, i32, i64, u8 = torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.int64, torch.uint8
V, T = ValueError, TypeError


def nbytes(desc, backward=False):
    lib = _lib.load()
    return int((lib.pnr_mlp_bwd_packed_bytes if backward else lib.pnr_mlp_packed_bytes)(ctypes.byref(desc)))


def image(desc, backward=False, device=None):
    return z(nbytes(desc, backward), dtype=u8, device=device)


ACTS, DYS = (off[-1] for off in ops.train_layout(D2, S))
ACTS32 = int(_lib.load().pnr_mlp_fp32_acts_floats(ctypes.byref(D32), S))
PACK_WS = int(_lib.load().pnr_mlp_pack_workspace_bytes(ctypes.byref(D2), 0))
B0, B3, B4, BB = nbytes(D2), nbytes(D3), nbytes(D4), nbytes(D2, True)
assert B3 < B4 < B0 and nbytes(D1, True) < BB        # "an image of another plan" below is a SHORTER one


def params(desc=D2, device=None, **over):
    p = {k: z(*s, device=device) for k, s in ops.param_shapes(desc).items()}
    p.update(over)
    return {k: v for k, v in p.items() if v is not None}


def draw(device=None):
    return ops.Draw(z(2, dtype=i64, device=device), 1)


def hits(rows=R, device=None):
    return z(rows, MH, 2, device=device), z(rows, MH, dtype=i32, device=device), z(rows, dtype=i32, device=device)


@pytest.fixture(autouse=True)
def _no_launch(monkeypatch):
    def stream():
        raise AssertionError("not refused: the op went on to its entry point")
    monkeypatch.setattr(ops, "_stream", stream)


BASE = {
    "stratified": lambda: dict(rays=z(R, 8), n_samples=N, t_rand=z(R, N), out=z(R, N)),
    "points": lambda: dict(rays=z(R, 8), z=z(R, N)),
    "embed": lambda: dict(x=z(5, 3), L=2),
    "mlp_forward_train": lambda: dict(desc=D2, packed=image(D2), rays=z(R, 8), z=z(R, N)),
    "mlp_backward": lambda: dict(desc=D2, packed_bwd=image(D2, True), d_raw=z(CH, S), acts=z(ACTS, dtype=bf16), n_rays=R, n_samples=N),
    "mlp_wgrad": lambda: dict(desc=D2, acts=z(ACTS, dtype=bf16), dys=z(DYS, dtype=bf16), n_samples=S, shapes=ops.param_shapes(D2)),
    "mlp_forward_train_fp32": lambda: dict(desc=D32, params=params(D32), rays=z(R, 8), z=z(R, N)),
    "mlp_backward_fp32": lambda: dict(desc=D32, params=params(D32), d_raw=z(CH, S), acts=z(ACTS32), n_rays=R, n_samples=N),
    "pack_mlp_device": lambda: dict(desc=D2, params=params(D2, "cuda:0"), out=image(D2, device="cuda:0"),
                                    workspace=z(PACK_WS, dtype=u8, device="cuda:0")),
    "mlp_forward": lambda: dict(desc=D2, packed=image(D2), rays=z(R, 8), z=z(R, N), channel_major=False, out=z(R, N, CH)),
    "composite": lambda: dict(raw=z(CH, S), z=z(R, N), rays=z(R, 8), n_sem=C, n_inst=K, noise=z(R, N), label_sem=z(R, N, dtype=i32),
                              label_inst=z(S, dtype=i32), out={"rgb": z(R, 3)}),
    "mlp_forward_composite": lambda: dict(desc=D2, packed=image(D2), rays=z(R, 8), z=z(R, N), label_sem=z(R, N, dtype=i32),
                                          label_inst=z(R, N, dtype=i32)),
    "mlp_forward_weights": lambda: dict(desc=D3, packed=image(D3), rays=z(R, 8), z=z(R, N), label_sem=z(R, N, dtype=i32),
                                        label_inst=z(R, N, dtype=i32)),
    "mlp_query": lambda: dict(desc=D4, packed=image(D4), points=z(5, 3), want=("sigma", "labels", "logits"), is_thing=z(C, dtype=i32),
                              out={"sem_logits": z(C, 5), "inst_logits": z(K, 5)}),
    "composite_backward": lambda: dict(raw=z(CH, S), z=z(R, N), rays=z(R, 8), n_sem=C, n_inst=K,
                                       grads={"rgb": z(R, 3), "depth": z(R), "weights": z(R, N), "semantic": z(R, C), "fix_instance": z(R, K)},
                                       noise=z(R, N), label_sem=z(R, N, dtype=i32), label_inst=z(R, N, dtype=i32), ce_sem=z(1), ce_inst=z(1)),
    "losses": lambda: dict(weights={"rgb": 1.0}, maps={"rgb": z(R, 3), "depth": z(R), "semantic": z(R, C), "fix_instance": z(R, K)},
                           targets={"rgb": z(R, 3), "depth": z(R), "semantic": z(R, dtype=i32), "instance": z(R, dtype=i32)}, n_sem=C, n_inst=K),
    "ce3d": lambda: dict(raw=z(CH, S), first_channel=4, n_classes=C, label=z(R, N, dtype=i32)),
    "sample_pdf": lambda: dict(z=z(R, N), weights=z(R, N), n_importance=NF, u=z(R, NF), out=z(R, N + NF)),
    "bbox_hits": lambda: dict(rays=z(R, 8), box=z(M, 15), max_hits=MH),
    "convex_hits": lambda: dict(rays=z(R, 8), planes=z(6, 4), offsets=z(2, dtype=i32), max_hits=MH, out=hits()),
    "ray_setup": lambda: dict(rays=z(R, 8), box=z(M, 15), box_ids=z(M, 2, dtype=i32), n_samples=N, max_hits=MH, t_rand=z(R, N)),
    "sample_pdf_labels": lambda: dict(z=z(R, N), weights=z(R, N), n_importance=NF, hits=hits(), box_ids=z(M, 2, dtype=i32), u=z(R, NF)),
    "restrict_rays": lambda: dict(rays=z(R, 8), hit_t=z(R, MH, 2), hit_count=z(R, dtype=i32)),
    "sample_labels": lambda: dict(z=z(R, N), hit_t=z(R, MH, 2), hit_box=z(R, MH, dtype=i32), hit_count=z(R, dtype=i32),
                                  box_ids=z(M, 2, dtype=i32)),
    "panoptic_labels": lambda: dict(sem=z(R, C), inst=z(R, K), is_thing=z(C, dtype=i32)),
    "confusion": lambda: dict(pred=z(R, dtype=i32), gt=z(R, dtype=i32), n_classes=C, conf=z(C, C, dtype=i64)),
}


def short(what, name, has, n, why):
    return "%s: %s holds %d elements, expected %d (%s)" % (what, name, has, n, why)


def least(what, name, has, n, why):
    return "%s: %s holds %d elements, needs at least %d (%s)" % (what, name, has, n, why)


def other(what, name, ref):
    return "%s: %s is on cuda:1, %s on cpu" % (what, name, ref)


def dtype(name, want, got):
    return "%s: expected %s, got %s" % (name, want, got)


RAYS = "8 floats per ray"
IMG, SAMPLE, LAYOUT = "the image of this descriptor", "one per sample", "train_layout"
FEWER = (R - 1) * N                                 # the samples of one ray fewer
ON1 = dict(device="cuda:1")


def level_cases(op, ref="z"):
    """the cases of an op that takes a level: rays against z's R, z itself"""
    return [
        (op, dict(rays=z(R - 1, 8)), V, short(op, "rays", 8 * R - 8, 8 * R, RAYS)),
        (op, dict(rays=z(R, 8, **ON1)), V, other(op, "rays", ref)),
        (op, dict(rays=z(R, 8, dtype=f64)), T, dtype("rays", f32, f64)),
        (op, dict(z=z(S)), V, "%s: z must be (R, N), got (128,)" % op),
        (op, dict(z=z(S), rays=z(R - 1, 8)), V, "%s: z must be (R, N), got (128,)" % op),
    ]


def packed_cases(op, desc_bytes, shorter, name="packed", ref="z"):
    """the cases of an op that takes a packed image: a shorter one (another plan's, or another network's), another device, a dtype"""
    return [
        (op, {name: z(shorter, dtype=u8)}, V, least(op, name, shorter, desc_bytes, IMG)),
        (op, {name: z(desc_bytes, dtype=u8, **ON1)}, V, other(op, name, ref)),
        (op, {name: z(desc_bytes)}, T, dtype(name, u8, f32)),
        (op, {name: zt(desc_bytes, dtype=u8)}, V, name + ": tensor must be contiguous"),
    ]


def label_cases(op):
    return [
        (op, dict(label_sem=z(FEWER, dtype=i32)), V, short(op, "label_sem", FEWER, S, SAMPLE)),
        (op, dict(label_inst=z(R - 1, N, dtype=i32)), V, short(op, "label_inst", FEWER, S, SAMPLE)),
        (op, dict(label_sem=z(R, N, dtype=i32, **ON1)), V, other(op, "label_sem", "z")),
        (op, dict(label_inst=z(R, N, dtype=i32, **ON1)), V, other(op, "label_inst", "z")),
        (op, dict(label_inst=z(R, N, dtype=i64)), T, dtype("label_inst", i32, i64)),
        (op, dict(label_sem=z(FEWER, dtype=i32), label_inst=z(FEWER, dtype=i32, **ON1)), V, short(op, "label_sem", FEWER, S, SAMPLE)),
    ]


def hit_cases(op, ref, wrap=None, with_box=True):
    """the cases of an op that takes hit lists made for other rays (`wrap`: they come as one argument of that name)"""
    def arg(**lists):
        if wrap is None:
            return lists
        t, b, c = hits()
        return {wrap: (lists.get("hit_t", t), lists.get("hit_box", b), lists.get("hit_count", c))}
    cases = [
        (op, arg(hit_t=z(R - 1, MH, 2)), V, "%s: hit_t must be (4, max_hits, 2), got (3, 2, 2)" % op),
        (op, arg(hit_t=z(R, MH, 3)), V, "%s: hit_t must be (4, max_hits, 2), got (4, 2, 3)" % op),
        (op, arg(hit_count=z(R - 1, dtype=i32)), V, "%s: hit_count must be (4,), got (3,)" % op),
        (op, arg(hit_count=z(R, dtype=i32, **ON1)), V, other(op, "hit_count", ref)),
        (op, arg(hit_t=z(R, MH, 2, **ON1)), V, other(op, "hit_t", ref)),
        (op, arg(hit_count=z(R, dtype=i64)), T, dtype("hit_count", i32, i64)),
        (op, arg(hit_t=z(R - 1, MH, 2), hit_count=z(R - 1, dtype=i32)), V, "%s: hit_t must be (4, max_hits, 2), got (3, 2, 2)" % op),
    ]
    if with_box:
        cases += [
            (op, arg(hit_box=z(R, MH - 1, dtype=i32)), V, "%s: hit_box must be (4, 2), got (4, 1)" % op),
            (op, arg(hit_box=z(R, MH, dtype=i32, **ON1)), V, other(op, "hit_box", ref)),
            (op, arg(hit_box=z(R, MH)), T, dtype("hit_box", i32, f32)),
            (op, arg(hit_box=z(R, MH - 1, dtype=i32), hit_count=z(R - 1, dtype=i32)), V, "%s: hit_count must be (4,), got (3,)" % op),
        ]
    return cases


def param_cases(op, desc, device=None):
    """one mis-shaped weight and one mis-shaped bias among the parameters (`device`: where the op wants them)"""
    return [
        (op, dict(params=params(desc, device, **{"pts_linears.1.weight": z(128, 127, device=device)})), V,
         "%s: parameter pts_linears.1.weight is (128, 127), the descriptor's network has (128, 128)" % op),
        (op, dict(params=params(desc, device, **{"semantic_linears.1.bias": z(C - 1, device=device)})), V,
         "%s: parameter semantic_linears.1.bias is (2,), the descriptor's network has (3,)" % op),
    ]


CASES = [
    # ------------------------------------------------------------------------------------------------ stratified
    ("stratified", dict(rays=z(R, 7)), V, "stratified: rays must be (R, 8), got (4, 7)"),
    ("stratified", dict(rays=z(R * 8)), V, "stratified: rays must be (R, 8), got (32,)"),
    ("stratified", dict(t_rand=z(R, N - 1)), V, short("stratified", "t_rand", S - R, S, SAMPLE)),
    ("stratified", dict(t_rand=z(R, N, **ON1)), V, other("stratified", "t_rand", "rays")),
    ("stratified", dict(t_rand=draw("cuda:1")), V, other("stratified", "call", "rays")),
    ("stratified", dict(t_rand=z(R, N, dtype=f64)), T, dtype("t_rand", f32, f64)),
    ("stratified", dict(out=z(R - 1, N)), V, "stratified: out must be a contiguous torch.float32 tensor of shape (4, 32) on cpu"),
    ("stratified", dict(rays=z(R, 7), t_rand=z(R, N - 1)), V, "stratified: rays must be (R, 8), got (4, 7)"),
    ("stratified", dict(out=z(R - 1, N), t_rand=z(R, N - 1)), V, "stratified: out must be a contiguous torch.float32 tensor of shape (4, 32) on cpu"),
    # ------------------------------------------------------------------------------------------------ points, embed
    *level_cases("points"),
    ("embed", dict(x=z(5, 2)), V, "embed: x must be (n, 3), got (5, 2)"),
    ("embed", dict(x=z(15)), V, "embed: x must be (n, 3), got (15,)"),
    ("embed", dict(x=z(5, 2, dtype=f64)), T, dtype("x", f32, f64)),
    # ------------------------------------------------------------------------------------------------ the training MLP
    *level_cases("mlp_forward_train"),
    *packed_cases("mlp_forward_train", B0, B4),
    ("mlp_forward_train", dict(rays=z(R - 1, 8), packed=z(B3, dtype=u8)), V, short("mlp_forward_train", "rays", 8 * R - 8, 8 * R, RAYS)),
    *packed_cases("mlp_backward", BB, nbytes(D1, True), "packed_bwd", "d_raw"),
    ("mlp_backward", dict(d_raw=z(CH - 1, S)), V, short("mlp_backward", "d_raw", (CH - 1) * S, CH * S, "(ch, n_rays * n_samples)")),
    ("mlp_backward", dict(n_rays=R + 1), V, short("mlp_backward", "d_raw", CH * S, CH * (S + N), "(ch, n_rays * n_samples)")),
    ("mlp_backward", dict(acts=z(ACTS - 1, dtype=bf16)), V, least("mlp_backward", "acts", ACTS - 1, ACTS, LAYOUT)),
    ("mlp_backward", dict(acts=z(ACTS, dtype=bf16, **ON1)), V, other("mlp_backward", "acts", "d_raw")),
    ("mlp_backward", dict(acts=z(ACTS)), T, dtype("acts", bf16, f32)),
    ("mlp_backward", dict(d_raw=z(CH - 1, S), packed_bwd=z(1, dtype=u8)), V, short("mlp_backward", "d_raw", (CH - 1) * S, CH * S, "(ch, n_rays * n_samples)")),
    ("mlp_backward", dict(packed_bwd=z(1, dtype=u8), acts=z(1, dtype=bf16)), V, least("mlp_backward", "packed_bwd", 1, BB, IMG)),
    ("mlp_wgrad", dict(acts=z(ACTS - 1, dtype=bf16)), V, least("mlp_wgrad", "acts", ACTS - 1, ACTS, LAYOUT)),
    ("mlp_wgrad", dict(dys=z(DYS - 1, dtype=bf16)), V, least("mlp_wgrad", "dys", DYS - 1, DYS, LAYOUT)),
    ("mlp_wgrad", dict(dys=z(DYS, dtype=bf16, **ON1)), V, other("mlp_wgrad", "dys", "acts")),
    ("mlp_wgrad", dict(dys=z(DYS)), T, dtype("dys", bf16, f32)),
    ("mlp_wgrad", dict(shapes={"pts_linears.0.weight": (128, 10)}), V,
     "mlp_wgrad: shapes['pts_linears.0.weight'] is (128, 10), the descriptor's network has (128, 9)"),
    ("mlp_wgrad", dict(shapes={"rgb_linear.bias": (4,)}), V, "mlp_wgrad: shapes['rgb_linear.bias'] is (4,), the descriptor's network has (3,)"),
    ("mlp_wgrad", dict(shapes={"rgb_linear.bias": (4,)}, acts=z(1, dtype=bf16), dys=z(1, dtype=bf16)), V, least("mlp_wgrad", "acts", 1, ACTS, LAYOUT)),
    ("mlp_wgrad", dict(shapes={"rgb_linear.bias": (4,)}, dys=z(1, dtype=bf16)), V, least("mlp_wgrad", "dys", 1, DYS, LAYOUT)),
    *level_cases("mlp_forward_train_fp32"),
    *param_cases("mlp_forward_train_fp32", D32),
    ("mlp_forward_train_fp32", dict(rays=z(R - 1, 8), params=params(D32, **{"alpha_linear.bias": z(2)})), V,
     short("mlp_forward_train_fp32", "rays", 8 * R - 8, 8 * R, RAYS)),
    *param_cases("mlp_backward_fp32", D32),
    ("mlp_backward_fp32", dict(d_raw=z(CH, S - 1)), V, "d_raw: expected (9, 128), got (9, 127)"),
    ("mlp_backward_fp32", dict(acts=z(ACTS32 - 1)), V, least("mlp_backward_fp32", "acts", ACTS32 - 1, ACTS32, "pnr_mlp_fp32_acts_floats")),
    ("mlp_backward_fp32", dict(d_raw=z(CH, S, **ON1)), V, other("mlp_backward_fp32", "d_raw", "acts")),
    ("mlp_backward_fp32", dict(acts=z(ACTS32, dtype=bf16)), T, dtype("acts", f32, bf16)),
    ("mlp_backward_fp32", dict(acts=z(1), params=params(D32, **{"alpha_linear.bias": z(2)})), V,
     least("mlp_backward_fp32", "acts", 1, ACTS32, "pnr_mlp_fp32_acts_floats")),
    *param_cases("pack_mlp_device", D2, "cuda:0"),
    ("pack_mlp_device", dict(out=z(B0, dtype=u8, **ON1)), V, "pack_mlp_device: out is on cuda:1, the parameters on cuda:0"),
    ("pack_mlp_device", dict(workspace=z(PACK_WS, dtype=u8, **ON1)), V, "pack_mlp_device: workspace is on cuda:1, the parameters on cuda:0"),
    ("pack_mlp_device", dict(out=z(B0, device="cuda:0")), T, dtype("out", u8, f32)),
    ("pack_mlp_device", dict(out=z(B0, device="cuda:0"), params=params(D2, "cuda:0", **{"alpha_linear.bias": z(2, device="cuda:0")})), T, dtype("out", u8, f32)),
    # ------------------------------------------------------------------------------------------------ mlp_forward
    *level_cases("mlp_forward"),
    *packed_cases("mlp_forward", B0, B3),
    ("mlp_forward", dict(out=z(R, N, CH - 1)), V, short("mlp_forward", "out", S * (CH - 1), S * CH, "(R, N, ch)")),
    ("mlp_forward", dict(out=z(R, N, CH, **ON1)), V, other("mlp_forward", "out", "z")),
    ("mlp_forward", dict(out=z(R, N, CH, dtype=f64)), T, dtype("raw", f32, f64)),
    ("mlp_forward", dict(channel_major=True, out=z(CH, S - 1)), V,
     "raw: expected shape (9, 128) with unit sample stride, got (9, 127) strides (127, 1)"),
    ("mlp_forward", dict(channel_major=True, out=z(CH, S, **ON1)), V, other("mlp_forward", "out", "z")),
    ("mlp_forward", dict(packed=z(B3, dtype=u8), out=z(R, N, CH - 1)), V, least("mlp_forward", "packed", B3, B0, IMG)),
    # ------------------------------------------------------------------------------------------------ composite
    *level_cases("composite"),
    *label_cases("composite"),
    ("composite", dict(raw=z(CH, S - 1)), V, "raw: expected shape (9, 128) with unit sample stride, got (9, 127) strides (127, 1)"),
    ("composite", dict(raw=z(CH, S, **ON1)), V, other("composite", "raw", "z")),
    ("composite", dict(channel_major=False, raw=z(R, N, CH - 1)), V, short("composite", "raw", S * (CH - 1), S * CH, "(R, N, ch)")),
    ("composite", dict(noise=z(R - 1, N)), V, short("composite", "noise", FEWER, S, SAMPLE)),
    ("composite", dict(noise=z(R, N, **ON1)), V, other("composite", "noise", "z")),
    ("composite", dict(noise=draw("cuda:1")), V, other("composite", "call", "z")),
    ("composite", dict(noise=z(R, N, dtype=f64)), T, dtype("noise", f32, f64)),
    ("composite", dict(out={"rgb": z(R - 1, 3)}), V, "out['rgb'] must be a contiguous fp32 tensor of shape (4, 3) on cpu"),
    ("composite", dict(noise=z(R - 1, N), label_sem=z(FEWER, dtype=i32)), V, short("composite", "noise", FEWER, S, SAMPLE)),
    ("composite", dict(raw=z(CH, S - 1), noise=z(R - 1, N)), V, "raw: expected shape (9, 128) with unit sample stride, got (9, 127) strides (127, 1)"),
    ("composite", dict(label_inst=z(FEWER, dtype=i32), out={"rgb": z(R - 1, 3)}), V, short("composite", "label_inst", FEWER, S, SAMPLE)),
    # ------------------------------------------------------------------------------------------------ the fused passes
    *level_cases("mlp_forward_composite"),
    *packed_cases("mlp_forward_composite", B0, B4),
    *label_cases("mlp_forward_composite"),
    ("mlp_forward_composite", dict(packed=z(B3, dtype=u8), label_sem=z(FEWER, dtype=i32)), V, least("mlp_forward_composite", "packed", B3, B0, IMG)),
    ("mlp_forward_composite", dict(sem_mode=1, wg_cap=8, packed=z(B3, dtype=u8)), V, least("mlp_forward_composite", "packed", B3, B0, IMG)),
    *level_cases("mlp_forward_weights"),
    *packed_cases("mlp_forward_weights", B3, B3 - 1),           # no plan has a shorter image: one byte short
    *label_cases("mlp_forward_weights"),
    ("mlp_forward_weights", dict(desc=D2, rays=z(R - 1, 8)), V,
     "mlp_forward_weights: needs the plan-3 image (net.packed(level, device, fused='sigma')), not plan 0"),
    *packed_cases("mlp_query", B4, B3, ref="points"),
    ("mlp_query", dict(is_thing=z(C, dtype=i32, **ON1)), V, other("mlp_query", "is_thing", "points")),
    ("mlp_query", dict(out={"sem_logits": z(C, 5, **ON1)}), V, other("mlp_query", "out['sem_logits']", "points")),
    ("mlp_query", dict(is_thing=z(C - 1, dtype=i32), packed=z(B3, dtype=u8)), V,
     "mlp_query: is_thing must hold n_sem=3 entries of a network with a semantic head"),
    ("mlp_query", dict(packed=z(B3, dtype=u8), out={"sem_logits": z(C, 4)}), V, least("mlp_query", "packed", B3, B4, IMG)),
    # ------------------------------------------------------------------------------------------------ composite_backward
    *level_cases("composite_backward"),
    *label_cases("composite_backward"),
    ("composite_backward", dict(raw=z(CH - 1, S)), V, short("composite_backward", "raw", (CH - 1) * S, CH * S, "(ch, R * N)")),
    ("composite_backward", dict(raw=z(CH, S, **ON1)), V, other("composite_backward", "raw", "z")),
    ("composite_backward", dict(raw=zt(CH, S)), V, "raw: tensor must be contiguous"),
    ("composite_backward", dict(noise=z(R - 1, N)), V, short("composite_backward", "noise", FEWER, S, SAMPLE)),
    ("composite_backward", dict(noise=draw("cuda:1")), V, other("composite_backward", "call", "z")),
    ("composite_backward", dict(grads={"rgb": z(R - 1, 3)}), V, short("composite_backward", "g_rgb", 3 * R - 3, 3 * R, "a gradient of R rows")),
    ("composite_backward", dict(grads={"depth": z(R - 1)}), V, short("composite_backward", "g_depth", R - 1, R, "a gradient of R rows")),
    ("composite_backward", dict(grads={"acc": z(R - 1)}), V, short("composite_backward", "g_acc", R - 1, R, "a gradient of R rows")),
    ("composite_backward", dict(grads={"weights": z(R, N - 1)}), V, short("composite_backward", "g_weights", S - R, S, "a gradient of R rows")),
    ("composite_backward", dict(grads={"semantic": z(R, C - 1)}), V,
     short("composite_backward", "g_semantic", R * C - R, R * C, "a gradient of R rows")),
    ("composite_backward", dict(grads={"fix_semantic": z(R - 1, C)}), V,
     short("composite_backward", "g_fix_semantic", R * C - C, R * C, "a gradient of R rows")),
    ("composite_backward", dict(grads={"instance": z(R, K - 1)}), V,
     short("composite_backward", "g_instance", R * K - R, R * K, "a gradient of R rows")),
    ("composite_backward", dict(grads={"fix_instance": z(R - 1, K)}), V,
     short("composite_backward", "g_fix_instance", R * K - K, R * K, "a gradient of R rows")),
    ("composite_backward", dict(grads={"rgb": z(R, 3, **ON1)}), V, other("composite_backward", "g_rgb", "z")),
    ("composite_backward", dict(ce_sem=z(1, **ON1)), V, other("composite_backward", "ce_sem", "z")),
    ("composite_backward", dict(raw=z(CH - 1, S), grads={"rgb": z(R - 1, 3)}), V,
     short("composite_backward", "raw", (CH - 1) * S, CH * S, "(ch, R * N)")),
    ("composite_backward", dict(grads={"weights": z(R, N - 1), "rgb": z(R - 1, 3)}), V,
     short("composite_backward", "g_rgb", 3 * R - 3, 3 * R, "a gradient of R rows")),
    # ------------------------------------------------------------------------------------------------ losses, ce3d
    ("losses", dict(maps={"rgb": z(R, 3), "semantic": z(R, C - 1)}), V, short("losses", "semantic", R * C - R, R * C, "R rows")),
    ("losses", dict(maps={"rgb": z(R, 3), "depth": z(R - 1)}), V, short("losses", "depth", R - 1, R, "R rows")),
    ("losses", dict(maps={"rgb": z(R, 3), "fix_instance": z(R - 1, K)}), V,
     short("losses", "fix_instance", R * K - K, R * K, "R rows")),
    ("losses", dict(targets={"rgb": z(R - 1, 3)}), V, short("losses", "rgb_gt", 3 * R - 3, 3 * R, "R rows")),
    ("losses", dict(targets={"rgb": z(R, 3), "depth": z(R - 1)}), V, short("losses", "depth_gt", R - 1, R, "R rows")),
    ("losses", dict(targets={"rgb": z(R, 3), "semantic": z(R - 1, dtype=i32)}), V,
     short("losses", "sem_gt", R - 1, R, "R rows")),
    ("losses", dict(targets={"rgb": z(R, 3), "instance": z(R - 1, dtype=i32)}), V,
     short("losses", "inst_gt", R - 1, R, "R rows")),
    ("losses", dict(targets={"rgb": z(R, 3, **ON1)}), V, other("losses", "rgb_gt", "the first map")),
    ("losses", dict(maps={"rgb": z(R, 3), "depth": z(R, **ON1)}), V, other("losses", "depth", "the first map")),
    ("losses", dict(targets={"rgb": z(R, 3), "semantic": z(R, dtype=i64)}), T, dtype("sem_gt", i32, i64)),
    ("losses", dict(maps={"rgb": z(R, 3), "depth": z(R - 1)}, targets={"rgb": z(R - 1, 3), "depth": z(R)}), V,
     short("losses", "depth", R - 1, R, "R rows")),
    ("ce3d", dict(label=z(FEWER, dtype=i32)), V, "raw: expected shape (9, 96) with unit sample stride, got (9, 128) strides (128, 1)"),
    ("ce3d", dict(raw=z(CH, S - 1)), V, "raw: expected shape (9, 128) with unit sample stride, got (9, 127) strides (127, 1)"),
    ("ce3d", dict(first_channel=CH - 2), V, "ce3d: channels 7 .. 9 are not all among raw's 9"),
    ("ce3d", dict(first_channel=-1), V, "ce3d: channels -1 .. 1 are not all among raw's 9"),
    ("ce3d", dict(label=z(R, N, dtype=i32, **ON1)), V, other("ce3d", "label", "raw")),
    ("ce3d", dict(label=z(R, N, dtype=i64)), T, dtype("label", i32, i64)),
    ("ce3d", dict(first_channel=CH - 2, label=z(R, N, dtype=i32, **ON1)), V, "ce3d: channels 7 .. 9 are not all among raw's 9"),
    # ------------------------------------------------------------------------------------------------ sample_pdf
    ("sample_pdf", dict(z=z(S)), V, "sample_pdf: z must be (R, Nc), got (128,)"),
    ("sample_pdf", dict(weights=z(R, N - 1)), V, short("sample_pdf", "weights", S - R, S, "one per coarse sample")),
    ("sample_pdf", dict(weights=z(R, N, **ON1)), V, other("sample_pdf", "weights", "z")),
    ("sample_pdf", dict(weights=z(R, N, dtype=f64)), T, dtype("weights", f32, f64)),
    ("sample_pdf", dict(u=z(R, NF - 1)), V, short("sample_pdf", "u", R * NF - R, R * NF, "n_importance per ray")),
    ("sample_pdf", dict(u=z(R, NF, **ON1)), V, other("sample_pdf", "u", "z")),
    ("sample_pdf", dict(u=draw("cuda:1")), V, other("sample_pdf", "call", "z")),
    ("sample_pdf", dict(out=z(R, N + NF - 1)), V, "sample_pdf: out must be a contiguous torch.float32 tensor of shape (4, 40) on cpu"),
    ("sample_pdf", dict(weights=z(R, N - 1), u=z(R, NF - 1)), V, short("sample_pdf", "weights", S - R, S, "one per coarse sample")),
    ("sample_pdf", dict(u=z(R, NF - 1), out=z(R, N)), V, short("sample_pdf", "u", R * NF - R, R * NF, "n_importance per ray")),
    # ------------------------------------------------------------------------------------------------ bbox_hits, convex_hits, ray_setup
    ("bbox_hits", dict(rays=z(R, 7)), V, "bbox_hits: rays must be (R, 8), got (4, 7)"),
    ("bbox_hits", dict(box=z(M, 14)), V, "bbox_hits: box must be (M, 15), got (3, 14)"),
    ("bbox_hits", dict(box=z(M * 15)), V, "bbox_hits: box must be (M, 15), got (45,)"),
    ("bbox_hits", dict(box=z(M, 15, **ON1)), V, other("bbox_hits", "box", "rays")),
    ("bbox_hits", dict(box=z(M, 15, dtype=f64)), T, dtype("box", f32, f64)),
    ("bbox_hits", dict(rays=z(R, 7), box=z(M, 14)), V, "bbox_hits: rays must be (R, 8), got (4, 7)"),
    ("convex_hits", dict(out=hits(R - 1)), V, "convex_hits: out must be a contiguous torch.float32 tensor of shape (4, 2, 2) on cpu"),
    ("convex_hits", dict(out=hits()[:2] + (z(R, dtype=i64),)), V, "convex_hits: out must be a contiguous torch.int32 tensor of shape (4,) on cpu"),
    ("ray_setup", dict(rays=z(R, 9)), V, "ray_setup: rays must be (R, 8), got (4, 9)"),
    ("ray_setup", dict(box=z(M, 16)), V, "ray_setup: box must be (M, 15), got (3, 16)"),
    ("ray_setup", dict(box_ids=z(M - 1, 2, dtype=i32)), V,
     short("ray_setup", "box_ids", 2 * M - 2, 2 * M, "a semantic and an instance id per box")),
    ("ray_setup", dict(box_ids=z(M, 2, dtype=i32, **ON1)), V, other("ray_setup", "box_ids", "rays")),
    ("ray_setup", dict(box_ids=z(M, 2, dtype=i64)), T, dtype("box_ids", i32, i64)),
    ("ray_setup", dict(t_rand=z(R - 1, N)), V, short("ray_setup", "t_rand", FEWER, S, SAMPLE)),
    ("ray_setup", dict(t_rand=z(R, N, **ON1)), V, other("ray_setup", "t_rand", "rays")),
    ("ray_setup", dict(t_rand=draw("cuda:1")), V, other("ray_setup", "call", "rays")),
    ("ray_setup", dict(out=z(R, N + 1)), V, "ray_setup: out must be a contiguous torch.float32 tensor of shape (4, 32) on cpu"),
    ("ray_setup", dict(box_ids=z(M - 1, 2, dtype=i32), t_rand=z(R - 1, N)), V,
     short("ray_setup", "box_ids", 2 * M - 2, 2 * M, "a semantic and an instance id per box")),
    ("ray_setup", dict(t_rand=z(R - 1, N), out=z(R, N + 1)), V, short("ray_setup", "t_rand", FEWER, S, SAMPLE)),
    # ------------------------------------------------------------------------------------------------ the ops that take hit lists
    ("sample_pdf_labels", dict(weights=z(R, N - 1)), V, short("sample_pdf_labels", "weights", S - R, S, "one per coarse sample")),
    ("sample_pdf_labels", dict(u=z(R, NF - 1)), V, short("sample_pdf_labels", "u", R * NF - R, R * NF, "n_importance per ray")),
    ("sample_pdf_labels", dict(box_ids=z(M, 2, dtype=i32, **ON1)), V, other("sample_pdf_labels", "box_ids", "z")),
    ("sample_pdf_labels", dict(weights=z(R, N - 1), hits=hits(R - 1)), V, short("sample_pdf_labels", "weights", S - R, S, "one per coarse sample")),
    *hit_cases("sample_pdf_labels", "z", wrap="hits"),
    ("restrict_rays", dict(rays=z(R, 7)), V, "restrict_rays: rays must be (R, 8), got (4, 7)"),
    *hit_cases("restrict_rays", "rays", with_box=False),
    ("sample_labels", dict(z=z(S)), V, "sample_labels: z must be (R, N), got (128,)"),
    ("sample_labels", dict(box_ids=z(M, 2, dtype=i32, **ON1)), V, other("sample_labels", "box_ids", "z")),
    ("sample_labels", dict(box_ids=z(M, 2)), T, dtype("box_ids", i32, f32)),
    *hit_cases("sample_labels", "z"),
    # ------------------------------------------------------------------------------------------------ panoptic_labels, confusion
    ("panoptic_labels", dict(inst=z(R - 1, K)), V, "panoptic_labels: sem must be (R, n_sem) and inst (R, n_inst), got (4, 3) and (3, 2)"),
    ("panoptic_labels", dict(sem=z(R * C), inst=None), V, "panoptic_labels: sem must be (R, n_sem) and inst (R, n_inst), got (12,) and None"),
    ("panoptic_labels", dict(is_thing=z(C - 1, dtype=i32)), V, short("panoptic_labels", "is_thing", C - 1, C, "one per class of sem")),
    ("panoptic_labels", dict(is_thing=z(C, dtype=i32, **ON1)), V, other("panoptic_labels", "is_thing", "sem")),
    ("panoptic_labels", dict(inst=z(R, K, **ON1)), V, other("panoptic_labels", "inst", "sem")),
    ("panoptic_labels", dict(is_thing=z(C)), T, dtype("is_thing", i32, f32)),
    ("panoptic_labels", dict(inst=z(R - 1, K), is_thing=z(C - 1, dtype=i32)), V,
     "panoptic_labels: sem must be (R, n_sem) and inst (R, n_inst), got (4, 3) and (3, 2)"),
    ("confusion", dict(gt=z(R - 1, dtype=i32)), V, short("confusion", "gt", R - 1, R, "one per element of pred")),
    ("confusion", dict(conf=z(C, C - 1, dtype=i64)), V, short("confusion", "conf", C * C - C, C * C, "(n_classes, n_classes)")),
    ("confusion", dict(gt=z(R, dtype=i32, **ON1)), V, other("confusion", "gt", "pred")),
    ("confusion", dict(conf=z(C, C, dtype=i64, **ON1)), V, other("confusion", "conf", "pred")),
    ("confusion", dict(conf=z(C, C, dtype=i32)), T, dtype("conf", i64, i32)),
    ("confusion", dict(gt=z(R - 1, dtype=i32), conf=z(C, C - 1, dtype=i64)), V, short("confusion", "gt", R - 1, R, "one per element of pred")),
]


@pytest.mark.parametrize("op,over,exc,message", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_by_type_and_whole_message(op, over, exc, message):
    args = BASE[op]()
    args.update(over)
    with pytest.raises(Exception) as e:
        getattr(ops, op).__wrapped__(**args)
    assert type(e.value) is exc and str(e.value) == message, "%s: %s" % (type(e.value).__name__, e.value)


def test_every_op_is_covered_and_its_base_arguments_pass_every_check():
    """the base arguments of every op reach the launch, so that each case above fails for the fault it names and no other; so do
    the other spellings the rule accepts: a Draw in place of the values, flat labels, arena slices longer than needed, and the
    network whose heads are one Linear; and a descriptor the library has no image for goes on to the entry point's own refusal"""
    assert {c[0] for c in CASES} == set(BASE)
    also = [("stratified", dict(t_rand=draw())), ("stratified", dict(t_rand=None, out=None)), ("composite", dict(noise=draw())),
            ("composite", dict(label_sem=z(S, dtype=i32), label_inst=None)), ("composite_backward", dict(noise=draw(), grads={})),
            ("composite_backward", dict(n_sem=0, n_inst=0, raw=z(4, S), grads={"semantic": z(1)}, label_sem=None, label_inst=None)),
            ("sample_pdf", dict(u=draw())), ("sample_pdf", dict(u=None, out=None)), ("ray_setup", dict(t_rand=draw(), box_ids=None)),
            ("sample_pdf_labels", dict(u=draw())), ("ce3d", dict(label=z(S, dtype=i32))), ("panoptic_labels", dict(inst=None, is_thing=None)),
            ("composite", dict(channel_major=False, raw=z(R, N, CH))), ("losses", dict(maps={"rgb": z(R, 3)}, targets={"rgb": z(R, 3)}, n_sem=0, n_inst=0)),
            ("mlp_forward", dict(packed=z(B0 + 64, dtype=u8), channel_major=True, out=z(CH, S))),
            ("mlp_backward", dict(acts=z(ACTS + 64, dtype=bf16), packed_bwd=z(BB + 64, dtype=u8))),
            ("mlp_wgrad", dict(dys=z(DYS + 64, dtype=bf16), shapes={"alpha_linear.weight": (1, 128), "not.a.parameter": (7,)})),
            ("mlp_backward", dict(desc=D65, packed_bwd=z(1, dtype=u8), d_raw=z(CH + 62, S), acts=z(ops.train_layout(D65, S)[0][-1], dtype=bf16))),
            ("mlp_forward_train", dict(desc=D1, packed=image(D1))), ("mlp_forward_composite", dict(desc=D1, packed=image(D1), sem_mode=1, wg_cap=8)),
            ("mlp_wgrad", dict(desc=D1, shapes=ops.param_shapes(D1))), ("pack_mlp_device", dict(desc=D1, params=params(D1, "cuda:0"), out=image(D1, device="cuda:0"))),
            ("mlp_forward_train_fp32", dict(params=params(D32, **{"rgb_linear.bias": None, "unknown.weight": z(7)})))]
    for op, over in [(op, {}) for op in BASE] + also:
        args = BASE[op]()
        args.update(over)
        with pytest.raises(AssertionError, match="not refused: the op went on to its entry point"):
            getattr(ops, op).__wrapped__(**args)


def test_an_absent_parameter_stays_a_null_pointer_and_the_host_packers_check_the_rest():
    """_param_struct checks the names that are present: the plan-3 image is packed without the layers it does not hold"""
    p = {k: cpu(*s) for k, s in ops.param_shapes(D3).items() if not k.startswith(("rgb_linear", "views_linears", "feature_linear"))}
    P, keep = ops._param_struct(D3, p, "cpu")
    assert not P.rgb_w and not P.views_b and P.alpha_w
    assert ops.pack_mlp(D3, p).numel() == B3
    for pack, what in ((ops.pack_mlp, "pack_mlp"), (ops.pack_mlp_bwd, "pack_mlp_bwd")):
        full = {k: cpu(*s) for k, s in ops.param_shapes(D2).items()}
        assert pack(D2, full).numel() == (B0 if pack is ops.pack_mlp else BB)
        with pytest.raises(ValueError) as e:
            pack(D2, dict(full, **{"views_linears.0.weight": cpu(64, 128)}))
        assert str(e.value) == "%s: parameter views_linears.0.weight is (64, 128), the descriptor's network has (64, 137)" % what
        with pytest.raises(ValueError) as e:
            pack(D2, dict(full, **{"pts_linears.0.bias": cpu(128, 1)}))
        assert str(e.value) == "%s: parameter pts_linears.0.bias is (128, 1), the descriptor's network has (128,)" % what


@pytest.mark.parametrize("geom", _pack_cases.geometries(), ids=lambda g: _pack_cases.GEOM_ID % g)
def test_param_shapes_is_the_table_of_the_pack_cases(geom):
    """tests/_pack_cases.shapes is written from network.py, independently of ops.py"""
    want = _pack_cases.shapes(geom)
    for precision in ("bf16", "fp32"):
        got = ops.param_shapes(_pack_cases.make_desc(geom, precision))
        assert got == want


def test_an_image_size_is_asked_of_the_library_once_per_descriptor(monkeypatch):
    """the per-chunk ops compare `packed` with a remembered size: pnr_mlp_packed_bytes builds a plan per call"""
    calls = []
    lib = _lib.load()
    real, good, bad = lib.pnr_mlp_packed_bytes, BASE["mlp_forward"](), dict(BASE["mlp_forward"](), packed=z(B3, dtype=u8))
    monkeypatch.setattr(ops, "_IMAGE_BYTES", {})
    monkeypatch.setattr(lib, "pnr_mlp_packed_bytes", lambda d: calls.append(1) or real(d))
    for _ in range(3):
        with pytest.raises(AssertionError, match="not refused"):
            ops.mlp_forward.__wrapped__(**good)
        with pytest.raises(ValueError, match="needs at least"):
            ops.mlp_forward.__wrapped__(**bad)
    assert len(calls) == 1
