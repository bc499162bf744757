"""Renderer.render over a pairwise covering set of its switches (tests/_render_cases.py) against the staged reference render
(tests/_render_ref.py).  Every case asserts (a) the exact key set and the leading (1, R), (b) every map bit for bit -- a mismatch is
a wiring bug, the suite documents every equality the reference rests on as exact --, (c) the ROUTE: which entry points ran, how
often per chunk, the plan of the fused images, the workgroup caps of the two-stream frame, and (d) the state: rng_state advances
by one exactly where the render draws, an inference render repeats its bits.  One case per level kernel is anchored to the oracle
on the render's own samples; four mis-wired renderers have to fail (b); the refused combinations are refused by name."""
from types import SimpleNamespace as NS

import pytest
import torch

import _render_cases as rc
import _render_ref as rr
from oracle import c_oracle as co
from oracle import torch_oracle as to
from panopticnerf_amd import make_network, make_renderer, ops, renderer as pnr_renderer, synthetic, train as pnr_train
from panopticnerf_amd.primitives import ConvexSet
from panopticnerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

CASES = rc.generate()
IDS = [rc.case_id(i, c) for i, c in enumerate(CASES)]
R = rc.R_RAYS
SEED = 977
_REF = {}           # case index -> the staged reference of that case (computed once; nothing modifies it)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _cfg(case, **extra):
    C, K = case["heads"]
    Nc, Nf = case["samples"]
    kw = dict(N_samples=Nc, N_importance=Nf, num_classes=C, num_instances=K, precision=case["precision"], head_tap=case["head_tap"],
              head_depth=2, max_hits=rr.max_hits(case), bbox_sampling=case["bbox_sampling"],
              semantic_activation=case["semantic_activation"], coarse_outputs=case["coarse_outputs"],
              fuse_composite=case["fuse_composite"], chunk_size=65536 if case["chunks"] == "one" else rc.CHUNK_SIZE,
              frame_outputs=case["chunks"] != "three_cat", overlap_levels=case["overlap_levels"], white_bkgd=case["white_bkgd"],
              lindisp=case["lindisp"], keep_weights=case["keep_weights"], share_coarse_fine=case["share_coarse_fine"],
              perturb=1.0, raw_noise_std=1.0, rng="device", rng_seed=SEED)           # (eval mode draws nothing of these)
    kw.update(extra)
    return NS(**kw)


def _net(case, dev, oracle_seeds=None):
    cfg = _cfg(case)
    torch.manual_seed(11)
    net = make_network(cfg)
    params = oc = None
    if oracle_seeds is None:
        synthetic.trained_like_(net, 0.05)
    else:                       # the anchor: the oracle's parameters, as test_gpu_render.py::_setup
        oc = to.mlp_config(n_sem=cfg.num_classes, n_inst=cfg.num_instances, head_tap=cfg.head_tap)
        params = {"coarse": to.init_params(oc, oracle_seeds[0], sigma_bias=0.05), "fine": to.init_params(oc, oracle_seeds[1], sigma_bias=0.05)}
        net.nerf_0.load_state_dict(params["coarse"])
        if net.nerf_1 is not None:
            net.nerf_1.load_state_dict(params["fine"])
        else:
            params["fine"] = params["coarse"]
    net = net.to(dev)
    net.train(rc.route(case).train)
    return (net, oc, params) if oracle_seeds is not None else net


def _boxes(case):
    """random_boxes(40) and a stack of 12 slabs across the view axis: alone the 40 boxes give a ray at most 5 hits, and the lists of
    max_hits = 33 have to be longer than the 8 that ray_setup keeps"""
    C, K = case["heads"]
    box, ids = synthetic.random_boxes(40, C, K)
    n = 12
    i = torch.arange(n, dtype=torch.float32)
    ctr = torch.stack([torch.zeros(n), torch.full((n,), 1.5), 12.0 + 4.0 * i], -1)
    ext = torch.stack([3.0 + 0.5 * i, 1.0 + 0.25 * i, torch.full((n,), 1.5)], -1)
    stack = torch.cat([ctr, torch.eye(3).reshape(1, 9).repeat(n, 1), ext], -1)
    sid = torch.stack([torch.arange(n) % max(C, 1), torch.arange(n) % max(K, 1)], -1).int()
    return torch.cat([box, stack], 0).contiguous(), torch.cat([ids, sid], 0).contiguous()


def _rays():
    rays = synthetic.camera_rays()[:: (1408 * 376) // R][:R].contiguous()
    assert rays.shape[0] == R
    return rays


def _batch(case, dev):
    batch = {"rays": _rays()[None].to(dev)}
    if case["prior"] in ("box8", "box33"):
        box, ids = _boxes(case)
        batch.update(bbox=box.to(dev), bbox_ids=ids.to(dev))
    elif case["prior"] == "prim8":
        box, ids = _boxes(case)
        batch.update(ConvexSet.from_boxes(box.numpy(), ids.numpy()).to(dev).batch())
    if case["mode"] == "eval_explicit":
        g = torch.Generator().manual_seed(3)
        Nc, Nf = case["samples"]
        batch["t_rand"] = torch.rand(1, R, Nc, generator=g).to(dev)
        if Nf > 0:
            batch["u"] = torch.rand(1, R, Nf, generator=g).to(dev)
    return batch


# ------------------------------------------------------------------------------------------------------------------ running
def _run(fn, net, grad):
    """fn() -> maps, under the case's autograd mode: (maps detached, {parameter: gradient} or None, loss or None).  The loss is
    test_gpu_rng.py::_maps_and_grads': the sum of the mean squares of the differentiable per-ray maps."""
    if not grad:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return out, None, None
    for p in net.parameters():
        p.grad = None
    out = fn()
    loss = sum((v.float() ** 2).mean() for k, v in out.items() if v.dim() >= 2 and v.requires_grad)
    loss.backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in out.items()},
            {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, loss.detach())


def _reference(i, net, batch, call):
    if i not in _REF:
        case = CASES[i]
        r = rc.route(case)
        t_rand, u, noise = batch.get("t_rand"), batch.get("u"), (None, None)
        if t_rand is not None:
            t_rand = t_rand[0].contiguous()
        if u is not None:
            u = u[0].contiguous()
        if r.draws:
            t_rand, u, noise = rr.materialised_draws(call, case, R)
        _REF[i] = _run(lambda: rr.staged_render(case, net, batch, t_rand, u, noise), net, r.grad)
    return _REF[i]


def _check_values(case, out, ref):
    """check b: every map of the render is the reference's, bit for bit"""
    n_chunks = rc.route(case).n_chunks
    assert set(out) == set(ref)
    for k in sorted(out):
        a, b = out[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dim() == 0 and n_chunks > 1 and not k.rsplit("_", 2)[-2] == "n":
            # ce3d_<field>_<lv> of several chunks: the count-weighted mean of the chunks' means, another association of the same
            # fp32 sum (merge_chunks) -- the loss's 1e-5; the counts ce3d_<field>_n_<lv> are sums of integers: exact
            assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item()), (k, a.item(), b.item())
            continue
        assert torch.equal(a, b), (k, (a.float() - b.float()).abs().max().item())


class Recorder:
    """recording pass-throughs around the entry points the dispatch chooses between, for the duration of one render"""

    def __init__(self):
        self.calls = []             # (name, rays of the call or None, plan or None, wg_cap or None)

    def wrap(self, name, fn):
        def through(*a, **k):
            rays = plan = cap = None
            if name in ("ray_setup", "bbox_hits", "convex_hits", "stratified"):
                rays = a[0].shape[0]
            elif name in ("mlp_forward_weights", "mlp_forward_composite", "mlp_forward"):
                rays, plan = a[3].shape[0], int(a[0].plan)
                if name == "mlp_forward_composite":
                    cap = int(k.get("wg_cap", a[10] if len(a) > 10 else 0))
            elif name in ("sample_pdf_labels", "sample_pdf"):
                rays = a[0].shape[0]
            elif name == "level_train":
                rays = a[2].shape[0]
            self.calls.append((name, rays, plan, cap))
            return fn(*a, **k)
        return through

    def install(self, m):
        for name in rc.RECORDED:
            owner = pnr_train if name == "level_train" else Renderer if name == "_render_overlapped" else ops
            m.setattr(owner, name, self.wrap(name, getattr(owner, name)))

    def count(self):
        return {n: sum(1 for c in self.calls if c[0] == n) for n in rc.RECORDED}


def _check_route(case, rec, dev):
    """check c"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    calls, wg = rc.expected_calls(case, cus)
    assert rec.count() == calls, (rec.count(), calls)
    sizes = sorted(e - s for s, e in pnr_renderer.chunk_plan(R, _cfg(case).chunk_size))
    assert len(sizes) == rc.route(case).n_chunks
    for name in rc.RECORDED:                        # every entry point once per chunk and level it serves, on that chunk's rays
        got = sorted(c[1] for c in rec.calls if c[0] == name and c[1] is not None)
        if got:
            per = len(got) // len(sizes)
            assert got == sorted(sizes * per), (name, got)
    fused = [c for c in rec.calls if c[0] == "mlp_forward_composite"]
    assert [c[2] for c in fused] == [2] * len(fused)                      # the two-tile image
    assert [c[3] for c in fused] == wg, ([c[3] for c in fused], wg)
    assert all(c[2] == 3 for c in rec.calls if c[0] == "mlp_forward_weights")
    assert all(c[2] == 0 for c in rec.calls if c[0] == "mlp_forward")
    return calls["_render_overlapped"] == 1


def _render_case(i, dev, monkeypatch, patch=None):
    """one render of case i with the recorders on -> everything the checks read"""
    case = CASES[i]
    r = rc.route(case)
    net = _net(case, dev)
    batch = _batch(case, dev)
    rend = make_renderer(_cfg(case), net)
    call = rend.rng_state.clone()
    assert call.tolist() == [SEED, 0]
    ref = _reference(i, net, batch, call)
    rec = Recorder()
    with monkeypatch.context() as m:
        if patch is not None:
            patch(m, case)
        rec.install(m)
        got = _run(lambda: rend.render(batch), net, r.grad)
    return NS(case=case, route=r, net=net, batch=batch, rend=rend, call=call, ref=ref, rec=rec, got=got)


# ------------------------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_render_equals_the_staged_reference(dev, monkeypatch, i):
    x = _render_case(i, dev, monkeypatch)
    case, r = x.case, x.route
    (out, grads, loss), (ref, ref_grads, ref_loss) = x.got, x.ref
    # a. keys and shapes
    assert set(out) == r.keys, (sorted(set(out) - r.keys), sorted(r.keys - set(out)))
    for k, v in out.items():
        assert k.startswith("ce3d") and v.dim() == 0 or tuple(v.shape[:2]) == (1, R), (k, tuple(v.shape))
    if case["prior"] == "box33":                     # the inputs do what they are for: lists longer than ray_setup keeps
        n_hit = ops.bbox_hits(x.batch["rays"][0].contiguous(), x.batch["bbox"], 33)[2]
        assert int((n_hit > rc.RAY_SETUP_MAX_HITS).sum()) >= 4 and int(n_hit.max()) <= 33
    # b. values
    _check_values(case, out, ref)
    if r.grad:
        assert grads.keys() == ref_grads.keys() and len(grads) > 0
        if r.n_chunks == 1:
            assert torch.equal(loss, ref_loss)
            for k in grads:
                assert torch.equal(grads[k], ref_grads[k]), k
        else:           # sums over chunks in another order: test_gpu_rng.py::test_training_draws_do_not_depend_on_the_chunk_plan
            assert abs(loss.item() - ref_loss.item()) <= 1e-5 * abs(ref_loss.item())
            for k in grads:
                assert ((grads[k] - ref_grads[k]).norm() / (ref_grads[k].norm() + 1e-30)).item() < 2e-3, k
    # c. route
    _check_route(case, x.rec, dev)
    # d. state
    assert x.rend.rng_state.tolist() == [SEED, 1 if r.draws else 0]
    if not r.train:
        with torch.no_grad():
            again = x.rend.render(x.batch)
        torch.cuda.synchronize()
        assert set(again) == set(out)
        for k in out:
            assert torch.equal(again[k], out[k]), k
        assert x.rend.rng_state.tolist() == [SEED, 0]
    # ... and the render of NO rays has the same per-ray maps with zero rows (no launch, nothing drawn; the training path's ce3d
    # scalars, means over no samples, are documented as absent: Renderer._output_maps)
    state = x.rend.rng_state.clone()
    none = {k: (v[:, :0] if k in ("rays", "t_rand", "u") else v) for k, v in x.batch.items()}
    with torch.set_grad_enabled(r.grad):
        empty = x.rend.render(none)
    maps = {k for k in r.keys if not k.startswith("ce3d")}
    assert set(empty) == maps, (sorted(set(empty) - maps), sorted(maps - set(empty)))
    for k, v in empty.items():
        assert v.dtype == out[k].dtype and tuple(v.shape) == (1, 0) + tuple(out[k].shape[2:]), k
    assert torch.equal(x.rend.rng_state, state)


def test_the_two_stream_frame_ran(dev, monkeypatch):
    """The cases whose rule gives workgroup caps on this device ran _render_overlapped (each case asserts its own route; this
    one says that there IS such a case, so that "overlapped == serial" is not vacuous)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    over = [i for i, c in enumerate(CASES) if rc.overlap_caps(c, cus) is not None]
    if not over:
        pytest.skip("the documented rule gives no workgroup caps for %d compute units: every frame of the matrix is serial here" % cus)
    x = _render_case(over[0], dev, monkeypatch)
    assert _check_route(x.case, x.rec, dev) and x.rend._side_streams != {}
    _check_values(x.case, x.got[0], x.ref[0])
    if cus == 256:
        assert [c[3] for c in x.rec.calls if c[0] == "mlp_forward_composite"] == [0, 192, 64, 192, 64, 0]


# ------------------------------------------------------------------------------------------------------------------ the anchor
@pytest.mark.parametrize("name", list(rc.ANCHORS))
def test_level_kernels_against_the_oracle_on_the_renders_own_samples(dev, name):
    """The staged reference, and so the matrix, is anchored to the operation: for one case per level kernel, with the oracle's
    parameters, every map of both levels is recomputed by the oracle on the render's own z_vals (test_gpu_render.py::
    _oracle_maps_on_hip_z) and held to the bars of identical stage inputs: 1e-4 in fp32, 1e-2 in bf16 against the bf16-emulating
    oracle (rays whose last sigma lies within bf16 noise of zero judged in fp32 only, as test_gpu_configs.py), depth 6e-3 m in fp32
    and 1e-2 of far = 100 m in bf16 (test_gpu_configs.py's)."""
    i = rc.find(CASES, **rc.ANCHORS[name])
    case = CASES[i]
    r = rc.route(case)
    net, oc, params = _net(case, dev, oracle_seeds=(4, 5))
    batch = _batch(case, dev)
    rend = make_renderer(_cfg(case), net)
    call = rend.rng_state.clone()
    out = _run(lambda: rend.render(batch), net, r.grad)[0]
    assert set(out) == r.keys
    rays = _rays()
    C, K = case["heads"]
    noise = [n.cpu() for n in rr.materialised_draws(call, case, R)[2]] if r.draws else [None, None]
    hits = ids = None
    if case["prior"] != "none":
        box, ids = _boxes(case)
        hits = co.bbox_hits(rays.numpy(), box.numpy(), rr.max_hits(case))
    bf16 = case["precision"] == "bf16"
    for lv in range(rc.n_levels(case)):
        z = out[f"z_vals_{lv}"][0].cpu()
        prm = params["coarse" if (lv == 0 or case["share_coarse_fine"]) else "fine"]
        raw = to.run_network(prm, oc, rays, z, emulate_bf16=bf16)
        ls = li = None
        if hits is not None:
            ls, li = (torch.tensor(a) for a in co.sample_labels(z.numpy(), *hits, ids.numpy()))
        want = to.raw2outputs(raw, z, rays[:, 3:6], C, K, noise[lv], ls, li, 1 if case["semantic_activation"] == "softmax" else 0,
                              case["white_bkgd"])
        last = raw[:, -1, 3] + (noise[lv][:, -1] if noise[lv] is not None else 0.0)
        ok = last.abs() > 2e-2 if bf16 else torch.ones(R, dtype=torch.bool)
        assert ok.sum() >= R // 2
        tol = 1e-2 if bf16 else 1e-4
        seen = 0
        for k in ("rgb", "acc", "weights", "semantic", "instance", "fix_semantic", "fix_instance"):
            if f"{k}_{lv}" in out:
                err = (out[f"{k}_{lv}"][0].cpu() - want[k])[ok].abs().max().item()
                print("%s %s level %d %s: %.3g (bar %g)" % (name, IDS[i], lv, k, err, tol))
                assert err < tol, (name, k, lv, err)
                seen += 1
        derr = (out[f"depth_{lv}"][0].cpu() - want["depth"])[ok].abs().max().item()
        dtol = 1e-2 * 100.0 if bf16 else 6e-3
        print("%s %s level %d depth: %.3g m (bar %g)" % (name, IDS[i], lv, derr, dtol))
        assert derr < dtol, (name, "depth", lv, derr)
        assert seen >= 1


# ------------------------------------------------------------------------------------------------------------------ teeth
def _ray_base_0(m, case):
    orig = Renderer.render_rays

    def render_rays(self, *a, **k):
        if k.get("rng") is not None:
            k["rng"] = (k["rng"][0], 0)                 # every chunk draws as if it held the batch's first rays
        return orig(self, *a, **k)
    m.setattr(Renderer, "render_rays", render_rays)


def _hull_ignored_for_primitives(m, case):
    orig = Renderer._preamble

    def _preamble(self, rays, box, *a, **k):
        keep = self.bbox_sampling
        if isinstance(box, pnr_renderer.Prims):
            self.bbox_sampling = "none"
        try:
            return orig(self, rays, box, *a, **k)
        finally:
            self.bbox_sampling = keep
    m.setattr(Renderer, "_preamble", _preamble)


def _white_bkgd_not_passed(m, case):
    orig = Renderer._level
    levels = rc.route(case).levels

    def _level(self, lv, *a, **k):
        keep = self.white_bkgd
        if levels[lv] == "fused":
            self.white_bkgd = False
        try:
            return orig(self, lv, *a, **k)
        finally:
            self.white_bkgd = keep
    m.setattr(Renderer, "_level", _level)


def _rows_one_chunk_late(m, case):
    orig = Renderer.render_rays
    state = {"prev": None}

    def render_rays(self, rays, *a, **k):
        rows, prev = k.get("out"), state["prev"]
        state["prev"] = rows
        if rows and prev and all(prev[key].shape == v.shape for key, v in rows.items()):
            k["out"] = prev                             # chunk c writes chunk c - 1's rows (equal-sized chunks: every shape fits)
        return orig(self, rays, *a, **k)
    m.setattr(Renderer, "render_rays", render_rays)


MISWIRED = {"ray_base_0": _ray_base_0, "hull_ignored_for_primitives": _hull_ignored_for_primitives,
            "white_bkgd_not_passed": _white_bkgd_not_passed, "rows_one_chunk_late": _rows_one_chunk_late}


@pytest.mark.parametrize("name", list(rc.TEETH))
def test_a_miswired_renderer_fails_the_value_check(dev, monkeypatch, name):
    """Four renderers wired wrongly in ways the dispatch invites -- each valid in shape, so nothing is refused -- on the case of the
    matrix that has to notice: check b fails, and names a map."""
    i = rc.find(CASES, **rc.TEETH[name])
    x = _render_case(i, dev, monkeypatch, patch=MISWIRED[name])
    assert set(x.got[0]) == x.route.keys                # (still the right keys: the values have to tell)
    with pytest.raises(AssertionError) as e:
        _check_values(x.case, x.got[0], x.ref[0])
    print("%s on %s: %s" % (name, IDS[i], str(e.value)[:120]))
    good = _render_case(i, dev, monkeypatch)            # ... and the same case, wired as it is, passes it
    _check_values(good.case, good.got[0], good.ref[0])


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("row", range(len(rc.REFUSED)))
def test_refused_combinations_are_refused_by_name(dev, row):
    a, b, msg = rc.REFUSED[row]
    case = {f: v[0] for f, v in rc.FACTORS.items()}
    case.update([a, b])
    assert rc.refused(case) is not None
    cfg = _cfg(case)
    net = make_network(cfg).to(dev).eval()
    with pytest.raises(ValueError, match=msg):
        make_renderer(cfg, net)
