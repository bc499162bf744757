"""Renderer / make_renderer -- host-side mirror of lib/networks/renderer (render,
render_rays; the reference source is not in the mount, so
key names follow SURVEY.md 8b and are documented in DESIGN.md).

`Renderer.render(batch)` orchestrates the HIP kernels per ray chunk:
    pnr_stratified -> [pnr_bbox_hits, pnr_sample_labels] -> pnr_mlp_forward(coarse)
    -> pnr_composite -> pnr_sample_pdf -> [labels] -> pnr_mlp_forward(fine) -> pnr_composite
with every intermediate (z, raw, weights) resident in HBM, raw in the channel-major layout
the compositing kernel streams.  No torch math is on the path.

batch keys:  "rays" (B,N_rays,8) = o,d,near,far  (required)
             "bbox" (M,15), "bbox_ids" (M,2) int32  (optional: 3D bbox prior)
             "prim_planes" (P,4), "prim_offsets" (M+1) int32, "prim_ids" (M,2) int32  (optional, instead of bbox: the prior as
             convex primitives, primitives.ConvexSet.batch(); hit lists from pnr_convex_hits, everything behind them unchanged)
             "t_rand" (B,N_rays,N_samples), "u" (B,N_rays,N_importance)  (optional explicit uniforms;
             otherwise drawn when cfg.perturb > 0: with torch.rand, or inside the kernels with cfg.rng = "device")
output keys, level l in {0 (coarse), 1 (fine)}:
             rgb_l (B,N_rays,3) depth_l acc_l (B,N_rays) weights_l z_vals_l (B,N_rays,N_l)
             semantic_l / fix_semantic_l (B,N_rays,C), instance_l / fix_instance_l (B,N_rays,K)
             cfg.coarse_outputs = "weights" (inference with a fine level): no rgb_0, semantic_0, instance_0
"""
import collections
import os

import torch

from . import ops


# the 3D prior as convex primitives (batch keys prim_planes / prim_offsets): travels through render() where the box table does
Prims = collections.namedtuple("Prims", "planes offsets")


def _get(cfg, name, default):
    return getattr(cfg, name, default) if cfg is not None else default


CHUNK_QUANTUM = 1024     # rays: at 64 and at 192 samples per ray a multiple of 1024 rays is a whole number of rounds of the
                         # MLP kernels' persistent grid (256 workgroups x 256 samples)
CHUNK_TAIL = 8           # a tail of at most chunk_size / CHUNK_TAIL rays joins the other chunks instead of becoming a chunk


def chunk_plan(n_rays, chunk_size):
    """[(start, end)] of the ray chunks of one render() call: BALANCED chunks instead of `chunk_size` pieces plus a tail.
    cfg.chunk_size bounds the working set (raw, acts, weights and the frame maps scale with it): n = ceil(R / chunk_size)
    chunks, except that a tail of at most chunk_size / 8 rays joins the others -- so a chunk never holds more than
    chunk_size * (1 + 1/8) rays plus one rounding quantum -- and every chunk but the last is rounded up to CHUNK_QUANTUM rays
    so that its MLP launches are whole rounds of the persistent grid.  A rank's 66,176-ray share of a 1408 x 376 frame over 8
    ranks is then ONE chunk (not 65,536 + a 640-ray chunk with its own ~14 launches), the full frame 7 x 66,560 + 63,488
    rays (every launch whole rounds) instead of 8 x 65,536 + 5,120."""
    n_rays, chunk_size = int(n_rays), max(1, int(chunk_size))
    if n_rays <= 0:
        return []
    n = -(-n_rays // chunk_size)
    if n > 1 and n_rays - (n - 1) * chunk_size <= chunk_size // CHUNK_TAIL:
        n -= 1
    size = -(-n_rays // n)
    if n > 1 and chunk_size >= CHUNK_QUANTUM * CHUNK_TAIL:
        size = -(-size // CHUNK_QUANTUM) * CHUNK_QUANTUM
    out, s = [], 0
    while s < n_rays:
        e = min(n_rays, s + size)
        out.append((s, e))
        s = e
    return out


def _keyed(res, z, lv):
    """a level's dict (the ops' key names) and its z as render keys: rgb -> rgb_<lv>, ..., z_vals_<lv>"""
    return {**{f"{k}_{lv}": v for k, v in res.items()}, f"z_vals_{lv}": z}


def _level_out(out, lv):
    """the inverse, for out=: level lv's caller-owned tensors of `out` under the ops' key names (z_vals is not the level's to write)"""
    return {k[:-2]: v for k, v in out.items() if k.endswith(f"_{lv}") and k != f"z_vals_{lv}"}


def _fill_rows(rows, o):
    """rows: a chunk's row slices of the frame, o: what the chunk returned -- anything it did not write in place (an output
    without an out= route) is copied in"""
    for k, v in o.items():
        if v.data_ptr() != rows[k].data_ptr():
            rows[k].copy_(v)


def _unflatten(maps, lead):
    """per-ray maps (R, ...) -> (*lead, ...); the training path's scalars as they are"""
    return {k: v if v.dim() == 0 else v.reshape(*lead, *v.shape[1:]) for k, v in maps.items()}


def merge_chunks(outs):
    """The chunks' render_rays dicts as one: per-ray maps concatenated; of the training path's per-level scalars,
    ce3d_<field>_n_<lv> (a chunk's number of LABELLED samples) is summed and ce3d_<field>_<lv> (the mean over them) is weighted
    by that count."""
    if len(outs) == 1:
        return outs[0]
    ret = {}
    for k in outs[0]:
        vs = [o[k] for o in outs]
        head, lv = k.rsplit("_", 1)
        if vs[0].dim() > 0:
            ret[k] = torch.cat(vs, 0)
        elif head.endswith("_n"):
            ret[k] = torch.stack(vs).sum()
        else:
            n = torch.stack([o[f"{head}_n_{lv}"] for o in outs])
            ret[k] = (torch.stack(vs) * n).sum() / n.sum().clamp(min=1.0)
    return ret


class Renderer:
    def __init__(self, net, cfg=None):
        self.net = net
        self.cfg = cfg
        self.N_samples = _get(cfg, "N_samples", 64)
        self.N_importance = _get(cfg, "N_importance", _get(cfg, "cascade_samples", 0))
        self.chunk_size = _get(cfg, "chunk_size", 65536)
        self.perturb = _get(cfg, "perturb", 0.0)
        self.raw_noise_std = _get(cfg, "raw_noise_std", 0.0)
        self.white_bkgd = _get(cfg, "white_bkgd", False)
        self.lindisp = _get(cfg, "lindisp", False)
        self.max_hits = _get(cfg, "max_hits", 8)
        self.sem_mode = {"none": 0, "logits": 0, "softmax": 1}[_get(cfg, "semantic_activation", "none")]
        # False: an inference render returns no weights_<lv> it does not need itself (weights_0 stays where a fine level samples it).
        # Under autograd the switch has no effect: train.level_train returns the weights of both levels (the losses may read them)
        self.keep_weights = _get(cfg, "keep_weights", True)
        # inference levels run the fused MLP + compositing pass where it applies (bf16, logits compositing, N % 32 == 0);
        # cfg.fuse_composite = False (or PNR_FUSE=0) keeps the two-kernel path with the raw image in HBM
        self.fuse = bool(_get(cfg, "fuse_composite", os.environ.get("PNR_FUSE", "1") != "0"))
        self.strict_hits = bool(_get(cfg, "strict_hits", False))
        # "all": every map of both levels.  "weights": an inference render (no autograd) returns the coarse level only for what the
        # fine level and the bbox prior read of it -- z_vals_0, weights_0, depth_0, acc_0 and fix_*_0 -- and evaluates it with the
        # sigma-only kernel (trunk + alpha_linear: ops.mlp_forward_weights) where that applies, bit for bit the same values; rgb_0,
        # semantic_0 and instance_0 are absent.  Under autograd (training) the switch has no effect: the losses read the coarse maps.
        self.coarse_outputs = _get(cfg, "coarse_outputs", "all")
        if self.coarse_outputs not in ("all", "weights"):
            raise ValueError("cfg.coarse_outputs must be 'all' or 'weights', not %r" % (self.coarse_outputs,))
        if self.coarse_outputs == "weights" and self.N_importance <= 0:
            raise ValueError("cfg.coarse_outputs = 'weights' needs a fine level (N_importance > 0): without one the coarse maps are "
                             "the render's output")
        # "none": stratified over [near, far] (canonical NeRF); "hull": rays that hit boxes are sampled over the hull of their
        # hit intervals (SURVEY.md 9 item 2 -- which of the two the reference does is unverifiable here: a switch)
        self.bbox_sampling = _get(cfg, "bbox_sampling", "none")
        if self.bbox_sampling not in ("none", "hull"):
            raise ValueError("cfg.bbox_sampling must be 'none' or 'hull', not %r" % (self.bbox_sampling,))
        self._overflow = None
        # training perturbation (t_rand, u) and sigma noise: "torch" draws them with torch.rand / torch.randn chunk by chunk; "device"
        # draws them inside the kernels from a counter-based stream (include/pnr.h "in-kernel RNG"): seeded by cfg.rng_seed, independent of
        # the chunk plan, replayable under a HIP graph, no uniform / noise tensors.  rng_state = (seed, offset) on the render device, one
        # offset per render() call that draws -- public so that checkpoints can save and restore it (None with "torch")
        self.rng = _get(cfg, "rng", "torch")
        if self.rng not in ("torch", "device"):
            raise ValueError("cfg.rng must be 'torch' or 'device', not %r" % (self.rng,))
        self.rng_state = None
        if self.rng == "device":
            seed = _get(cfg, "rng_seed", None)
            seed = torch.initial_seed() if seed is None else int(seed)        # (reads torch's seed; draws nothing from its generator)
            seed = (seed + 2 ** 63) % 2 ** 64 - 2 ** 63                        # as int64 bits
            p0 = next(iter(net.parameters()), None)
            self.rng_state = torch.tensor([seed, 0], dtype=torch.int64, device=p0.device if p0 is not None else "cpu")
        # inference frames of several chunks are written into frame-sized maps chunk by chunk (no concatenation at the end);
        # cfg.frame_outputs = False (or PNR_FRAME_OUT=0) restores per-chunk maps + torch.cat
        self.frame_outputs = bool(_get(cfg, "frame_outputs", os.environ.get("PNR_FRAME_OUT", "1") != "0"))
        # inference frames of several chunks: the fine level of chunk c runs BESIDE the coarse level of chunk c + 1 (two streams, the
        # two-tile MLP launches capped to 3/4 and 1/4 of the compute units = the levels' 192 : 64 samples), so the small per-ray
        # kernels of one chunk overlap with those of the other instead of standing between the MLP launches (_render_overlapped);
        # cfg.overlap_levels = False (or PNR_OVERLAP=0) keeps every launch of a frame on the caller's stream
        self.overlap_levels = bool(_get(cfg, "overlap_levels", os.environ.get("PNR_OVERLAP", "1") != "0"))
        self._side_streams = {}
        if self.N_importance > 0 and getattr(net, "nerf_1", None) is None and not getattr(net, "share_coarse_fine", False):
            raise ValueError("make_renderer: cfg asks for a fine pass (N_importance / cascade_samples = %d) but the network "
                             "was built without a fine NeRF -- build it with make_network(cfg) from the SAME cfg, or set "
                             "cfg.share_coarse_fine = True to evaluate one NeRF at both levels on purpose" % self.N_importance)

    def _preamble(self, rays, box, box_ids, t_rand, z_out):
        """a chunk's per-ray preamble: (hits or None, z of the coarse level, its labels or None)"""
        hits = lab0 = None
        hull = self.bbox_sampling == "hull"
        prims = isinstance(box, Prims)
        if box is not None and not prims and self.max_hits <= ops.RAY_SETUP_MAX_HITS:
            # rows a8 + a3 in one launch: hit lists, z and the coarse labels (pnr_ray_setup; bit for bit the separate kernels)
            hits, z, ls0, li0 = ops.ray_setup(rays, box, box_ids, self.N_samples, self.max_hits, self.lindisp, t_rand, hull, out=z_out)
            lab0 = (ls0, li0)
        else:
            if prims:       # convex primitives: their own producer of the hit lists, then the separate kernels (no fused twin)
                hits = ops.convex_hits(rays, box.planes, box.offsets, self.max_hits)
            elif box is not None:
                hits = ops.bbox_hits(rays, box, self.max_hits)
            rays_s = ops.restrict_rays(rays, hits[0], hits[2]) if (hits is not None and hull) else rays
            z = ops.stratified(rays_s, self.N_samples, self.lindisp, t_rand, out=z_out)
        return hits, z, lab0

    # --- the stages of one chunk; render_rays composes them on the caller's stream, _render_overlapped on its side streams
    def _labels(self, z, hits, box_ids, lab=None):
        """(semantic, instance) labels of the samples z: `lab` where the kernel that made z labelled them, (None, None) without a prior"""
        if lab is not None:
            return lab
        return ops.sample_labels(z, hits[0], hits[1], hits[2], box_ids) if hits is not None else (None, None)

    def _noise(self, lv, z, train, rng):
        """the sigma noise of a training level: a tensor, an ops.Draw (device RNG) or None"""
        if not (self.raw_noise_std > 0 and train):
            return None
        if rng is not None:
            return ops.Draw(rng[0], 3 + lv, rng[1], self.raw_noise_std)
        return torch.randn(z.shape, device=z.device) * self.raw_noise_std

    def _need_weights(self, lv):
        return self.keep_weights or (lv == 0 and self.N_importance > 0)     # (the fine level samples the coarse weights)

    def _level(self, lv, rays, z, labels, noise, out, grad, wg_cap=0):
        """One level of one chunk: the MLP and the compositing of the samples z -> the level's dict under the ops' key names.
        out: the level's caller-owned tensors (_level_out; inference only).  wg_cap: the fused plan-2 launch on at most that many
        workgroups (_render_overlapped)."""
        net, dev = self.net, rays.device
        ls, li = labels
        n0 = net.nerf(0)
        if grad:
            from . import train as _train       # autograd path
            return _train.level_train(self, lv, rays, z, ls, li, noise)
        weights_only = lv == 0 and self.coarse_outputs == "weights"
        need_w = self._need_weights(lv)
        d = net.nerf(lv).desc(net.precision)
        if weights_only and self.fuse and ops.sigma_pass_supported(d, z.shape[1], noise):
            desc, img = net.packed(0, dev, fused="sigma")          # trunk + sigma only (pnr_mlp_forward_composite, plan 3)
            return ops.mlp_forward_weights(desc, img, rays, z, ls, li, out=out)
        if not weights_only and self.fuse and ops.fused_supported(d, z.shape[1], self.sem_mode, noise):
            # rows a5 + a6 in one pass: no raw image round trip (pnr_mlp_forward_composite, its own chunk order)
            desc, img = net.packed(lv, dev, fused=ops.fused_image(self.sem_mode))
            return ops.mlp_forward_composite(desc, img, rays, z, ls, li, self.white_bkgd, need_w, out=out, sem_mode=self.sem_mode,
                                             wg_cap=wg_cap)
        # the two-kernel level.  Weights only (fp32, sigma noise, an N the sigma pass does not take): the full level, its maps dropped
        desc, img = net.packed(lv, dev)
        raw = ops.mlp_forward(desc, img, rays, z, channel_major=True)
        res = ops.composite(raw, z, rays, n0.n_sem, n0.n_inst, True, noise, ls, li, self.sem_mode, self.white_bkgd, need_w, out=out)
        return {k: v for k, v in res.items() if k not in ops.WEIGHTS_ONLY_DROPS} if weights_only else res

    def _resample(self, z, weights, hits, box_ids, u, z_out):
        """(z of the fine level, its labels or None) from the coarse level's z and weights"""
        w0 = weights.detach().contiguous()
        if hits is not None:        # rows a7 + a8 in one launch: the wave that merged a ray's samples labels them
            z_fine, ls1, li1 = ops.sample_pdf_labels(z, w0, self.N_importance, hits, box_ids, u, out=z_out)
            return z_fine, (ls1, li1)
        z_fine, _, _ = ops.sample_pdf(z, w0, self.N_importance, u, want_samples=False, out=z_out)
        return z_fine, None

    # --- one chunk of rays: the reference's render_rays (row a2)
    def render_rays(self, rays, box=None, box_ids=None, t_rand=None, u=None, train=False, grad=False, out=None, rng=None):
        """rng: (call, ray_base) of the device RNG (cfg.rng = "device": render() issued the call, ray_base = this chunk's first row
        of the flattened batch) -- t_rand, u and the sigma noise are then drawn inside the kernels.  out: optional {output key:
        caller-owned tensor of this chunk's shape} (inference only) -- render() passes row slices of the frame-sized maps, so the
        chunks of a frame are never concatenated.  Every launch goes to the caller's stream and no event is made: a call can be
        captured in a HIP graph."""
        Nc, Nf = self.N_samples, self.N_importance
        dev = rays.device
        out = out if (out and not grad) else {}
        draw = self.perturb > 0 and train
        if t_rand is None and draw:
            t_rand = ops.Draw(rng[0], 1, rng[1]) if rng is not None else torch.rand((rays.shape[0], Nc), device=dev)
        hits, z, lab0 = self._preamble(rays, box, box_ids, t_rand, out.get("z_vals_0"))
        if hits is not None and self.strict_hits:          # accumulated on the device; checked ONCE at the end of render() (a single sync)
            over = torch.stack([(hits[2] > self.max_hits).sum(), hits[2].max()])
            self._overflow = over if self._overflow is None else torch.stack([self._overflow[0] + over[0],
                                                                              torch.maximum(self._overflow[1], over[1])])
        lab0 = self._labels(z, hits, box_ids, lab0)
        o0 = self._level(0, rays, z, lab0, self._noise(0, z, train, rng), _level_out(out, 0), grad)
        ret = _keyed(o0, z, 0)
        if Nf > 0:
            if u is None and draw:
                u = ops.Draw(rng[0], 2, rng[1]) if rng is not None else torch.rand((rays.shape[0], Nf), device=dev)
            z_fine, lab1 = self._resample(z, o0["weights"], hits, box_ids, u, out.get("z_vals_1"))
            lab1 = self._labels(z_fine, hits, box_ids, lab1)
            o1 = self._level(1, rays, z_fine, lab1, self._noise(1, z_fine, train, rng), _level_out(out, 1), grad)
            ret.update(_keyed(o1, z_fine, 1))
        return ret

    def _output_maps(self, R, has_box, dev, grad=False):
        """THE maps of a render of R rays -- keys, shapes and dtypes as render_rays returns them, both levels, allocated and not
        written: what a frame of several chunks is rendered into (every chunk gets its row slices as out=) and, at R = 0, what
        a render of no rays returns.  fix_* only with a prior; no level 1 without a fine level; cfg.coarse_outputs = "weights"
        (inference: not grad) drops the coarse maps that mode does not make.  Under autograd (grad: only the render of no rays
        asks) the per-ray keys are train.level_train's: the weights of both levels whatever cfg.keep_weights says.  The training
        path's per-level scalars (ce3d_*: means over labelled samples, and their counts) are not maps and are not here."""
        n0 = self.net.nerf(0)
        lab = True if has_box else None
        Nc, Nf = self.N_samples, self.N_importance
        ret = {}
        for lv, N in ((0, Nc), (1, Nc + Nf)) if Nf > 0 else ((0, Nc),):
            drop = ops.WEIGHTS_ONLY_DROPS if (lv == 0 and not grad and self.coarse_outputs == "weights") else ()
            m = ops._maps(None, R, N, n0.n_sem, n0.n_inst, lab, lab, grad or self._need_weights(lv), dev, drop=drop)
            ret.update(_keyed(m, torch.empty((R, N), device=dev, dtype=torch.float32), lv))
        return ret

    def _empty_outputs(self, lead, has_box, dev, grad=False):
        """render() of zero rays: every output key of a non-empty call, with zero rows and no launch (the edge case a caller
        hits with an empty shard: n_rays < world, or a mask that selects nothing)."""
        return _unflatten(self._output_maps(0, has_box, dev, grad), lead)

    # --- inference frames of several chunks: the levels of neighbouring chunks side by side
    def _overlap_caps(self, dev, plan, grad, train, has_box, t_rand, u):
        """(coarse, fine) workgroup caps of the overlapped frame, or None where it does not apply: inference, >= 2 chunks, both levels
        on the two-tile kernel (the only launch that takes PNR_MLP_WG_CAP), frame-sized outputs, and a device whose compute units
        split into two multiples of 8 (one per XCD: the dispatcher deals workgroups round-robin over the 8 XCDs, and a ninth
        workgroup on a 32-CU XCD waits for a whole launch -- 196 + 60 took 25 ms where 192 + 64 takes 14.2, tools/overlap_probe.py) in
        the ratio of the levels' samples within 5 %.  Not with cfg.coarse_outputs = "weights": the sigma-only coarse kernel takes no
        workgroup cap, and the split above assumes the same cost per sample at both levels -- such frames run serially.  Nor with
        explicit t_rand / u in the batch (the overlapped chunks take none), with cfg.strict_hits (its overflow count is gathered chunk
        by chunk on one stream), with cfg.fuse_composite = False, or while the caller's stream is being captured (events across
        streams).  The preamble is no condition: frames behind max_hits > 8 or convex primitives overlap too."""
        if (not self.overlap_levels or grad or train or len(plan) < 2 or not self.fuse or not self.frame_outputs or self.N_importance <= 0
                or self.strict_hits or t_rand is not None or u is not None or self.raw_noise_std > 0 and train
                or self.coarse_outputs == "weights" or torch.cuda.is_current_stream_capturing()):
            return None
        net, Nc, Nt = self.net, self.N_samples, self.N_samples + self.N_importance
        for lv, N in ((0, Nc), (1, Nt)):
            d = net.nerf(lv).desc(net.precision)
            if not ops.fused_supported(d, N, self.sem_mode, None) or net.packed(lv, dev, fused=ops.fused_image(self.sem_mode))[0].plan != 2:
                return None
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        cap_c = int(round(cus * Nc / float(Nc + Nt) / 8.0)) * 8
        cap_f = cus - cap_c
        if cus % 8 or cap_c < 8 or cap_f < 8 or abs((Nc / float(cap_c)) / (Nt / float(cap_f)) - 1.0) > 0.05:
            return None
        return cap_c, cap_f

    def _render_overlapped(self, rays, box, box_ids, plan, caps, lead):
        """Chunks alternate between two side streams; a chunk's whole chain (ray_setup, coarse MLP, combine, sample_pdf + labels, fine
        MLP, combine) stays on its stream, and ONE cross-stream rule aligns the pipeline: the coarse MLP of chunk c + 1 (on cap_c
        workgroups) waits for chunk c's sample_pdf, i.e. starts together with chunk c's fine MLP (on cap_f workgroups).  The first
        coarse and the last fine launch have the device to themselves.  Same kernels on the same inputs as the serial frame: every
        map is the same bits (tests/test_gpu_configs.py::test_full_frame_in_one_launch_equals_the_chunked_frame).  However the loop
        ends, the caller's stream waits for both side streams: rays, boxes and the frame go back to the allocator on that stream."""
        dev = rays.device
        cap_c, cap_f = caps
        last = len(plan) - 1
        frame = self._output_maps(rays.shape[0], box is not None, dev)
        main = torch.cuda.current_stream(dev)
        if dev not in self._side_streams:
            self._side_streams[dev] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
        side = self._side_streams[dev]
        start = torch.cuda.Event()
        start.record(main)
        for st in side:
            st.wait_event(start)           # rays, boxes, the frame maps: everything the side streams read or write exists
        prev_pdf = None
        pre = {}                        # chunk -> its preamble, where that was issued early

        def preamble(cj):
            sj, ej = plan[cj]
            return self._preamble(rays[sj:ej], box, box_ids, None, frame["z_vals_0"][sj:ej])
        try:
            for ci, (s, e) in enumerate(plan):
                r, st = rays[s:e], side[ci & 1]
                out = {k: v[s:e] for k, v in frame.items()}
                with torch.cuda.stream(st):
                    hits, z, lab0 = pre.pop(ci) if ci in pre else preamble(ci)
                    lab0 = self._labels(z, hits, box_ids, lab0)
                    if prev_pdf is not None:
                        st.wait_event(prev_pdf)             # the coarse MLP starts beside the other chunk's fine level
                    o0 = self._level(0, r, z, lab0, None, _level_out(out, 0), False, 0 if ci == 0 else cap_c)
                    z_fine, lab1 = self._resample(z, o0["weights"], hits, box_ids, None, out["z_vals_1"])
                    prev_pdf = torch.cuda.Event()
                    prev_pdf.record(st)
                    if ci + 2 <= last:
                        pre[ci + 2] = preamble(ci + 2)      # of the chunk after next, in front of this chunk's fine MLP
                    lab1 = self._labels(z_fine, hits, box_ids, lab1)
                    o1 = self._level(1, r, z_fine, lab1, None, _level_out(out, 1), False, 0 if ci == last else cap_f)
                    _fill_rows(out, {**_keyed(o0, z, 0), **_keyed(o1, z_fine, 1)})
        finally:
            for st in side:
                done = torch.cuda.Event()
                done.record(st)
                main.wait_event(done)
        return _unflatten(frame, lead)

    # --- the plugin entry point (row a1)
    def render(self, batch):
        rays = batch["rays"]
        if not rays.is_cuda:
            raise RuntimeError("Renderer.render: batch['rays'] must be on the GPU (no CPU fallback)")
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.net.parameters())
        if grad and self.net.precision not in ("bf16", "fp32"):
            raise ValueError("Renderer.render: precision must be 'bf16' (the training path) or 'fp32' (its parity mode)")
        lead = rays.shape[:-1]
        rays = rays.reshape(-1, 8).float().contiguous()
        R = rays.shape[0]
        box = batch.get("bbox")
        box_ids = batch.get("bbox_ids")
        if batch.get("prim_planes") is not None:
            if box is not None:
                raise ValueError("Renderer.render: the batch has both 'bbox' and 'prim_planes' -- one prior per render: turn the "
                                 "cuboids into primitives with ConvexSet.from_boxes and join the sets with ConvexSet.concat")
            if batch.get("prim_offsets") is None or batch.get("prim_ids") is None:
                raise ValueError("Renderer.render: 'prim_planes' comes with 'prim_offsets' and 'prim_ids' (ConvexSet.batch())")
            box = Prims(batch["prim_planes"].reshape(-1, 4).float().contiguous(), batch["prim_offsets"].reshape(-1).int().contiguous())
            box_ids = batch["prim_ids"].reshape(-1, 2).int().contiguous()
            if box_ids.shape[0] != box.offsets.numel() - 1:
                raise ValueError("Renderer.render: prim_ids has %d rows for %d primitives" % (box_ids.shape[0], box.offsets.numel() - 1))
        elif box is not None:
            box = box.reshape(-1, 15).float().contiguous()
            box_ids = box_ids.reshape(-1, 2).int().contiguous()
        self._overflow = None
        if R == 0:          # (before t_rand / u: uniforms for no rays have no second dimension to infer)
            return self._empty_outputs(lead, box is not None, rays.device, grad)
        t_rand, u = batch.get("t_rand"), batch.get("u")
        if t_rand is not None:
            t_rand = t_rand.reshape(R, -1).float().contiguous()
        if u is not None:
            u = u.reshape(R, -1).float().contiguous()
        train = self.net.training
        plan = chunk_plan(R, self.chunk_size)
        caps = self._overlap_caps(rays.device, plan, grad, train, box is not None, t_rand, u)
        if caps is not None:
            return self._render_overlapped(rays, box, box_ids, plan, caps, lead)
        call = None
        if self.rng == "device" and train and (self.perturb > 0 or self.raw_noise_std > 0):
            if self.rng_state.device != rays.device:
                self.rng_state = self.rng_state.to(rays.device)
            call = ops.rng_begin(self.rng_state)        # one offset per call; every chunk and level draws from it
        # inference frames of several chunks: frame-sized maps, every chunk writes its own rows
        frame = self._output_maps(R, box is not None, rays.device) if (len(plan) > 1 and not grad and self.frame_outputs) else None
        outs = []
        for s, e in plan:
            rows = None if frame is None else {k: v[s:e] for k, v in frame.items()}
            o = self.render_rays(rays[s:e], box, box_ids,
                                 None if t_rand is None else t_rand[s:e],
                                 None if u is None else u[s:e], train, grad, out=rows,
                                 rng=None if call is None else (call, s))
            if frame is not None:
                _fill_rows(rows, o)
            else:
                outs.append(o)
        if self._overflow is not None:
            n_over, worst = (int(v) for v in self._overflow.tolist())         # the one device sync of strict_hits
            self._overflow = None
            if n_over > 0:
                raise RuntimeError("Renderer.render: %d ray(s) cross more than max_hits = %d boxes (up to %d): the farthest "
                                   "intervals were dropped -- raise cfg.max_hits" % (n_over, self.max_hits, worst))
        return _unflatten(frame if frame is not None else merge_chunks(outs), lead)

    # --- a whole frame of a camera (panopticnerf_amd/camera.py): rays for the pixels that see anything, maps as images
    def render_view(self, camera, c2w, near, far, bbox=None, bbox_ids=None, prims=None):
        """Render one frame of `camera` (camera.Pinhole / Fisheye / Equirect) at pose c2w (3x4, host values): rays are made for
        camera.valid_pix() only -- a fisheye frame skips the pixels outside the lens (and the user mask) --, rendered by
        render() (chunking, overlap and fused-plan decisions are render()'s), and every per-ray output is placed into a
        (height, width, ...) image that is 0 where a pixel sees nothing; "valid" (height, width) bool says where that is.
        Labels derived from such maps (ops.panoptic_labels, shard.label_maps) must be set to -1, the evaluator's "ignore",
        where valid is False: the argmax of an all-zero pixel is class 0, not "nothing".  prims: a primitives.ConvexSet as the
        prior instead of bbox / bbox_ids (moved to the network's device on first use).  depth_* of a Fisheye or Equirect frame
        is range along the unit-length ray, of a Pinhole frame z-depth (camera.py).  An Equirect frame is the panorama: every
        map over longitude x latitude, every pixel valid.  Inference only."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.net.parameters()):
            raise RuntimeError("Renderer.render_view is inference only: call it under torch.no_grad() (training batches are made "
                               "with camera.rays(pix=...) and rendered with render())")
        p0 = next(iter(self.net.parameters()), None)
        if p0 is None or not p0.is_cuda:
            raise RuntimeError("Renderer.render_view: the network must be on the GPU (no CPU fallback)")
        dev, H, W = p0.device, camera.height, camera.width
        pix = camera.valid_pix(dev)
        whole = pix.numel() == H * W
        batch = {"rays": camera.rays(c2w, near, far, pix=None if whole else pix, device=dev)}
        if bbox is not None:
            batch.update(bbox=bbox, bbox_ids=bbox_ids)
        if prims is not None:
            if prims.device != dev:
                prims.to(dev)
            batch.update(prims.batch())
        out = self.render(batch)
        valid = torch.ones((H, W), dtype=torch.bool, device=dev)
        if whole:
            ret = {k: v.reshape(H, W, *v.shape[1:]) for k, v in out.items()}
        else:
            idx = pix.long()
            valid = torch.zeros(H * W, dtype=torch.bool, device=dev).index_fill_(0, idx, True).reshape(H, W)
            ret = {}
            for k, v in out.items():
                img = torch.zeros((H * W,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
                ret[k] = img.index_copy_(0, idx, v).reshape(H, W, *v.shape[1:])
        ret["valid"] = valid
        return ret


def make_renderer(cfg, network):
    """Reference plugin surface: make_renderer(cfg, network) -> obj with .render(batch)."""
    return Renderer(network, cfg)
