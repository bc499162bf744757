/*
 * pnr.h -- C-ABI of libpnr.so, the MI355X (gfx950) implementation of PanopticNeRF's
 * render_rays hot path (BASELINE.json north_star).
 *
 * Which reference interface each entry point replaces.  The mounted reference
 * (/root/reference) contains only README.md -- README.md:7 / README.md:13 name the code
 * branches (`panopticnerf360`, `panopticnerf`) that hold lib/networks/renderer and are NOT
 * in the mount -- so no file:line can be cited for the functions themselves.  Each entry
 * below names the reference function (as BASELINE.json's north_star names it) and the
 * SURVEY.md section-8a row that specifies its arithmetic:
 *
 *   pnr_stratified      render_rays' stratified z sampler                 (8a row a3)
 *   pnr_points          pts = o + d*z                                     (8a row a3)
 *   pnr_embed           Embedder / get_embedder                           (8a row a4)
 *   pnr_mlp_*           Network (NeRF 8x256 MLP + semantic/instance heads) (8a row a5)
 *   pnr_mlp_forward_train / pnr_mlp_backward   autograd of the Network   (8a row a9)
 *   pnr_composite       raw2outputs (+ panoptic logit / fixed-field maps) (8a row a6)
 *   pnr_composite_backward   autograd backward of raw2outputs            (8a row a9)
 *   pnr_sample_pdf      sample_pdf + sorted merge with the coarse z       (8a row a7)
 *   pnr_bbox_hits       ray / 3D-bbox intersection (bbox prior)           (8a row a8)
 *   pnr_convex_hits     ray / convex-polytope intersection (bounding primitives as half-spaces)   (8a row a8)
 *   pnr_sample_labels   per-sample fixed semantic / instance labels        (8a row a8)
 *   pnr_ray_setup       a8 + a3 + a8 of the coarse level in one launch    (8a rows a3, a8)
 *   pnr_sample_pdf_labels   a7 + a8 of the fine level in one launch       (8a rows a7, a8)
 *   pnr_*_rng, pnr_rng_begin / _fill   the above with torch.rand / torch.randn drawn in the kernel (8a rows a3, a6, a7, a9)
 *   pnr_sample_batch    the dataset's ray batches: pixel sampling, rays and targets of posed frames
 *   pnr_census, pnr_sgm_aggregate / _select, pnr_disparity_depth   the dataset's SGM stereo depth
 *   pnr_mesh_count / _emit   a labelled triangle mesh of the field (no reference counterpart: the reference ships no extractor)
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns every buffer; the library never allocates, frees or synchronises;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default);
 *   - int return: 0 = PNR_OK, negative = error; pnr_last_error() gives the text
 *     (thread-local);  no C++ exception crosses the ABI;
 *   - re-entrant; graph-capture safe (no hipMalloc / sync inside).
 * Arrays are dense row-major fp32 / int32 unless a stride is given.
 */
#ifndef PNR_H
#define PNR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNR_OK 0
#define PNR_EINVAL (-1)  /* bad argument (size, alignment, unsupported configuration) */
#define PNR_EHIP (-2)    /* a HIP runtime call failed; see pnr_last_error() */
#define PNR_ENODEV (-3)  /* no gfx950 device */

#define PNR_PREC_BF16 0  /* bf16 MFMA, fp32 accumulate (v_mfma_f32_32x32x16_bf16) */
#define PNR_PREC_FP32 1  /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32), parity mode */

int pnr_version(void);
const char* pnr_last_error(void);
/* Name of device `dev` copied to buf (host). Returns PNR_ENODEV if it is not gfx950. */
int pnr_device_check(int dev, char* buf_host, int buflen);

/* ---- a3: stratified sampler.  rays (R,8) = o(3) d(3) near far.  t_rand (R,N) or NULL
 * (perturb == 0).  z_out (R,N).  Bit-exact with oracle/pnr_oracle.c:pnro_stratified. */
int pnr_stratified(const float* rays, int64_t n_rays, int n_samples, int lindisp,
                   const float* t_rand, float* z_out, void* stream);

/* pts_out (R,N,3) = o + d*z.  Bit-exact with pnro_points. */
int pnr_points(const float* rays, const float* z, int64_t n_rays, int n_samples, float* pts_out,
               void* stream);

/* ---- a4: Embedder.  x (n,3) -> out (n, 3+6L), [x, sin(2^k x), cos(2^k x)]_k. */
int pnr_embed(const float* x, int64_t n, int L, float* out, void* stream);

/* ---- a5: fused NeRF MLP + heads.
 * Geometry of one network.  Trunk: D layers of width W (W = 128 or 256), skip-concat of
 * gamma(x) after layer `skip` (-1 = none).  sigma, feature(W), views(W+dir -> W/2), rgb.
 * Optional heads W -> head_W -> n_sem / n_inst (0 = absent). */
typedef struct pnr_mlp_desc {
    int32_t D, W, skip;
    int32_t xyz_L, dir_L;
    int32_t n_sem, n_inst, head_W;
    int32_t precision; /* PNR_PREC_* */
    int32_t plan;      /* chunk order of the packed image: 0 = classic (every kernel); 1 = fused-inference order, 2 = two-tile order,
                          see pnr_mlp_fused_plan; 3 = sigma only (opt-in, below) -- only pnr_mlp_forward_composite / _tiles /
                          pnr_composite_combine accept 1..3; 4 = field query (opt-in) -- only pnr_mlp_query accepts it */
    int32_t head_tap;  /* what the semantic / instance heads read: 0 = the trunk output h (default), 1 = the feature_linear
                          output (the reference's tap point cannot be checked here, so it is a switch) */
    int32_t head_depth;/* 0 or 2 = W -> head_W -> n (ReLU between; default), 1 = one Linear W -> n */
    int32_t schedule;  /* time structure of the bf16 weight stream (tests and A/B tools; the arithmetic, the packed image and the
                          results are identical bit for bit): 0 = default (ping-pong k_mlp_pp for inference launches, lock-step
                          k_mlp_fused for the training forward), 1 = lock-step everywhere, 2 = ping-pong everywhere */
    int32_t clk_probe[2]; /* diagnostics (libpnr_bench.so, tools/): low / high 32 bits of a 16-byte aligned DEVICE address of 16 bytes;
                             when non-zero the forward MLP kernels launched with this descriptor write {shader cycles, 100 MHz ticks}
                             of workgroup 0's first wave there (their ratio = the mean shader clock during the launch).  0 = off.
                             A descriptor field, not a setter: the library keeps no mutable state (round 5) */
    int32_t flags;     /* PNR_MLP_* bits, 0 by default */
} pnr_mlp_desc;
/* ZERO-INITIALISE the whole descriptor (memset / = {0}) before setting fields: clk_probe and flags are READ by every entry point
 * that takes a descriptor -- a stale clk_probe is a device address the forward kernels store to.  Every pnr_mlp_* call rejects
 * (PNR_EINVAL) flags with undefined bits and a clk_probe that is not 16-byte aligned. */

#define PNR_MLP_SOFTMAX 1      /* pnr_mlp_forward_composite / pnr_mlp_forward_tiles composite softmax(logits) over each learned field's
                                  channels instead of the logits (the reference's semantic_activation = softmax; pnr_composite's
                                  sem_mode 1).  Needs an image whose plan has a softmax kernel -- a head's logit blocks must be in
                                  registers together: plan 2 (the k_mlp_tt_*sm_* kernels, round 6) or plan 1; ask
                                  pnr_mlp_fused_plan WITH this flag set in desc.flags (0 = none: use pnr_mlp_forward + pnr_composite);
                                  PNR_EINVAL otherwise */
#define PNR_MLP_WG_CAP(n) (((n) & 0x1FF) << 16)  /* plan 2 (pnr_mlp_forward_composite / _tiles): launch on at most n workgroups (= compute units;
                                  0 = all of them).  Two launches with caps that add up to the device can run SIDE BY SIDE on two streams --
                                  one level of a chunk beside the other level of the next: Renderer's cfg.overlap_levels.  Same results. */
#define PNR_MLP_TRACE 0x7A00   /* diagnostics BUILDS of the library only (make EXTRA_TT=trace | abl; the shipped library refuses the
                                  flag), with plan 2: the trace build of k_mlp_tt -- clk_probe must then address (64 + workgroups) * 4
                                  bytes (workgroups <= number of CUs; tools/tt_trace.py allocates 1280): 64 per-unit s_memtime stamps
                                  of workgroup 0's first wave, then every workgroup's cycles.  + (a << 4), a in 1..7: its timing-only
                                  ablation a (bits 4..6 -- bit 0 stays PNR_MLP_SOFTMAX) */

/* Dense fp32 parameters in HOST memory, row-major (out,in), nn.Linear convention.
 * pts_w[i]/pts_b[i] for i < D.  Head pointers may be NULL when the head is absent; with head_depth = 1 a head is the single
 * Linear sem1_w / inst1_w of shape (n, W) and sem0_* / inst0_* are NULL. */
typedef struct pnr_mlp_params_host {
    const float* const* pts_w; const float* const* pts_b;
    const float* alpha_w; const float* alpha_b;
    const float* feature_w; const float* feature_b;
    const float* views_w; const float* views_b;
    const float* rgb_w; const float* rgb_b;
    const float* sem0_w; const float* sem0_b; const float* sem1_w; const float* sem1_b;
    const float* inst0_w; const float* inst0_b; const float* inst1_w; const float* inst1_b;
} pnr_mlp_params_host;

/* Bytes of the packed (MFMA-fragment-ordered) parameter image for `desc`; <0 on error. */
int64_t pnr_mlp_packed_bytes(const pnr_mlp_desc* desc);
/* Pack host parameters into packed_host (pnr_mlp_packed_bytes bytes, host). Pure CPU. */
int pnr_mlp_pack(const pnr_mlp_desc* desc, const pnr_mlp_params_host* params, void* packed_host);

/* Device-side packer: same image as pnr_mlp_pack (backward = 0) / pnr_mlp_pack_bwd (backward = 1), written
 * straight from the live parameter tensors on the GPU -- no host round trip per optimiser step.
 * params_dev: the struct itself (and its pts_w / pts_b pointer arrays) in HOST memory, every pointer in it a
 * DEVICE pointer.  workspace: device scratch of pnr_mlp_pack_workspace_bytes bytes (fragment descriptors).
 * packed: device buffer of pnr_mlp_packed_bytes / pnr_mlp_bwd_packed_bytes bytes.  Three small host->device
 * copies (header, chunk table, descriptors) and one kernel are enqueued on `stream`, and `stream` is synchronised
 * once before returning (the copies read call-local host staging memory): the ONE entry point that synchronises;
 * it is set-up work -- never call it inside graph capture, use pnr_mlp_repack_device there.
 * The alignment gap: the data area starts at the next multiple of 1024 behind the chunk table, and the bytes between
 * the two belong to the image (they count in pnr_mlp_packed_bytes).  pnr_mlp_pack / pnr_mlp_pack_bwd zero them; the
 * device packer writes the header, the table and the data area and LEAVES THE GAP as the caller handed it in, so a
 * device image equals the host image byte for byte only in a buffer whose gap was zero (ops.pack_mlp_device allocates
 * zeros).  Nothing outside [0, packed bytes) and [0, workspace bytes) is written. */
int64_t pnr_mlp_pack_workspace_bytes(const pnr_mlp_desc* desc, int backward);
int pnr_mlp_pack_device(const pnr_mlp_desc* desc, const pnr_mlp_params_host* params_dev, int backward,
                        void* workspace, void* packed, void* stream);
/* The packing kernel alone, for parameters that CHANGED IN PLACE since a pnr_mlp_pack_device call with the same desc,
 * parameter pointers, workspace and packed buffer (an optimiser step): no host-to-device copy, graph-capture safe. */
int pnr_mlp_repack_device(const pnr_mlp_desc* desc, const pnr_mlp_params_host* params_dev, int backward,
                          void* workspace, void* packed, void* stream);

/* Evaluate the network on every sample of every ray:
 *   pts = o + d*z, viewdir = d/||d||, raw = MLP(gamma(pts), gamma(viewdir)).
 * packed: device copy of the pnr_mlp_pack image.  rays (R,8), z (R,N).
 * raw element (sample s = r*N+i, channel c) is written at raw[s*raw_stride_s + c*raw_stride_c],
 * channels = [r g b sigma | n_sem | n_inst].  Channel-major (stride_s=1, stride_c=R*N) is the
 * fast layout; sample-major (stride_s=4+n_sem+n_inst, stride_c=1) is the reference's. */
int pnr_mlp_forward(const pnr_mlp_desc* desc, const void* packed, const float* rays, const float* z,
                    int64_t n_rays, int n_samples, float* raw, int64_t raw_stride_s,
                    int64_t raw_stride_c, void* stream);

/* ---- a5 + a6 fused (inference): evaluate the network and composite in ONE pass -- the raw image (4 + n_sem + n_inst floats per
 * sample) never goes to HBM.  The fused MLP's epilogue keeps per 32-sample tile one record (csrc/pnr_mlp_fuse.h: transmittance
 * factor and the weighted logit sums) and per sample (local weight, raw r, g, b): 26 B per sample instead of 324 at 45 / 32
 * heads; a second small kernel finishes each ray from them (acc / depth / rgb sums, the fixed fields, the logits).  Replaces the pair
 * pnr_mlp_forward + pnr_composite (same reference rows: render_rays' network call + raw2outputs, /root/reference/README.md:13
 * points to the branch that holds them) under: bf16, logits compositing (sem_mode 0), no sigma noise, n_samples a
 * multiple of 32 in [32, 256], n_sem + n_inst <= 128.  Results equal the two-kernel path to fp32 rounding (the sums are
 * associated per tile).  Outputs as pnr_composite's (any may be null; fix_* need their labels); weights (R,N) optional.
 * workspace: pnr_mlp_forward_composite_workspace_bytes(desc, n_rays, n_samples, weights != null) device bytes (tile records,
 * per-sample quadruples and 128 B per ray: |d| and gamma(d / |d|) once per ray, written by a pre-kernel for the plan-2 kernel --
 * which takes at most 2^24 rays per call; plan 3: records of the transmittance factor alone and the quadruples, no per-ray table). */
/* Chunk order for images that only pnr_mlp_forward_composite will consume: the BEST plan `desc`'s geometry has.
 *   1: the fused-inference plan (bf16, W = 256, 1..2 semantic and 0..1 instance logit blocks of 32): the appearance branch, then
 *      BOTH head hidden layers, then the two logit layers as ONE chunk (k_mlp_pp: 8 waves, one 32-sample tile per wave);
 *   2: the two-tile plan (the 8 x 256 network of the BASELINE configs: D = 8, skip = 4, L = 10 / 4, head_tap 0; no heads, a
 *      semantic head of up to 64 classes, that plus an instance head of up to 32, or a semantic head of 65..96 classes alone; any head_tap / head_depth): no chunk above 33 fragments, consumed by
 *      k_mlp_tt -- hand-placed gfx950 assembly, one wave per SIMD, two tiles per wave, every LDS weight fragment feeds two MFMAs
 *      (csrc/asm/gen_mlp_tt.py);
 *   0: the classic order, which every entry point accepts.
 * Set desc.plan to the returned value (or to a smaller supported one: plan 1 needs a semantic head) before pnr_mlp_packed_bytes / pnr_mlp_pack* and keep it
 * for the forward call.  Same arithmetic per layer under every plan: records and maps are bit-identical (head_depth 1: plan 2 against
 * plan 0 to fp32 rounding).  With PNR_MLP_SOFTMAX in desc.flags the answer is the best plan that has a SOFTMAX kernel (2, 1, or 0 = none).
 *
 * Plan 3, the sigma-only image (never returned here: set desc.plan = 3 yourself).  For a level that is read only for its compositing
 * weights -- the coarse level of a frame with a fine level.  bf16, W = 128 or 256, any trunk: the trunk chunked as in plan 1 (layer 0
 * as one chunk), then ONE 32-row block whose row 3 is alpha_linear over h (bias alpha_b) and every other row zero; no feature, views,
 * rgb or head layers (pnr_mlp_pack* read only pts_* and alpha_*).  Through pnr_mlp_forward_composite / pnr_mlp_forward_tiles /
 * pnr_composite_combine with rgb, sem and inst NULL (PNR_EINVAL otherwise): depth, acc, weights and fix_* are the bits every other
 * plan of the same network gives; the records hold no logit sums, so n_sem / n_inst only size fix_*; PNR_MLP_SOFTMAX is accepted and
 * has no effect; N a multiple of 32 in [32, 256] as for every plan.  pnr_mlp_forward and the backward refuse it (plan 0 only). */
int pnr_mlp_fused_plan(const pnr_mlp_desc* desc);
int64_t pnr_mlp_forward_composite_workspace_bytes(const pnr_mlp_desc* desc, int64_t n_rays, int n_samples, int want_weights);
int pnr_mlp_forward_composite(const pnr_mlp_desc* desc, const void* packed, const float* rays, const float* z,
                              int64_t n_rays, int n_samples, const int32_t* label_sem, const int32_t* label_inst,
                              int white_bkgd, float* rgb, float* depth, float* acc, float* weights, float* sem,
                              float* inst, float* fix_sem, float* fix_inst, void* workspace, void* stream);

/* The two halves of pnr_mlp_forward_composite as separate calls (it is exactly these two, in this order, on one workspace):
 * pnr_mlp_forward_tiles runs the fused MLP -- per 32-sample tile one record (transmittance factor, logit sums), per sample
 * (local weight, raw r, g, b) -- and pnr_composite_combine finishes every ray from them (k_composite_combine: one wave per ray).
 * Same arguments and conditions as pnr_mlp_forward_composite. */
int pnr_mlp_forward_tiles(const pnr_mlp_desc* desc, const void* packed, const float* rays, const float* z, int64_t n_rays,
                          int n_samples, void* workspace, void* stream);
int pnr_composite_combine(const pnr_mlp_desc* desc, const void* workspace, const float* z, int64_t n_rays, int n_samples,
                          const int32_t* label_sem, const int32_t* label_inst, int white_bkgd, float* rgb, float* depth,
                          float* acc, float* weights, float* sem, float* inst, float* fix_sem, float* fix_inst, void* stream);

/* Field query: what the network holds AT A 3D POINT -- density and the two panoptic distributions, none of which reads a view
 * direction (no ray, no z, no rgb).  Needs the plan-4 image (never returned by pnr_mlp_fused_plan: set desc.plan = 4 yourself
 * before pnr_mlp_packed_bytes / pnr_mlp_pack*; bf16, W = 128 or 256, every trunk plan 3 takes, heads of any width up to 256):
 * plan 3's chunks (trunk, layer 0 as one chunk; the sigma block), then feature_linear where head_tap = 1 and a head exists, then
 * the head layers chunked as in plan 0.  Every fragment is plan 0's fragment of the same layer, block and k-step, and the kernel
 * (k_mlp_pp_field) multiplies them in plan 0's order: sigma and the logits are BIT FOR BIT rows 3, 4.., 4 + n_sem.. of
 * pnr_mlp_forward's raw image at the same fp32 position (a ray with o = point, z = 0).  pnr_mlp_pack* read pts_*, alpha_*, the
 * heads, and feature_* only where it is in the image.
 *   points      (n_points, 3) fp32, contiguous.  0 <= n_points < 2^31 - 4096 per call; n_points = 0 returns PNR_OK at once.
 *   sigma       (n_points) fp32: the raw pre-activation density (no relu, no noise), or NULL.
 *   sem_label, inst_label, panoptic   (n_points) int32 or NULL: argmax of the head's logits taken in registers -- the largest value,
 *               the lowest index among equals, a NaN read as -inf (the rule of pnr_panoptic_labels).  With is_thing (int32[n_sem])
 *               inst_label = -1 where the point's semantic class is not a thing; panoptic = class * 1000 + instance, or the class
 *               where there is no instance (pnr_panoptic_labels' contract; with no instance head panoptic = class).
 *   sem_logits  (n_sem, logit_stride), inst_logits (n_inst, logit_stride) fp32 channel-major, logit_stride >= n_points, or NULL.
 * Any subset of the outputs (at least one); a NULL output is never written, and layers no requested output needs are not
 * evaluated or streamed (sigma alone: trunk + alpha_linear; semantic outputs alone: no instance head; instance outputs of a
 * two-head network evaluate the semantic head as well -- the weight stream is sequential).  A point's outputs depend on that
 * point alone.  PNR_EINVAL before any device work for a bad argument (null desc / packed / points, every output null, an output or
 * is_thing for a head the descriptor lacks, logit_stride < n_points, plan != 4, not bf16, unsupported geometry).  Never
 * synchronises; capture-safe after one eager call per geometry.
 * pnr_mlp_query_supported: host only, 1 where the kernel exists for desc's geometry (desc.plan is ignored). */
int pnr_mlp_query(const pnr_mlp_desc* desc, const void* packed, const float* points, int64_t n_points,
                  float* sigma, int32_t* sem_label, int32_t* inst_label, int32_t* panoptic, const int32_t* is_thing,
                  float* sem_logits, float* inst_logits, int64_t logit_stride, void* stream);
int pnr_mlp_query_supported(const pnr_mlp_desc* desc);

/* ---- a9 (training): forward that also saves what the backward needs, the data-gradient pass, and the
 * buffer layouts.  bf16 only; n_sem, n_inst <= 64.
 *   acts : bf16, pnr_mlp_train_layout's acts_off[D+6] elements -- gamma(x), gamma(d) and every layer's output, one
 *          slot-ordered region of S_pad x width per tensor (S = n_rays*n_samples, S_pad = S rounded up to 256), followed by
 *          one gate BIT per element of every ReLU output (what pnr_mlp_backward reads);
 *   dys  : bf16, dys_off[D+7] elements -- every layer's pre-activation gradient dY, same layout (plus the output
 *          layers' dY = d_raw in bf16: [rgb,sigma] in 32 slots, semantic and instance logits in 64 slots each), written by
 *          pnr_mlp_backward (rows S..S_pad: zeros) for pnr_mlp_wgrad's dW = dY^T X;
 *   d_raw: (4+n_sem+n_inst, S) channel-major fp32 (pnr_composite_backward's output).
 * Slot order (csrc/pnr_mlp_layout.h): slot fb*32 + hi*16 + r <-> feature fb*32 + (r&3) + 8*(r>>2) + 4*hi.
 * Saved-tensor layout of a region (csrc/pnr_mlp_layout.h, pnr_saved_chunk): the 16-byte chunk c = slot/8 of sample s lives
 * in the 128-byte line [s >> 3][c] at position (s & 7) ^ (4 * ((c >> 1) & 1)) -- a wave's store writes full lines and a
 * 64-sample tile is one contiguous block for the weight-gradient kernel.  The buffers are opaque to callers. */
int pnr_mlp_train_layout(const pnr_mlp_desc* desc, int64_t n_samples, int64_t* acts_off_host /* D+7 */,
                         int64_t* dys_off_host /* D+8 */);
int pnr_mlp_forward_train(const pnr_mlp_desc* desc, const void* packed, const float* rays, const float* z,
                          int64_t n_rays, int n_samples, float* raw, int64_t raw_stride_s,
                          int64_t raw_stride_c, void* acts, void* stream);
int64_t pnr_mlp_bwd_packed_bytes(const pnr_mlp_desc* desc);
int pnr_mlp_pack_bwd(const pnr_mlp_desc* desc, const pnr_mlp_params_host* params, void* packed_host);
int pnr_mlp_backward(const pnr_mlp_desc* desc, const void* packed_bwd, const float* d_raw, const void* acts,
                     void* dys, int64_t n_rays, int n_samples, void* stream);

/* Weight gradients (the third K3 kernel): for every Linear of the network
 *     dW = dY^T X   and   db = sum over samples of dY,
 * computed from `acts` (pnr_mlp_forward_train) and `dys` (pnr_mlp_backward) of the same n_samples = n_rays * n_samples.
 * grads_dev: a pnr_mlp_params_host whose pointers are DEVICE pointers to the fp32 GRADIENT buffers, one per parameter,
 *   nn.Linear layout ((out,in) row-major / (out)); every one of them is fully overwritten (not accumulated).  The struct
 *   and its pts_w / pts_b arrays live in host memory.
 * workspace: device scratch of pnr_mlp_wgrad_workspace_bytes bytes (per-slab partial sums; deterministic reduction).
 * Replaces autograd's per-layer  grad_output.t() @ input  and  grad_output.sum(0)  for nn.Linear. */
int64_t pnr_mlp_wgrad_workspace_bytes(const pnr_mlp_desc* desc, int64_t n_samples);
int pnr_mlp_wgrad(const pnr_mlp_desc* desc, const void* acts, const void* dys, int64_t n_samples,
                  const pnr_mlp_params_host* grads_dev, void* workspace, void* stream);

/* ---- a9, fp32 PARITY MODE of the training path (precision = "fp32" with autograd): the same three steps in plain fp32 -- the
 * mode in which a parameter gradient can be checked to 1e-4 against fp32 autograd of the reference arithmetic, and in which a
 * user can tell the precision of the bf16 path from a defect.  Not a performance path (one generic strided fp32 GEMM kernel per
 * Linear and direction, deterministic fixed-order reductions).  Parameters are NOT packed: params_dev is a pnr_mlp_params_host
 * in host memory whose pointers are DEVICE pointers to the dense (out,in) row-major fp32 parameters (the nn.Parameter tensors
 * themselves), as for pnr_mlp_pack_device.  head_depth 1 | 2 and head_tap 0 | 1 are supported; desc.precision is ignored.
 *   acts      : fp32, pnr_mlp_fp32_acts_floats(desc, n_rays * n_samples) floats, layout below;
 *   raw       : as pnr_mlp_forward (any strides);   d_raw: channel-major (4+n_sem+n_inst, >= S) fp32, channel stride given;
 *   grads_dev : like pnr_mlp_wgrad's -- DEVICE pointers to the fp32 gradient buffers, every one fully overwritten;
 *   workspace : pnr_mlp_backward_fp32_workspace_bytes device bytes: the gradients in flight, S (3 W + 2 (W/2)) floats, then
 *               ceil(S / 2048) blocks of weight- and bias-gradient partial sums, each as large as the widest weight gradient
 *               of the call (rows x columns, + rows where the Linear has a bias; with head_depth 1 a head's own W -> n Linear
 *               counts, and is the widest at W = 128 from n around 132 upward).
 * Replaces torch autograd of the reference's Network for the fp32 case.
 *
 * Layout of acts (S = n_rays * n_samples, sample s = ray * n_samples + i): regions in this order, without gaps, each dense
 * row-major [S][width] fp32, the first at float 0 and the last ending at pnr_mlp_fp32_acts_floats:
 *   EX       [S][3 + 6 xyz_L]  gamma(x) of the point o + d z: x, then per band k (sin(2^k x), cos(2^k x)), 3 columns each
 *   ED       [S][3 + 6 dir_L]  gamma(d) of d / ||d||, same column order
 *   X_1..X_D [S][W] each       post-ReLU outputs of pts_linears.0 .. D-1 (X_D is the trunk output h)
 *   F        [S][W]            feature_linear's output (no ReLU)
 *   G        [S][W/2]          post-ReLU output of views_linears.0
 *   SH_sem   [S][W/2]          post-ReLU hidden layer of the semantic head: present only if n_sem > 0 and head_depth != 1
 *   SH_inst  [S][W/2]          the same for the instance head (n_inst > 0 and head_depth != 1)
 * The backward takes every ReLU gate from these saved outputs (x > 0). */
int64_t pnr_mlp_fp32_acts_floats(const pnr_mlp_desc* desc, int64_t n_samples);
int64_t pnr_mlp_backward_fp32_workspace_bytes(const pnr_mlp_desc* desc, int64_t n_samples);
int pnr_mlp_forward_train_fp32(const pnr_mlp_desc* desc, const pnr_mlp_params_host* params_dev, const float* rays,
                               const float* z, int64_t n_rays, int n_samples, float* raw, int64_t raw_stride_s,
                               int64_t raw_stride_c, float* acts, void* stream);
int pnr_mlp_backward_fp32(const pnr_mlp_desc* desc, const pnr_mlp_params_host* params_dev, const float* d_raw,
                          int64_t d_raw_stride_c, const float* acts, int64_t n_rays, int n_samples,
                          const pnr_mlp_params_host* grads_dev, void* workspace, void* stream);

/* ---- a6: raw2outputs.  raw strides as above.  noise (R,N) or NULL; label_* (R,N) int32 or
 * NULL (fixed bbox-prior field, -1 = none).  sem_mode 0: composite logits; 1: softmax first.
 * Any output pointer may be NULL.  weights (R,N); rgb (R,3); depth (R); acc (R);
 * sem/fix_sem (R,n_sem); inst/fix_inst (R,n_inst).  n_samples % 4 == 0, n_samples <= 256. */
int pnr_composite(const float* raw, int64_t raw_stride_s, int64_t raw_stride_c, const float* z,
                  const float* rays, const float* noise, const int32_t* label_sem,
                  const int32_t* label_inst, int64_t n_rays, int n_samples, int n_sem, int n_inst,
                  int sem_mode, int white_bkgd, float* rgb, float* depth, float* acc, float* weights,
                  float* sem, float* inst, float* fix_sem, float* fix_inst, void* stream);

/* ---- a9 (backward of a6): gradient of the composited maps w.r.t. raw.  Channel-major images only
 * (raw_stride_s == 1).  g_* are the upstream gradients of the forward outputs of the same name
 * (any may be NULL = zero); g_weights (R,N) is the gradient of the weights output.  d_raw has raw's
 * shape and layout.  sem_mode 0 (logit compositing) only; no gradient flows into z (sample_pdf's
 * output is detached in the reference). */
int pnr_composite_backward(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                           const float* noise, int64_t n_rays, int n_samples, int n_sem, int n_inst,
                           const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                           const float* g_inst, const float* g_weights, float* d_raw, void* stream);

/* pnr_composite_backward plus the two gradient sources the trainer's loss wrapper adds:
 *   g_fix_sem (R,n_sem) / g_fix_inst (R,n_inst): gradients of the FIXED (bbox-prior) maps; since
 *     fix_x[c] = sum_i w_i [label_i == c], they reach the densities through the weights: dL/dw_i += g_fix_x[label_i];
 *   ce_sem / ce_inst: DEVICE scalars s; adds s * (softmax_c(raw logits of sample) - [c == label]) to d_raw for every
 *     sample with 0 <= label < n_sem (n_inst; other labels are ignored, as in the fixed fields) -- the gradient of the
 *     per-sample 3D cross-entropy whose value pnr_ce3d computes (s = upstream gradient * loss weight / number of labelled
 *     samples).
 * label_sem / label_inst (R,N) int32 are the labels pnr_sample_labels produced for this level. */
int pnr_composite_backward2(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                            const float* noise, int64_t n_rays, int n_samples, int n_sem, int n_inst,
                            const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                            const float* g_inst, const float* g_weights, const int32_t* label_sem,
                            const int32_t* label_inst, const float* g_fix_sem, const float* g_fix_inst,
                            const float* ce_sem, const float* ce_inst, float* d_raw, void* stream);
/* ... and with pnr_composite's sem_mode: 1 = the semantic / instance maps composite softmax(logits) per sample
 * (g_sem / g_inst are then gradients of probability maps):  d x_{i,c} = w_i s_c (g_c - sum_k g_k s_k),
 * dL/dw_i += sum_k g_k s_k. */
int pnr_composite_backward3(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                            const float* noise, int64_t n_rays, int n_samples, int n_sem, int n_inst, int sem_mode,
                            const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                            const float* g_inst, const float* g_weights, const int32_t* label_sem,
                            const int32_t* label_inst, const float* g_fix_sem, const float* g_fix_inst,
                            const float* ce_sem, const float* ce_inst, float* d_raw, void* stream);

/* ---- 8f-1: the trainer's loss wrapper (the reference's NetworkWrapper) on the maps of
 * one level, fused with the gradient of the weighted total w.r.t. every map.  All reductions are means:
 *   [0] rgb      mean over rays and channels of (rgb - rgb_gt)^2
 *   [1] depth    mean over rays with depth_gt > 0 of |depth - depth_gt|  (depth_l2: squared error)
 *   [2] sem      mean over rays with 0 <= sem_gt < n_sem of CE(softmax(sem), sem_gt)      (learned field, 2D pseudo label)
 *   [3] fix_sem  mean over the same rays of -log(fix_sem[sem_gt] + fix_eps)                (fixed bbox-prior field)
 *   [4] inst, [5] fix_inst: the same two terms for the instance field
 *   [6] total = sum of w_x * term_x;  losses_out is 8 floats on the DEVICE.
 * Any map / target / gradient pointer may be NULL (its term is skipped / its gradient not written).  g_x has the
 * shape of map x and receives d total / d x.  workspace: pnr_losses_workspace_bytes(n_rays) device bytes.
 * Replaces ~30 eager torch launches per level (mse_loss, l1_loss, cross_entropy, nll_loss and their backwards). */
typedef struct pnr_loss_cfg {
    float w_rgb, w_depth, w_sem, w_fix_sem, w_inst, w_fix_inst;
    int32_t depth_l2;
    float fix_eps;
    int32_t maps_are_prob;   /* 1: sem / inst are composited PROBABILITIES (pnr_composite sem_mode 1): their 2D term is
                                -log(map[label] + fix_eps) like the fixed field's, not a softmax cross-entropy */
} pnr_loss_cfg;
int64_t pnr_losses_workspace_bytes(int64_t n_rays);
int pnr_losses(const pnr_loss_cfg* cfg, int64_t n_rays, int n_sem, int n_inst, const float* rgb, const float* depth,
               const float* sem, const float* fix_sem, const float* inst, const float* fix_inst, const float* rgb_gt,
               const float* depth_gt, const int32_t* sem_gt, const int32_t* inst_gt, float* losses_out, float* g_rgb,
               float* g_depth, float* g_sem, float* g_fix_sem, float* g_inst, float* g_fix_inst, void* workspace, void* stream);

/* Per-sample 3D cross-entropy (forward value) of the learned logits raw[first_channel .. +n_classes) (channel-major,
 * sample stride 1) against label (n_samples) int32, -1 = unlabelled: out2 (device) = {mean CE over labelled samples,
 * their count}.  Gradient: pnr_composite_backward2's ce_sem / ce_inst. */
int64_t pnr_ce3d_workspace_bytes(int64_t n_samples);
int pnr_ce3d(const float* raw, int64_t raw_stride_c, int first_channel, int n_classes, const int32_t* label,
             int64_t n_samples, float* out2, void* workspace, void* stream);

/* ---- 8f-2: ray generation, the dataset-side producer of batch['rays'] (the reference builds rays from the KITTI-360
 * intrinsics and poses in lib/datasets/kitti360/, not in the mount).  intr4_host = {fx, fy, cx, cy} and c2w12_host =
 * 3x4 row-major camera-to-world [R | t] (x right, y down, z forward) are HOST arrays (copied into the launch).
 * Pixel (i = column, j = row): d = R * ((i - cx)/fx, (j - cy)/fy, 1), o = t; d is not normalised.
 * pix (n_rays) int32 linear pixel indices j*width + i on the device, or NULL = the whole frame (n_rays = width*height).
 * rays (n_rays, 8) = o d near far.  Bit-exact with pnro_gen_rays. */
int pnr_gen_rays(const float* intr4_host, const float* c2w12_host, int width, int height, float near_, float far_,
                 const int32_t* pix, int64_t n_rays, float* rays, void* stream);

/* ---- cameras: fisheye and equirect ray generation and 3D -> 2D projection for all three camera models (csrc/pnr_camera.hip,
 * where pnr_gen_rays above lives too; what every kernel shares of a camera is csrc/pnr_camera_dev.h; DESIGN.md
 * "Fisheye cameras").  The fisheye model is the unified omnidirectional (MEI) model with two radial terms, as the public
 * KITTI-360 calibration files parametrise it; cam7_host = {xi, k1, k2, gamma1, gamma2, u0, v0}.  Camera axes as pnr_gen_rays.
 *
 * Projection of a camera-space point p (the defining direction):
 *   (x, y, z) = p / |p|;  x /= z + xi;  y /= z + xi;  r2 = x^2 + y^2;  s = 1 + k1 r2 + k2 r2^2
 *   u = gamma1 x s + u0;  v = gamma2 y s + v0
 *   in the domain iff z + xi > 0 and xi z + 1 > 0 (the second: for xi > 1 no pixel sees a direction behind the rim
 *   z = -1/xi; without it such a point would fold back into the image) and |p| is finite in float32.
 * Un-projection of pixel (i, j), its inverse:
 *   x = (i - u0)/gamma1;  y = (j - v0)/gamma2;  rd = sqrt(x^2 + y^2)
 *   r (1 + k1 r^2 + k2 r^4) = rd solved for r by PNR_FISHEYE_NEWTON_STEPS Newton steps from r = rd (no data-dependent exit)
 *   (x, y) *= r / rd (rd == 0: unchanged);  r2 = x^2 + y^2;  disc = 1 + (1 - xi^2) r2
 *   valid iff disc >= 0 (and r2 finite);  lam = (xi + sqrt(disc)) / (r2 + 1);  d_cam = (lam x, lam y, lam - xi)
 *   d = R d_cam, o = t.  d is UNIT LENGTH (pnr_gen_rays' d has z_cam = 1): depth along such a ray is range, not z-depth.
 * Every operation is a single + - * / sqrt in one fixed order (tests/_camera_ref.py restates it in float32, bit for bit). */
#define PNR_FISHEYE_NEWTON_STEPS 8      /* float32 is as close to float64 as it gets from 4 steps on (tests/test_camera_ref.py) */
#define PNR_CAMERA_PINHOLE 0            /* pnr_project_points: cam_host = {fx, fy, cx, cy} */
#define PNR_CAMERA_FISHEYE 1            /* pnr_project_points: cam_host = cam7 */
#define PNR_CAMERA_EQUIRECT 3           /* pnr_project_points: cam_host = {lon0, dlon, lat0, dlat}; word 2 is unassigned and refused */

/* The panoramic (equirectangular) camera (DESIGN.md 8 "Panoramic camera"): an image over longitude x latitude.
 * cam4_host = {lon0, dlon, lat0, dlat} in HALF-TURNS (units of pi).  Pixel (i, j), camera axes as pnr_gen_rays:
 *   lam = lon0 + ((float)i + 0.5f) * dlon      longitude, 0 along +z, positive towards +x
 *   psi = lat0 + ((float)j + 0.5f) * dlat      downward pitch, -0.5 straight up, +0.5 straight down
 *   (sl, cl) = sincospi(lam);  (sp, cp) = sincospi(psi);  d_cam = (cp * sl, sp, cp * cl)
 *   d = R d_cam in the accumulation order of the fisheye ray ((R0 dx + R1 dy) + R2 dz), o = t.
 * A full sphere is {-1, 2/W, -0.5, 1/H}.  d is UNIT LENGTH (depth along it is range, as for fisheye rays); every pixel is valid.
 *
 * sine, cosine and arctangent are part of the rule -- argument reduction in half-turns and the fixed float32 polynomials
 * below, one rounding per operation, no fused multiply-add -- so tests/_pano_ref.py restates the model in numpy float32 bit
 * for bit, like the other two:
 *   sincospi(x):  k = rintf(2x) (ties to even);  r = x - 0.5f k (exact, |r| <= 1/4);  t = r r;
 *                 s = r P(t),  c = Q(t),  P and Q by Horner's scheme in t from the highest coefficient down;
 *                 q = (int)k & 3 selects (sin, cos) = (s, c), (c, -s), (-s, -c) or (-c, s).
 *   atan2pi(y, x), in half-turns:  ax = |x|, ay = |y|, mx = max(ax, ay), mn = min(ax, ay);  mx == 0 gives 0;  a = mn / mx;
 *                 a > PNR_TAN_PI_8:  a' = (a - 1)/(a + 1), base = 0.25;  else a' = a, base = 0;
 *                 r = base + a' A(a' a') (Horner);  ay > ax: r = 0.5 - r;  x < 0: r = 1 - r;  y < 0: r = -r
 *                 (comparisons: -0 counts as +0).
 * P, Q: the Taylor coefficients of sin(pi r) / r and cos(pi r) in t = r^2; A: an odd 6-term fit of atan(a) / (pi a) in a^2 on
 * |a| <= tan(pi/8) (relative error 6e-10 before rounding).  Written as exact float32 values.
 *
 * Projection of a camera-space point p (after p_cam and |p_cam| as for the other models):
 *   lam = atan2pi(p0, p2);  h = sqrtf(p0 p0 + p2 p2);  psi = atan2pi(p1, h)
 *   u = (lam - lon0)/dlon - 0.5f;  v = (psi - lat0)/dlat - 0.5f
 *   longitude is periodic with per = 2.0f / fabsf(dlon) pixels:  u < -0.5f: u += per;  else u >= W - 0.5f: u -= per  (one wrap at
 *   most: a full circle has no seam, a partial range may cross +-180 degrees)
 *   in the domain iff |p_cam| > 0 and |p_cam| is finite in float32. */
#define PNR_SINPI_P0 0x1.921fb6p+1f     /*  3.14159274   */
#define PNR_SINPI_P1 -0x1.4abbcep+2f    /* -5.16771269   */
#define PNR_SINPI_P2 0x1.466bc6p+1f     /*  2.55016398   */
#define PNR_SINPI_P3 -0x1.32d2ccp-1f    /* -0.599264503  */
#define PNR_SINPI_P4 0x1.507834p-4f     /*  0.0821458846 */
#define PNR_COSPI_Q0 0x1.000000p+0f     /*  1            */
#define PNR_COSPI_Q1 -0x1.3bd3ccp+2f    /* -4.93480206   */
#define PNR_COSPI_Q2 0x1.03c1f0p+2f     /*  4.05871201   */
#define PNR_COSPI_Q3 -0x1.55d3c8p+0f    /* -1.33526278   */
#define PNR_COSPI_Q4 0x1.e1f506p-3f     /*  0.235330626  */
#define PNR_COSPI_Q5 -0x1.a6d1f2p-6f    /* -0.0258068908 */
#define PNR_ATANPI_A0 0x1.45f306p-2f    /*  0.318309873  */
#define PNR_ATANPI_A1 -0x1.b29948p-4f   /* -0.106103212  */
#define PNR_ATANPI_A2 0x1.04bc78p-4f    /*  0.0636563003 */
#define PNR_ATANPI_A3 -0x1.7352dap-5f   /* -0.0453275926 */
#define PNR_ATANPI_A4 0x1.13b6a6p-5f    /*  0.0336564295 */
#define PNR_ATANPI_A5 -0x1.3ab9c6p-6f   /* -0.0192093309 */
#define PNR_TAN_PI_8 0x1.a8279ap-2f     /*  0.41421357   */

/* rays (n_rays, 8) = o d near far as pnr_gen_rays (16-byte aligned); pix / n_rays as pnr_gen_rays.  valid (n_rays) bytes or
 * NULL: 1 where the pixel sees anything.  A pixel that does not gets o, d = 0, near = far = 0 and valid = 0, never NaN. */
int pnr_gen_rays_fisheye(const float* cam7_host, const float* c2w12_host, int width, int height, float near_, float far_,
                         const int32_t* pix, int64_t n_rays, float* rays, uint8_t* valid, void* stream);

/* Panoramic rays: rays (n_rays, 8) as pnr_gen_rays_fisheye, no valid bytes (every pixel sees something); pix / n_rays as
 * pnr_gen_rays.  PNR_EINVAL before any launch: null camera or pose, dlon == 0 or dlat == 0, a non-finite parameter, |lon0| > 1,
 * |dlon| * width > 2 (more than a full circle), a row whose pitch leaves [-0.5, 0.5] (the edges lat0 and lat0 + height * dlat),
 * bad sizes, n_rays != width*height without pix.  pnr_project_points and pnr_reproject check an equirect camera the same way. */
int pnr_gen_rays_equirect(const float* cam4_host, const float* c2w12_host, int width, int height, float near_, float far_,
                          const int32_t* pix, int64_t n_rays, float* rays, void* stream);

/* World points (n, 3) -> uv (n, 2) pixel coordinates (u = column, v = row, pixel centres at integers), range (n) = the
 * distance |p_cam| from the camera centre, valid (n) bytes = inside the projection's domain (pinhole: z_cam > 0) AND inside
 * the image (-0.5 <= u < width - 0.5, -0.5 <= v < height - 0.5).  w2c12_host: 3x4 row-major world-to-camera (host).  The
 * pinhole branch is the inverse of pnr_gen_rays: u = fx x/z + cx.  Outside the domain uv = 0; never NaN.  Any output NULL =
 * not written.  model: PNR_CAMERA_PINHOLE, _FISHEYE or _EQUIRECT (4, 7, 4 camera floats); any other word is refused. */
int pnr_project_points(int model, const float* cam_host, const float* w2c12_host, int width, int height, const float* points,
                       int64_t n, float* uv, float* range, uint8_t* valid, void* stream);

/* ---- cross-view reprojection (csrc/pnr_warp.hip; DESIGN.md 8 "Cross-view reprojection"): where a pixel of a source view,
 * lifted with the source's depth image, lands in a target view, and whether the target sees it.  The reference's evaluator is
 * not in the mount: every convention below (nearest pixel, the depth test and its default tolerance, the codes) is this
 * build's and unpinned.  Float32 throughout, every operation a single + - * / sqrt in the order given (tests/_warp_ref.py
 * restates the rule in float32, bit for bit).
 *
 * Source pixel p = pix[r] (int32, device), or p = r with pix NULL and n = width_src*height_src, as pnr_gen_rays.  The source
 * maps (depth_src, label_src) are IMAGES indexed by p, the target maps (depth_tgt, label_tgt) images indexed by q; the
 * outputs match (n) and uv (n, 2) are indexed by r.
 *   1. ray (o, d) of p from the source camera and c2w_src: the ray of pnr_gen_rays / pnr_gen_rays_fisheye /
 *      pnr_gen_rays_equirect (near, far unused).
 *   2. t = depth_src[p].  NOTHING TO REPROJECT (code -1) if the fisheye pixel sees nothing, or !(t > 0), or t is not finite
 *      (or p is outside the source image).
 *   3. X_k = o_k + t * d_k (one multiply, one add).  Right for both models: a pinhole d has z_cam = 1 and its depth is
 *      z-depth, a fisheye or equirect d is unit length and its depth is range.
 *   4. (u, v), |p_cam|, p_cam.z of X in the target camera with w2c_tgt: the arithmetic of pnr_project_points.  Outside the
 *      projection's domain or outside the image the pixel LEAVES THE VIEW (code -2).
 *   5. nearest target pixel: iu = min((int)floor(u + 0.5), width_tgt - 1), iv likewise, q = iv*width_tgt + iu (the min:
 *      u + 0.5 may round up to width_tgt).
 *   6. expected depth e in the TARGET's convention: p_cam.z for a pinhole target, |p_cam| for a fisheye or equirect target.  With
 *      depth_tgt: dt = depth_tgt[q]; !(dt > 0) or dt not finite: UNKNOWN (code -3); else visible iff
 *      |e - dt| <= tol_abs + tol_rel * e, otherwise OCCLUDED (code -4).  depth_tgt NULL: no test, the pixel is visible.
 *   7. match[r] = q when visible, else the code.  uv[r] = (u, v) of step 4 (0, 0 outside the domain and for code -1).
 *   8. with label_src and label_tgt (both or neither) and agree: a visible pixel whose ls = label_src[p] and lt = label_tgt[q]
 *      are both in [0, n_classes) counts agree[ls*n_classes + lt] += 1 -- the cross-view confusion matrix; multi-view
 *      consistency is its trace over its sum.  stats[0..4] += the number of pixels that were matched / -1 / -2 / -3 / -4.
 *      agree (n_classes^2) and stats (5) are device int64 arrays the caller zeroes once and accumulates into over pairs
 *      (integer atomics: exact, order-independent).  1 <= n_classes <= 8192; up to 128 through a per-block LDS histogram.
 * cam_*_host: {fx, fy, cx, cy}, cam7 or {lon0, dlon, lat0, dlat} by model (PNR_CAMERA_*); c2w_src12_host, w2c_tgt12_host: 3x4 row-major, host values
 * copied into the launch (baked into a stream capture).  Any of match, uv, agree, stats may be NULL.  Never synchronises.
 * PNR_EINVAL before any launch: unknown model, null camera / pose / depth_src, zero focal length or gamma, an equirect camera
 * that pnr_gen_rays_equirect refuses, bad size, labels
 * given on one side only, agree without labels, negative or non-finite tolerance, n_classes out of range.  n == 0: PNR_OK. */
int pnr_reproject(int model_src, const float* cam_src_host, const float* c2w_src12_host, int width_src, int height_src,
                  const int32_t* pix, int64_t n, const float* depth_src,
                  int model_tgt, const float* cam_tgt_host, const float* w2c_tgt12_host, int width_tgt, int height_tgt,
                  const float* depth_tgt, float tol_abs, float tol_rel,
                  const int32_t* label_src, const int32_t* label_tgt, int n_classes,
                  int32_t* match, float* uv, int64_t* agree, int64_t* stats, void* stream);

/* ---- point splatting (csrc/pnr_splat.hip; DESIGN.md 8 "Point splatting"): the forward direction of the above -- world points
 * (a LiDAR scan, labelled 3D points, a lifted view) scattered into a view of any camera model through a z-buffer, and
 * depth-error metrics against the depth image that makes.  Conventions (nearest pixel, square footprint, the key, the
 * metrics' default range) are this build's and unpinned, as for reprojection.  Float32 throughout, every operation a single
 * + - * / sqrt in the order given (tests/_splat_ref.py restates the rule in numpy, bit for bit).
 *
 * pnr_splat_points.  For point i of points (n, 3) (device), THE CONTRACT:
 *   1. (u, v), |p_cam|, p_cam.z and the domain flag of the point in the camera with w2c: the arithmetic of pnr_project_points.
 *      The point LEAVES THE VIEW unless it is in the projection's domain and -0.5 <= u < width - 0.5, -0.5 <= v < height - 0.5.
 *      A NaN or Inf coordinate ends here by these comparisons.
 *   2. nearest pixel as reprojection step 5: iu = min((int)floor(u + 0.5), width - 1), iv likewise.
 *   3. depth e in the view's convention: p_cam.z for a pinhole, |p_cam| for a fisheye or equirect view.  The point is CLIPPED
 *      unless e >= near_ && e <= far_.  0 <= near_ <= far_; far_ may be +inf (a pinhole z that overflowed then lands as +inf).
 *   4. key = ((uint64) bits(e) << 32) | (uint32)(index_base + i).  e > 0 here, and a positive float's bits order as its value.
 *   5. for every pixel (iu + dx, iv + dy) with |dx|, |dy| <= radius that lies inside the image:
 *      zbuf[q] = min(zbuf[q], key), an unsigned 64-bit atomic minimum.  radius is 0, 1 or 2.  The footprint is clipped at the
 *      image border and NEVER WRAPPED: not at the seam of a full-circle equirect image either.
 *   6. stats[0..2] += the number of points that landed / left the view / were clipped (device int64, integer atomics).
 * zbuf: caller-owned device int64 (height * width), initialised to all ones (-1) = empty; an empty cell can never equal a key
 * (its high word is a NaN pattern).  It ACCUMULATES over calls: several scans, frames or chunks of one cloud use distinct
 * index_base ranges, and the result is the same whatever their order or chunking -- the nearest point wins, a depth tie goes
 * to the lowest index.  cam_host / w2c12_host as pnr_project_points: host values copied into the launch (baked into a stream
 * capture).  stats may be NULL.  Never synchronises.  PNR_EINVAL before any launch: unknown model, null camera / pose / points
 * / zbuf, zero focal length or gamma, an equirect camera that pnr_gen_rays_equirect refuses, bad size, radius outside 0 .. 2,
 * near_ < 0 or far_ < near_ (or NaN), index_base < 0 or index_base + n > 2^31 - 1.  n == 0: PNR_OK.
 *
 * pnr_splat_resolve: per cell q of zbuf (n_pix), depth[q] = the float of the high word, or 0.0f where the cell is empty (the
 * "unknown" depth of pnr_reproject: the image can go straight in as depth_tgt); index[q] = the low word as int32, or -1.
 * Either output may be NULL.
 *
 * pnr_depth_metrics: pred, gt (n) float32, mask (n) uint8 or NULL.  A pixel COUNTS when (mask is NULL or mask[i] != 0) and
 * g = gt[i] is finite and d_min <= g <= d_max (0 < d_min <= d_max, both finite).  A counted pixel whose p = pred[i] is not
 * positive and finite adds 1 to counts[4] (missing) and nothing else.  Otherwise counts[0] += 1; in float32
 * ratio = fmaxf(p / g, g / p) (two divisions) and counts[1..3] += ratio < 1.25f / < 1.5625f / < 1.953125f (strict); in double
 * d = (double)p - (double)g and sums[0..4] += |d|, d*d, |d| / g, d*d / g, (log p - log g)^2 (each one operation per symbol).
 * counts: device int64[5], integer atomics, exact.  sums: device double[5]; each term is accumulated per thread, reduced per
 * wave and per block in a fixed order and written as a per-block partial into workspace; a one-block second kernel adds the
 * partials in block order and the total once into sums.  No floating atomics: two calls on the same input give the same bits.
 * Both arrays accumulate over calls (the caller zeroes them once).  workspace: pnr_depth_metrics_workspace_bytes(n) bytes,
 * 8-byte aligned (-1 for n < 0).  PNR_EINVAL before any launch: n < 0, a bad range, a null pred / gt / sums / counts /
 * workspace, misaligned sums / counts / workspace.  n == 0: PNR_OK. */
int pnr_splat_points(int model, const float* cam_host, const float* w2c12_host, int width, int height, const float* points,
                     int64_t n, int64_t index_base, float near_, float far_, int radius, int64_t* zbuf, int64_t* stats,
                     void* stream);
int pnr_splat_resolve(const int64_t* zbuf, int64_t n_pix, float* depth, int32_t* index, void* stream);
int64_t pnr_depth_metrics_workspace_bytes(int64_t n);
int pnr_depth_metrics(const float* pred, const float* gt, const uint8_t* mask, int64_t n, float d_min, float d_max,
                      double* sums, int64_t* counts, void* workspace, void* stream);

/* ---- stereo matching (csrc/pnr_stereo.hip; DESIGN.md 8 "Stereo depth"): a rectified 8-bit pair -> disparity in sixteenths of a
 * pixel -> depth, the producer of the stereo depth that the loss wrapper and the frame table consume.  The reference's matcher
 * is not in the mount: the rule is this build's and unpinned.  Everything is integer except step 6 (tests/_sgm_ref.py restates
 * the rule twice, bit for bit).
 *
 * Inputs: left, right (H, W) uint8, rectified (a match of left pixel x lies at right pixel x - d, d >= 0).  D = max_disp, a
 * multiple of 16 in 16 .. 256.  0 < P1 <= P2 <= 192, so one path cost, at most 63 + P2, fits a byte.  paths is 4 or 8.
 * uniqueness in 0 .. 99.  lr_tol >= 0, or -1 for "no left-right check".  THE CONTRACT:
 *   1. CENSUS.  The window is 9 wide x 7 high with a replicated border (row and column indices clamped into the image).  The 62
 *      neighbours are visited in row-major order from the top-left, skipping the centre: w = (w << 1) | (neighbour < centre).
 *      The output is (H, W) 64-bit words with bits 62 and 63 zero.
 *   2. MATCHING COST.  C(y, x, d) = popcount(cl[y, x] ^ cr[y, x - d]) for x - d >= 0, otherwise C = 63, one more than any Hamming
 *      distance can be.
 *   3. PATH AGGREGATION.  The directions r = (dy, dx) in this order: (0, +1), (0, -1), (+1, 0), (-1, 0); then, for 8 paths,
 *      (+1, +1), (+1, -1), (-1, +1), (-1, -1).  Where p - r is outside the image, L_r(p, d) = C(p, d).  Otherwise
 *        L_r(p, d) = C(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + P1, L_r(p-r, d+1) + P1, m + P2) - m,   m = min_k L_r(p-r, k).
 *      Terms with d - 1 or d + 1 outside [0, D) are absent.  S = sum_r L_r is an (H, W, D) uint16 volume with d fastest, at most
 *      8 (63 + 192) = 2040.  S is an OUTPUT of the entry point and part of the contract.
 *   4. SELECTION.  d* = argmin_d S(p, d), the lowest d on ties; best = S(p, d*).  Right disparity:
 *      dR(y, xr) = argmin_k S(y, xr + k, k) over k < D, xr + k < W, the lowest k on ties.  The codes are tested in this order and
 *      the first that applies wins:
 *        -1 when x - d* < 0;
 *        -2 when second (100 - uniqueness) < best 100, where second = min S(p, k) over |k - d*| > 1 (no such k: the test passes);
 *        -3 when lr_tol >= 0 and |dR(y, x - d*) - d*| > lr_tol.
 *   5. SUB-PIXEL, in sixteenths.  The offset is 0 when d* is 0 or D - 1, or when den = S- + S+ - 2 best is 0, with S- = S(p, d* - 1)
 *      and S+ = S(p, d* + 1).  Otherwise num = 8 (S- - S+) and offset = floor((2 num + den) / (2 den)), floored toward -inf; it
 *      lies in -8 .. 8.  d16 (H, W) int16 = 16 d* + offset when valid, else the code.
 *   6. DEPTH.  disp = d16 * 0.0625f (exact); depth = fb / disp with fb = fx * baseline, one float32 multiply made on the host, and
 *      one correctly rounded float32 division.  depth = 0 where d16 <= 0 or where the quotient is not in [d_min, d_max]: the
 *      "no depth" of the frame table.
 *
 * Buffers (device, caller-owned): census images int64 (H, W); S uint16 (H, W, D), 32-byte aligned, NOT required to be zeroed --
 * the first direction stores, the others add, one launch per direction on `stream`; workspace: pnr_sgm_workspace_bytes bytes
 * (0 in this build -- nothing is staged --, so it may be NULL; -1 for arguments pnr_sgm_aggregate refuses).  pnr_sgm_select:
 * disp_right (H, W) int16 is an output (dR) and the left-right check's table; it may be NULL only when lr_tol < 0.
 * pnr_disparity_depth: d16 (n) int16, depth (n) float32; fb positive and finite, 0 < d_min <= d_max (d_max may be +inf); n == 0:
 * PNR_OK.  All capture-safe on the one stream.  PNR_EINVAL before any launch: width or height < 1 or more than 2^31 - 1 pixels,
 * max_disp not a multiple of 16 in 16 .. 256, P1 <= 0, P1 > P2, P2 > 192, paths not 4 or 8, uniqueness outside 0 .. 99,
 * lr_tol < -1, a null pointer (but workspace, and disp_right as above), a misaligned S, n < 0, a bad fb or range. */
int pnr_census(const uint8_t* img, int width, int height, int64_t* out, void* stream);
int64_t pnr_sgm_workspace_bytes(int width, int height, int max_disp, int paths);
int pnr_sgm_aggregate(const int64_t* census_l, const int64_t* census_r, int width, int height, int max_disp, int p1, int p2,
                      int paths, uint16_t* S, void* workspace, void* stream);
int pnr_sgm_select(const uint16_t* S, int width, int height, int max_disp, int uniqueness, int lr_tol, int16_t* d16,
                   int16_t* disp_right, void* stream);
int pnr_disparity_depth(const int16_t* d16, int64_t n, float fb, float d_min, float d_max, float* depth, void* stream);

/* ---- mesh extraction (csrc/pnr_mesh.hip; DESIGN.md 8 "Mesh extraction"): a lattice of field values, as Network.query_grid
 * returns it, -> a triangle mesh of the surface field = level, with the lattice point each vertex takes its label from.  The
 * method is marching tetrahedra on the Kuhn split: no ambiguous cases, and neighbouring cubes agree on every face diagonal, so
 * the surface is watertight by construction.  The reference ships no extractor: the rule is this build's and unpinned
 * (tests/_mesh_ref.py restates it twice, bit for bit).  THE CONTRACT:
 *
 *   LATTICE.  field is float32 (res_z, res_y, res_x).  Point (ix, iy, iz) has flat index n = (iz res_y + iy) res_x + ix and the
 *     position lo + (i + 0.5) step per axis in float32: (float) i + 0.5f, one multiply, one add, never an FMA.  lo and step are
 *     query_grid's: float32 lo, and step = (hi32 - lo32) / res32, one subtraction and one division.
 *   INSIDE.  A point is inside iff field > level.  NaN is outside, +Inf inside.
 *   CELLS.  Cube c has the corners c + {0,1}^3 and exists for c_i <= res_i - 2.  It is cut into six tetrahedra, one per
 *     permutation pi of the axes in lexicographic order: xyz, xzy, yxz, yzx, zxy, zyx (tetrahedron 0 .. 5; parities
 *     0 1 1 0 0 1).  Tetrahedron pi has the corners w0 = c, w1 = w0 + e_pi1, w2 = w1 + e_pi2, w3 = c + (1, 1, 1).
 *   VERTICES.  A mesh vertex lies on a lattice edge whose two ends differ in "inside".  Every edge of the split is (a, a + off)
 *     with off a non-zero vector of {0,1}^3: seven kinds, kind = off_x + 2 off_y + 4 off_z - 1, and the edge is OWNED by its
 *     lower end a.  With f_a, f_b the values and p_a, p_b the positions of the owner and the far end:
 *         t = (level - f_a) / (f_b - f_a)       two subtractions, one correctly rounded division
 *         t = 0.5 if t is NaN, else 0 if t < 0, else 1 if t > 1
 *         p = p_a + t (p_b - p_a)               per component: subtract, multiply, add, each rounded
 *     always from the owner, whichever end is inside, so every tetrahedron round the edge gets the same bits.  Vertices are
 *     numbered by (owner's flat index, kind) ascending.  src[v] = the flat index of the edge's INSIDE end.
 *   TRIANGLES.  case = sum over k of (w_k inside) << k.  With I the inside and O the outside corners of a tetrahedron, each
 *     ascending in w order, and (x, y) the vertex on the edge between corners x and y:
 *         one inside corner     (I0,O0) (I0,O1) (I0,O2)
 *         three                 (I0,O0) (I1,O0) (I2,O0)
 *         two                   the quad q0 = (I0,O0), q1 = (I0,O1), q2 = (I1,O1), q3 = (I1,O0) as (q0, q1, q2) and (q0, q2, q3)
 *     A triangle keeps its first vertex; its second and third are swapped where the table says so, so that
 *     (p1 - p0) x (p2 - p0) points from the inside corners towards the outside ones.  swap[case][parity of pi]:
 *         case    0    1    2    3    4    5    6    7    8    9   10   11   12   13   14   15
 *         even    0    0    1    0    0    1    0    0    1    0    1    1    0    0    1    0
 *         odd     0    1    0    1    1    0    1    1    0    1    0    0    1    1    0    0
 *     Triangles are numbered by (the cube's flat index over the lattice, tetrahedron 0 .. 5, triangle 0 .. 1) ascending.
 *     Zero-area triangles (a lattice value equal to level) are kept.  If any res_i < 2 there is no cube and the mesh is empty:
 *     totals = {0, 0}, not an error.
 *   LIMITS.  At most (2^31 - 1) / 12 = 178956970 lattice points, so that every count fits an int32 scan; faces is int32.
 *
 * pnr_mesh_count classifies every point, scans the counts and writes totals[0] = vertices, totals[1] = triangles (DEVICE int64[2],
 * 8-byte aligned) and the workspace pnr_mesh_emit reads: pnr_mesh_workspace_bytes(res) bytes, 16-byte aligned, caller-owned, to
 * be left alone between the two calls (-1 for a lattice the entry points refuse).  pnr_mesh_emit, with the same field, lattice
 * and level, writes vertices (V, 3) float32, faces (T, 3) int32 and src (V) int64, V and T being the totals: the caller reads
 * them between the two calls, which is the one synchronisation of an extraction and the caller's.  lo_host, step_host: three HOST
 * floats each, copied into the launch.  src may be NULL; vertices and faces may be NULL only when their total is 0 (a NULL output
 * is never written, and src is written only with vertices).  Neither entry point synchronises or allocates; both are
 * capture-safe, no kernel waits on another workgroup and nothing is atomic: two calls give the same bits.
 * PNR_EINVAL before any launch, from both: a res < 1; a lattice over the limit; a non-finite level; a null field or workspace;
 * a misaligned field (4 bytes) or workspace (16).  pnr_mesh_count also: a null or misaligned (8) totals.  pnr_mesh_emit also: a
 * null lo_host or step_host, a non-finite lo or step, a misaligned vertices, faces (4) or src (8). */
int64_t pnr_mesh_workspace_bytes(int res_x, int res_y, int res_z);
int pnr_mesh_count(const float* field, int res_x, int res_y, int res_z, float level, void* workspace, int64_t* totals, void* stream);
int pnr_mesh_emit(const float* field, int res_x, int res_y, int res_z, float level, const float* lo_host, const float* step_host,
                  const void* workspace, float* vertices, int32_t* faces, int64_t* src, void* stream);

/* ---- nearest neighbours (csrc/pnr_nn.hip; DESIGN.md 8 "Nearest neighbours and geometry metrics"): an exact fixed-radius
 * nearest-neighbour search between two clouds, the reconstruction metrics accumulated from its answers (accuracy, completeness,
 * Chamfer distance, precision / recall / F-score), and surface points of a triangle mesh at a given density.  The reference ships
 * none of this: the rules are this build's and unpinned (tests/_nn_ref.py restates them in numpy, bit for bit).  Float32
 * throughout unless stated, every operation a single + - * / sqrt in the order given, never an FMA; denormals are not flushed.
 *
 * NEAREST NEIGHBOUR.  ref (n, 3) and query (m, 3) float32, a radius D = max_dist with 0 < D < inf.  r2 = D * D.  THE CONTRACT:
 *   1. the squared distance of a query q to ref[j]: dx = qx - rx, dy = qy - ry, dz = qz - rz, d2 = (dx*dx + dy*dy) + dz*dz.
 *   2. ref[j] is a CANDIDATE iff its three coordinates are finite and d2 <= r2.
 *   3. the answer is the candidate with the smallest key = ((uint64) bits(d2) << 32) | (uint32) j: the nearest candidate, a
 *      distance tie going to the lowest index.  It is the key of point splatting.
 *   4. index[i] = that j, or -1 where there is no candidate; dist2[i] = that d2, or +inf.  A query with a non-finite coordinate
 *      gets -1 and +inf and is counted apart.
 *   5. stats[0..2] += the number of queries that found a neighbour / had none in the radius / were invalid (device int64,
 *      integer atomics: a block-wide count, then one atomic per block and counter).  stats may be NULL.
 * The result equals brute force over all n, whatever the acceleration structure.  THE STRUCTURE is a spatial hash, so there are
 * no bounds to compute and nothing to read back:
 *   Dp = D * PNR_NN_PAD (1.0009765625f), h = 2 * Dp, inv = 1 / h: three float32 operations on the host.
 *   The origin o is ref[0], read ON THE DEVICE by every thread (a captured build follows the data); (0, 0, 0) if ref[0] is not
 *     finite or n == 0.
 *   The cell of p per axis: c = clamp(floorf((p - o) * inv), -2^20, 2^20), clamped AS A FLOAT and then converted to int
 *     (PNR_NN_CELL_CLAMP).
 *   bucket = ((cx * PNR_NN_HASH_X) ^ (cy * PNR_NN_HASH_Y) ^ (cz * PNR_NN_HASH_Z)) & (T - 1) in 32-bit unsigned arithmetic;
 *     T = table_size is a power of two in 2 .. PNR_NN_MAX_TABLE chosen by the caller (the Python layer: max(1024, the power
 *     of two at or above 2 n), at most PNR_NN_MAX_TABLE).
 *   A query visits the buckets of every cell of the box [c(q - Dp), c(q + Dp)] per axis and tests every record in them by
 *     steps 1 .. 3.  Collisions and a bucket visited twice are harmless under a minimum.
 *   WHY THIS EQUALS BRUTE FORCE.  A candidate has real |qx - rx| <= D (1 + 2^-21) < Dp.  For floats, r >= x implies r >= fl(x),
 *     so rx lies in [fl(qx - Dp), fl(qx + Dp)].  The subtraction of o, the multiplication by a positive inv, floorf and the clamp
 *     are all monotone non-decreasing, so c(q - Dp) <= c(r) <= c(q + Dp) at any coordinate magnitude.  Far from the origin the
 *     cells only get coarser, or collapse into the clamp cell: that costs time and never a neighbour.
 *   HOW LARGE THE BOX IS.  In real arithmetic the two corners are exactly one cell apart (h = 2 Dp): 2 cells per axis, 8 buckets.
 *     The rounding of q -+ Dp moves them apart by up to ulp(q) / (2 Dp) cells more, and the multiplication by up to 2^-23 of the
 *     cell coordinate, so a box can reach 3 cells on an axis where ulp(q) comes near Dp or the coordinate near the clamp, 4 where
 *     both happen; once ulp(q) > 2 Dp both corners round to q and the box is one cell.  The kernel loops over whatever the two
 *     corners give.  Both h and 1 / h must be finite: with a denormal D below about 1.47e-39, 1 / h would be +inf and the corners
 *     of a query next to the origin the two clamp cells, 2^21 cells apart -- such a D is refused.
 * pnr_nn_build, three launches and a scan on the one stream behind a launch that zeroes the counts (a kernel, not a memset: a
 * captured build is a plain chain of kernel nodes), no kernel waiting on another workgroup: (1) every finite reference
 * point adds 1 to its bucket's count with an int32 atomic (non-finite points are skipped and never appear in the table);
 * (2) an exclusive int32 scan of the counts into start[0 .. T] (block sums, one block over the sums, add back:
 * csrc/pnr_scan_dev.h); (3) a returning int32 atomic on the bucket's cursor places the point's 16-byte record
 * (x, y, z, bits = j) into records (n, 4) float32, in bucket order -- a candidate is then ONE 16-byte load.  The order of the
 * records inside a bucket depends on arrival and is NOT part of the rule; the outputs of a query do not depend on it.
 * n == 0 zero-fills start (a NULL start is then left alone).  start: device int32 (T + 1); records: device (n, 4) float32,
 * 16-byte aligned; workspace: pnr_nn_workspace_bytes(n, T) bytes, 8-byte aligned, free again when the build has run (-1 for
 * arguments the build refuses).  pnr_nn_query takes the SAME ref, n, max_dist and table_size and the start and records the
 * build filled; it clamps every start pair into [0, n] before looping, so a damaged table can give wrong answers but never an
 * out-of-range read.  One thread per query, no host synchronisation in either: both are capture-safe on the one stream.
 * PNR_EINVAL before any launch, from both: n (or m) outside 0 .. 2^31 - 1; max_dist not positive and finite, so large that
 * 2 Dp overflows, or so small that 1 / (2 Dp) does; table_size not a power of two in 2 .. 2^28; a null or misaligned pointer (4 bytes; records 16; workspace and
 * stats 8).  pnr_nn_build with n == 0 and pnr_nn_query with m == 0: PNR_OK before the pointer checks.
 *
 * CLOUD METRICS.  pnr_cloud_metrics: index, dist2 (m) as a query wrote them, D = max_dist as above, and n_tau <= PNR_CLOUD_MAX_TAU
 * (8) thresholds tau_k with 0 < tau_k <= D (HOST floats, copied into the launch).  Query i COUNTS iff dist2[i] is not NaN and --
 * the choice this build makes of the two possible -- query (m, 3), the coordinates that were asked, is NULL or holds three finite
 * coordinates at row i: pass the queries and the invalid ones (written as -1 / +inf) are left out; pass NULL and every row counts.
 * A counted query is FOUND iff index[i] >= 0.  In double: d = sqrt((double) dist2[i]) if found, else (double) D.
 *   sums[0] += d, sums[1] += d * d                                            (device double[2])
 *   counts[0] += 1, counts[1] += !found, counts[2 + k] += found and dist2[i] <= tau_k * tau_k (one float32 multiply) for k < n_tau
 *                                                                             (device int64[2 + PNR_CLOUD_MAX_TAU], integer atomics, exact)
 * The sums take the fixed order of pnr_depth_metrics: per-thread stride, the wave's butterfly, waves in order, a per-block partial
 * in workspace, and a one-block second launch that adds the partials in block order and the total once into sums.  No floating
 * atomics: two calls on the same input and the same box give the same bits.  Both arrays accumulate over calls (the caller
 * zeroes them once).  workspace: pnr_cloud_metrics_workspace_bytes(m) bytes, 8-byte aligned (-1 for m outside 0 .. 2^31 - 1).
 * PNR_EINVAL before any launch: a bad m or max_dist; n_tau outside 0 .. 8; a null tau_host with n_tau > 0; a tau_k that is not in
 * (0, D]; a null index / dist2 / sums / counts / workspace; a misaligned pointer (4 bytes; sums, counts and workspace 8).
 * m == 0: PNR_OK after the checks of the values.
 *
 * MESH SAMPLING.  vertices (V, 3) float32, faces (F, 3) int32, a density rho (points per unit area; finite, >= 0) and a 64-bit
 * seed = (seed_lo, seed_hi), the Philox key.  With Philox(c) = pnr_philox4x32_10 of the counter c under that key and U(w) =
 * (w >> 8) * 2^-24 (pnr_uniform of "in-kernel RNG").  Per triangle t with corners p0, p1, p2:
 *   e1 = p1 - p0, e2 = p2 - p0; n = e1 x e2, each component (a*b) - (c*d) with both products rounded;
 *   s = (nx*nx + ny*ny) + nz*nz; area = 0.5f * sqrtf(s), correctly rounded.
 *   u_t = U(word x of Philox({t, 0, 0, 0}));  k_t = min((int) floorf((area * rho) + u_t), PNR_SAMPLE_MAX_PER_FACE): the expected
 *   count is area * rho, so small triangles are not biased away.  k_t = 0 if area is not finite or a face index is outside 0 .. V - 1.
 *   Point j < k_t of triangle t draws (x, y, ., .) = Philox({t, 1 + j, 0, 0}): u = U(x), v = U(y); if u + v > 1 both are
 *   replaced by 1 - u and 1 - v; p = (p0 + u*e1) + v*e2 per component, each operation rounded.
 * The points come in triangle order, then j order: nothing is atomic, so the output is the same on every call.
 * pnr_mesh_sample_count writes k_t, scans it in place into start (F + 1) device int32 (the shared scan), and writes the 64-bit
 * total into total (device int64, 8-byte aligned).  The caller reads total -- the one synchronisation of a sampling, and the
 * caller's -- refuses a total above 2^31 - 1 (the int32 scan has then wrapped), allocates, and calls pnr_mesh_sample_emit with
 * the same mesh and seed, start and n_points = total: points (n_points, 3) float32 and face (n_points) int32, the triangle of
 * each point.  workspace: pnr_mesh_sample_workspace_bytes(F) bytes, 4-byte aligned.  Neither entry point synchronises or
 * allocates.  PNR_EINVAL before any launch: V outside 0 .. 2^31 - 1 or F outside 0 .. 2^31 - 2; rho negative, NaN or infinite;
 * a null or misaligned pointer; n_points outside 0 .. 2^31 - 1, or positive with F == 0.  F == 0: start[0] = 0 and total = 0
 * (a NULL one is left alone).  n_points == 0: PNR_OK, no launch. */
#define PNR_NN_PAD 1.0009765625f            /* Dp = D * (1 + 2^-10) */
#define PNR_NN_CELL_CLAMP 1048576.0f        /* 2^20 */
#define PNR_NN_HASH_X 73856093u
#define PNR_NN_HASH_Y 19349663u
#define PNR_NN_HASH_Z 83492791u
#define PNR_NN_MAX_TABLE 268435456          /* 2^28 buckets */
#define PNR_CLOUD_MAX_TAU 8
#define PNR_SAMPLE_MAX_PER_FACE 65535
int64_t pnr_nn_workspace_bytes(int64_t n, int64_t table_size);
int pnr_nn_build(const float* ref, int64_t n, float max_dist, int64_t table_size, int32_t* start, float* records, void* workspace,
                 void* stream);
int pnr_nn_query(const float* ref, int64_t n, float max_dist, int64_t table_size, const int32_t* start, const float* records,
                 const float* query, int64_t m, int32_t* index, float* dist2, int64_t* stats, void* stream);
int64_t pnr_cloud_metrics_workspace_bytes(int64_t m);
int pnr_cloud_metrics(const int32_t* index, const float* dist2, const float* query, int64_t m, float max_dist,
                      const float* tau_host, int n_tau, double* sums, int64_t* counts, void* workspace, void* stream);
int64_t pnr_mesh_sample_workspace_bytes(int64_t n_faces);
int pnr_mesh_sample_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, float rho, int64_t seed,
                          int32_t* start, int64_t* total, void* workspace, void* stream);
int pnr_mesh_sample_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t seed,
                         const int32_t* start, int64_t n_points, float* points, int32_t* face, void* stream);

/* ---- 8f-4: label-map post-processing and evaluator counters (what follows the path in the reference's evaluate loop;
 * its evaluator is not in the mount, conventions are this build's -- DESIGN.md 8).
 * pnr_panoptic_labels: sem_label = argmax_c sem (lowest index on ties); inst_label = argmax_k inst where is_thing[sem_label]
 *   != 0 (is_thing NULL: every class), else -1; panoptic = class*1000 + instance on things, class on stuff.  Any output
 *   may be NULL.  sem (R,n_sem), inst (R,n_inst) or NULL, is_thing (n_sem) int32 device or NULL.
 * pnr_confusion: conf[gt*n_classes + pred] += 1 over pixels with both labels in [0, n_classes) (gt < 0 = ignore); conf is a
 *   device (n_classes^2) int64 array the caller zeroes once and accumulates into over frames.  Integer atomics: exact.
 *   n_classes <= 8192 (above 128 without the per-block LDS histogram: used for the segment-pair counts of PQ).
 *   mIoU / accuracy are a handful of flops on that matrix (host side); PSNR = -10 log10 of pnr_losses' rgb term. */
int pnr_panoptic_labels(const float* sem, const float* inst, const int32_t* is_thing, int64_t n_rays, int n_sem, int n_inst,
                        int32_t* sem_label, int32_t* inst_label, int32_t* panoptic, void* stream);
int pnr_confusion(const int32_t* pred, const int32_t* gt, int64_t n, int n_classes, int64_t* conf, void* stream);

/* ---- a7: sample_pdf + merge.  z (R,Nc), weights (R,Nc) coarse; u (R,Nf) or NULL (det).
 * z_samples (R,Nf) and inds (R,Nf) int32 may be NULL; z_fine (R,Nc+Nf) sorted union or NULL.
 * Indices / z_samples bit-exact with pnro_sample_pdf.  Nc <= 256, Nc+Nf <= 512. */
int pnr_sample_pdf(const float* z, const float* weights, const float* u, int64_t n_rays, int n_coarse,
                   int n_fine, float* z_samples, int32_t* inds, float* z_fine, void* stream);

/* ---- a8: bbox prior.  box (M,15) = centre(3) rotation rows(9) half extents(3).
 * Per ray the max_hits NEAREST intersected boxes (smallest t_in; ties: lower box index), stored in ascending
 * (t_in, box index) order: hit_t (R,max_hits,2), hit_box (R,max_hits) int32 (-1 pad).  hit_count (R) int32 is the
 * TRUE number of intersected boxes: a value > max_hits reports that the farthest ones were dropped (grow max_hits);
 * pnr_sample_labels uses min(hit_count, max_hits) entries.  Bit-exact with pnro_bbox_hits.
 *
 * The rule per ray (o, d, near, far) and box (float32, no contraction of mul + add, one correctly rounded reciprocal):
 *     p = o - c;  tmin = near;  tmax = far
 *     for each box axis a (rotation row r):  ol = (r0*p0 + r1*p1) + r2*p2;  dl = (r0*d0 + r1*d1) + r2*d2;  inv = 1 / dl
 *         t1 = (-e_a - ol) * inv;  t2 = (e_a - ol) * inv;  tmin = max(tmin, min(t1, t2));  tmax = min(tmax, max(t1, t2))
 *     hit  <=>  tmin <= tmax
 * a8: min / max.  Here and in the hull of pnr_restrict_rays, min / max are fminf / fmaxf with both open cases fixed: a NaN
 * operand loses (the other one is returned), and -0.0 orders BELOW +0.0: min(-0, +0) = min(+0, -0) = -0, max = +0 (what
 * v_min_f32 / v_max_f32 return; C leaves it open, so the oracle spells it out in pnro_fminf / pnro_fmaxf).  It decides the sign
 * of a zero t_in -- a zero-extent box through the origin, near = 0 -- and with it the sign of z[0] under the hull switch.
 * So along a box axis (dl = +-0) a ray inside the slab keeps its interval (t = -+inf), outside it misses, and exactly on a
 * face it misses too (0 * inf = NaN loses against the other face's infinity); d = 0 hits the boxes that strictly contain o. */
int pnr_bbox_hits(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits,
                  float* hit_t, int32_t* hit_box, int32_t* hit_count, void* stream);

/* ---- a8b: convex bounding primitives.  The scene's primitives as convex polytopes in half-space form -- cuboids, the prisms
 * of an ear-clipped extruded polygon, any closed convex mesh (panopticnerf_amd/primitives.py builds the table):
 *   planes  (P,4) float32, one (n0, n1, n2, dd) per plane, 16-byte aligned; the inside of a plane is n.x <= dd;
 *   offsets (M+1) int32, CSR: primitive m owns planes offsets[m] .. offsets[m+1]-1.  Non-decreasing, offsets[M] <= P (the
 *           caller's contract: the kernel reads what offsets names and checks nothing).
 * Ids stay the (M,2) int32 table of pnr_sample_labels; the pieces of one decomposed object repeat its ids.
 *
 * The rule per ray (o, d, near, far) and primitive, THE CONTRACT (float32, no contraction of mul + add, one correctly rounded
 * division; fminf / fmaxf return the other operand when one is NaN):
 *
 *     tmin = near; tmax = far
 *     for each plane of the primitive, in table order:
 *         dn = (n0*d0 + n1*d1) + n2*d2
 *         on = (n0*o0 + n1*o1) + n2*o2
 *         s  = dd - on
 *         if dn > 0:  tmax = fminf(tmax, s / dn)        leaving
 *         if dn < 0:  tmin = fmaxf(tmin, s / dn)        entering
 *         if dn == 0 and s < 0:  tmax = -inf            parallel and outside (-0.0 counts as 0)
 *     hit  <=>  tmin <= tmax                            (pnr_bbox_hits' comparator: a grazing ray, tmin == tmax, hits)
 *
 * So a primitive without planes is the whole ray [near, far]; a ray with d = 0 (an invalid fisheye pixel) hits exactly the
 * primitives whose every plane has s >= 0 (those that contain its origin), with [near, far]; and the result does not depend on
 * the early exit the kernel takes once a whole wave has missed a primitive.
 *
 * The kept list is pnr_bbox_hits': the max_hits NEAREST intervals in ascending (t_in, primitive index) order in hit_t
 * (R,max_hits,2) / hit_box (R,max_hits) (pads 0.0f / -1), hit_count (R) the TRUE number of primitives hit.  Abutting intervals
 * of one object's pieces are NOT merged.  max_hits >= 1 (lists of up to 8 entries are built in LDS, longer ones in the output
 * rows).  n_rays == 0 and n_prim == 0 are valid (n_prim == 0: every list empty, every count 0; planes / offsets may be NULL).
 * Never synchronises, never allocates: capture-safe.  The arithmetic differs from pnr_bbox_hits' slab test (which multiplies
 * by a reciprocal in the box frame): the two agree on a cuboid to rounding, not bit for bit. */
int pnr_convex_hits(const float* rays, int64_t n_rays, const float* planes, const int32_t* offsets, int n_prim, int max_hits,
                    float* hit_t, int32_t* hit_box, int32_t* hit_count, void* stream);

/* Sampling restricted to the bbox prior (cfg.bbox_sampling = "hull"; SURVEY.md 9 item 2 -- whether the reference samples
 * [near, far] or the hit intervals cannot be checked here, so it is a switch): rays_out = rays with near / far replaced by the
 * hull [min t_in, max t_out] of the ray's kept intervals (min(hit_count, max_hits) entries of hit_t); rays without a hit are
 * copied unchanged.  rays_out may not alias rays.  Bit-exact with pnro_restrict_rays. */
int pnr_restrict_rays(const float* rays, int64_t n_rays, const float* hit_t, const int32_t* hit_count, int max_hits,
                      float* rays_out, void* stream);

/* box_ids (M,2) int32 = (semantic id, instance id).  label_* (R,N) int32. */
int pnr_sample_labels(const float* z, int64_t n_rays, int n_samples, const float* hit_t,
                      const int32_t* hit_box, const int32_t* hit_count, int max_hits,
                      const int32_t* box_ids, int32_t* label_sem, int32_t* label_inst, void* stream);

/* a8 + a3 (+ a8) in one launch -- the coarse level's per-ray preamble: hit lists exactly as pnr_bbox_hits writes them, z_out (R,N)
 * exactly as pnr_stratified (over the hull of each ray's kept intervals with hull != 0, as pnr_restrict_rays + pnr_stratified),
 * and, when label_sem / label_inst are given, the labels pnr_sample_labels would produce for z_out.  max_hits in [1, 8]
 * (larger lists: the separate entry points).  Replaces, with pnr_sample_pdf_labels, four of the reference render_rays' per-chunk
 * steps by one launch each. */
int pnr_ray_setup(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits, const int32_t* box_ids,
                  int n_samples, int lindisp, const float* t_rand, int hull, float* hit_t, int32_t* hit_box,
                  int32_t* hit_count, float* z_out, int32_t* label_sem, int32_t* label_inst, void* stream);

/* a7 + a8 in one launch: z_fine (R, n_coarse + n_fine) exactly as pnr_sample_pdf, and label_sem / label_inst (same shape)
 * exactly as pnr_sample_labels(z_fine, ...) -- the wave that merged a ray's samples labels them. */
int pnr_sample_pdf_labels(const float* z, const float* weights, const float* u, int64_t n_rays, int n_coarse, int n_fine,
                          float* z_fine, const float* hit_t, const int32_t* hit_box, const int32_t* hit_count,
                          int max_hits, const int32_t* box_ids, int32_t* label_sem, int32_t* label_inst, void* stream);

/* ---- in-kernel RNG ("an in-kernel RNG is a separate fast path").  The _rng twins below draw the uniforms /
 * the sigma noise that their plain entry points take as tensors INSIDE the kernel, from one counter-based stream contract:
 *
 *   generator  Philox4x32-10 (Random123; panopticnerf_amd/csrc/pnr_philox.h): no per-thread state, any draw recomputable anywhere.
 *   call       {seed, offset}: two int64 in DEVICE memory, read by the kernels when they RUN (not at launch), so a captured
 *              graph draws fresh numbers on every replay.  pnr_rng_begin writes it from a caller-owned state.
 *   key        (lo32(seed), hi32(seed)).
 *   counter    sample j of global ray g = ray_base + r (r: the ray's row in the launch), stream tag t:
 *              (j >> 2 | t << 24, (uint32) g, lo32(offset), hi32(offset));  the draw is word j & 3 of the output block.
 *   tags       1 = stratified jitter (t_rand), 2 = sample_pdf uniforms (u), 3 + level = sigma noise of that level (the
 *              renderer's convention; any tag in 1..255 is accepted), 16 = pixel and 17 = frame draws of pnr_sample_batch
 *              (integers, not uniforms: "training frames" below).
 *   uniform    (w >> 8) * 2^-24, in [0, 1) like torch.rand.
 *   normal     Box-Muller on the word pairs (2k, 2k + 1) of a block: u1 = ((w_2k >> 8) + 1) 2^-24, u2 = (w_2k+1 >> 8) 2^-24,
 *              r = sqrt(-2 log u1), n_2k = r cos(2 pi u2), n_2k+1 = r sin(2 pi u2);  noise = scale * n.  One Philox call gives
 *              the four consecutive samples a compositing lane holds.
 *
 * The draws of a ray depend on (seed, offset, tag, g, j) only: not on the launch, its grid or how a batch is cut into chunks.
 * Every _rng entry point refuses (PNR_EINVAL, before any device work) a NULL descriptor or call, a tag outside 1..255, a
 * scale < 0 (or NaN), ray_base < 0 and ray_base + n_rays > 2^32. */
typedef struct pnr_rng {
    const int64_t* call;   /* DEVICE {seed, offset} (pnr_rng_begin) */
    int64_t ray_base;      /* global index of the launch's ray 0 */
    int32_t tag;           /* stream tag, 1..255 */
    float scale;           /* normal draws: noise = scale * n (uniform draws ignore it) */
} pnr_rng;

/* One thread: call[0..1] = state[0..1], then state[1] += 1.  state and call are caller-owned DEVICE int64[2]; the library keeps
 * no state.  One begin per render() call: every chunk and level of the call shares its `call`. */
int pnr_rng_begin(int64_t* state, int64_t* call, void* stream);
/* out (n_rays, n_samples) = the stream's draws: uniforms (normal == 0) or scale * normals (normal != 0).  The link between the
 * explicit-tensor entry points and the _rng twins, and the op for callers that want the tensors. */
int pnr_rng_fill(const pnr_rng* rng_host, int64_t n_rays, int n_samples, int normal, float* out, void* stream);
/* pnr_stratified with t_rand (R,N) = the stream's uniforms. */
int pnr_stratified_rng(const float* rays, int64_t n_rays, int n_samples, int lindisp, const pnr_rng* rng_host, float* z_out,
                       void* stream);
/* pnr_ray_setup with t_rand (R,N) = the stream's uniforms. */
int pnr_ray_setup_rng(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits, const int32_t* box_ids,
                      int n_samples, int lindisp, const pnr_rng* rng_host, int hull, float* hit_t, int32_t* hit_box,
                      int32_t* hit_count, float* z_out, int32_t* label_sem, int32_t* label_inst, void* stream);
/* pnr_sample_pdf / pnr_sample_pdf_labels with u (R, n_fine) = the stream's uniforms. */
int pnr_sample_pdf_rng(const float* z, const float* weights, const pnr_rng* rng_host, int64_t n_rays, int n_coarse, int n_fine,
                       float* z_samples, int32_t* inds, float* z_fine, void* stream);
int pnr_sample_pdf_labels_rng(const float* z, const float* weights, const pnr_rng* rng_host, int64_t n_rays, int n_coarse,
                              int n_fine, float* z_fine, const float* hit_t, const int32_t* hit_box, const int32_t* hit_count,
                              int max_hits, const int32_t* box_ids, int32_t* label_sem, int32_t* label_inst, void* stream);
/* pnr_composite with noise (R,N) = rng->scale * the stream's normals. */
int pnr_composite_rng(const float* raw, int64_t raw_stride_s, int64_t raw_stride_c, const float* z, const float* rays,
                      const pnr_rng* noise_host, const int32_t* label_sem, const int32_t* label_inst, int64_t n_rays, int n_samples,
                      int n_sem, int n_inst, int sem_mode, int white_bkgd, float* rgb, float* depth, float* acc, float* weights,
                      float* sem, float* inst, float* fix_sem, float* fix_inst, void* stream);
/* pnr_composite_backward3 with the same noise REGENERATED from the descriptor (no noise tensor is saved). */
int pnr_composite_backward_rng(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                               const pnr_rng* noise_host, int64_t n_rays, int n_samples, int n_sem, int n_inst, int sem_mode,
                               const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                               const float* g_inst, const float* g_weights, const int32_t* label_sem,
                               const int32_t* label_inst, const float* g_fix_sem, const float* g_fix_inst,
                               const float* ce_sem, const float* ce_inst, float* d_raw, void* stream);

/* ---- training frames: a device-resident set of posed images and the kernel that draws a ray batch from it (csrc/pnr_batch.hip;
 * DESIGN.md "Training frames").  One launch picks n_rays (frame, pixel) pairs, builds their rays and gathers their targets.
 * The frame table is read from DEVICE memory when the kernel RUNS, like the rng call: a captured graph's replays each draw a
 * fresh batch, and a table edited after the capture is what later replays see.
 *
 * pnr_frame: one frame, 144 bytes (a multiple of 16; the array is 16-byte aligned), fields in this order:
 *   offset   0  int32  model       PNR_CAMERA_PINHOLE | PNR_CAMERA_FISHEYE | PNR_CAMERA_EQUIRECT
 *            4  int32  width, height
 *           12  float  cam[7]      pinhole: fx, fy, cx, cy (the rest unused); fisheye: cam7 of pnr_gen_rays_fisheye; equirect:
 *                                  lon0, dlon, lat0, dlat (the rest unused; valid_pix = 0, every pixel drawable)
 *           40  float  c2w[12]     3x4 row-major camera-to-world
 *           88  float  near_, far_
 *           96  int64  n_valid     number of drawable pixels (0: the frame is never drawn)
 *          104  uint64 valid_pix   device address of n_valid int32 linear pixel indices j*width + i; 0 = every pixel (n_valid =
 *                                  width*height)
 *          112  uint64 rgb         device address of uint8 (height, width, 3); required
 *          120  uint64 depth       device address of float (height, width); 0 = none
 *          128  uint64 sem         device address of int16 (height, width) semantic labels; 0 = none
 *          136  uint64 inst        device address of int16 (height, width) instance labels; 0 = none
 * Beside the records: cum, int64[capacity + 1], cum[0] = 0 and cum[f + 1] = cum[f] + n_valid of frame f, and n_frames, one int32 = F.
 *
 * Draw rule (integer arithmetic only; the stream contract is the in-kernel RNG's, below).  Stream tags: PNR_TAG_PIXEL = 16 and
 * PNR_TAG_FRAME = 17; rng_host->tag must be PNR_TAG_PIXEL.  For the launch's ray r, global ray
 * g = ray_base + r:
 *   (w0, w1, ., .) = the Philox block of (j = 0, tag 16, g);  W = w0 * 2^32 + w1;  mulhi64(a, b) = floor(a * b / 2^64)
 *   mode 0 (pooled):  n = cum[F];  idx = mulhi64(W, n);  the frame is the f with cum[f] <= idx < cum[f + 1] (binary search; a frame
 *                     with n_valid = 0 is never chosen);  k = idx - cum[f]
 *   mode 1 (one frame per call):  (v0, v1, ., .) = the block of (j = 0, tag 17, g = 0) -- global ray 0 whatever ray_base is, so
 *                     every rank of a step draws the same frame;  f = mulhi64(v0 * 2^32 + v1, F);  k = mulhi64(W, n_valid[f])
 *   pixel p = valid_pix[k], or k where valid_pix is 0.
 * Draws are WITH REPLACEMENT: two rays of a batch may be the same pixel (at 4096 rays from 10^7 pixels about one pair per batch).
 * A ray's draw depends on (seed, offset, g) and the table only: the batches of ranks 0 .. w-1 (ray_base = rank * n_rays)
 * concatenated are the w * n_rays batch of one rank, bit for bit.
 *
 * Outputs per ray (any may be NULL = not wanted):
 *   rays (n_rays, 8), 16-byte aligned: bit for bit what pnr_gen_rays / pnr_gen_rays_fisheye / pnr_gen_rays_equirect write for
 *   that frame and pixel
 *   rgb (n_rays, 3) = (float) byte / 255.0f (a division);  depth (n_rays) as stored, 0 where the frame has no depth image (what
 *   pnr_losses reads as "no depth");  sem, inst (n_rays) int32, -1 where the frame has none;  frame_out, pix_out (n_rays) int32.
 * What the host cannot see: F == 0, cum[F] == 0 or (mode 1) n_valid[f] == 0.  The kernel then writes rays = 0, rgb = depth = 0,
 * labels = -1 and frame_out = pix_out = -1 for every ray; nothing is divided and no null address is read.
 * Refused (PNR_EINVAL, before any launch): a null or misaligned table (frames 16, cum 8, n_frames 4 bytes), a mode outside 0 / 1,
 * what every _rng entry point refuses, a tag clash -- any tag but PNR_TAG_PIXEL (1 .. 15 belong to the render streams, which may
 * share the call; 17 is the frame stream) --, misaligned rays.  n_rays = 0 returns PNR_OK at once. */
typedef struct pnr_frame {
    int32_t model, width, height;
    float cam[7];
    float c2w[12];
    float near_, far_;
    int64_t n_valid;
    uint64_t valid_pix, rgb, depth, sem, inst;
} pnr_frame;
#define PNR_TAG_PIXEL 16
#define PNR_TAG_FRAME 17
#define PNR_SAMPLE_POOLED 0
#define PNR_SAMPLE_FRAME 1
int pnr_sample_batch(const pnr_frame* frames, const int64_t* cum, const int32_t* n_frames, int mode, const pnr_rng* rng_host,
                     int64_t n_rays, float* rays, float* rgb, float* depth, int32_t* sem, int32_t* inst, int32_t* frame_out,
                     int32_t* pix_out, void* stream);

/* ---- depth fusion (csrc/pnr_fusion.hip; DESIGN.md 8 "Depth fusion"): posed depth frames of a pnr_frame table -> a truncated
 * signed distance volume (TSDF) on the lattice of query_grid and mesh extraction, with an optional mean colour and an optional
 * majority label per lattice point: the step between the depth producers (stereo, render_view, splatting) and pnr_mesh_*.  The
 * reference ships no fusion: the rule is this build's and unpinned.  Float32 throughout except the integer label vote, every
 * operation a single + - * / in the order given (tests/_tsdf_ref.py restates the rule three times, twice bit for bit).
 *
 * LATTICE.  Point (ix, iy, iz) has flat index n = (iz res_y + iy) res_x + ix and the position X_k = lo_k + ((float)i_k + 0.5f)
 *   step_k: one multiply, one add, never an FMA -- the positions of mesh extraction.  lo_host, step_host: three HOST floats each.
 * VOLUME.  Caller-owned device arrays indexed by n, which ACCUMULATE over calls; the caller initialises them once:
 *     tsdf        float32        0      the running mean of phi
 *     weight      float32        0      the number of observations, capped at w_max
 *     rgb         float32 (., 3) 0      optional: the running mean of the colour BYTES, 0 .. 255
 *     rgb_weight  float32        0      optional, with rgb
 *     label       int32         -1      optional: the packed majority key (sem << 16 | (uint16) inst), -1 = nothing voted
 *     conf        int32          0      optional, with label: the vote's counter
 * THE CONTRACT.  For every lattice point, the frames f = f0 .. f1 - 1 of the table are taken IN ORDER; w2c (F, 12) float32 on the
 * device holds row f = the 3x4 row-major world-to-camera of frame f (camera.invert_pose of its c2w).  Per frame:
 *   1. the frame is skipped if its depth address is 0.
 *   2. (u, v), |p_cam|, p_cam.z and the domain flag of X in the frame's camera with w2c row f: the arithmetic of
 *      pnr_project_points (umax = (float)width - 0.5f).  Skipped unless in the domain and -0.5 <= u < width - 0.5,
 *      -0.5 <= v < height - 0.5.
 *   3. nearest pixel as reprojection step 5: iu = min((int)floor(u + 0.5), width - 1), iv likewise, q = iv width + iu.
 *   4. d = depth[q].  Skipped unless d > 0, d is finite and d <= max_depth (max_depth may be +inf).
 *   5. e = the depth in the view's convention: p_cam.z for a pinhole, |p_cam| for a fisheye or equirect frame.  s = e - d.
 *      Skipped if s > trunc: the point is hidden behind the observed surface.
 *   6. phi = s < -trunc ? -1.0f : s / trunc.  POSITIVE MEANS BEHIND THE OBSERVED SURFACE -- the opposite of the usual sign,
 *      because mesh extraction calls field > level inside.
 *   7. tsdf = (tsdf * weight + phi) / (weight + 1.0f);  weight = min(weight + 1.0f, w_max).  w_max >= 1, +inf allowed.
 *   8. if s >= -trunc and rgb is given (and the frame's rgb address is not 0): with cw = rgb_weight,
 *      c_k = (c_k * cw + (float)byte_k) / (cw + 1.0f) for the three channels of rgb[q], then rgb_weight = min(cw + 1.0f, w_max).
 *   9. if s >= -trunc, label is given, the frame has sem and ls = sem[q] >= 0:  key = (ls << 16) | (uint16)(inst ? inst[q] : -1),
 *      and one step of Boyer-Moore majority voting in integers: label == key: conf = min(conf + 1, 2^30); else conf == 0:
 *      label = key, conf = 1; else conf -= 1.
 * The table and the pose rows are read from DEVICE memory when the kernel runs, as for pnr_sample_batch: a record edited after a
 * capture is what later replays see.  A point's result depends on the frames and their order only, so one call over [f0, f1)
 * equals the calls over [f0, k) and [k, f1), bit for bit.  No atomics: two runs give the same bits.  Never synchronises;
 * capture-safe.  PNR_EINVAL before any launch: null frames, w2c, tsdf or weight; rgb without rgb_weight or the reverse, label
 * without conf or the reverse; a misaligned table (frames, w2c: 16 bytes) or volume array (4); f0 < 0 or f1 < f0; a res < 1 or
 * more than 2^31 - 1 points; null, non-finite lo or step, or a zero step; !(trunc > 0) or a non-finite trunc; !(max_depth > 0);
 * !(w_max >= 1).  f0 == f1 returns PNR_OK at once.  The entry point cannot see the table's length: f1 <= F is the caller's. */
#define PNR_TSDF_BLOCK 256              /* threads (= lattice points) a workgroup */
#define PNR_TSDF_BLOCKS_PER_CU 8        /* the grid's cap per compute unit; the rest is walked grid-stride */
int pnr_tsdf_integrate(const pnr_frame* frames, const float* w2c, int f0, int f1, int res_x, int res_y, int res_z,
                       const float* lo_host, const float* step_host, float trunc, float max_depth, float w_max,
                       float* tsdf, float* weight, float* rgb, float* rgb_weight, int32_t* label, int32_t* conf, void* stream);

/* ---- volume ray casting (csrc/pnr_fusion.hip; DESIGN.md 8 "Volume ray casting"): a TSDF volume seen from any camera -- the way
 * back from the volume of "depth fusion" to an image: depth, surface normal and the nearest lattice point per pixel.  The
 * reference ships no fusion: the rule is this build's and unpinned.  Float32 throughout, every operation a single + - * /,
 * floor, sqrt, min or max in the order given, never an FMA (tests/_raycast_ref.py restates the rule three times, twice bit for
 * bit).  min and max are fminf / fmaxf.
 *
 * INPUTS.  The camera (model, cam_host, c2w12_host, width, height) as pnr_project_points takes its camera, but the pose is
 *   camera-to-world; near_, far_; the lattice (res, lo_host, step_host) and the device arrays tsdf, weight of "depth fusion";
 *   min_weight; dt = the march step in units of the ray parameter; max_steps.
 * OUTPUTS.  Caller-owned device arrays, one element per pixel q = j width + i:
 *     depth   float32        0 unless HIT
 *     normal  float32 (., 3) 0 unless HIT     optional (NULL: not written)
 *     src     int32         -1 unless HIT     optional (NULL: not written)
 *     code    uint8          PNR_RAYCAST_HIT, _NO_RAY (pnr_camera_ray says the pixel sees nothing), _MISSED (the ray does not meet
 *                            the lattice between near and far) or _NO_SURFACE (the ray left the lattice, passed far or used up
 *                            max_steps without a crossing)
 * THE RULE, per pixel (i, j):
 *   1. RAY.  o, d, near, far = pnr_camera_ray(model, cam, c2w, i, j, near_, far_, ok), unchanged: the ray of pnr_gen_rays*.  A
 *      pinhole d is not normalised (the parameter is z-depth), a fisheye or equirect d is unit length (the parameter is range),
 *      so depth is in the convention of render_view.  !ok: NO_RAY.
 *   2. LATTICE COORDINATES, once per ray:  og_k = (o_k - lo_k) / step_k - 0.5f,  dg_k = d_k / step_k.  A sample at parameter t has
 *      g_k = og_k + t * dg_k; trilinear interpolation is defined for 0 <= g_k <= res_k - 1, hence every res_k >= 2.
 *   3. CLIP.  t_in = near, t_out = far; per axis k = x, y, z: if dg_k == 0 the ray misses when og_k < 0 or og_k > (float)(res_k - 1);
 *      otherwise ta = (0 - og_k) / dg_k, tb = ((float)(res_k - 1) - og_k) / dg_k, t_in = max(t_in, min(ta, tb)), t_out =
 *      min(t_out, max(ta, tb)).  MISSED unless t_in <= t_out.
 *   4. MARCH.  Samples n = 0, 1, ... at t_n = t_in + (float)n * dt while t_n <= t_out and n < max_steps.
 *   5. SAMPLE at t.  Per axis: c_k = clamp((int)floor(g_k), 0, res_k - 2) -- the floor is clamped to [0, 2^30] as a float before
 *      the conversion, which is then in range whatever g_k is -- and f_k = clamp(g_k - (float)c_k, 0, 1) = min(max(., 0), 1).  The
 *      eight corners are the lattice points (c_x + a, c_y + b, c_z + c), a, b, c in {0, 1}.  The sample is OBSERVED iff all eight
 *      have weight >= min_weight.  Its value: the lerp p + f * (q - p) along x for the four x-pairs, then along y for the two
 *      pairs of results, then along z.  The value of an unobserved sample is never used: NaN or garbage in tsdf where weight
 *      fails the test cannot leak.
 *   6. CROSSING.  The sign is depth fusion's: positive is BEHIND the surface.  The first n >= 1 whose samples n - 1 and n are both
 *      observed with v_{n-1} < 0 <= v_n is the hit; otherwise marching goes on.  So a ray that starts behind a surface, a crossing
 *      with an unobserved sample on either side, and the back of the band (+ to -) are no hits.  No hit: NO_SURFACE.
 *   7. HIT.  r = v_{n-1} / (v_{n-1} - v_n);  depth = t* = t_{n-1} + (t_n - t_{n-1}) * r.  One more sample is taken at t*: cell c*,
 *      fraction f*.  src = the flat index ("depth fusion") of the nearest corner (c*_k + (f*_k >= 0.5f ? 1 : 0)), whether or not
 *      that sample is observed.  If it is observed: the gradient of the trilinear interpolant -- for x the difference q - p of
 *      each x-pair, lerped along y then z; for y the y-pairs, lerped along x then z; for z the z-pairs, lerped along x then y --,
 *      each component divided by step_k, len = sqrt((gx gx + gy gy) + gz gz), normal = (-gx / len, -gy / len, -gz / len): a
 *      world-space unit vector out of the surface, towards observed free space.  Not observed, or len not positive and finite:
 *      normal = 0, and the pixel is still a HIT.
 * The camera and the pose are host values baked into the launch; the volume is read when the kernel runs (a captured launch sees
 * what was integrated since).  No atomics: two runs give the same bits.  Never synchronises; capture-safe.  PNR_EINVAL before any
 * launch: an unknown model; null camera or pose; null tsdf, weight, depth or code; a misaligned array (4 bytes); width or height
 * < 1 or more than 2^31 - 1 pixels; a camera the model's checks refuse (a zero focal length, gamma or step; pnr_gen_rays_equirect's);
 * a res < 2 or more than 2^31 - 1 points; null, non-finite lo or step, or a zero step; !(dt > 0) or a non-finite dt; max_steps
 * < 0; !(min_weight > 0); !(near_ >= 0); !(far_ > near_). */
#define PNR_RAYCAST_HIT 0
#define PNR_RAYCAST_NO_RAY 1
#define PNR_RAYCAST_MISSED 2
#define PNR_RAYCAST_NO_SURFACE 3
#define PNR_RAYCAST_TILE 8              /* a wave is a TILE x TILE block of pixels */
#define PNR_RAYCAST_BLOCK 256           /* threads (= pixels) a workgroup: four tiles side by side */
int pnr_tsdf_raycast(int model, const float* cam_host, const float* c2w12_host, int width, int height, float near_, float far_,
                     int res_x, int res_y, int res_z, const float* lo_host, const float* step_host, const float* tsdf,
                     const float* weight, float min_weight, float dt, int max_steps, float* depth, float* normal, int32_t* src,
                     uint8_t* code, void* stream);

/* ---- mesh ray casting (csrc/pnr_meshcast.hip; DESIGN.md 8 "Mesh ray casting"): a triangle mesh seen from any camera, or along a
 * list of rays -- the first hit per ray: depth, face, barycentric weights, nearest corner, flat normal and side.  The reference
 * ships none of this: the rule is this build's and unpinned (tests/_meshcast_ref.py restates it in numpy, bit for bit).  Float32
 * throughout unless stated, every operation a single + - * / sqrt in the order given, never an FMA; divide and sqrt correctly
 * rounded; denormals are not flushed.  THE ANSWER IS DEFINED BY BRUTE FORCE OVER ALL FACES; the index below only prunes.
 *
 * INPUTS.  vertices (V, 3) float32, faces (F, 3) int32.  The ray of element q is
 *   pnr_mesh_raycast:   o, d, near, far = pnr_camera_ray(model, cam, c2w, i, j, near_, far_, ok) unchanged, q = j width + i;
 *   pnr_mesh_cast_rays: the record rays[q] = (o, d, near, far) of an (n, 8) array, ok = true.
 *   NO_RAY if !ok, if a component of o or d is not finite, if d = 0, or if !(0 <= near <= far) (a NaN fails; far may be +inf).
 *   depth is the ray parameter t of the hit: z-depth in a pinhole frame, range in a fisheye or equirect frame (render_view's
 *   and pnr_tsdf_raycast's convention).
 * RAY-TRIANGLE TEST: the watertight test of Woop, Benthin and Wald (JCGT 2013), two-sided.  Once per ray:
 *   kz = the axis of largest |d_k|, the lowest axis on a tie; kx = kz + 1, ky = kx + 1 (mod 3), swapped if d[kz] < 0;
 *   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
 *  Per face with corners v0, v1, v2:
 *   A = v0 - o, B = v1 - o, C = v2 - o;   Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz], Az = Sz * A[kz]; B and C alike.
 *   U = Cx * By - Cy * Bx,  V = Ax * Cy - Ay * Cx,  W = Bx * Ay - By * Ax.
 *   If any of the three is exactly 0, all three are recomputed in double -- both products exact, one subtraction -- and rounded
 *   to float32 once.
 *   MISS if one of U, V, W is < 0 and one is > 0.   det = (U + V) + W;  MISS if det == 0.
 *   t = ((U * Az + V * Bz) + W * Cz) / det + 0.0f (the addition turns -0 into +0).  MISS unless near <= t <= far: a NaN misses.
 *   BOX TEST.  M = the largest of the nine |A_k|, |B_k|, |C_k| (max, in any order: exact), e = PNR_MESHCAST_BOX_TOL * M (2^-17,
 *   one multiply).  Per world axis k: q_k = t * d_k (the hit point relative to the origin), lo_k = min(min(A_k, B_k), C_k),
 *   hi_k = max(max(A_k, B_k), C_k);  MISS unless lo_k - e <= q_k <= hi_k + e on all three axes.  t is a mean of the corners'
 *   depths Az, Bz, Cz along the ray's dominant axis with weights U, V, W; for a ray that crosses the face its error is a few
 *   2^-24 of the largest |depth|, so that of every q_k = t d_k is a few 2^-24 of max |A[kz]| <= M (|d_k| <= |d[kz]|): inside
 *   e with a factor of some thirty to spare, at any distance from the face and any incidence -- along the face's normal the
 *   error of t d shrinks with the sine of the incidence as the error of t grows with its inverse.  For a ray nearly IN the
 *   plane of a face U, V, W are cancellation noise and t an arbitrary mean of Az, Bz, Cz: such a "hit" far from the face is
 *   none.  The test also ties every hit to the box the index files the face under, which is what makes the index exact
 *   (DESIGN.md).  Watertightness is that of the edge functions: a ray through a shared edge passes the sign test of both
 *   faces; it hits unless the noise of t carries the hit point out of the widened boxes of both, which takes a ray within
 *   about 2^-17 of the planes of both AND a crossing that close to the rim of both boxes.
 * WINNER: the hit with the smallest key ((uint64) bits(t) << 32) | (uint32) face -- the key of pnr_splat_points and pnr_nn_query:
 *   the nearest face, a tie in t going to the lowest face index (t >= +0, so the bits order as the values do).
 * OUTPUTS, caller-owned device arrays, one element per ray; the optional ones may be NULL:
 *     depth   float32          t                                                          0 off a hit
 *     face    int32            the winning face                                           -1
 *     code    uint8            PNR_RAYCAST_HIT, _NO_RAY or _MISSED
 *     bary    float32 (., 3)   U / det, V / det, W / det: the weights of v0, v1, v2       0        optional
 *     vertex  int32            the index of the corner with the largest weight, the       -1       optional
 *                              first on a tie: what per-vertex labels are read through
 *     normal  float32 (., 3)   below                                                      0        optional
 *     side    int8             +1 / -1                                                    0        optional
 *   n = (v1 - v0) x (v2 - v0), each component (a * b) - (c * d);  dot = (nx * dx + ny * dy) + nz * dz;  side = +1 if dot < 0 -- the
 *   ray met the side the winding normal points to --, else -1.  len = sqrt((nx nx + ny ny) + nz nz); normal = n / len, negated
 *   if side = -1, so it faces the ray's origin: the convention of pnr_tsdf_raycast and pnr_depth_normals that pnr_icp_accumulate
 *   expects.  len not positive and finite: normal = 0 and the element is still a HIT.
 * THE INDEX: a uniform grid res_x x res_y x res_z over the box from lo with cells of size cell (HOST values; inv_k = 1 / cell_k, one
 *   float32 division).  Grid coordinates g_k(p) = (p_k - lo_k) * inv_k.  PAD = PNR_MESHCAST_PAD = 1/16 cell.
 *   pnr_mesh_grid_bounds: bounds[0..2] / [3..5] = the smallest / largest coordinate per axis over the corners of USABLE faces (every
 *     index in range, every coordinate finite), +inf / -inf if there is none; bounds[6] = the bits of their number (uint32),
 *     bounds[7] = 0.  Integer atomics on order-preserving keys: exact in any order.  The caller widens the box and picks res.
 *   pnr_mesh_grid_count: every usable face adds 1 (int32 atomic) to every cell of [floor(min g_k - PAD), floor(max g_k + PAD)] per
 *     axis over its corners, clamped to the grid as floats; then the shared scan (csrc/pnr_scan_dev.h) into start[0 .. cells] and
 *     the 64-bit entry total into total.  The caller reads total -- its synchronisation --, refuses one above 2^31 - 1, allocates
 *     records (total, 12) float32 and calls pnr_mesh_grid_fill with the same mesh, grid, start and workspace: a returning atomic on
 *     the cell's cursor places the 48-byte record (v0, v1, v2, bits = face, 0, 0): a candidate is three 16-byte loads, no gather.
 *     The fill CONSUMES the cursors its count left in the workspace: one fill per count, nothing else using the workspace in
 *     between; a second fill needs a second count (it would place records below their cells' ranges, inside the array).
 *     The order of the records in a cell depends on arrival and is not part of the rule.  cell index = (cz res_y + cy) res_x + cx.
 *   A CAST computes og = (o - lo) * inv, dg = d * inv per axis, and its REACH = max_k (|og_k| + (float)(res_k + 1)) * cell_k: a
 *     bound in world units on every |component| of a corner of the grid's faces relative to the origin.  It takes THE PLAIN LOOP
 *     over all faces unless reach <= PNR_MESHCAST_MAX_REACH (4096) * the smallest cell_k -- then the box test's tolerance is at
 *     most 2^-5 of any cell, half a PAD --, or if some og_k or dg_k is not finite, the dominant dg_k is 0, or the clip below
 *     overflows: a camera very far from a small mesh, or a grid of very unequal cells, is slow and right.  Otherwise the ray is
 *     clipped to [near, far] and to the grid box widened by PAD; no overlap: MISSED.  It walks the layers of the axis of largest
 *     |dg_k| in order from the one it enters in; per layer the parameters at which it enters and leaves the slab, clamped to the
 *     clip, give the other two coordinates at both, and every cell of [floor(min - PAD), floor(max + PAD)] on those two axes is
 *     visited, every record in it tested by the rule above and the smallest key kept, wherever that hit lies.  After a layer
 *     the walk stops once the best hit lies more than PAD short of the layer's far face.  Start pairs are clamped into
 *     [0, n_entries]: a damaged table can give wrong answers, never an out-of-range read.  DESIGN.md argues why the outputs equal
 *     the plain loop's whatever res is.
 * The casts read the mesh and the index when the kernel runs, never synchronise and are capture-safe; the camera, the pose and
 * the grid's res, lo and cell are host values baked into the launch.  workspace: pnr_mesh_grid_workspace_bytes(res) bytes, 8-byte
 * aligned, the same block for bounds, count and fill (-1 for a res outside 1 .. PNR_MESHCAST_MAX_RES).
 * PNR_EINVAL before any launch: V or F outside 0 .. 2^31 - 1; null vertices or faces of a non-empty mesh; a misaligned array (4
 * bytes; records and rays 16; workspace and total 8); a res outside 1 .. 1024; null or non-finite lo; a cell that is not positive and
 * finite with a finite inverse; n_entries outside 0 .. 2^31 - 1; a null start, or null records with n_entries > 0; null depth, face
 * or code; pnr_mesh_raycast: an unknown model, null camera or pose, a bad image size, a camera the model's checks refuse,
 * !(near_ >= 0), !(far_ > near_); pnr_mesh_cast_rays: n_rays outside 0 .. 2^31 - 1, null rays (n_rays == 0: PNR_OK before the other
 * checks).  F == 0 is no error: every ray that is one is MISSED. */
#define PNR_MESHCAST_PAD 0.0625f
#define PNR_MESHCAST_BOX_TOL 0x1p-17f
#define PNR_MESHCAST_MAX_RES 1024
#define PNR_MESHCAST_MAX_REACH 4096.0f
int64_t pnr_mesh_grid_workspace_bytes(int res_x, int res_y, int res_z);
int pnr_mesh_grid_bounds(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, float* bounds,
                         void* workspace, void* stream);
int pnr_mesh_grid_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int res_x, int res_y,
                        int res_z, const float* lo_host, const float* cell_host, int32_t* start, int64_t* total, void* workspace,
                        void* stream);
int pnr_mesh_grid_fill(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int res_x, int res_y,
                       int res_z, const float* lo_host, const float* cell_host, const int32_t* start, int64_t n_entries,
                       float* records, void* workspace, void* stream);
int pnr_mesh_raycast(int model, const float* cam_host, const float* c2w12_host, int width, int height, float near_, float far_,
                     const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int res_x, int res_y,
                     int res_z, const float* lo_host, const float* cell_host, const int32_t* start, const float* records,
                     int64_t n_entries, float* depth, int32_t* face, uint8_t* code, float* bary, int32_t* vertex, float* normal,
                     int8_t* side, void* stream);
int pnr_mesh_cast_rays(const float* rays, int64_t n_rays, const float* vertices, int64_t n_vertices, const int32_t* faces,
                       int64_t n_faces, int res_x, int res_y, int res_z, const float* lo_host, const float* cell_host,
                       const int32_t* start, const float* records, int64_t n_entries, float* depth, int32_t* face, uint8_t* code,
                       float* bary, int32_t* vertex, float* normal, int8_t* side, void* stream);

/* ---- pose tracking (csrc/pnr_icp.hip; DESIGN.md 8 "Pose tracking"): the pose of a live depth frame refined against a model view
 * -- a view (camera M, c2w_M, depth, world-space normal) as pnr_tsdf_raycast writes it -- by projective association and a
 * point-to-plane Gauss-Newton iteration.  The reference ships no tracker: the rule is this build's and unpinned.  The pose lives
 * in DEVICE memory (pose12: 12 float32, the 3x4 row-major camera-to-world of the live frame) and is read and updated there, so a
 * chain of accumulate / solve launches needs no host read.  Per pixel float32, every operation a single + - * / sqrt, fminf or
 * fmaxf in the order given, never an FMA; the sums and the solve are IEEE double, one operation per symbol (tests/_icp_ref.py
 * restates the rule: per pixel twice, bit for bit; the solve in Python floats, bit for bit).
 *
 * pnr_icp_accumulate: one linearisation.  Per live pixel q = j width_l + i, IN THIS ORDER; the first failing test gives the code:
 *   1. t = depth_l[q].  NO_DEPTH unless t > 0 and t is finite.  (o, d) = pnr_camera_ray(model_l, cam_l, IDENTITY pose, i, j): o = 0
 *      and d is the model's own direction; !ok (a fisheye pixel outside the lens): NO_DEPTH.  p_cam = (t d_x, t d_y, t d_z).
 *   2. with the rows (r0 r1 r2 | T) of pose12:  qv_k = (r0 x + r1 y) + r2 z of p_cam,  p_k = qv_k + T_k.
 *   3. (u, v) and the domain flag of p in the model view with w2c_m: the arithmetic of pnr_project_points (umax = (float)width_m
 *      - 0.5f).  OUTSIDE unless in the domain and -0.5 <= u < width_m - 0.5, -0.5 <= v < height_m - 0.5.  Nearest pixel as
 *      reprojection step 5: a = min((int)floor(u + 0.5), width_m - 1), b likewise, mq = b width_m + a.
 *   4. dm = depth_m[mq], n = normal_m[mq].  NO_MODEL unless dm > 0 and dm is finite, every component of n is finite and not all
 *      three are 0 (pnr_tsdf_raycast writes depth 0 and normal 0 off the surface: no code image is needed).
 *   5. (o_m, d_m) = pnr_camera_ray(model_m, cam_m, c2w_m, a, b); !ok: NO_MODEL.  m_k = o_m,k + dm d_m,k;  e_k = m_k - p_k.
 *      TOO_FAR unless (e_x e_x + e_y e_y) + e_z e_z <= dist_max * dist_max (so a NaN is TOO_FAR).
 *   6. BACK_FACING if (n_x qv_x + n_y qv_y) + n_z qv_z >= 0: the model surface does not face the live camera.
 *   7. MATCH:  r = (n_x e_x + n_y e_y) + n_z e_z;  c = qv x n, each component one a b - c d: c_x = qv_y n_z - qv_z n_y,
 *      c_y = qv_z n_x - qv_x n_z, c_z = qv_x n_y - qv_y n_x;  J = (c_x, c_y, c_z, n_x, n_y, n_z).  The twist x = (omega, v) is about
 *      the live camera's centre: p' = R_delta qv + T + v, so r' = r - J x to first order.
 * SUMS over the MATCH pixels, in double: A_ab += (double)J_a (double)J_b for a <= b, row by row (slots 0 .. 20: A_00 A_01 .. A_05
 *   A_11 .. A_55), g_a += (double)J_a (double)r (slots 21 .. 26), E += (double)r (double)r (slot 27); the products are exact.  An
 *   exact integer count (slot 28, an int64).  A thread takes the pixels q = first + k stride in that order, a wave reduces by the
 *   xor butterfly (32, 16, .. 1), the four waves of a workgroup add as ((w0 + w1) + w2) + w3, and every workgroup writes ONE ROW of
 *   PNR_ICP_ROW 8-byte slots.  No floating atomics: two runs give the same bits.
 * WORKSPACE: pnr_icp_workspace_bytes(n_pix) bytes (-1 for n_pix < 1 or > 2^31 - 1), 8-byte aligned: slot 0 = the number of rows
 *   written (int64, the grid: at most PNR_ICP_MAX_BLOCKS and one workgroup per compute unit), then the rows in block order.
 * OPTIONAL per-pixel outputs (NULL: not written): code uint8 (PNR_ICP_*), residual float32 (r, 0 unless MATCH).
 * The cameras, c2w_m and w2c_m (camera.invert_pose of c2w_m: float64 on the host, rounded once) are host values baked into the
 * launch; pose12, the depth images and the normals are read when the kernel runs.  Never synchronises; capture-safe.  PNR_EINVAL
 * before any launch: an unknown model; a null camera or model pose; width or height < 1 or more than 2^31 - 1 pixels on either
 * side; a camera the model's checks refuse; null depth_l, pose12, depth_m, normal_m or workspace; pose12, the images or residual
 * misaligned (4 bytes) or workspace (8); dist_max not positive, or its square not finite.
 *
 * pnr_icp_solve: ONE workgroup.  n_pix is pnr_icp_accumulate's width_l * height_l (it bounds the rows read whatever slot 0 holds).
 *   1. COMBINE: every slot of the rows is added in block order from 0.0 (the count in integers).
 *   2. count < min_matches: TOO_FEW.  With update == 0 the entry point stops here: status OK, nothing solved, pose12 untouched
 *      (the last row of a track: count and E at the final pose).
 *   3. CHOLESKY A = L L^T, column j = 0 .. 5:  s = A_jj;  s = s - L_jk L_jk for k = 0 .. j - 1;  DEGENERATE unless
 *      s > 2^-30 A_jj (the pivot against its own diagonal entry of A);  L_jj = sqrt(s);  for i = j + 1 .. 5:  s = A_ij;
 *      s = s - L_ik L_jk for k = 0 .. j - 1;  L_ij = s / L_jj.
 *   4. FORWARD  y_i = (g_i - sum) / L_ii, i = 0 .. 5, the sum subtracted term by term: s = g_i; s = s - L_ik y_k for k = 0 .. i - 1.
 *      BACK  x_i = s / L_ii, i = 5 .. 0:  s = y_i;  s = s - L_ki x_k for k = i + 1 .. 5.   omega = x_0..2, v = x_3..5.
 *   5. w2 = (omega_x omega_x + omega_y omega_y) + omega_z omega_z, v2 likewise.  STEP_TOO_LARGE unless w2 <= max_rot max_rot and
 *      v2 <= max_trans max_trans (doubles; a NaN is too large).
 *   6. a = sin(theta) / theta and b = (1 - cos(theta)) / theta^2 as their power series in s = w2, PNR_ICP_SERIES_TERMS terms in
 *      Horner form:  a = ca_7;  a = a s + ca_k for k = 6 .. 0, with ca_k = (-1)^k / (2k + 1)!;  b the same with
 *      cb_k = (-1)^k / (2k + 2)! -- each coefficient the correctly rounded quotient of 1.0 and the (exact) factorial.  No sqrt and
 *      no libm call.  The first dropped terms at the cap s = 0.25 are 2^-64.4 and 2^-68.5.
 *      R_delta:  diagonal  D_ii = 1.0 + b (omega_i omega_i - s);  off the diagonal  D_ij = a K_ij + b (omega_i omega_j)  with
 *      K = [omega]x: K_01 = -omega_z, K_02 = omega_y, K_10 = omega_z, K_12 = -omega_x, K_20 = -omega_y, K_21 = omega_x.
 *   7. R'_ij = (D_i0 R_0j + D_i1 R_1j) + D_i2 R_2j  and  T'_i = T_i + v_i  in double on the float32 pose, each rounded to float32
 *      once at the store: R' = R_delta R, T' = T + v.  The kernel does not re-orthonormalise.
 *   history row (5 doubles, device): count, E, w2, v2, status.  w2 and v2 are 0 where nothing was solved (TOO_FEW, DEGENERATE,
 *   update == 0).  pose12 is left bit for bit unchanged unless the status is OK and update != 0.
 * Never synchronises; capture-safe.  PNR_EINVAL before any launch: null or misaligned workspace, history (8 bytes) or pose12 (4);
 * n_pix < 1 or > 2^31 - 1; min_matches < 1; !(max_rot > 0) or max_rot > PNR_ICP_MAX_ROT (the series' cap); !(max_trans > 0)
 * (+inf allowed). */
#define PNR_ICP_MATCH 0
#define PNR_ICP_NO_DEPTH 1
#define PNR_ICP_OUTSIDE 2
#define PNR_ICP_NO_MODEL 3
#define PNR_ICP_TOO_FAR 4
#define PNR_ICP_BACK_FACING 5
#define PNR_ICP_OK 0
#define PNR_ICP_TOO_FEW 1
#define PNR_ICP_DEGENERATE 2
#define PNR_ICP_STEP_TOO_LARGE 3
#define PNR_ICP_SUMS 28                 /* 21 of A, 6 of g, E */
#define PNR_ICP_ROW 29                  /* 8-byte slots a workgroup writes: the sums and the count */
#define PNR_ICP_MAX_BLOCKS 256          /* the grid's limit: what pnr_icp_workspace_bytes sizes for */
#define PNR_ICP_SERIES_TERMS 8
#define PNR_ICP_MAX_ROT 0.5f            /* radians: the largest max_rot pnr_icp_solve accepts */
int64_t pnr_icp_workspace_bytes(int64_t n_pix);
int pnr_icp_accumulate(int model_l, const float* cam_l_host, int width_l, int height_l, const float* depth_l, const float* pose12,
                       int model_m, const float* cam_m_host, const float* c2w_m12_host, const float* w2c_m12_host, int width_m,
                       int height_m, const float* depth_m, const float* normal_m, float dist_max, void* workspace, uint8_t* code,
                       float* residual, void* stream);
int pnr_icp_solve(const void* workspace, int64_t n_pix, int64_t min_matches, float max_rot, float max_trans, int update,
                  float* pose12, double* history_row, void* stream);

/* ---- depth front end (csrc/pnr_depth.hip; DESIGN.md 8 "Depth front end"): what turns any depth image into a view -- an
 * edge-preserving filter with a speckle rule, then vertices and normals, so that "pose tracking" can take a depth frame as its
 * model view.  The reference ships neither: the rule is this build's and unpinned.  Float32 throughout, every operation a single
 * + - * /, sqrt or comparison in the order given, never an FMA (tests/_depth_ref.py restates both rules three times, twice bit
 * for bit).  A depth t is VALID iff t > 0 and t is finite (so a NaN is not).  No atomics: two runs give the same bits.  Neither
 * entry point synchronises; both are capture-safe, and the images are read when the kernel runs.
 *
 * pnr_depth_filter.  g_host[0 .. radius]: the spatial weights by |offset|, made by the host (exp(-k k / (2 sigma_space^2)) in
 *   float64, rounded once: the kernel calls no exp).  Per pixel (i, j) with centre depth c = depth_in[j width + i]:
 *   1. c not valid: depth_out = 0, support = 0.  Holes are not filled.
 *   2. sigma = sigma_a + sigma_b * c;  acc = ws = 0, count = 0.
 *   3. the window row-major: dy = -radius .. radius outside, dx = -radius .. radius inside.  The neighbour t = depth_in at
 *      (i + dx, j + dy) is USED iff it lies inside the image, t is valid, and u > 0 with x = (t - c) / sigma, u = 1 - x * x (a NaN
 *      is not used; the centre has x = 0 and is always used).  Then w = (g[|dy|] * g[|dx|]) * (u * u);  acc = acc + w * t;
 *      ws = ws + w;  count = count + 1.  The range weight is a compact biweight: no transcendental.
 *   4. depth_out = acc / ws if count >= min_support, else 0 (the speckle rule: an isolated pixel has no support).
 *      support (int16, optional; NULL: not written) = count, at most (2 radius + 1)^2 = 289.
 *   PNR_EINVAL before any launch: width or height < 1 or more than 2^31 - 1 pixels; null depth_in, depth_out or g_host; depth_in
 *   or depth_out misaligned (4 bytes) or support (2); depth_in == depth_out; radius outside 0 .. PNR_DEPTH_MAX_RADIUS; a g entry
 *   that is not positive and finite; sigma_a or sigma_b negative or not finite, or both 0; min_support < 1.
 *
 * pnr_depth_normals.  The camera (model, cam_host, c2w12_host, width, height) as pnr_tsdf_raycast takes it; mc2 = min_cos^2,
 *   rounded on the host.  Per pixel q = (i, j) with t = depth[q], IN THIS ORDER; the first failing test gives the code:
 *   1. (o, d) = pnr_camera_ray(model, cam, c2w, i, j).  NO_DEPTH unless t is valid and the ray is ok.  v_k = t * d_k;
 *      vertex_k = o_k + v_k.
 *   2. the neighbours one pixel left, right, up and down.  One is USABLE iff it lies inside the image (no longitude wrap), its own
 *      test 1 passes, and |t_nb - t| <= jump_a + jump_b * t.
 *   3. per image axis (x: left / right, y: up / down):  both usable: D = v(next) - v(previous);  one usable: v(next) - v or
 *      v - v(previous);  neither, on either axis: NO_NEIGHBOUR.  The differences are of v, never of vertex: the camera's origin
 *      would cost the low bits at large world coordinates.
 *   4. c = Dx x Dy, each component one a b - c d:  c_x = Dx_y Dy_z - Dx_z Dy_y,  c_y = Dx_z Dy_x - Dx_x Dy_z,
 *      c_z = Dx_x Dy_y - Dx_y Dy_x.  cc = (c_x c_x + c_y c_y) + c_z c_z;  len = sqrt(cc).  DEGENERATE unless len > 0 and finite.
 *   5. s = (c_x v_x + c_y v_y) + c_z v_z;  vv = (v_x v_x + v_y v_y) + v_z v_z.  GRAZING if s * s < (mc2 * cc) * vv.
 *   6. OK:  n_k = c_k / len, negated if s > 0: the normal faces the camera, pnr_tsdf_raycast's convention, which
 *      pnr_icp_accumulate's BACK_FACING test expects.
 *   OUTPUTS.  normal float32 (., 3): 0 unless OK.  vertex float32 (., 3), optional: o + v wherever test 1 passed, 0 elsewhere.
 *   code uint8, optional: PNR_NORMAL_*.
 *   PNR_EINVAL before any launch: an unknown model; null camera or pose; width or height < 1 or more than 2^31 - 1 pixels; a camera
 *   the model's checks refuse; null depth or normal; depth, normal or vertex misaligned (4 bytes); jump_a or jump_b negative or NaN
 *   (+inf allowed: no gate); mc2 outside [0, 1]. */
#define PNR_DEPTH_MAX_RADIUS 8
#define PNR_DEPTH_TILE_X 32             /* pixels a workgroup of k_depth_filter: TILE_X x TILE_Y, one thread each */
#define PNR_DEPTH_TILE_Y 8
#define PNR_NORMALS_TILE_X 32           /* the same of k_depth_normals */
#define PNR_NORMALS_TILE_Y 8
#define PNR_NORMAL_OK 0
#define PNR_NORMAL_NO_DEPTH 1
#define PNR_NORMAL_NO_NEIGHBOUR 2
#define PNR_NORMAL_DEGENERATE 3
#define PNR_NORMAL_GRAZING 4
int pnr_depth_filter(int width, int height, const float* depth_in, int radius, const float* g_host, float sigma_a, float sigma_b,
                     int min_support, float* depth_out, int16_t* support, void* stream);
int pnr_depth_normals(int model, const float* cam_host, const float* c2w12_host, int width, int height, const float* depth,
                      float jump_a, float jump_b, float mc2, float* normal, float* vertex, uint8_t* code, void* stream);

/* ---- connected components (csrc/pnr_components.hip; tests/_cc_ref.py restates the rule in numpy): the components of an image, a
 * lattice or a triangle mesh, numbered in a fixed order, with the size of each.  The reference ships none of this: the rule is this
 * build's and unpinned.  The result is exact and the same on every call, whatever the schedule.
 *
 * ELEMENTS AND LINKS.  A lattice (res_z, res_y, res_x) is indexed flat, i = (iz * res_y + iy) * res_x + ix; an image is the
 *   lattice with res_z = 1.  Two neighbouring elements are LINKED iff both are foreground and the mode's test holds.
 *   full = 0: neighbours differ by +-1 on exactly one axis (6 in a volume, 4 in an image).
 *   full = 1: neighbours differ by at most 1 on every axis and are not the element itself (26 in a volume, 8 in an image).
 *   Nothing wraps and nothing links across the lattice border.
 * MODES.  PNR_CC_KEYS, int32 data: an element is foreground iff key >= 0; two neighbours are linked iff their keys are equal.  A
 *   mask is keys {-1, 0}; a panoptic lattice is its ids.
 *   PNR_CC_VALUES, float32 data with tol >= 0 (+inf allowed, NaN refused): an element is foreground iff the value is finite and
 *   > 0 (the "0 = no depth" convention); two neighbours are linked iff fabsf(a - b) <= tol, one float32 subtraction.  A component
 *   is the transitive closure of the links: a ~ b ~ c joins a and c even where |a - c| > tol.
 * OUTPUTS.  labels (int32, the data's shape): -1 on background, on foreground the component's number in 0 .. count - 1.  The
 *   components are numbered by their lowest flat index: raster order of the first element.  count: (1) int64 on the device.
 *   size (int32, the data's shape; NULL: not wanted): the number of elements of the element's own component, 0 on background.
 * MESHES.  The elements are the vertices 0 .. n_vertices - 1; a face links its three vertices.  A face with an index outside that
 *   range links nothing and gets face_label = -1; a vertex used by no valid face gets vertex_label = -1.  The components are
 *   numbered by their lowest vertex index; face_label[f] is the label of its vertices; face_size[f] (NULL: not wanted) the number
 *   of valid faces of the face's component, 0 for a face that is not valid.
 * STATISTICS.  pnr_cc_stats, once the caller knows count: from labels and size as above, sizes (n_components) int32 and boxes
 *   (n_components, 6) int32 (NULL: not wanted) = (ix_min, iy_min, iz_min, ix_max, iy_max, iz_max) in lattice indices.  Rows >=
 *   n_components are never written; an element whose label is outside 0 .. n_components - 1 is skipped.
 * HOW.  Union-find on a parent array P with P[i] <= i, in the labels buffer: (1) P[i] = i on foreground, -1 on background;
 *   (2) every element unites with its backward neighbours (smaller flat index: 3 or 13 in a volume, 2 or 4 in an image), a face
 *   unites (v0, v1) and (v1, v2): find both roots and, where they differ, an int32 atomic minimum of the smaller into the larger
 *   root's entry, repeated from the returned value where that was no longer a root; (3) P[i] = its root, a flag per root, one
 *   integer atomic add per element (per valid face) into the root's counter; (4) the shared exclusive scan of the flags: the
 *   rank, and the 64-bit total = count; (5) labels[i] = rank[P[i]], size[i] = counter[P[i]].  The root of a finished component is
 *   its lowest index whatever the interleaving.  A lattice takes steps (1) and (2) in two levels: a workgroup labels a tile of
 *   PNR_CC_TILE_X x _Y elements of an image (res_z = 1), PNR_CC_TILE3_X x _Y x _Z of a volume, in LDS by the same union-find on
 *   tile-local indices, whose order is the flat order, and writes P[i] = the global index of the tile-local root; only the links
 *   across tile borders then go to global memory.  A build with -DPNR_CC_FLAT takes them in one level, every link a global
 *   atomic: the baseline the tiled form was measured against, the same bits.  No kernel waits on another workgroup; every pointer chase steps only to a
 *   strictly smaller non-negative index and stops otherwise, so a kernel terminates on any memory content.  No float atomics,
 *   no 64-bit atomics.  A call is a plain chain of kernel nodes (no memset): capture-safe, and it never synchronises.
 * LIMITS.  At most 2^31 - 2 elements (n + 1 int32 entries are scanned).  labels and size may not overlap the data or each other.
 * workspace: pnr_cc_workspace_bytes(n_elements) bytes, 8-byte aligned (-1 for n outside 0 .. 2^31 - 2); n_elements = n_vertices
 *   for a mesh.  PNR_EINVAL before any launch: an unknown mode; full outside {0, 1}; tol negative or NaN (values mode); a res < 0,
 *   or a lattice over the limit; V outside 0 .. 2^31 - 2 or F outside 0 .. 2^31 - 1; n_components outside 0 .. 2^31 - 2; a null or
 *   misaligned pointer (4 bytes; count and workspace 8); overlapping data and outputs.  A lattice with a res of 0 and a mesh
 *   without vertices have no elements: count = 0, every face_label = -1, nothing else is written. */
#define PNR_CC_KEYS 0
#define PNR_CC_VALUES 1
#define PNR_CC_TILE_X 32                /* the tile a workgroup labels in LDS first: TILE_X x TILE_Y elements of an image, */
#define PNR_CC_TILE_Y 8                 /* one thread each; */
#define PNR_CC_TILE3_X 8                /* TILE3_X x TILE3_Y x TILE3_Z of a volume */
#define PNR_CC_TILE3_Y 8
#define PNR_CC_TILE3_Z 4
int64_t pnr_cc_workspace_bytes(int64_t n_elements);
int pnr_cc_label(const void* data, int mode, float tol, int res_x, int res_y, int res_z, int full, int32_t* labels, int32_t* size,
                 int64_t* count, void* workspace, void* stream);
int pnr_cc_mesh(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* vertex_label, int32_t* face_label,
                int32_t* face_size, int64_t* count, void* workspace, void* stream);
int pnr_cc_stats(const int32_t* labels, const int32_t* size, int res_x, int res_y, int res_z, int64_t n_components, int32_t* sizes,
                 int32_t* boxes, void* stream);

/* ---- diagnostics.  Measurement helpers (hipEvent timing, MFMA / HBM ceilings of the device) live in libpnr_bench.so
 * (include/pnr_bench.h), not here: every export of this library is stream-ordered, never synchronises and keeps no mutable
 * state -- the one diagnostic hook of the MLP kernels is a descriptor field (pnr_mlp_desc.clk_probe). */

#ifdef __cplusplus
}
#endif
#endif /* PNR_H */
