// Loss wrapper of the trainer (the reference's NetworkWrapper computes RGB MSE, a stereo-depth
// loss, 2D pseudo-label cross-entropies on the learned and on the fixed (bbox-prior) fields, and a 3D cross-entropy
// of the learned field against the bbox labels).  No reference file exists in the mount
// (SURVEY.md 0): the terms follow that description, every constant is an argument, and DESIGN.md 9 lists what has to
// be re-checked against the branch.
//
//   pnr_losses : one pass over the rays of a level -- all per-ray terms AND the gradient of their weighted sum
//                w.r.t. every rendered map (what autograd would hand to raw2outputs' backward).  HBM-bound and tiny
//                (R x (5 + 2(C+K)) floats); what it removes is ~30 eager launches per level.
//   pnr_ce3d   : forward value of the per-sample 3D cross-entropy, streaming the channel-major raw logits.  Its
//                gradient is fused into k_composite_bwd (pnr_composite_backward2: ce_sem / ce_inst).
// Reductions are two-stage with a fixed order (per-block partials, then one block): bit-for-bit deterministic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "pnr_common.h"
#include "pnr_composite_dev.h"

#define LS_THREADS 256
#define LS_TERMS 8        /* rgb, depth, sem, fix_sem, inst, fix_inst, (unused), (unused) */

struct LossArgs {
    pnr_loss_cfg cfg;
    int64_t R; int C, K;
    const float *rgb, *depth, *sem, *fix_sem, *inst, *fix_inst;
    const float *rgb_gt, *depth_gt; const int32_t *sem_gt, *inst_gt;
    float *g_rgb, *g_depth, *g_sem, *g_fix_sem, *g_inst, *g_fix_inst;
    int* counts;            // [0] rays with depth_gt > 0, [1] with a semantic label, [2] with an instance label
    float* partial;         // [blocks][LS_TERMS]
    float* losses;          // [8]: the six means, the weighted total, 0
    int n_blocks;
};

__global__ __launch_bounds__(LS_THREADS) void k_loss_count(LossArgs a)
{
    int nd = 0, ns = 0, ni = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        if (a.depth && a.depth_gt && a.depth_gt[r] > 0.0f) ++nd;
        if (a.sem_gt && a.sem_gt[r] >= 0 && a.sem_gt[r] < a.C) ++ns;
        if (a.inst_gt && a.inst_gt[r] >= 0 && a.inst_gt[r] < a.K) ++ni;
    }
    // integer atomics: order-independent
    if (nd) atomicAdd(&a.counts[0], nd);
    if (ns) atomicAdd(&a.counts[1], ns);
    if (ni) atomicAdd(&a.counts[2], ni);
}

// ---- the per-ray terms: LS_GROUP = 16 lanes per ray (16 rays per block), the lanes of a group split the classes of a field.
// (Round 4: one THREAD per ray walked its 45 + 45 + 32 + 32 map entries alone -- strided, three passes, 16 workgroups at a
// 4096-ray batch: 61 us per level where the data is 2.6 MB.)  Every reduction has a fixed order: per-lane partial sums over
// c = lane, lane + 16, ..., then the xor butterfly 8, 4, 2, 1 inside the group, then the 16 rays of a block in ray order.
#define LS_GROUP 16
#define LS_RAYS (LS_THREADS / LS_GROUP)

__device__ __forceinline__ float group_sum(float v)
{
#pragma unroll
    for (int d = LS_GROUP / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, LS_GROUP);
    return v;
}
__device__ __forceinline__ float group_max(float v)
{
#pragma unroll
    for (int d = LS_GROUP / 2; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, LS_GROUP));
    return v;
}

// cross-entropy of one ray's logits against label, the group's lanes striding over the classes; writes
// scale * (softmax - onehot) to g (if non-null); every lane returns the value
__device__ __forceinline__ float ce_row(const float* logit, int n_cls, int label, float scale, float* g, int l)
{
    float mx = -INFINITY;
    for (int c = l; c < n_cls; c += LS_GROUP) mx = fmaxf(mx, logit[c]);
    mx = group_max(mx);
    float den = 0.0f;
    for (int c = l; c < n_cls; c += LS_GROUP) den += expf(logit[c] - mx);
    den = group_sum(den);
    if (g)
        for (int c = l; c < n_cls; c += LS_GROUP) g[c] = scale * (expf(logit[c] - mx) / den - (c == label ? 1.0f : 0.0f));
    // log den first, then the exact-difference mx - x_label: (mx + logf(den)) - x_label rounds at the size of mx, which made the
    // value depend on a common shift of the row (|mx| 2^-25: 3e-5 at logits around 1000)
    return logf(den) + (mx - logit[label]);
}

__global__ __launch_bounds__(LS_THREADS) void k_loss_maps(LossArgs a)
{
    __shared__ float red[LS_RAYS][LS_TERMS];
    const int l = threadIdx.x & (LS_GROUP - 1), grp = threadIdx.x / LS_GROUP;
    const int64_t r = (int64_t)blockIdx.x * LS_RAYS + grp;
    float t[LS_TERMS];                      // the ray's terms: identical on every lane of the group
#pragma unroll
    for (int i = 0; i < LS_TERMS; ++i) t[i] = 0.0f;
    const float nd = (float)(a.counts[0] > 0 ? a.counts[0] : 1), ns = (float)(a.counts[1] > 0 ? a.counts[1] : 1),
                ni = (float)(a.counts[2] > 0 ? a.counts[2] : 1);
    if (r < a.R) {                          // uniform over the group
        if (a.rgb && a.rgb_gt) {
            const float k = a.cfg.w_rgb * 2.0f / (3.0f * (float)a.R);
            float dd = 0.0f;
            if (l < 3) {
                const float d = a.rgb[r * 3 + l] - a.rgb_gt[r * 3 + l];
                dd = d * d;
                if (a.g_rgb) a.g_rgb[r * 3 + l] = k * d;
            }
            // channels 0, 1, 2 in order, as the sequential form added them
            t[0] = (__shfl(dd, 0, LS_GROUP) + __shfl(dd, 1, LS_GROUP)) + __shfl(dd, 2, LS_GROUP);
        }
        if (a.depth && a.depth_gt) {
            const float gt = a.depth_gt[r];
            float g = 0.0f;
            if (gt > 0.0f) {
                const float d = a.depth[r] - gt;
                if (a.cfg.depth_l2) { t[1] = d * d; g = a.cfg.w_depth * 2.0f * d / nd; }
                else { t[1] = fabsf(d); g = a.cfg.w_depth * (d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f) / nd; }
            }
            if (a.g_depth && l == 0) a.g_depth[r] = g;
        }
        auto field = [&](const float* logit, const float* fix, const int32_t* gt, int n_cls, float w_ce, float w_fix, float n,
                         float* g_logit, float* g_fix, float& t_ce, float& t_fix) {
            const int lab = gt ? gt[r] : -1;
            const bool valid = lab >= 0 && lab < n_cls;
            if (logit) {
                float* g = g_logit ? g_logit + r * n_cls : nullptr;
                if (a.cfg.maps_are_prob) {              // probability map: NLL of the labelled class
                    float p = 1.0f;
                    if (valid) { p = logit[r * n_cls + lab] + a.cfg.fix_eps; t_ce = -logf(p); }
                    if (g) for (int c = l; c < n_cls; c += LS_GROUP) g[c] = (valid && c == lab) ? -w_ce / (p * n) : 0.0f;
                } else if (valid) t_ce = ce_row(logit + r * n_cls, n_cls, lab, w_ce / n, g, l);
                else if (g) for (int c = l; c < n_cls; c += LS_GROUP) g[c] = 0.0f;
            }
            if (fix) {
                float* g = g_fix ? g_fix + r * n_cls : nullptr;
                float p = 1.0f;
                if (valid) { p = fix[r * n_cls + lab] + a.cfg.fix_eps; t_fix = -logf(p); }
                if (g) for (int c = l; c < n_cls; c += LS_GROUP) g[c] = (valid && c == lab) ? -w_fix / (p * n) : 0.0f;
            }
        };
        if (a.C) field(a.sem, a.fix_sem, a.sem_gt, a.C, a.cfg.w_sem, a.cfg.w_fix_sem, ns, a.g_sem, a.g_fix_sem, t[2], t[3]);
        if (a.K) field(a.inst, a.fix_inst, a.inst_gt, a.K, a.cfg.w_inst, a.cfg.w_fix_inst, ni, a.g_inst, a.g_fix_inst, t[4], t[5]);
    }
    // block sums in a fixed order: the rays of the block in ray order
    if (l == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) red[grp][i] = t[i];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = 0.0f;
        for (int w = 0; w < LS_RAYS; ++w) v += red[w][threadIdx.x];
        a.partial[(int64_t)blockIdx.x * LS_TERMS + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void k_loss_final(LossArgs a)
{
    // per term: lane i adds blocks i, i + 64, ... in that order, then a fixed butterfly (deterministic; a full frame has
    // ~2000 partials, one lane walking them all costs >100 us)
    const int i = threadIdx.x;
    float total = 0.0f;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        float v = 0.0f;
        for (int b = i; b < a.n_blocks; b += 64) v += a.partial[(int64_t)b * LS_TERMS + t];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        const float n = t == 0 ? 3.0f * (float)a.R : t == 1 ? (float)(a.counts[0] > 0 ? a.counts[0] : 1)
                      : t <= 3 ? (float)(a.counts[1] > 0 ? a.counts[1] : 1) : (float)(a.counts[2] > 0 ? a.counts[2] : 1);
        v /= n;
        const float w = t == 0 ? a.cfg.w_rgb : t == 1 ? a.cfg.w_depth : t == 2 ? a.cfg.w_sem : t == 3 ? a.cfg.w_fix_sem
                      : t == 4 ? a.cfg.w_inst : a.cfg.w_fix_inst;
        if (i == 0) a.losses[t] = v;
        total += w * v;                         // fixed order t = 0..5
    }
    if (i == 0) { a.losses[6] = total; a.losses[7] = 0.0f; }
}

PNR_EXPORT int64_t pnr_losses_workspace_bytes(int64_t n_rays)
{
    if (n_rays < 0) return -1;
    const int64_t blocks = (n_rays + LS_RAYS - 1) / LS_RAYS;
    return 64 + (blocks > 0 ? blocks : 1) * LS_TERMS * (int64_t)sizeof(float);
}

PNR_EXPORT int pnr_losses(const pnr_loss_cfg* cfg, int64_t n_rays, int n_sem, int n_inst, const float* rgb, const float* depth,
                          const float* sem, const float* fix_sem, const float* inst, const float* fix_inst, const float* rgb_gt,
                          const float* depth_gt, const int32_t* sem_gt, const int32_t* inst_gt, float* losses_out, float* g_rgb,
                          float* g_depth, float* g_sem, float* g_fix_sem, float* g_inst, float* g_fix_inst, void* workspace, void* stream)
{
    PNR_REQUIRE(cfg && losses_out && workspace, "pnr_losses: null pointer");
    PNR_REQUIRE(n_rays >= 1 && n_sem >= 0 && n_inst >= 0, "pnr_losses: bad size");
    PNR_REQUIRE(!(sem || fix_sem) || (n_sem > 0 && sem_gt), "pnr_losses: semantic maps need n_sem > 0 and sem_gt");
    PNR_REQUIRE(!(inst || fix_inst) || (n_inst > 0 && inst_gt), "pnr_losses: instance maps need n_inst > 0 and inst_gt");
    hipStream_t st = (hipStream_t)stream;
    LossArgs a;
    memset(&a, 0, sizeof(a));
    a.cfg = *cfg; a.R = n_rays; a.C = (sem || fix_sem) ? n_sem : 0; a.K = (inst || fix_inst) ? n_inst : 0;
    a.rgb = rgb; a.depth = depth; a.sem = sem; a.fix_sem = fix_sem; a.inst = inst; a.fix_inst = fix_inst;
    a.rgb_gt = rgb_gt; a.depth_gt = depth_gt; a.sem_gt = sem_gt; a.inst_gt = inst_gt;
    a.g_rgb = g_rgb; a.g_depth = g_depth; a.g_sem = g_sem; a.g_fix_sem = g_fix_sem; a.g_inst = g_inst; a.g_fix_inst = g_fix_inst;
    a.counts = (int*)workspace; a.partial = (float*)((char*)workspace + 64); a.losses = losses_out;
    a.n_blocks = (int)((n_rays + LS_RAYS - 1) / LS_RAYS);
    PNR_HIP(hipMemsetAsync(workspace, 0, 64, st));
    const int cblocks = (int)((n_rays + LS_THREADS - 1) / LS_THREADS);
    const int cgrid = cblocks < 1024 ? cblocks : 1024;
    hipLaunchKernelGGL(k_loss_count, dim3(cgrid), dim3(LS_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_loss_maps, dim3(a.n_blocks), dim3(LS_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(64), 0, st, a);
    PNR_CHECK_LAUNCH("pnr_losses");
    return PNR_OK;
}

// ------------------------------------------------------------------------------- per-sample 3D cross-entropy (forward)
struct Ce3dArgs {
    const float* raw; int64_t sc; int ch0, n_cls;
    const int32_t* label; int64_t S;
    float* partial;          // [blocks][2] = (sum of CE, count)
    float* out;              // [2] = (mean CE over labelled samples, count)
    int n_blocks;
};

__global__ __launch_bounds__(LS_THREADS) void k_ce3d(Ce3dArgs a)
{
    __shared__ float red[LS_THREADS / 64][2];
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float ce = 0.0f, cnt = 0.0f;
    if (s < a.S) {
        const int lab = a.label[s];
        if (lab >= 0 && lab < a.n_cls) {
            const float* p = a.raw + (int64_t)a.ch0 * a.sc + s;
            float mx = -INFINITY, den = 0.0f, at = 0.0f;
            for (int c = 0; c < a.n_cls; ++c) {          // online log-sum-exp: one pass over the channel rows
                const float v = p[(int64_t)c * a.sc];
                lse_step(mx, den, v);                    // the step k_composite_bwd takes for this term's gradient
                if (c == lab) at = v;
            }
            ce = logf(den) + (mx - at);             // as in ce_row: invariant under a common shift of the logits
            cnt = 1.0f;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { ce += __shfl_xor(ce, d, 64); cnt += __shfl_xor(cnt, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = ce; red[threadIdx.x >> 6][1] = cnt; }
    __syncthreads();
    if (threadIdx.x < 2) {
        float v = 0.0f;
        for (int w = 0; w < LS_THREADS / 64; ++w) v += red[w][threadIdx.x];
        a.partial[(int64_t)blockIdx.x * 2 + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void k_ce3d_final(Ce3dArgs a)
{
    // lane i adds blocks i, i + 64, ... in that order, then a fixed butterfly: deterministic, and not one lane walking
    // thousands of partials (that cost 170 us).  double: counts up to 2^31 stay exact.
    const int i = threadIdx.x;
    double sum = 0.0, cnt = 0.0;
    for (int b = i; b < a.n_blocks; b += 64) {
        sum += (double)a.partial[(int64_t)b * 2];
        cnt += (double)a.partial[(int64_t)b * 2 + 1];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sum += __shfl_xor(sum, d, 64); cnt += __shfl_xor(cnt, d, 64); }
    if (i == 0) { a.out[0] = (float)(sum / (cnt > 0.0 ? cnt : 1.0)); a.out[1] = (float)cnt; }
}

PNR_EXPORT int64_t pnr_ce3d_workspace_bytes(int64_t n_samples)
{
    if (n_samples < 0) return -1;
    const int64_t blocks = (n_samples + LS_THREADS - 1) / LS_THREADS;
    return (blocks > 0 ? blocks : 1) * 2 * (int64_t)sizeof(float);
}

PNR_EXPORT int pnr_ce3d(const float* raw, int64_t raw_stride_c, int first_channel, int n_classes, const int32_t* label,
                        int64_t n_samples, float* out2, void* workspace, void* stream)
{
    PNR_REQUIRE(raw && label && out2 && workspace, "pnr_ce3d: null pointer");
    PNR_REQUIRE(n_samples >= 1 && n_classes >= 1 && first_channel >= 0 && raw_stride_c >= n_samples, "pnr_ce3d: bad size");
    Ce3dArgs a;
    a.raw = raw; a.sc = raw_stride_c; a.ch0 = first_channel; a.n_cls = n_classes; a.label = label; a.S = n_samples;
    a.partial = (float*)workspace; a.out = out2;
    a.n_blocks = (int)((n_samples + LS_THREADS - 1) / LS_THREADS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ce3d, dim3(a.n_blocks), dim3(LS_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_ce3d_final, dim3(1), dim3(64), 0, st, a);
    PNR_CHECK_LAUNCH("pnr_ce3d");
    return PNR_OK;
}
