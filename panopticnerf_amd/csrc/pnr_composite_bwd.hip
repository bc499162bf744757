// K4-bwd: backward of raw2outputs (the reverse scan).  HBM-bound: reads raw
// once, writes d_raw once.  Same lane mapping as the forward kernel (pnr_composite.hip): a ray is
// owned by SUB = pow2ceil(N/4) lanes, 4 consecutive samples per lane; channel-major images.
//
//   w_i = alpha_i T_i,  T_i = prod_{j<i} (1 - alpha_j + 1e-10),  alpha_i = 1 - exp(-relu(sigma_i) delta_i)
//   out_c = sum_i w_i v_ci        (v = sigmoid(raw) for rgb, raw for the logit fields, z for depth, 1 for acc)
//   G_i   = dL/dw_i = sum_c g_c v_ci + g_depth z_i + g_acc + g_w_i
//   dL/dv_ci = w_i g_c
//   dL/dsigma_i = [sigma_i > 0] delta_i (1 - alpha_i) ( G_i T_i - S_i / (1 - alpha_i + 1e-10) ),
//                 S_i = sum_{k>i} G_k w_k      (segmented reverse scan over the ray)
// sample_pdf's output is detached in the reference, so no gradient flows into z.
// Fixed (bbox-prior) fields have no learnable input.  Softmax-composited fields (sem_mode 1) are
// not differentiated here (forward-only option); the caller is told so.
#include "pnr_composite_dev.h"

struct CompositeBwdArgs {
    const float* raw; int64_t sc;          // channel-major: element (s, c) at raw[c*sc + s]
    const float* z; const float* rays; const float* noise;
    int64_t R; int N, C, K;
    const float *g_rgb, *g_depth, *g_acc, *g_sem, *g_inst, *g_w;   // upstream grads (any may be null)
    float* d_raw;                          // (4+C+K, R*N) channel-major
    // fixed (bbox-prior) fields: fix_x[c] = sum_i w_i [label_i == c]  =>  dL/dw_i += g_fix_x[label_i]
    const int32_t *label_sem, *label_inst; // (R,N), -1 = none; needed by g_fix_* and ce_*
    const float *g_fix_sem, *g_fix_inst;   // (R,C), (R,K) or null
    // per-sample 3D cross-entropy of the learned logits against the bbox labels (pnr_ce3d is its forward):
    // d_raw[c][s] += *ce_x * (softmax_c(raw_x[:, s]) - [c == label_s])  for 0 <= label_s < C (K): other labels are ignored
    const float *ce_sem, *ce_inst;         // device scalars (upstream gradient * weight / count) or null
    int sem_mode;                          // 0: logits are composited; 1: softmax(logits) per sample is composited
};

// one row's arithmetic at a time: without the fence hipcc interleaves the expf chains of a whole batch of rows (8 rows x 4 samples)
// for instruction-level parallelism and needs ~175 registers for it -- at the 128 the launch bound grants it spilled ~45 of them
#define BWD_ROW_FENCE __builtin_amdgcn_sched_barrier(0)
// Per ray-group width (SUB lanes per ray): waves per SIMD the launch bound asks for, logit rows per pipelined batch (two batches
// resident), rows in flight in the log-sum-exp / dot passes.  One ray per wave (N > 64: SUB >= 32) means R waves in all -- 4096 at the
// training batch, 16 per CU -- so the kernel is capped at 128 VGPRs (4 waves per SIMD: the launch is resident at once; at its
// natural 149 registers it ran in two rounds) and keeps little in flight; several rays per wave (N <= 64) means few waves and
// nothing to gain from the cap, so those instances keep 3 waves per SIMD and deeper batches.  Same box, 4096 rays, 45 + 32 fields,
// tools/composite_bwd_time.py (d_raw bit-identical throughout): N = 192  229 us before -> 168 (cap 4, 2 + 4 rows) / 176-179 (cap 4,
// 4 + 4 / 4 + 8 rows) / 192 (no cap, pipelined only);  N = 64  95 -> 77 (no cap, 4 + 8) / 84-86 (capped).
#ifndef BWD_WAVES
#define BWD_WAVES(SUB) ((SUB) >= 32 ? 4 : 3)
#endif
#ifndef BWD_PB_OF
#define BWD_PB_OF(SUB) ((SUB) >= 32 ? 2 : 4)
#endif
#ifndef BWD_CB_OF
#define BWD_CB_OF(SUB) ((SUB) >= 32 ? 4 : 8)
#endif

// SM: softmax compositing (sem_mode 1) -- a template parameter so that the default (logit compositing) instance carries neither
// the dot products nor their branches in its register budget
// Rng = PnrRngDev (pnr_composite_backward_rng): the forward's sigma noise regenerated from the in-kernel stream (k_composite's lane
// mapping, so lane q's four samples are one Philox block); the plain instances (empty pack) are the kernel as it was
template <int SUB, bool SM, class... Rng>
__global__ __launch_bounds__(256, BWD_WAVES(SUB)) void k_composite_bwd(CompositeBwdArgs a, const Rng... rng)
{
    constexpr bool RNG = sizeof...(Rng) > 0;
    constexpr int CB = BWD_CB_OF(SUB);      // channel rows in flight per lane (log-sum-exp / dot passes)
    constexpr int BWD_PB = BWD_PB_OF(SUB);  // logit rows per pipelined batch of the main pass
    RayLanes<SUB, 1> rl(a.R);               // the forward kernel's mapping: SUB lanes per ray x 4 samples per lane
    const int N = a.N, q = rl.q;
    PnrRngKey key;
    if constexpr (RNG) key = pnr_rng_key(rng...);

    const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;     // this wave, and the waves of the grid
    const int64_t step = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t grp = first; grp < rl.n_groups; grp += step) {
        rl.at(grp, a.R, N);
        const int64_t ray = rl.ray, rayc = rl.rayc, s0 = rl.s0;
        const bool active = rl.act[0];

        // ---- recompute alpha, T, w: k_composite's own chain and scan (pnr_composite_dev.h); only the product differs -- here
        // T = Tl excl first, since T is needed by itself
        const uint32_t ob = (uint32_t)s0 * 4u;          // byte offset of the lane's first sample in a row (R * N < 2^30: the launcher checks)
        const f4 zz = ld4o(a.z, ob, active);
        f4 sg = ld4o(a.raw + 3 * a.sc, ob, active);
        add_sigma_noise4<RNG>(sg.v, active, key, (uint32_t)ray, (uint32_t)q, a.noise, row_at(a.noise, ob));
        const float dn = ray_dir_norm(a.rays, rayc);
        const float znext = __shfl_down(zz.v[0], 1, 64);
        f4 alpha, dist, Tl;            // Tl: product of this lane's earlier factors
        float P = alpha_chain<4>(zz.v, znext, sg.v, rl.i0, N, dn, alpha.v, Tl.v, dist.v);
        if (!active) P = 1.0f;
        const float excl = scan_excl_shfl<SUB>(P, q);
        f4 T, w;
#pragma unroll
        for (int k = 0; k < 4; ++k) { T.v[k] = Tl.v[k] * excl; w.v[k] = active ? alpha.v[k] * T.v[k] : 0.0f; }

        // ---- G_i and the per-channel value gradients (one pass over the channel rows)
        f4 G;
        {
            const float gd = a.g_depth ? a.g_depth[rayc] : 0.0f, ga = a.g_acc ? a.g_acc[rayc] : 0.0f;
            const f4 gw = a.g_w ? ld4o(a.g_w, ob, active) : f4{{0, 0, 0, 0}};
#pragma unroll
            for (int k = 0; k < 4; ++k) G.v[k] = fmaf(gd, zz.v[k], ga) + gw.v[k];
        }
        int ls[4], li[4];
        ld4_labels(a.label_sem + s0, a.label_sem && active, ls);
        ld4_labels(a.label_inst + s0, a.label_inst && active, li);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (a.g_fix_sem && ls[k] >= 0 && ls[k] < a.C) G.v[k] += a.g_fix_sem[rayc * a.C + ls[k]];
            if (a.g_fix_inst && li[k] >= 0 && li[k] < a.K) G.v[k] += a.g_fix_inst[rayc * a.K + li[k]];
        }
        // 3D cross-entropy: per-sample log-sum-exp of each learned field (one extra pass over its channel rows)
        const float ces = (a.ce_sem && a.label_sem) ? *a.ce_sem : 0.0f, cei = (a.ce_inst && a.label_inst) ? *a.ce_inst : 0.0f;
        f4 mx_s, den_s, mx_i, den_i;
        auto lse = [&](int nch, int ch0, f4& mx, f4& den) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { mx.v[k] = -INFINITY; den.v[k] = 0.0f; }
            // CB channel rows requested before the first is consumed: with 4 waves per SIMD and one 1 KiB load in flight per
            // wave the pass ran at ~2 TB/s (4096 rays = 16 waves per CU)
            for (int c0 = 0; c0 < nch; c0 += CB) {
                f4 v[CB];
#pragma unroll
                for (int j = 0; j < CB; ++j) v[j] = ld4o(a.raw + (int64_t)(ch0 + (c0 + j < nch ? c0 + j : nch - 1)) * a.sc, ob, active);
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    if (c0 + j >= nch) break;
#pragma unroll
                    for (int k = 0; k < 4; ++k) lse_step(mx.v[k], den.v[k], v[j].v[k]);     // k_ce3d's step: this is its gradient
                    BWD_ROW_FENCE;
                }
            }
        };
        // The 3D term touches labelled samples only, and most rays cross no box at all: a wave none of whose samples carries a
        // label skips the pass (wave-uniform; mx / den are then never read -- the `lab < 0` guard below).  The pass is a read of
        // every logit row plus two expf per value: at 4096 rays (16 waves per CU, one ray group each) it was half the kernel.
        bool lab_s = false, lab_i = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) { lab_s |= ls[k] >= 0 && ls[k] < a.C; lab_i |= li[k] >= 0 && li[k] < a.K; }
        const bool wave_s = __builtin_amdgcn_ballot_w64(lab_s) != 0, wave_i = __builtin_amdgcn_ballot_w64(lab_i) != 0;
        if ((ces != 0.0f && wave_s) || (SM && a.g_sem)) lse(a.C, 4, mx_s, den_s);
        if ((cei != 0.0f && wave_i) || (SM && a.g_inst)) lse(a.K, 4 + a.C, mx_i, den_i);
        // softmax compositing: map_c = sum_i w_i s_{i,c}, s = softmax(x_i).  Needs dot_i = sum_c g_c s_{i,c}:
        //   dL/dw_i += dot_i,   d x_{i,c} = w_i s_{i,c} (g_c - dot_i)
        f4 dot_s = {{0, 0, 0, 0}}, dot_i = {{0, 0, 0, 0}};
        auto gdot = [&](int nch, int ch0, const float* gp, const f4& mx, const f4& den, f4& dot) {
            for (int c0 = 0; c0 < nch; c0 += CB) {
                f4 v[CB];
#pragma unroll
                for (int j = 0; j < CB; ++j) v[j] = ld4o(a.raw + (int64_t)(ch0 + (c0 + j < nch ? c0 + j : nch - 1)) * a.sc, ob, active);
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    if (c0 + j >= nch) break;
                    const float gc = gp[rayc * nch + c0 + j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) dot.v[k] = fmaf(gc, softmax_of(v[j].v[k], mx.v[k], den.v[k]), dot.v[k]);
                }
            }
        };
        if (SM && a.g_sem) gdot(a.C, 4, a.g_sem, mx_s, den_s, dot_s);
        if (SM && a.g_inst) gdot(a.K, 4 + a.C, a.g_inst, mx_i, den_i, dot_i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gc = a.g_rgb ? a.g_rgb[rayc * 3 + c] : 0.0f;
            const f4 r = ld4o(a.raw + (int64_t)c * a.sc, ob, active);
            f4 dr;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = sigmoid_of(r.v[k]);
                G.v[k] = fmaf(gc, v, G.v[k]);
                dr.v[k] = w.v[k] * gc * v * (1.0f - v);
            }
            st4o(a.d_raw + (int64_t)c * a.sc, ob, dr, active);
        }
        const int CK = a.C + a.K;
        // The logit rows, BWD_PB rows per batch, software-pipelined: the next batch's loads are issued BEFORE this batch's
        // stores.  vmcnt is one in-order counter for loads and stores on this part, so a load issued behind a store is not seen
        // as landed until the store is acknowledged -- with the loads in front, the wait the compiler emits is a counted one
        // that leaves the stores in flight.  (One ray group per wave and 16 waves per CU at 4096 rays: the kernel is a chain of
        // memory round trips, not a bandwidth problem.)
        auto fetch_rows = [&](int c0, f4 (&rb)[BWD_PB], float (&gcb)[BWD_PB]) {
#pragma unroll
            for (int j = 0; j < BWD_PB; ++j) {
                const int c = c0 + j < CK ? c0 + j : CK - 1;
                const bool is_s = c < a.C;
                const float* gp = is_s ? a.g_sem : a.g_inst;
                gcb[j] = gp ? gp[rayc * (is_s ? a.C : a.K) + (is_s ? c : c - a.C)] : 0.0f;
                rb[j] = ld4o(a.raw + (int64_t)(4 + c) * a.sc, ob, active);
            }
        };
        auto do_rows = [&](int c0, const f4 (&rb)[BWD_PB], const float (&gcb)[BWD_PB]) {
#pragma unroll
            for (int j = 0; j < BWD_PB; ++j) {
                const int c = c0 + j;
                if (c >= CK) break;
                const bool is_s = c < a.C;
                const float* gp = is_s ? a.g_sem : a.g_inst;
                const float gc = gcb[j];
                const f4 r = rb[j];
                f4 dr;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (SM && gp) {
                        const float sc = softmax_of(r.v[k], is_s ? mx_s.v[k] : mx_i.v[k], is_s ? den_s.v[k] : den_i.v[k]);
                        dr.v[k] = w.v[k] * sc * (gc - (is_s ? dot_s.v[k] : dot_i.v[k]));
                    } else {
                        G.v[k] = fmaf(gc, r.v[k], G.v[k]);
                        dr.v[k] = w.v[k] * gc;
                    }
                }
                const float ce = is_s ? ces : cei;
                if (ce != 0.0f) {
                    const int cc = is_s ? c : c - a.C;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int lab = is_s ? ls[k] : li[k];
                        if (lab < 0 || lab >= (is_s ? a.C : a.K)) continue;
                        const float pc = softmax_of(r.v[k], is_s ? mx_s.v[k] : mx_i.v[k], is_s ? den_s.v[k] : den_i.v[k]);
                        dr.v[k] += ce * (pc - (lab == cc ? 1.0f : 0.0f));
                    }
                }
                st4o(a.d_raw + (int64_t)(4 + c) * a.sc, ob, dr, active);
                BWD_ROW_FENCE;
            }
        };
        {
            f4 rbA[BWD_PB], rbB[BWD_PB];
            float gA[BWD_PB], gB[BWD_PB];
            if (CK > 0) fetch_rows(0, rbA, gA);
            for (int c0 = 0; c0 < CK; c0 += 2 * BWD_PB) {
                if (c0 + BWD_PB < CK) fetch_rows(c0 + BWD_PB, rbB, gB);
                do_rows(c0, rbA, gA);
                if (c0 + BWD_PB >= CK) break;
                if (c0 + 2 * BWD_PB < CK) fetch_rows(c0 + 2 * BWD_PB, rbA, gA);
                do_rows(c0 + BWD_PB, rbB, gB);
            }
        }

        if (SM) {
#pragma unroll
            for (int k = 0; k < 4; ++k) G.v[k] += dot_s.v[k] + dot_i.v[k];
        }
        // ---- S_i = sum_{k>i} G_k w_k : lane-local suffix, then a segmented reverse (suffix) scan over lanes
        f4 gwk;
#pragma unroll
        for (int k = 0; k < 4; ++k) gwk.v[k] = active ? G.v[k] * w.v[k] : 0.0f;
        const float lane_tot = (gwk.v[0] + gwk.v[1]) + (gwk.v[2] + gwk.v[3]);
        float y = lane_tot;                 // inclusive suffix sum over lanes q..SUB-1 of the group
#pragma unroll
        for (int d = 1; d < SUB; d <<= 1) {
            const float t = __shfl_down(y, d, 64);
            if (q + d < SUB) y += t;
        }
        float after = __shfl_down(y, 1, 64);     // sum over the lanes after this one
        if (q == SUB - 1) after = 0.0f;
        f4 S;
        S.v[3] = after;
        S.v[2] = S.v[3] + gwk.v[3];
        S.v[1] = S.v[2] + gwk.v[2];
        S.v[0] = S.v[1] + gwk.v[1];
        f4 ds;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float om = 1.0f - alpha.v[k];
            const float dalpha = G.v[k] * T.v[k] - S.v[k] / alpha_factor(alpha.v[k]);
            ds.v[k] = (sg.v[k] > 0.0f) ? dist.v[k] * om * dalpha : 0.0f;
        }
        st4o(a.d_raw + 3 * a.sc, ob, ds, active);
    }
}

static int composite_backward_impl(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                                   const float* noise, int64_t n_rays, int n_samples, int n_sem, int n_inst, int sem_mode,
                                   const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                                   const float* g_inst, const float* g_weights, const int32_t* label_sem,
                                   const int32_t* label_inst, const float* g_fix_sem, const float* g_fix_inst,
                                   const float* ce_sem, const float* ce_inst, float* d_raw, void* stream, const PnrRngDev* rng = nullptr)
{
    PNR_REQUIRE(n_samples >= 4 && n_samples <= 256 && (n_samples % 4) == 0,
                "pnr_composite_backward: n_samples=%d must be a multiple of 4 in [4,256]", n_samples);
    if (n_rays <= 0) return PNR_OK;
    PNR_REQUIRE(n_rays * (int64_t)n_samples < ((int64_t)1 << 30), "pnr_composite_backward: R*N=%lld must stay below 2^30 (32-bit byte "
                "offsets inside a channel row): split the batch", (long long)(n_rays * (int64_t)n_samples));
    PNR_REQUIRE(raw && z && rays && d_raw, "pnr_composite_backward: null pointer");
    PNR_REQUIRE((raw_stride_c % 4) == 0 && (((uintptr_t)raw | (uintptr_t)d_raw | (uintptr_t)z | (uintptr_t)noise |
                                            (uintptr_t)g_weights | (uintptr_t)label_sem | (uintptr_t)label_inst) & 15) == 0,
                "pnr_composite_backward: channel-major, 16-byte aligned images required");
    PNR_REQUIRE((!g_fix_sem && !ce_sem) || label_sem, "pnr_composite_backward: g_fix_sem / ce_sem need label_sem");
    PNR_REQUIRE((!g_fix_inst && !ce_inst) || label_inst, "pnr_composite_backward: g_fix_inst / ce_inst need label_inst");
    CompositeBwdArgs a;
    a.raw = raw; a.sc = raw_stride_c; a.z = z; a.rays = rays; a.noise = noise; a.R = n_rays; a.N = n_samples;
    a.C = n_sem; a.K = n_inst; a.g_rgb = g_rgb; a.g_depth = g_depth; a.g_acc = g_acc; a.g_sem = g_sem; a.g_inst = g_inst;
    a.g_w = g_weights; a.d_raw = d_raw;
    a.label_sem = label_sem; a.label_inst = label_inst; a.g_fix_sem = g_fix_sem; a.g_fix_inst = g_fix_inst;
    a.ce_sem = ce_sem; a.ce_inst = ce_inst; a.sem_mode = sem_mode;
    int sub = 1;
    while (sub < n_samples / 4) sub <<= 1;
    const int rpw = 64 / sub;
    const int64_t n_groups = (n_rays + rpw - 1) / rpw;
    const int grid = pnr_grid_cap((n_groups + 3) / 4, 8);
    hipStream_t st = (hipStream_t)stream;
    composite_dispatch<1, 2, 4, 8, 16, 32, 64>(sub, true, sem_mode, rng, [&](auto S, auto, auto SM, const auto&... r) {
        hipLaunchKernelGGL((k_composite_bwd<decltype(S)::value, decltype(SM)::value, std::decay_t<decltype(r)>...>), dim3(grid), dim3(256), 0, st,
                           a, r...);
    });
    PNR_CHECK_LAUNCH("pnr_composite_backward");
    return PNR_OK;
}

PNR_EXPORT int pnr_composite_backward(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                                      const float* noise, int64_t n_rays, int n_samples, int n_sem, int n_inst,
                                      const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                                      const float* g_inst, const float* g_weights, float* d_raw, void* stream)
{
    return composite_backward_impl(raw, raw_stride_c, z, rays, noise, n_rays, n_samples, n_sem, n_inst, 0, g_rgb, g_depth, g_acc, g_sem,
                                   g_inst, g_weights, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_raw, stream);
}

PNR_EXPORT int pnr_composite_backward2(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                                       const float* noise, int64_t n_rays, int n_samples, int n_sem, int n_inst,
                                       const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                                       const float* g_inst, const float* g_weights, const int32_t* label_sem,
                                       const int32_t* label_inst, const float* g_fix_sem, const float* g_fix_inst,
                                       const float* ce_sem, const float* ce_inst, float* d_raw, void* stream)
{
    return composite_backward_impl(raw, raw_stride_c, z, rays, noise, n_rays, n_samples, n_sem, n_inst, 0, g_rgb, g_depth, g_acc, g_sem,
                                   g_inst, g_weights, label_sem, label_inst, g_fix_sem, g_fix_inst, ce_sem, ce_inst, d_raw, stream);
}

PNR_EXPORT int pnr_composite_backward3(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                                       const float* noise, int64_t n_rays, int n_samples, int n_sem, int n_inst, int sem_mode,
                                       const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                                       const float* g_inst, const float* g_weights, const int32_t* label_sem,
                                       const int32_t* label_inst, const float* g_fix_sem, const float* g_fix_inst,
                                       const float* ce_sem, const float* ce_inst, float* d_raw, void* stream)
{
    PNR_REQUIRE(sem_mode == 0 || sem_mode == 1, "pnr_composite_backward: sem_mode must be 0 (logits) or 1 (softmax)");
    return composite_backward_impl(raw, raw_stride_c, z, rays, noise, n_rays, n_samples, n_sem, n_inst, sem_mode, g_rgb, g_depth, g_acc,
                                   g_sem, g_inst, g_weights, label_sem, label_inst, g_fix_sem, g_fix_inst, ce_sem, ce_inst, d_raw, stream);
}

PNR_EXPORT int pnr_composite_backward_rng(const float* raw, int64_t raw_stride_c, const float* z, const float* rays,
                                          const pnr_rng* noise_host, int64_t n_rays, int n_samples, int n_sem, int n_inst, int sem_mode,
                                          const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_sem,
                                          const float* g_inst, const float* g_weights, const int32_t* label_sem,
                                          const int32_t* label_inst, const float* g_fix_sem, const float* g_fix_inst,
                                          const float* ce_sem, const float* ce_inst, float* d_raw, void* stream)
{
    PnrRngDev rng;
    const int rc = pnr_rng_check(noise_host, n_rays < 0 ? 0 : n_rays, "pnr_composite_backward_rng", &rng);
    if (rc) return rc;
    PNR_REQUIRE(sem_mode == 0 || sem_mode == 1, "pnr_composite_backward_rng: sem_mode must be 0 (logits) or 1 (softmax)");
    return composite_backward_impl(raw, raw_stride_c, z, rays, nullptr, n_rays, n_samples, n_sem, n_inst, sem_mode, g_rgb, g_depth, g_acc,
                                   g_sem, g_inst, g_weights, label_sem, label_inst, g_fix_sem, g_fix_inst, ce_sem, ce_inst, d_raw, stream,
                                   &rng);
}
