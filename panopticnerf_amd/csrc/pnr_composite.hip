// K4: raw2outputs -- transmittance / alpha-compositing scan of RGB, depth, acc and the
// panoptic (semantic / instance) logit and fixed-field maps.  SURVEY.md 8a row a6; the
// reference function is raw2outputs in lib/networks/renderer (branch not in the mount, see
// include/pnr.h).  HBM-bound: every (sigma, rgb, logit) value is read exactly once.
//
// Mapping (wave64): a ray of N samples (N % 4 == 0, N <= 256) is owned by a group of
// SUB = pow2ceil(N/4) consecutive lanes (compile-time), each lane holding 4 consecutive samples,
// so with the channel-major raw image written by the MLP kernel every channel row of a ray group
// is one 16 B-per-lane coalesced load (N=64: 4 rays per wave, 1 KiB per wave-load; N=192: one ray
// per wave, 768 B).
//   * T(t): segmented (width SUB) wave-level inclusive product scan of the per-lane products of
//     (1 - alpha + 1e-10) -- the "wavefront-level prefix sum" of BASELINE.json's north_star.
//   * channel sums: 8 channel rows per batch; the NEXT batch's 8 loads are issued before the
//     current batch is reduced, so >= 6 KiB per wave stays in flight through the butterflies.
//   * fixed (bbox-prior) fields: a per-ray histogram of the sample labels in LDS, accumulated
//     in 2^-30 fixed point with integer ds_add (associative => bit-reproducible whatever the
//     order), instead of one compare-select reduction per class.
// Nothing is re-read, so samples are staged in registers, not LDS: there is no reuse for LDS
// to serve (cdna_hip_programming.md common mistake 7).
// The pieces the kernels below are assembled from (rows, ray-group prologue, sigma noise, alpha chain, scans, the fixed-field
// histogram, log-sum-exp, row store, host dispatch) are pnr_composite_dev.h's, shared with the backward kernel.
#include "pnr_composite_dev.h"

struct CompositeArgs {
    const float* raw; int64_t stride_s, stride_c;
    const float* z; const float* rays; const float* noise;
    const int32_t* label_sem; const int32_t* label_inst;
    int64_t R; int N, C, K, sem_mode, white_bkgd;
    float *rgb, *depth, *acc, *weights, *sem, *inst, *fix_sem, *fix_inst;
    int use_hist;       // 1: LDS histogram for the fixed fields (fits in LDS), 0: reduction fallback
};

#ifndef CMP_GRID_PER_CU
#define CMP_GRID_PER_CU 8      /* resident 256-thread workgroups per CU the grid is capped at (grid-stride over the rest) */
#endif
#ifndef CMP_UB
#define CMP_UB 8        // channel rows per batch
#endif

__device__ __forceinline__ float dot4(const f4& w, const f4& v)
{
    return fmaf(w.v[3], v.v[3], fmaf(w.v[2], v.v[2], fmaf(w.v[1], v.v[1], w.v[0] * v.v[0])));
}

// Rng = PnrRngDev (pnr_composite_rng): the sigma noise is the in-kernel stream's -- lane q of a ray holds samples 4 q .. 4 q + 3 =
// one Philox block; the plain instances (empty pack) are the kernel as it was
template <bool CH_MAJOR, int SUB, bool SOFTMAX, class... Rng>
__global__ __launch_bounds__(256) void k_composite(CompositeArgs a, const Rng... rng)
{
    constexpr bool RNG = sizeof...(Rng) > 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];   // [4 waves][RPW][C+K] when use_hist
    RayLanes<SUB, 1> rl(a.R);              // SUB lanes per ray x 4 samples per lane
    const int wave = threadIdx.x >> 6;
    const int N = a.N, q = rl.q;
    const int CK = a.C + a.K;
    const int nq = 3 + CK;                 // composited raw channels: rgb, semantic, instance (sigma excluded)
    uint32_t* hist = s_hist + ((size_t)wave * rl.RPW + rl.g) * CK;
    PnrRngKey key;
    if constexpr (RNG) key = pnr_rng_key(rng...);

    const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;     // this wave, and the waves of the grid
    const int64_t step = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t grp = first; grp < rl.n_groups; grp += step) {
        rl.at(grp, a.R, N);
        const int64_t ray = rl.ray, s0 = rl.s0;
        const bool active = rl.act[0];
        const bool writer = active && q == 0;

        // ---- phase 1: weights.  z and sigma of a ray group are the head of the dependent chain (load -> exp -> scan -> weights)
        const f4 zz = ld4(a.z + s0, active);
        f4 sg = load4<CH_MAJOR>(a.raw, a.stride_s, a.stride_c, s0, 3, active);
        // first batch of channel rows: in flight while the weights are computed
        f4 nxt[CMP_UB];
#pragma unroll
        for (int j = 0; j < CMP_UB; ++j) nxt[j] = load4<CH_MAJOR>(a.raw, a.stride_s, a.stride_c, s0, j < 3 ? j : j + 1, active && j < nq);
        add_sigma_noise4<RNG>(sg.v, active, key, (uint32_t)ray, (uint32_t)q, a.noise, a.noise + s0);
        const float dn = ray_dir_norm(a.rays, rl.rayc);
        const float znext = __shfl_down(zz.v[0], 1, 64);   // first sample of the next lane
        f4 alpha, Tl, w;
        float P = alpha_chain<4>(zz.v, znext, sg.v, rl.i0, N, dn, alpha.v, Tl.v);
        if (!active) P = 1.0f;
        const float excl = scan_excl_shfl<SUB>(P, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) w.v[k] = active ? (alpha.v[k] * Tl.v[k]) * excl : 0.0f;
        if (a.weights) st4(a.weights + s0, w.v, active);
        const float accv = group_sum<SUB>((w.v[0] + w.v[1]) + (w.v[2] + w.v[3]));
        const float depv = group_sum<SUB>(dot4(w, zz));
        if (writer) {
            if (a.depth) a.depth[ray] = depv;
            if (a.acc) a.acc[ray] = accv;
        }

        // ---- fixed (bbox-prior) fields
        const bool want_fs = a.fix_sem && a.label_sem && a.C, want_fi = a.fix_inst && a.label_inst && a.K;
        if (want_fs || want_fi) {
            int ls[4], li[4];
            ld4_labels(a.label_sem + s0, active && want_fs, ls);
            ld4_labels(a.label_inst + s0, active && want_fi, li);
            if (a.use_hist) {
                hist_zero<SUB>(hist, q, CK);
#pragma unroll
                for (int k = 0; k < 4; ++k) hist_add(hist, w.v[k], want_fs, ls[k], a.C, want_fi, li[k], a.K);
                if (rl.valid) hist_store<SUB>(hist, q, ray, want_fs, a.fix_sem, a.C, want_fi, a.fix_inst, a.K);
            } else {
                // the histogram does not fit LDS: one compare-select reduction per class
                for (int c = 0; c < CK; ++c) {
                    const bool is_s = c < a.C;
                    if ((is_s && !want_fs) || (!is_s && !want_fi)) continue;
                    const int cc = is_s ? c : c - a.C;
                    float p = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) p += ((is_s ? ls[k] : li[k]) == cc) ? w.v[k] : 0.0f;
                    const float r = group_sum<SUB>(p);
                    if (writer) (is_s ? a.fix_sem : a.fix_inst)[ray * (is_s ? a.C : a.K) + cc] = r;
                }
            }
        }

        // ---- softmax mode: per-sample max / denominator of each learned field (extra pass over its rows)
        f4 mx_s, den_s, mx_i, den_i;
        if constexpr (SOFTMAX) {
            auto field_stats = [&](int nch, int ch0, f4& mx, f4& den) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { mx.v[k] = -INFINITY; den.v[k] = 0.0f; }
                for (int c = 0; c < nch; ++c) {
                    const f4 v = load4<CH_MAJOR>(a.raw, a.stride_s, a.stride_c, s0, ch0 + c, active);
#pragma unroll
                    for (int k = 0; k < 4; ++k) lse_step(mx.v[k], den.v[k], v.v[k]);
                }
            };
            field_stats(a.C, 4, mx_s, den_s);
            field_stats(a.K, 4 + a.C, mx_i, den_i);
        }

        // ---- phase 2: all composited channels, CMP_UB rows per batch.  Each row's weighted partial sum is
        // taken as soon as the row is used and its register is immediately re-armed with the row of the NEXT
        // batch, so 8 loads (6-8 KiB per wave) are in flight through the butterflies below.
#pragma unroll 1
        for (int q0 = 0; q0 < nq; q0 += CMP_UB) {
            float r[CMP_UB];
            const bool more = q0 + CMP_UB < nq;
#pragma unroll
            for (int j = 0; j < CMP_UB; ++j) {
                const int qq = q0 + j;
                f4 v = nxt[j];
                if (qq < 3) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v.v[k] = sigmoid_of(v.v[k]);
                } else if constexpr (SOFTMAX) {
                    const bool fs = (qq - 3) < a.C;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v.v[k] = softmax_of(v.v[k], fs ? mx_s.v[k] : mx_i.v[k], fs ? den_s.v[k] : den_i.v[k]);
                }
                r[j] = dot4(w, v);
                const int q2 = qq + CMP_UB;               // >= 8 > 3: never an rgb row -> raw channel q2 + 1
                if (more) nxt[j] = load4<CH_MAJOR>(a.raw, a.stride_s, a.stride_c, s0, q2 + 1, active && q2 < nq);
            }
            group_sum_batch<SUB, CMP_UB>(r);
            if (writer) store_rows<CMP_UB>(a, ray, q0, nq, r, accv);
        }
    }
}

// ------------------------------------------------------------------------------- second mapping (channel-major raw)
// L lanes per ray x M = 4*M4 CONSECUTIVE samples per lane (N <= L*M): the weighted partial sum is M FMAs per lane, and
// both the transmittance scan and the per-ray sums stay inside a 16-lane DPP row (row_shr / quad_perm / row_mirror: no
// LDS crossbar, no bpermute); CMP2_UB rows (x M4 loads) are in flight per wave through the reductions.
// Measured on MI355X against the 4-samples-per-lane mapping above, same process and buffers (tools/composite_ab.py,
// profiles/README.md): N = 64 as 8 lanes x 8 samples (8 rays per wave): +1..3 % -> used for 32 < N <= 64;
// N = 192 as 16 lanes x 12 samples (every lane busy, ~3x fewer issued instructions per byte): -1..-4 % at 4 or 8 rows
// in flight, -9 % at 2 -> NOT used there: at N = 192 the kernel is bound by what HBM delivers for 768-byte pieces, not
// by instruction issue.  So only <8, 2> is instantiated (for N in 36..64, M4 is always 2).
#ifndef CMP2_UB
#define CMP2_UB 8
#endif

// Rng = PnrRngDev: lane q's samples i0 + 4 j + k (i0 = q M, a multiple of 4) take word k of Philox block i0 / 4 + j
template <int L, int M4, bool SOFTMAX, class... Rng>
__global__ __launch_bounds__(256) void k_composite2(CompositeArgs a, const Rng... rng)
{
    constexpr bool RNG = sizeof...(Rng) > 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];   // [4 waves][RPW][C+K] when use_hist
    constexpr int M = 4 * M4;
    RayLanes<L, M4> rl(a.R);
    const int wave = threadIdx.x >> 6;
    const int N = a.N, q = rl.q, i0 = rl.i0;
    const int CK = a.C + a.K;
    const int nq = 3 + CK;
    uint32_t* hist = s_hist + ((size_t)wave * rl.RPW + rl.g) * CK;
    const int64_t sc = a.stride_c;
    PnrRngKey key;
    if constexpr (RNG) key = pnr_rng_key(rng...);

    const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;     // this wave, and the waves of the grid
    const int64_t step = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t grp = first; grp < rl.n_groups; grp += step) {
        rl.at(grp, a.R, N);
        const int64_t ray = rl.ray, s0 = rl.s0;
        const bool (&act)[M4] = rl.act;
        const bool writer = rl.valid && q == 0;

        // ---- phase 1: weights
        float zz[M], w[M];
        ld_row<M4>(a.z + s0, act, zz);
        ld_row<M4>(a.raw + 3 * sc + s0, act, w);                  // sigma, becomes the weights below
        float nxt[CMP2_UB][M];
#pragma unroll
        for (int j = 0; j < CMP2_UB; ++j) {
            if (j < nq) ld_row<M4>(a.raw + (int64_t)(j < 3 ? j : j + 1) * sc + s0, act, nxt[j]);
        }
#pragma unroll
        for (int j = 0; j < M4; ++j)
            add_sigma_noise4<RNG>(w + 4 * j, act[j], key, (uint32_t)ray, (uint32_t)((i0 >> 2) + j), a.noise, a.noise + s0 + 4 * j);
        const float dn = ray_dir_norm(a.rays, rl.rayc);
        const float znext = dpp_or<0x101>(zz[0], 0.0f);           // row_shl:1 -- first sample of the next lane
        float alpha[M], Tl[M];
        float P = alpha_chain<M>(zz, znext, w, i0, N, dn, alpha, Tl);
        if (!act[0]) P = 1.0f;
        const float excl = scan_excl_dpp<L>(P, q);
        float accp = 0.0f, depp = 0.0f;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            w[k] = act[k >> 2] ? (alpha[k] * Tl[k]) * excl : 0.0f;
            accp += w[k];
            depp = fmaf(w[k], zz[k], depp);
        }
        if (a.weights) {
#pragma unroll
            for (int j = 0; j < M4; ++j) st4(a.weights + s0 + 4 * j, w + 4 * j, act[j]);
        }
        const float accv = group_sum<L>(accp);
        const float depv = group_sum<L>(depp);
        if (writer) {
            if (a.depth) a.depth[ray] = depv;
            if (a.acc) a.acc[ray] = accv;
        }

        // ---- fixed (bbox-prior) fields: always the histogram here (composite_impl sends a ray whose bins do not fit to k_composite)
        const bool want_fs = a.fix_sem && a.label_sem && a.C, want_fi = a.fix_inst && a.label_inst && a.K;
        if (want_fs || want_fi) {
            hist_zero<L>(hist, q, CK);
#pragma unroll
            for (int j = 0; j < M4; ++j) {
                int ls[4], li[4];
                ld4_labels(a.label_sem + s0 + 4 * j, act[j] && want_fs, ls);
                ld4_labels(a.label_inst + s0 + 4 * j, act[j] && want_fi, li);
#pragma unroll
                for (int k = 0; k < 4; ++k) hist_add(hist, w[4 * j + k], want_fs, ls[k], a.C, want_fi, li[k], a.K);
            }
            if (rl.valid) hist_store<L>(hist, q, ray, want_fs, a.fix_sem, a.C, want_fi, a.fix_inst, a.K);
        }

        // ---- softmax mode: per-sample max / denominator of each learned field (extra pass over its rows)
        float mx_s[SOFTMAX ? M : 1], den_s[SOFTMAX ? M : 1], mx_i[SOFTMAX ? M : 1], den_i[SOFTMAX ? M : 1];
        if constexpr (SOFTMAX) {
            auto field_stats = [&](int nch, int ch0, float (&mx)[M], float (&den)[M]) {
#pragma unroll
                for (int k = 0; k < M; ++k) { mx[k] = -INFINITY; den[k] = 0.0f; }
                for (int c = 0; c < nch; ++c) {
                    float v[M];
                    ld_row<M4>(a.raw + (int64_t)(ch0 + c) * sc + s0, act, v);
#pragma unroll
                    for (int k = 0; k < M; ++k) lse_step(mx[k], den[k], v[k]);
                }
            };
            field_stats(a.C, 4, mx_s, den_s);
            field_stats(a.K, 4 + a.C, mx_i, den_i);
        }

        // ---- phase 2: every composited channel, CMP2_UB rows per batch; a row's registers are re-armed with the row of
        // the next batch as soon as its partial sum is taken
#pragma unroll 1
        for (int q0 = 0; q0 < nq; q0 += CMP2_UB) {
            float r[CMP2_UB];
#pragma unroll
            for (int j = 0; j < CMP2_UB; ++j) {
                const int qq = q0 + j;
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    float v = nxt[j][k];
                    if (qq < 3) v = sigmoid_of(v);
                    else if constexpr (SOFTMAX) {
                        const bool fs = (qq - 3) < a.C;
                        v = softmax_of(v, fs ? mx_s[k] : mx_i[k], fs ? den_s[k] : den_i[k]);
                    }
                    acc = fmaf(w[k], v, acc);
                }
                r[j] = acc;
                const int q2 = qq + CMP2_UB;                     // >= 4 > 3: never an rgb row -> raw channel q2 + 1
                if (q2 < nq) ld_row<M4>(a.raw + (int64_t)(q2 + 1) * sc + s0, act, nxt[j]);
            }
            group_sum_batch<L, CMP2_UB>(r);
            if (writer) store_rows<CMP2_UB>(a, ray, q0, nq, r, accv);
        }
    }
}

static int composite_impl(const float* raw, int64_t raw_stride_s, int64_t raw_stride_c, const float* z, const float* rays,
                          const float* noise, const PnrRngDev* rng, const int32_t* label_sem, const int32_t* label_inst, int64_t n_rays,
                          int n_samples, int n_sem, int n_inst, int sem_mode, int white_bkgd, float* rgb, float* depth, float* acc,
                          float* weights, float* sem, float* inst, float* fix_sem, float* fix_inst, void* stream)
{
    PNR_REQUIRE(n_rays <= 0 || (raw && z && rays), "pnr_composite: null pointer");
    PNR_REQUIRE(n_samples >= 4 && n_samples <= 256 && (n_samples % 4) == 0,
                "pnr_composite: n_samples=%d must be a multiple of 4 in [4,256]", n_samples);
    PNR_REQUIRE(n_sem >= 0 && n_inst >= 0 && (sem_mode == 0 || sem_mode == 1), "pnr_composite: bad field sizes");
    PNR_REQUIRE((((uintptr_t)z) & 15) == 0, "pnr_composite: z must be 16-byte aligned");
    PNR_REQUIRE(!weights || (((uintptr_t)weights) & 15) == 0, "pnr_composite: weights must be 16-byte aligned");
    PNR_REQUIRE((((uintptr_t)noise) & 15) == 0 && (((uintptr_t)label_sem) & 15) == 0 && (((uintptr_t)label_inst) & 15) == 0,
                "pnr_composite: noise / label arrays must be 16-byte aligned");
    if (n_rays <= 0) return PNR_OK;
    CompositeArgs a;
    a.raw = raw; a.stride_s = raw_stride_s; a.stride_c = raw_stride_c; a.z = z; a.rays = rays; a.noise = noise;
    a.label_sem = label_sem; a.label_inst = label_inst; a.R = n_rays; a.N = n_samples; a.C = n_sem; a.K = n_inst;
    a.sem_mode = sem_mode; a.white_bkgd = white_bkgd; a.rgb = rgb; a.depth = depth; a.acc = acc; a.weights = weights;
    a.sem = sem; a.inst = inst; a.fix_sem = fix_sem; a.fix_inst = fix_inst;
    const bool want_fix = (fix_sem && label_sem && n_sem) || (fix_inst && label_inst && n_inst);
    const bool ch_major = raw_stride_s == 1 && (raw_stride_c % 4) == 0 && (((uintptr_t)raw) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    // per-ray histograms of a 4-wave workgroup with `rpw` rays per wave
    auto hist_bytes = [&](int rpw) { return (size_t)4 * rpw * (n_sem + n_inst) * sizeof(uint32_t); };
    auto grid_for = [&](int rpw) { return pnr_grid_cap(((n_rays + rpw - 1) / rpw + 3) / 4, CMP_GRID_PER_CU); };
    // second mapping (8 lanes x 8 consecutive samples per lane): channel-major images with 33..64 samples per ray, when the
    // histogram fits LDS (the reduction fallback exists only in k_composite)
    if (ch_major && n_samples > 32 && n_samples <= 64 && (!want_fix || hist_bytes(8) <= 48 * 1024)) {
        a.use_hist = want_fix ? 1 : 0;
        const size_t lds = want_fix ? hist_bytes(8) : 0;
        composite_dispatch<8>(8, true, sem_mode, rng, [&](auto L, auto, auto SM, const auto&... r) {
            hipLaunchKernelGGL((k_composite2<decltype(L)::value, 2, decltype(SM)::value, std::decay_t<decltype(r)>...>), dim3(grid_for(8)), dim3(256),
                               lds, st, a, r...);
        });
        PNR_CHECK_LAUNCH("pnr_composite");
        return PNR_OK;
    }
    int sub = 1;
    while (sub < n_samples / 4) sub <<= 1;
    const int rpw = 64 / sub;
    a.use_hist = (want_fix && hist_bytes(rpw) <= 48 * 1024) ? 1 : 0;
    const size_t lds = a.use_hist ? hist_bytes(rpw) : 0;
    composite_dispatch<1, 2, 4, 8, 16, 32, 64>(sub, ch_major, sem_mode, rng, [&](auto S, auto CH, auto SM, const auto&... r) {
        hipLaunchKernelGGL((k_composite<decltype(CH)::value, decltype(S)::value, decltype(SM)::value, std::decay_t<decltype(r)>...>),
                           dim3(grid_for(rpw)), dim3(256), lds, st, a, r...);
    });
    PNR_CHECK_LAUNCH("pnr_composite");
    return PNR_OK;
}

PNR_EXPORT int pnr_composite(const float* raw, int64_t raw_stride_s, int64_t raw_stride_c, const float* z,
                             const float* rays, const float* noise, const int32_t* label_sem,
                             const int32_t* label_inst, int64_t n_rays, int n_samples, int n_sem, int n_inst,
                             int sem_mode, int white_bkgd, float* rgb, float* depth, float* acc, float* weights,
                             float* sem, float* inst, float* fix_sem, float* fix_inst, void* stream)
{
    return composite_impl(raw, raw_stride_s, raw_stride_c, z, rays, noise, nullptr, label_sem, label_inst, n_rays, n_samples, n_sem, n_inst,
                          sem_mode, white_bkgd, rgb, depth, acc, weights, sem, inst, fix_sem, fix_inst, stream);
}

// sigma noise drawn in the kernel: channel-major images only (what the renderer composites)
PNR_EXPORT int pnr_composite_rng(const float* raw, int64_t raw_stride_s, int64_t raw_stride_c, const float* z, const float* rays,
                                 const pnr_rng* noise_host, const int32_t* label_sem, const int32_t* label_inst, int64_t n_rays,
                                 int n_samples, int n_sem, int n_inst, int sem_mode, int white_bkgd, float* rgb, float* depth, float* acc,
                                 float* weights, float* sem, float* inst, float* fix_sem, float* fix_inst, void* stream)
{
    PnrRngDev rng;
    const int rc = pnr_rng_check(noise_host, n_rays < 0 ? 0 : n_rays, "pnr_composite_rng", &rng);
    if (rc) return rc;
    PNR_REQUIRE(n_rays <= 0 || (raw_stride_s == 1 && (raw_stride_c % 4) == 0 && (((uintptr_t)raw) & 15) == 0),
                "pnr_composite_rng: channel-major, 16-byte aligned raw images only");
    return composite_impl(raw, raw_stride_s, raw_stride_c, z, rays, nullptr, &rng, label_sem, label_inst, n_rays, n_samples, n_sem, n_inst,
                          sem_mode, white_bkgd, rgb, depth, acc, weights, sem, inst, fix_sem, fix_inst, stream);
}

// ------------------------------------------------------------------------------- second half of the fused path
// k_composite_combine: finishes every ray from what the fused MLP epilogue wrote (pnr_mlp_fuse.h) -- the N / 32 per-tile
// records (Q, logit sums) and the N per-sample quadruples (lw, r, g, b):
//   T_k = prod_{k' < k} Q_k',  w_i = T_{i / 32} lw_i,
//   acc / depth / rgb = sum_i w_i {1, z_i, sigmoid(rgb_i)},  fix_x[c] = sum_i w_i [label_i == c],  logits_c = sum_k T_k S_c(k).
// One wave per ray, lane = sample (i = lane + 64 j) for the per-sample part and lane = column for the logits; 26 B per sample of
// traffic at 45 / 32 heads (+ z, + 4 B per labelled field) instead of the raw image's 324 B.  The fixed fields are a
// fixed-point histogram in LDS (integer adds: order-independent, deterministic).
// LOGITS: the records hold the C + K logit sums behind Q (every plan but 3).  Plan 3 (k_mlp_pp_sigma) writes records of Q alone:
// no logit map can be produced, and C / K only size the fix_* histograms.
struct CombineArgs {
    const float* rec; int rec_floats; const float4* ps; const float* z; const int32_t* lab_s; const int32_t* lab_i;
    int64_t R; int N, C, K, white_bkgd;
    float *rgb, *depth, *acc, *weights, *sem, *inst, *fix_sem, *fix_inst;
};

template <bool LOGITS>
__global__ __launch_bounds__(256) void k_composite_combine(CombineArgs a)
{
    __shared__ uint32_t hist_all[4][128];       // C + K <= 128 (pnr_mlp_forward_composite)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ray = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (ray >= a.R) return;                      // wave-uniform
    const int N = a.N, T = N >> 5, RF = a.rec_floats, C = a.C, K = a.K, CK = C + K;
    const float* __restrict__ rec = a.rec + ray * T * RF;
    const float4* __restrict__ ps = a.ps + ray * N;
    const float* __restrict__ zr = a.z + ray * N;
    const bool want_s = a.lab_s && a.fix_sem && C, want_i = a.lab_i && a.fix_inst && K;
    const int32_t* __restrict__ lsr = want_s ? a.lab_s + ray * N : nullptr;
    const int32_t* __restrict__ lir = want_i ? a.lab_i + ray * N : nullptr;
    // Everything this ray reads is requested up front -- the kernel waits for memory 84 % of its cycles (rocprofv3, round 3),
    // and the weights store below would otherwise fence every later load behind it (the pointers may alias for all hipcc knows)
    float q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = k < T ? rec[k * RF] : 1.0f;
    float4 pv[4];
    float zv[4];
    int lsv[4], liv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        const bool in = i < N;
        pv[j] = in ? ps[i] : float4{0.0f, 0.0f, 0.0f, 0.0f};
        zv[j] = in ? zr[i] : 0.0f;
        lsv[j] = (in && want_s) ? lsr[i] : -1;
        liv[j] = (in && want_i) ? lir[i] : -1;
    }
    float lg[2][8];                              // the logit sums of this lane's columns (c = lane, lane + 64), per tile
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int k = 0; k < 8; ++k) lg[h][k] = (LOGITS && k < T && lane + 64 * h < CK) ? rec[k * RF + PNR_FUSE_REC_LOGITS + lane + 64 * h] : 0.0f;
    float Tk[8];
    float t = 1.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        Tk[k] = t;
        if (k < T) t *= q[k];
    }
    uint32_t* hist = hist_all[wv];
    if (want_s || want_i) hist_zero<64>(hist, lane, CK);
    float r5[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        if (i < N) {
            const float4 p = pv[j];
            float tk = Tk[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) tk = (i >> 5) == k ? Tk[k] : tk;
            const float w = tk * p.x;
            r5[0] += w;
            r5[1] = fmaf(w, zv[j], r5[1]);
            r5[2] = fmaf(w, sigmoid_of(p.y), r5[2]);
            r5[3] = fmaf(w, sigmoid_of(p.z), r5[3]);
            r5[4] = fmaf(w, sigmoid_of(p.w), r5[4]);
            if (a.weights) a.weights[ray * N + i] = w;
            if (want_s || want_i) hist_add(hist, w, want_s, lsv[j], C, want_i, liv[j], K);
        }
    }
    group_sum_batch<64, 5>(r5);
    if (lane == 0) {
        if (a.acc) a.acc[ray] = r5[0];
        if (a.depth) a.depth[ray] = r5[1];
    }
    if (lane < 3 && a.rgb) {
        const float v = lane == 0 ? r5[2] : lane == 1 ? r5[3] : r5[4];
        a.rgb[ray * 3 + lane] = a.white_bkgd ? v + (1.0f - r5[0]) : v;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        if (c >= CK) continue;
        if constexpr (LOGITS) {
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) if (k < T) v = fmaf(Tk[k], lg[h][k], v);
            if (c < C) { if (a.sem) a.sem[ray * C + c] = v; }
            else if (a.inst) a.inst[ray * K + (c - C)] = v;
        }
        if (c < C) { if (want_s) a.fix_sem[ray * C + c] = hist_read(hist, c); }
        else if (want_i) a.fix_inst[ray * K + (c - C)] = hist_read(hist, c);
    }
}

int pnr_composite_combine_launch(const float* rec, int rec_floats, bool logit_sums, const float4* ps, const float* z,
                                 const int32_t* label_sem, const int32_t* label_inst, int64_t R, int N, int C, int K, int white_bkgd,
                                 float* rgb, float* depth, float* acc, float* weights, float* sem, float* inst, float* fix_sem,
                                 float* fix_inst, hipStream_t st)
{
    CombineArgs a;
    a.rec = rec; a.rec_floats = rec_floats; a.ps = ps; a.z = z; a.lab_s = label_sem; a.lab_i = label_inst;
    a.R = R; a.N = N; a.C = C; a.K = K; a.white_bkgd = white_bkgd;
    a.rgb = rgb; a.depth = depth; a.acc = acc; a.weights = weights; a.sem = sem; a.inst = inst; a.fix_sem = fix_sem; a.fix_inst = fix_inst;
    const int64_t blocks = (R + 3) / 4;
    if (logit_sums) hipLaunchKernelGGL(k_composite_combine<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_composite_combine<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    PNR_CHECK_LAUNCH("pnr_mlp_forward_composite (combine)");
    return PNR_OK;
}
