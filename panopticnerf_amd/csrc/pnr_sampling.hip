// K1 / K1b / K2 / K5: per-ray sample generation, Embedder, sample_pdf + merge, bbox prior (ray generation: pnr_camera.hip).
// gfx950 only.  The sampler, sample_pdf and bbox kernels are BIT-EXACT restatements of
// oracle/pnr_oracle.c (pnro_stratified / pnro_points / pnro_sample_pdf / pnro_bbox_hits /
// pnro_sample_labels), which since round 3 pins TORCH'S OWN op order (linspace two-sided, sum in
// ATen's vector order, cumsum in double): same operations in the same order, one rounding each.  The arithmetic that has to
// be exact lives once, in pnr_sampling_dev.h (which also turns contraction off for this file); the kernels here are loops,
// LDS layout and schedule around those pieces.
// Reference functions these replace (the reference source
// is not in the mount, include/pnr.h explains the citation form).
#include "pnr_common.h"
#include "pnr_philox.h"
#include "pnr_sampling_dev.h"
#include <stdlib.h>
#include <string.h>

// One thread per sample; HBM-bound: reads 8 B/ray amortised (+4 B t_rand), writes 4 B.
// Rng = PnrRngDev (pnr_stratified_rng): the jitter is the in-kernel stream's uniform of the sample instead of t_rand[s]; the plain
// instance k_stratified<> (empty pack) is the kernel as it was.
template <class... Rng>
__global__ __launch_bounds__(256) void k_stratified(const float* __restrict__ rays, int64_t R, int N,
                                                     int lindisp, const float* __restrict__ t_rand,
                                                     float* __restrict__ z_out, const Rng... rng)
{
    constexpr bool RNG = sizeof...(Rng) > 0;
    PnrRngKey key;
    if constexpr (RNG) key = pnr_rng_key(rng...);
    const int64_t total = R * N;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total;
         s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = s / N;
        const int i = (int)(s - r * N);
        if constexpr (RNG) {
            const float t = pnr_rng_uniform_at(key, (uint32_t)r, i);
            z_out[s] = strat_sample(rays[r * 8 + 6], rays[r * 8 + 7], i, N, lindisp, &t);
        } else {
            z_out[s] = strat_sample(rays[r * 8 + 6], rays[r * 8 + 7], i, N, lindisp, t_rand ? t_rand + s : nullptr);
        }
    }
}

__global__ __launch_bounds__(256) void k_points(const float* __restrict__ rays, const float* __restrict__ z,
                                                 int64_t R, int N, float* __restrict__ pts)
{
    const int64_t total = R * N * 3;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = e / 3;
        const int a = (int)(e - s * 3);
        const int64_t r = s / N;
        const float m = rays[r * 8 + 3 + a] * z[s];
        pts[e] = rays[r * 8 + a] + m;
    }
}

// ------------------------------------------------------------------------------- a4
// One thread per OUTPUT element so that the (n, 3+6L) sample-major image is written fully
// coalesced.  Trig-bound (cdna_hip_programming.md App. B): accurate sinf/cosf (ocml) because
// arguments reach 2^(L-1)*|x|.  The fused MLP kernel computes gamma() in registers instead.
__global__ __launch_bounds__(256) void k_embed(const float* __restrict__ x, int64_t n, int L,
                                                float* __restrict__ out)
{
    const int E = 3 + 6 * L;
    const int64_t total = n * E;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = e / E;
        const int c = (int)(e - s * E);
        float v;
        if (c < 3) {
            v = x[s * 3 + c];
        } else {
            const int k = (c - 3) / 6, j = (c - 3) - 6 * k;
            const int a = j % 3;
            const float arg = x[s * 3 + a] * ldexpf(1.0f, k);
            v = (j < 3) ? sinf(arg) : cosf(arg);
        }
        out[e] = v;
    }
}

// ------------------------------------------------------------------------------- a7
// One 64-lane workgroup (= one wavefront) per ray.  The CDF is accumulated by lane 0 in the
// oracle's sequential fp32 order (the bit-exact index requirement, SURVEY.md section 7 "hard
// parts"); everything else is lane-parallel: bins, pdf, one upper_bound per u, and a bitonic
// sort of the Nc+Nf union in LDS (a rank-based merge when the new samples are already ascending).  LDS: 7 KiB.
// With lab.label_sem set the wave that merged a ray's samples also labels them (k_sample_labels' rule on the sorted z it still
// holds in LDS): the fine level's labels without a second pass over z (pnr_sample_pdf_labels; one launch less per chunk).
struct PdfLabelArgs {
    const float* hit_t; const int32_t* hit_box; const int32_t* hit_count; int max_hits; const int32_t* box_ids;
    int32_t* label_sem; int32_t* label_inst;
};
#define PDF_MAXC 256
#define PDF_MAXT 512
template <int MAXC, int MAXT, class... Rng>
__device__ __forceinline__ void sample_pdf_body(const float* __restrict__ z, const float* __restrict__ weights,
                                                    const float* __restrict__ u, int64_t R, int Nc, int Nf,
                                                    float* __restrict__ zs_out, int32_t* __restrict__ inds_out,
                                                    float* __restrict__ zfine_out, const PdfLabelArgs lab, const Rng&... rng)
{
    constexpr bool RNG = sizeof...(Rng) > 0;
    PnrRngKey key;         // RNG: u of (ray r, sample i) is the in-kernel stream's uniform (pnr_sample_pdf_rng)
    if constexpr (RNG) key = pnr_rng_key(rng...);
    // MAXC / MAXT: the LDS footprint sets how many rays a CU has in flight, and this kernel is all latency (dependent LDS searches,
    // a dozen barriers per ray): 9.4 KiB per ray held 17 waves per CU, the <64, 256> instance (64 + 128 samples: every BASELINE
    // config) 3.4 KiB holds the CU's 32
    __shared__ float s_z[MAXC], s_w[MAXC], s_pdf[MAXC], s_cdf[MAXC], s_bins[MAXC];
    __shared__ float s_sort[MAXT], s_out[MAXT];
    __shared__ float s_total, s_part[32];
    const int lane = threadIdx.x;
    const int nb = Nc - 1, nw = Nc - 2, Nt = Nc + Nf;
    const int P = pdf_padded(Nt);
    auto labels = [&](int64_t r, const float* sorted) {       // sorted: the ray's Nt merged depths in LDS (written before a barrier)
        if (!lab.label_sem) return;
        const int mh = lab.max_hits;
        const int cnt = lab.hit_count[r] < mh ? lab.hit_count[r] : mh;
        for (int i = lane; i < Nt; i += 64) {
            const int best = label_hit(sorted[i], cnt, [&](int h, float& ti, float& to) {
                ti = lab.hit_t[(r * mh + h) * 2];
                to = lab.hit_t[(r * mh + h) * 2 + 1];
            });
            int ls, li;
            hit_ids(best, lab.hit_box + r * mh + best, lab.box_ids, &ls, &li);
            lab.label_sem[r * Nt + i] = ls;
            lab.label_inst[r * Nt + i] = li;
        }
    };
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        for (int i = lane; i < Nc; i += 64) {
            s_z[i] = z[r * Nc + i];
            s_w[i] = weights[r * Nc + i];
        }
        __syncthreads();
        for (int k = lane; k < nb; k += 64) s_bins[k] = 0.5f * (s_z[k + 1] + s_z[k]);
        const float total = pdf_torch_total(s_w, nw, s_part, &s_total, lane);
        for (int j = lane; j < nw; j += 64) s_pdf[j] = (s_w[j + 1] + 1e-5f) / total;
        __syncthreads();
        pdf_cdf(lane < nw ? s_pdf[lane < nw ? lane : 0] : 0.0f, nw, nw <= 64, s_pdf, s_cdf, lane);
        for (int i = lane; i < Nf; i += 64) {
            float uu;
            if constexpr (RNG) uu = pnr_rng_uniform_at(key, (uint32_t)r, i);
            else uu = u ? u[r * Nf + i] : pnr_linspace01(i, Nf);
            int lo = 0, hi = nb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_cdf[mid] <= uu) lo = mid + 1; else hi = mid;
            }
            const float zs = pdf_invert(uu, lo, nb, s_cdf, s_bins);
            if (zs_out) zs_out[r * Nf + i] = zs;
            if (inds_out) inds_out[r * Nf + i] = lo;
            s_sort[Nc + i] = zs;
        }
        if (zfine_out) {
            __syncthreads();
            // Are the new samples already ascending?  (Always with deterministic u: the inverse CDF is monotone.)  Then the
            // sorted union is a MERGE of two sorted lists: an element's final position is its own index plus the number
            // of elements of the OTHER list that precede it (binary searches; coarse samples go first on ties).  The
            // 36-stage LDS bitonic sort below was 2/3 of this kernel's time; it remains for random u.
            bool asc = true;
            for (int i = lane; i + 1 < Nf; i += 64) asc = asc && (s_sort[Nc + i] <= s_sort[Nc + i + 1]);
            for (int i = lane; i + 1 < Nc; i += 64) asc = asc && (s_z[i] <= s_z[i + 1]);
            if (__all(asc)) {
                for (int i = lane; i < Nc; i += 64) {          // coarse z[i]: + #samples strictly below it
                    const float v = s_z[i];
                    int lo = 0, hi = Nf;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_sort[Nc + mid] < v) lo = mid + 1; else hi = mid; }
                    s_out[i + lo] = v;
                }
                for (int j = lane; j < Nf; j += 64) {          // sample zs[j]: + #coarse z at or below it
                    const float v = s_sort[Nc + j];
                    int lo = 0, hi = Nc;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_z[mid] <= v) lo = mid + 1; else hi = mid; }
                    s_out[j + lo] = v;
                }
                __syncthreads();
                for (int i = lane; i < Nt; i += 64) zfine_out[r * Nt + i] = s_out[i];
                labels(r, s_out);
                __syncthreads();
                continue;
            }
            for (int i = lane; i < Nc; i += 64) s_sort[i] = s_z[i];
            for (int i = Nt + lane; i < P; i += 64) s_sort[i] = INFINITY;
            __syncthreads();
            pdf_bitonic(s_sort, P, lane);
            for (int i = lane; i < Nt; i += 64) zfine_out[r * Nt + i] = s_sort[i];
            labels(r, s_sort);
        }
        __syncthreads();
    }
}

// ---- the inference frame's instance (round 6): deterministic u, merged z_fine (+ labels) only, Nc <= 64, Nc + Nf <= 256.
// Same operations on the same values as sample_pdf_body -- bit for bit -- with a different instruction stream: the general body ran
// 8 waves per SIMD with SGPRs spilled to VGPR lanes (249 v_readlane / 147 v_writelane in its code) and VGPRs to scratch, and the
// kernel is bound by ISSUE, not latency.  Here: lane = coarse sample, z / w / pdf / bins in registers (neighbours by DPP); the
// searches are branch-free fixed-depth bisections over LDS (upper / lower bound of a SORTED list = the number of elements <= / <
// the key: identical to the general body's loops whenever the lists are sorted, and the merge path is only taken when they are);
// a ray's hit list is loaded once, one entry per lane, its ids looked up once per hit instead of once per sample, and broadcast by
// v_readlane with the hit loop outermost (the same sequence of comparisons per sample).  Unsorted lists (never with deterministic
// u and a monotone CDF) fall back to the bitonic sort in a function of its own.
__device__ __noinline__ void pdf_bitonic_fallback(float* s_sort, const float* s_z, const float* s_zs, int Nc, int Nf, int P, int lane)
{
    const int Nt = Nc + Nf;
    for (int i = lane; i < Nc; i += 64) s_sort[i] = s_z[i];
    for (int i = lane; i < Nf; i += 64) s_sort[Nc + i] = s_zs[i];
    for (int i = Nt + lane; i < P; i += 64) s_sort[i] = INFINITY;
    __syncthreads();
    pdf_bitonic(s_sort, P, lane);
}

#ifndef PDF_DET_WPE
#define PDF_DET_WPE 8           /* waves per SIMD the register allocation is held to.  The kernel is bound by LATENCY (a dozen dependent LDS round trips
                                   per ray, one ray per wave): at its natural 73 VGPRs (6 waves) it is SLOWER than the general body at 8 waves
                                   (1.06 against 0.94 ms per frame's 8 launches) although it issues a third of the instructions; held to 64
                                   registers 0.87 (profiles/r06/r06d, same box) */
#endif
#if PDF_DET_WPE
__attribute__((amdgpu_waves_per_eu(PDF_DET_WPE, PDF_DET_WPE)))
#endif
__global__ __launch_bounds__(64) void k_sample_pdf_det(const float* __restrict__ z, const float* __restrict__ weights, int64_t R, int Nc,
                                                        int Nf, float* __restrict__ zfine_out, const PdfLabelArgs lab)
{
    __shared__ float s_z[64], s_w[64], s_pdf[64], s_cdf[64], s_bins[64];
    __shared__ float s_zs[192], s_out[256];
    __shared__ float s_total, s_part[32];
    const int lane = threadIdx.x;
    const int nb = Nc - 1, nw = Nc - 2, Nt = Nc + Nf;
    int topc = 1, topf = 1;                     // the largest powers of two <= Nc, <= Nf: first strides of the bisections
    while (topc * 2 <= Nc) topc *= 2;
    while (topf * 2 <= Nf) topf *= 2;
    const int mh = lab.max_hits;
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        const float* __restrict__ zr = z + r * Nc;
        const float* __restrict__ wr = weights + r * Nc;
        const float zl = lane < Nc ? zr[lane] : 0.0f, wl = lane < Nc ? wr[lane] : 0.0f;
        // the ray's hit list, one kept entry per lane (requested now, used at the end)
        int cnt = 0, h_ls = -1, h_li = -1;
        float h_ti = 0.0f, h_to = 0.0f;
        if (lab.label_sem) {
            const int c0 = lab.hit_count[r];
            cnt = c0 < mh ? c0 : mh;
            if (lane < cnt) {
                const float2 t2 = *reinterpret_cast<const float2*>(lab.hit_t + (r * mh + lane) * 2);
                h_ti = t2.x; h_to = t2.y;
                hit_ids(lane, lab.hit_box + r * mh + lane, lab.box_ids, &h_ls, &h_li);
            }
        }
        s_z[lane] = zl;
        s_w[lane] = wl;
        const float zn = __shfl_down(zl, 1, 64), wn = __shfl_down(wl, 1, 64);
        s_bins[lane] = 0.5f * (zn + zl);             // bins[k] = 0.5 (z[k + 1] + z[k]), k < nb
        __syncthreads();
        const float total = pdf_torch_total(s_w, nw, s_part, &s_total, lane);
        const float pl = lane < nw ? (wn + 1e-5f) / total : 0.0f;      // pdf[j] = (w[j + 1] + 1e-5) / total
        s_pdf[lane] = pl;
        pdf_cdf(pl, nw, true, s_pdf, s_cdf, lane);       // Nc <= 64 here
        // inverse CDF at the Nf deterministic u: upper bound over cdf[0 .. nb) by bisection (cdf is non-decreasing) -- this kernel's
        // own search (fixed depth, branch-free), kept apart from sample_pdf_body's loop: it is the point of the instance
        bool asc = lane + 1 >= Nc || zl <= zn;
        for (int i = lane; i < Nf; i += 64) {
            const float uu = pnr_linspace01(i, Nf);
            int pos = 0;
            for (int st = topc; st >= 1; st >>= 1) {
                const int p = pos + st, q = p <= nb ? p : nb;
                pos = (p <= nb && s_cdf[q - 1] <= uu) ? p : pos;
            }
            s_zs[i] = pdf_invert(uu, pos, nb, s_cdf, s_bins);
        }
        __syncthreads();
        for (int i = lane; i + 1 < Nf; i += 64) asc = asc && (s_zs[i] <= s_zs[i + 1]);
        if (__all(asc)) {
            // merge by rank: coarse z[i] goes to i + #{samples < z[i]}, sample zs[j] to j + #{coarse z <= zs[j]}
            if (lane < Nc) {
                int pos = 0;
                for (int st = topf; st >= 1; st >>= 1) {
                    const int p = pos + st, q = p <= Nf ? p : Nf;
                    pos = (p <= Nf && s_zs[q - 1] < zl) ? p : pos;
                }
                s_out[lane + pos] = zl;
            }
            for (int j = lane; j < Nf; j += 64) {
                const float v = s_zs[j];
                int pos = 0;
                for (int st = topc; st >= 1; st >>= 1) {
                    const int p = pos + st, q = p <= Nc ? p : Nc;
                    pos = (p <= Nc && s_z[q - 1] <= v) ? p : pos;
                }
                s_out[j + pos] = v;
            }
            __syncthreads();
        } else {
            pdf_bitonic_fallback(s_out, s_z, s_zs, Nc, Nf, pdf_padded(Nt), lane);
        }
        // the sorted union, and its labels (k_sample_labels' rule: the containing interval with the smallest t_in, lowest index first).
        // A kept copy of label_hit + hit_ids on purpose: the hit loop is OUTERMOST over v_readlane broadcasts of the per-lane entries,
        // four samples per lane in registers, ids carried along -- the shared pieces loop over hits per sample from memory
        float* __restrict__ zo = zfine_out + r * Nt;
        for (int i0 = 0; i0 < Nt; i0 += 256) {
            float zz[4];
            int best[4], ls[4], li[4];
            float bt[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + lane + 64 * k;
                zz[k] = i < Nt ? s_out[i < Nt ? i : 0] : 0.0f;
                best[k] = -1; ls[k] = -1; li[k] = -1; bt[k] = 0.0f;
                if (i < Nt) zo[i] = zz[k];
            }
            if (lab.label_sem) {
                for (int h = 0; h < cnt; ++h) {
                    const float ti = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h_ti), h));
                    const float to = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h_to), h));
                    const int hs = __builtin_amdgcn_readlane(h_ls, h), hi2 = __builtin_amdgcn_readlane(h_li, h);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool take = ti <= zz[k] && zz[k] <= to && (best[k] < 0 || ti < bt[k]);
                        best[k] = take ? h : best[k];
                        bt[k] = take ? ti : bt[k];
                        ls[k] = take ? hs : ls[k];
                        li[k] = take ? hi2 : li[k];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = i0 + lane + 64 * k;
                    if (i < Nt) {
                        lab.label_sem[r * Nt + i] = ls[k];
                        lab.label_inst[r * Nt + i] = li[k];
                    }
                }
            }
        }
        __syncthreads();
    }
}

// four instances: <64, 256> (64 + 128 samples: every BASELINE config) held to 64 registers, with 3.4 KiB of LDS 8 waves per SIMD; the
// general one <PDF_MAXC, PDF_MAXT> (up to 256 + 256 samples) is bound by its 9.1 KiB of LDS per ray and left to the compiler's own
// range (1 .. 8); each with Rng = PnrRngDev, u drawn in the kernel (pnr_sample_pdf_rng / pnr_sample_pdf_labels_rng; u is then null)
template <int MAXC, int MAXT, class... Rng>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MAXC <= 64 ? 8 : 1, 8)))
void k_sample_pdf(const float* __restrict__ z, const float* __restrict__ weights, const float* __restrict__ u, int64_t R, int Nc, int Nf,
                  float* __restrict__ zs_out, int32_t* __restrict__ inds_out, float* __restrict__ zfine_out, const PdfLabelArgs lab,
                  const Rng... rng)
{
    sample_pdf_body<MAXC, MAXT>(z, weights, u, R, Nc, Nf, zs_out, inds_out, zfine_out, lab, rng...);
}

// ------------------------------------------------------------------------------- a8
// One thread per ray; the box table is wave-uniform (scalar loads, L2/K$ resident: M*60 B).
__global__ __launch_bounds__(256) void k_bbox_hits(const float* __restrict__ rays, int64_t R,
                                                    const float* __restrict__ box, int M, int max_hits,
                                                    float* __restrict__ hit_t, int32_t* __restrict__ hit_box,
                                                    int32_t* __restrict__ hit_count)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R;
         r += (int64_t)gridDim.x * blockDim.x) {
        const RayRec ry = ray_load(rays, r);
        const auto list = hit_rows(hit_t, hit_box, r, max_hits);        // built in place, in the ray's output rows
        hit_init(list, max_hits);
        int cnt = 0;
        for (int m = 0; m < M; ++m) {
            float tmin, tmax;
            slab_interval(box + m * 15, ry, &tmin, &tmax);
            if (tmin <= tmax) hit_insert(list, cnt, max_hits, tmin, tmax, m);
        }
        hit_count[r] = cnt;             // TRUE number of intersected boxes
    }
}

// a8 + a3 + a8 in one launch (the coarse level's per-ray preamble: k_bbox_hits, k_restrict_rays' hull, k_stratified and
// k_sample_labels were four launches and three passes over the hit lists).  Phase 1, one thread per ray: the slab tests with the
// ray's kept intervals in LDS ([entry][thread]: conflict-free; k_bbox_hits keeps them in global memory) -- same operations in the
// same order, so the hit lists are k_bbox_hits' bit for bit.  Phase 2, lane = sample: z and the labels, written in whole rows.
// 64 rays per 4-wave workgroup: phase 1 occupies one wave (one thread per ray is all the parallelism it has; as one wave per SIMD
// of a 256-ray workgroup, phase 2 ran at 42 us against the separate kernels' 26), the other three are in the phase 2 of the CU's
// other workgroups.  65,536 rays x 64 samples, 64 boxes: 50 us against 27 + 11 + 15 for the three kernels (profiles/r05/r05l).  max_hits <= 8 (7 KiB of LDS); the separate kernels remain for larger lists.
#define SETUP_MAXH 8
struct RaySetupArgs {
    const float* rays; int64_t R; const float* box; int M; int max_hits; const int32_t* box_ids;
    int N, lindisp, hull; const float* t_rand;
    float* hit_t; int32_t* hit_box; int32_t* hit_count; float* z; int32_t* label_sem; int32_t* label_inst;
};
// Rng = PnrRngDev (pnr_ray_setup_rng): the jitter of sample i of ray r is the in-kernel stream's uniform (r, i) instead of
// t_rand; k_ray_setup<> (empty pack) is the plain kernel
template <class... Rng>
__global__ __launch_bounds__(256) void k_ray_setup(const RaySetupArgs a, const Rng... rng)
{
    constexpr bool RNG = sizeof...(Rng) > 0;
    __shared__ float2 s_t[SETUP_MAXH][64];      // (t_in, t_out)
    __shared__ float s_nr[64], s_fr[64];
    __shared__ int s_hb[SETUP_MAXH][64], s_cnt[64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int mh = a.max_hits, N = a.N;
    PnrRngKey key;
    if constexpr (RNG) key = pnr_rng_key(rng...);
    for (int64_t base = (int64_t)blockIdx.x * 64; base < a.R; base += (int64_t)gridDim.x * 64) {
        const int64_t r = base + tid;
        if (tid < 64 && r < a.R) {              // phase 1: the block's first wave (the others are in another block's phase 2)
            // A kept copy on purpose of ray_load, slab_interval, hit_init / hit_insert / the flush and hit_hull (pnr_sampling_dev.h), on
            // the LDS column: assembled from the shared pieces (same registers, LDS and bits) this kernel measured 52.6 us against 50.6
            // per 65,536 rays, the parent's own spread being 0.5 (profiles/sampling_frame/ab.txt).  Change the pieces and this together.
            const float4 ra = *reinterpret_cast<const float4*>(a.rays + r * 8), rb = *reinterpret_cast<const float4*>(a.rays + r * 8 + 4);
            const float o0 = ra.x, o1 = ra.y, o2 = ra.z, d0 = ra.w, d1 = rb.x, d2 = rb.y;
            float nr = rb.z, fr = rb.w;
            for (int h = 0; h < SETUP_MAXH; ++h) { s_hb[h][tid] = -1; s_t[h][tid] = make_float2(0.0f, 0.0f); }
            int cnt = 0;
            for (int m = 0; m < a.M; ++m) {
                const float* b = a.box + m * 15;
                const float p0 = o0 - b[0], p1 = o1 - b[1], p2 = o2 - b[2];
                float tmin = nr, tmax = fr;
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    const float r0 = b[3 + 3 * x], r1 = b[4 + 3 * x], r2 = b[5 + 3 * x];
                    const float ol = (r0 * p0 + r1 * p1) + r2 * p2;
                    const float dl = (r0 * d0 + r1 * d1) + r2 * d2;
                    const float inv = 1.0f / dl;
                    const float e = b[12 + x];
                    const float t1 = (-e - ol) * inv, t2 = (e - ol) * inv;
                    tmin = fmaxf(tmin, fminf(t1, t2));
                    tmax = fminf(tmax, fmaxf(t1, t2));
                }
                if (tmin <= tmax) {             // hit_insert: the max_hits nearest, ascending (t_in, box index)
                    const int n = cnt < mh ? cnt : mh;
                    int pos = n;
                    while (pos > 0 && s_t[pos - 1][tid].x > tmin) --pos;
                    if (pos < mh) {
                        for (int k = (n < mh ? n : mh - 1); k > pos; --k) {
                            s_t[k][tid] = s_t[k - 1][tid];
                            s_hb[k][tid] = s_hb[k - 1][tid];
                        }
                        s_t[pos][tid] = make_float2(tmin, tmax);
                        s_hb[pos][tid] = m;
                    }
                    ++cnt;
                }
            }
            a.hit_count[r] = cnt;
            const int kept = cnt < mh ? cnt : mh;
            for (int h = 0; h < mh; ++h) {
                *reinterpret_cast<float2*>(a.hit_t + (r * mh + h) * 2) = s_t[h][tid];
                a.hit_box[r * mh + h] = s_hb[h][tid];
            }
            if (a.hull && kept > 0) {           // hit_hull: the hull of the kept intervals replaces [near, far]
                float lo = s_t[0][tid].x, hi = s_t[0][tid].y;
                for (int h = 1; h < kept; ++h) {
                    lo = fminf(lo, s_t[h][tid].x);
                    hi = fmaxf(hi, s_t[h][tid].y);
                }
                nr = lo; fr = hi;
            }
            s_nr[tid] = nr; s_fr[tid] = fr; s_cnt[tid] = kept;
        }
        __syncthreads();
        // Phase 2: each of the four waves takes 16 of the 64 rays, one ray in hand at a time.  Everything a ray needs from LDS is
        // requested for RU rays at once (wave-uniform addresses: broadcast reads), so the chains overlap; the hit loop runs over
        // registers with the ray's own (wave-uniform) count.
        constexpr int RU = 2;
        for (int rr = wv * 16; rr < wv * 16 + 16; rr += RU) {
            if (base + rr >= a.R) break;                            // wave-uniform
            float nr[RU], fr[RU];
            int cnt[RU], hb[RU][SETUP_MAXH];
            float2 iv[RU][SETUP_MAXH];
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int t = rr + u;
                // wave-uniform values: scalar registers (as vector registers these 26 values per ray set the occupancy)
                auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
                nr[u] = uni(s_nr[t]); fr[u] = uni(s_fr[t]);
                cnt[u] = __builtin_amdgcn_readfirstlane(s_cnt[t]);
#pragma unroll
                for (int h = 0; h < SETUP_MAXH; ++h) {
                    const float2 v = s_t[h][t];
                    iv[u][h] = make_float2(uni(v.x), uni(v.y));
                    hb[u][h] = __builtin_amdgcn_readfirstlane(s_hb[h][t]);
                }
            }
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int64_t ray = base + rr + u;
                if (ray >= a.R) break;                              // wave-uniform
                for (int i = lane; i < N; i += 64) {
                    const int64_t s = ray * N + i;
                    float zz;
                    if constexpr (RNG) {
                        const float t = pnr_rng_uniform_at(key, (uint32_t)ray, i);
                        zz = strat_sample(nr[u], fr[u], i, N, a.lindisp, &t);
                    } else {
                        zz = strat_sample(nr[u], fr[u], i, N, a.lindisp, a.t_rand ? a.t_rand + s : nullptr);
                    }
                    a.z[s] = zz;
                    if (a.label_sem) {
                        int best = -1, m = -1;
                        float bt = 0.0f;
#pragma unroll
                        // A kept copy of label_hit + hit_ids on purpose: unrolled over the ray's entries in (scalar) REGISTERS, the
                        // box index carried along -- label_hit's loop reads each entry through an accessor, per sample
                        for (int h = 0; h < SETUP_MAXH; ++h) {
                            if (h >= cnt[u]) break;
                            const float ti = iv[u][h].x, to = iv[u][h].y;
                            if (ti <= zz && zz <= to && (best < 0 || ti < bt)) { best = h; bt = ti; m = hb[u][h]; }
                        }
                        int ls = -1, li = -1;
                        if (best >= 0) {
                            ls = a.box_ids[m * 2];
                            li = a.box_ids[m * 2 + 1];
                        }
                        a.label_sem[s] = ls;
                        a.label_inst[s] = li;
                    }
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_sample_labels(const float* __restrict__ z, int64_t R, int N,
                                                        const float* __restrict__ hit_t,
                                                        const int32_t* __restrict__ hit_box,
                                                        const int32_t* __restrict__ hit_count, int max_hits,
                                                        const int32_t* __restrict__ box_ids,
                                                        int32_t* __restrict__ label_sem,
                                                        int32_t* __restrict__ label_inst)
{
    const int64_t total = R * N;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total;
         s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = s / N;
        const float zz = z[s];
        const int cnt = hit_count[r] < max_hits ? hit_count[r] : max_hits;     // hit_count is the true count (overflow)
        const int best = label_hit(zz, cnt, [&](int h, float& ti, float& to) {
            ti = hit_t[(r * max_hits + h) * 2];
            to = hit_t[(r * max_hits + h) * 2 + 1];
        });
        // hit_ids, spelled out: through the shared piece this kernel measured 14.6 us against 14.3 per 65,536 x 64 samples in three
        // sessions, the parent's spread being 0.3 (profiles/sampling_frame/ab.txt)
        int ls = -1, li = -1;
        if (best >= 0) {
            const int m = hit_box[r * max_hits + best];
            ls = box_ids[m * 2];
            li = box_ids[m * 2 + 1];
        }
        label_sem[s] = ls;
        label_inst[s] = li;
    }
}

// ------------------------------------------------------------------------------- C-ABI
PNR_EXPORT int pnr_stratified(const float* rays, int64_t n_rays, int n_samples, int lindisp,
                              const float* t_rand, float* z_out, void* stream)
{
    PNR_REQUIRE(n_rays >= 0 && n_samples >= 1, "pnr_stratified: bad size R=%lld N=%d", (long long)n_rays, n_samples);
    if (n_rays == 0) return PNR_OK;     // empty input is a no-op
    PNR_REQUIRE(rays && z_out, "pnr_stratified: null pointer");
    const int64_t total = n_rays * n_samples;
    hipLaunchKernelGGL(k_stratified<>, dim3(pnr_grid_cap((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       rays, n_rays, n_samples, lindisp, t_rand, z_out);
    PNR_CHECK_LAUNCH("pnr_stratified");
    return PNR_OK;
}

PNR_EXPORT int pnr_stratified_rng(const float* rays, int64_t n_rays, int n_samples, int lindisp, const pnr_rng* rng_host,
                                  float* z_out, void* stream)
{
    PnrRngDev rng;
    const int rc = pnr_rng_check(rng_host, n_rays, "pnr_stratified_rng", &rng);
    if (rc) return rc;
    PNR_REQUIRE(n_rays >= 0 && n_samples >= 1 && n_samples <= (1 << 26), "pnr_stratified_rng: bad size R=%lld N=%d", (long long)n_rays,
                n_samples);
    if (n_rays == 0) return PNR_OK;
    PNR_REQUIRE(rays && z_out, "pnr_stratified_rng: null pointer");
    const int64_t total = n_rays * n_samples;
    hipLaunchKernelGGL(k_stratified<PnrRngDev>, dim3(pnr_grid_cap((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       rays, n_rays, n_samples, lindisp, (const float*)nullptr, z_out, rng);
    PNR_CHECK_LAUNCH("pnr_stratified_rng");
    return PNR_OK;
}

PNR_EXPORT int pnr_points(const float* rays, const float* z, int64_t n_rays, int n_samples, float* pts_out,
                          void* stream)
{
    PNR_REQUIRE(n_rays >= 0 && n_samples >= 1, "pnr_points: bad size");
    if (n_rays == 0) return PNR_OK;
    PNR_REQUIRE(rays && z && pts_out, "pnr_points: null pointer");
    const int64_t total = n_rays * n_samples * 3;
    hipLaunchKernelGGL(k_points, dim3(pnr_grid_cap((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       rays, z, n_rays, n_samples, pts_out);
    PNR_CHECK_LAUNCH("pnr_points");
    return PNR_OK;
}

PNR_EXPORT int pnr_embed(const float* x, int64_t n, int L, float* out, void* stream)
{
    PNR_REQUIRE(n >= 0 && L >= 0 && L <= 16, "pnr_embed: bad size n=%lld L=%d", (long long)n, L);
    if (n == 0) return PNR_OK;
    PNR_REQUIRE(x && out, "pnr_embed: null pointer");
    const int64_t total = n * (3 + 6 * L);
    hipLaunchKernelGGL(k_embed, dim3(pnr_grid_cap((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       x, n, L, out);
    PNR_CHECK_LAUNCH("pnr_embed");
    return PNR_OK;
}

// The one launch of the a7 family.  k_sample_pdf_det when that is what is asked (deterministic u, merged z_fine (+ labels) only)
// and it fits; else the general body, its small instance when the padded union does.  rng: u drawn in the kernel (never
// k_sample_pdf_det: its u is deterministic).
static void launch_sample_pdf(const float* z, const float* weights, const float* u, const PnrRngDev* rng, int64_t n_rays, int n_coarse,
                              int n_fine, float* z_samples, int32_t* inds, float* z_fine, const PdfLabelArgs& lab, hipStream_t st)
{
    const dim3 grid(pnr_grid_cap(n_rays, 32)), block(64);
    const bool small = n_coarse <= 64 && pdf_padded(n_coarse + n_fine) <= 256;
    auto go = [&](auto kernel, auto... r) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, z, weights, u, n_rays, n_coarse, n_fine, z_samples, inds, z_fine, lab, r...);
    };
    // PNR_SAMPLE_PDF_GENERAL: A/B switch (tests, tools): the general body everywhere
    if (!rng && !u && !z_samples && !inds && z_fine && small && n_fine <= 192 && lab.max_hits <= 64 && !getenv("PNR_SAMPLE_PDF_GENERAL"))
        hipLaunchKernelGGL(k_sample_pdf_det, grid, block, 0, st, z, weights, n_rays, n_coarse, n_fine, z_fine, lab);
    else if (rng)
        go(small ? k_sample_pdf<64, 256, PnrRngDev> : k_sample_pdf<PDF_MAXC, PDF_MAXT, PnrRngDev>, *rng);
    else
        go(small ? k_sample_pdf<64, 256> : k_sample_pdf<PDF_MAXC, PDF_MAXT>);
}

// One body behind the four entry points: name = the entry point's own (it is in every message); with_rng: rng_host is checked and u
// drawn in the kernel; labels: the hit lists and label outputs of the _labels forms (a7 + a8: z_fine as pnr_sample_pdf, and the
// labels pnr_sample_labels would give for it, in the same launch), null for the plain forms.
static int sample_pdf_impl(const char* name, const float* z, const float* weights, const float* u, bool with_rng, const pnr_rng* rng_host,
                           int64_t n_rays, int n_coarse, int n_fine, float* z_samples, int32_t* inds, float* z_fine,
                           const PdfLabelArgs* labels, void* stream)
{
    PnrRngDev rng;
    if (with_rng) {
        const int rc = pnr_rng_check(rng_host, n_rays < 0 ? 0 : n_rays, name, &rng);
        if (rc) return rc;
    }
    PNR_REQUIRE(n_rays <= 0 || (z && weights && (!labels || z_fine)), "%s: null pointer", name);
    PNR_REQUIRE(!labels || n_rays <= 0 || (labels->hit_t && labels->hit_box && labels->hit_count && labels->box_ids && labels->label_sem &&
                                           labels->label_inst), "%s: null pointer", name);
    PNR_REQUIRE(n_coarse >= 3 && n_coarse <= PDF_MAXC, "%s: n_coarse=%d outside [3,%d]", name, n_coarse, PDF_MAXC);
    PNR_REQUIRE(n_fine >= 1 && n_coarse + n_fine <= PDF_MAXT, "%s: n_coarse+n_fine=%d > %d", name, n_coarse + n_fine, PDF_MAXT);
    PNR_REQUIRE(!labels || labels->max_hits >= 1, "%s: bad max_hits", name);
    if (n_rays <= 0) return PNR_OK;
    launch_sample_pdf(z, weights, u, with_rng ? &rng : nullptr, n_rays, n_coarse, n_fine, z_samples, inds, z_fine,
                      labels ? *labels : PdfLabelArgs{}, (hipStream_t)stream);
    PNR_CHECK_LAUNCH(name);
    return PNR_OK;
}

PNR_EXPORT int pnr_sample_pdf(const float* z, const float* weights, const float* u, int64_t n_rays, int n_coarse,
                              int n_fine, float* z_samples, int32_t* inds, float* z_fine, void* stream)
{
    return sample_pdf_impl("pnr_sample_pdf", z, weights, u, false, nullptr, n_rays, n_coarse, n_fine, z_samples, inds, z_fine, nullptr, stream);
}

PNR_EXPORT int pnr_sample_pdf_rng(const float* z, const float* weights, const pnr_rng* rng_host, int64_t n_rays, int n_coarse,
                                  int n_fine, float* z_samples, int32_t* inds, float* z_fine, void* stream)
{
    return sample_pdf_impl("pnr_sample_pdf_rng", z, weights, nullptr, true, rng_host, n_rays, n_coarse, n_fine, z_samples, inds, z_fine, nullptr,
                           stream);
}

PNR_EXPORT int pnr_sample_pdf_labels(const float* z, const float* weights, const float* u, int64_t n_rays, int n_coarse, int n_fine,
                                     float* z_fine, const float* hit_t, const int32_t* hit_box, const int32_t* hit_count,
                                     int max_hits, const int32_t* box_ids, int32_t* label_sem, int32_t* label_inst, void* stream)
{
    const PdfLabelArgs lab{hit_t, hit_box, hit_count, max_hits, box_ids, label_sem, label_inst};
    return sample_pdf_impl("pnr_sample_pdf_labels", z, weights, u, false, nullptr, n_rays, n_coarse, n_fine, nullptr, nullptr, z_fine, &lab, stream);
}

PNR_EXPORT int pnr_sample_pdf_labels_rng(const float* z, const float* weights, const pnr_rng* rng_host, int64_t n_rays, int n_coarse,
                                         int n_fine, float* z_fine, const float* hit_t, const int32_t* hit_box, const int32_t* hit_count,
                                         int max_hits, const int32_t* box_ids, int32_t* label_sem, int32_t* label_inst, void* stream)
{
    const PdfLabelArgs lab{hit_t, hit_box, hit_count, max_hits, box_ids, label_sem, label_inst};
    return sample_pdf_impl("pnr_sample_pdf_labels_rng", z, weights, nullptr, true, rng_host, n_rays, n_coarse, n_fine, nullptr, nullptr, z_fine,
                           &lab, stream);
}

// a8 + a3 (+ a8): hit lists as pnr_bbox_hits, z as pnr_stratified (over the hull of the kept intervals with hull != 0:
// pnr_restrict_rays), labels as pnr_sample_labels (label_sem / label_inst may both be null), in one launch.  max_hits <= 8.
static int ray_setup_impl(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits, const int32_t* box_ids,
                          int n_samples, int lindisp, const float* t_rand, const PnrRngDev* rng, int hull, float* hit_t, int32_t* hit_box,
                          int32_t* hit_count, float* z_out, int32_t* label_sem, int32_t* label_inst, void* stream);

PNR_EXPORT int pnr_ray_setup(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits, const int32_t* box_ids,
                             int n_samples, int lindisp, const float* t_rand, int hull, float* hit_t, int32_t* hit_box,
                             int32_t* hit_count, float* z_out, int32_t* label_sem, int32_t* label_inst, void* stream)
{
    return ray_setup_impl(rays, n_rays, box, n_box, max_hits, box_ids, n_samples, lindisp, t_rand, nullptr, hull, hit_t, hit_box, hit_count,
                          z_out, label_sem, label_inst, stream);
}

PNR_EXPORT int pnr_ray_setup_rng(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits, const int32_t* box_ids,
                                 int n_samples, int lindisp, const pnr_rng* rng_host, int hull, float* hit_t, int32_t* hit_box,
                                 int32_t* hit_count, float* z_out, int32_t* label_sem, int32_t* label_inst, void* stream)
{
    PnrRngDev rng;
    const int rc = pnr_rng_check(rng_host, n_rays < 0 ? 0 : n_rays, "pnr_ray_setup_rng", &rng);
    if (rc) return rc;
    PNR_REQUIRE(n_samples <= (1 << 26), "pnr_ray_setup_rng: n_samples=%d > 2^26", n_samples);
    return ray_setup_impl(rays, n_rays, box, n_box, max_hits, box_ids, n_samples, lindisp, nullptr, &rng, hull, hit_t, hit_box, hit_count,
                          z_out, label_sem, label_inst, stream);
}

static int ray_setup_impl(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits, const int32_t* box_ids,
                          int n_samples, int lindisp, const float* t_rand, const PnrRngDev* rng, int hull, float* hit_t, int32_t* hit_box,
                          int32_t* hit_count, float* z_out, int32_t* label_sem, int32_t* label_inst, void* stream)
{
    PNR_REQUIRE(n_rays >= 0 && n_samples >= 1, "pnr_ray_setup: bad size R=%lld N=%d", (long long)n_rays, n_samples);
    PNR_REQUIRE(max_hits >= 1 && max_hits <= SETUP_MAXH, "pnr_ray_setup: max_hits=%d outside [1,%d] (use the separate entry points)",
                max_hits, SETUP_MAXH);
    PNR_REQUIRE(n_box >= 0 && (n_box == 0 || box), "pnr_ray_setup: bad box table");
    if (n_rays == 0) return PNR_OK;
    PNR_REQUIRE(rays && hit_t && hit_box && hit_count && z_out, "pnr_ray_setup: null pointer");
    PNR_REQUIRE((label_sem != nullptr) == (label_inst != nullptr) && (!label_sem || box_ids || n_box == 0),
                "pnr_ray_setup: labels need both outputs and box_ids");
    PNR_REQUIRE((((uintptr_t)rays) & 15) == 0 && (((uintptr_t)hit_t) & 7) == 0, "pnr_ray_setup: rays must be 16-byte aligned");
    RaySetupArgs a;
    a.rays = rays; a.R = n_rays; a.box = box; a.M = n_box; a.max_hits = max_hits; a.box_ids = box_ids;
    a.N = n_samples; a.lindisp = lindisp; a.hull = hull; a.t_rand = t_rand;
    a.hit_t = hit_t; a.hit_box = hit_box; a.hit_count = hit_count; a.z = z_out; a.label_sem = label_sem; a.label_inst = label_inst;
    if (rng)
        hipLaunchKernelGGL(k_ray_setup<PnrRngDev>, dim3(pnr_grid_cap((n_rays + 63) / 64)), dim3(256), 0, (hipStream_t)stream, a, *rng);
    else
        hipLaunchKernelGGL(k_ray_setup<>, dim3(pnr_grid_cap((n_rays + 63) / 64)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_ray_setup");
    return PNR_OK;
}

PNR_EXPORT int pnr_bbox_hits(const float* rays, int64_t n_rays, const float* box, int n_box, int max_hits,
                             float* hit_t, int32_t* hit_box, int32_t* hit_count, void* stream)
{
    PNR_REQUIRE(n_rays <= 0 || (rays && hit_t && hit_box && hit_count), "pnr_bbox_hits: null pointer");
    PNR_REQUIRE(n_box >= 0 && (n_box == 0 || box), "pnr_bbox_hits: bad box table");
    PNR_REQUIRE(max_hits >= 1 && max_hits <= 64, "pnr_bbox_hits: max_hits=%d outside [1,64]", max_hits);
    if (n_rays <= 0) return PNR_OK;
    hipLaunchKernelGGL(k_bbox_hits, dim3(pnr_grid_cap((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       rays, n_rays, box, n_box, max_hits, hit_t, hit_box, hit_count);
    PNR_CHECK_LAUNCH("pnr_bbox_hits");
    return PNR_OK;
}

PNR_EXPORT int pnr_sample_labels(const float* z, int64_t n_rays, int n_samples, const float* hit_t,
                                 const int32_t* hit_box, const int32_t* hit_count, int max_hits,
                                 const int32_t* box_ids, int32_t* label_sem, int32_t* label_inst, void* stream)
{
    PNR_REQUIRE(n_rays <= 0 || (z && hit_t && hit_box && hit_count && box_ids && label_sem && label_inst),
                "pnr_sample_labels: null pointer");
    PNR_REQUIRE(n_samples >= 1 && max_hits >= 1, "pnr_sample_labels: bad size");
    if (n_rays <= 0) return PNR_OK;
    const int64_t total = n_rays * n_samples;
    hipLaunchKernelGGL(k_sample_labels, dim3(pnr_grid_cap((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, z, n_rays, n_samples, hit_t, hit_box, hit_count, max_hits, box_ids,
                       label_sem, label_inst);
    PNR_CHECK_LAUNCH("pnr_sample_labels");
    return PNR_OK;
}

// ---- a8 / a3 switch: sampling restricted to the bbox prior ("is z uniform in [near, far] or restricted to
// bbox hit intervals?" -- the reference's answer is not in the mount; this is the restricted form as a CONFIG switch,
// cfg.bbox_sampling = "hull").  A ray that hits boxes is sampled over the hull of its kept intervals, [min t_in, max t_out]
// (the slab test starts from [near, far], so the hull already lies inside it); a ray without a hit keeps [near, far].  Only
// the near / far columns of the ray record change: everything downstream (stratified, sample_pdf, labels) is unchanged.
__global__ __launch_bounds__(256) void k_restrict_rays(const float* __restrict__ rays, int64_t R, const float* __restrict__ hit_t,
                                                        const int32_t* __restrict__ hit_count, int max_hits, float* __restrict__ out)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = *reinterpret_cast<const float4*>(rays + r * 8);
        float4 b = *reinterpret_cast<const float4*>(rays + r * 8 + 4);
        const int cnt = hit_count[r] < max_hits ? hit_count[r] : max_hits;
        if (cnt > 0) hit_hull(HitRows<const float, const int32_t>{hit_t + r * max_hits * 2, nullptr}, cnt, &b.z, &b.w);
        *reinterpret_cast<float4*>(out + r * 8) = a;
        *reinterpret_cast<float4*>(out + r * 8 + 4) = b;
    }
}

PNR_EXPORT int pnr_restrict_rays(const float* rays, int64_t n_rays, const float* hit_t, const int32_t* hit_count, int max_hits,
                                 float* rays_out, void* stream)
{
    PNR_REQUIRE(n_rays >= 0 && max_hits >= 1, "pnr_restrict_rays: bad size");
    if (n_rays == 0) return PNR_OK;
    PNR_REQUIRE(rays && hit_t && hit_count && rays_out, "pnr_restrict_rays: null pointer");
    PNR_REQUIRE(((((uintptr_t)rays) | ((uintptr_t)rays_out)) & 15) == 0, "pnr_restrict_rays: ray records must be 16-byte aligned");
    hipLaunchKernelGGL(k_restrict_rays, dim3(pnr_grid_cap((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rays, n_rays,
                       hit_t, hit_count, max_hits, rays_out);
    PNR_CHECK_LAUNCH("pnr_restrict_rays");
    return PNR_OK;
}
