// The shared frame of the sampling and hit-list family: k_stratified, k_sample_pdf<...>, k_sample_pdf_det, k_bbox_hits, k_ray_setup,
// k_sample_labels, k_restrict_rays (pnr_sampling.hip) and k_convex_hits (pnr_prims.hip).  Every piece that is BIT-EXACT-critical
// against oracle/pnr_oracle.c exists once here -- torch's linspace and sum order, the double-precision cumsum, the inverse-CDF
// interpolation, the slab test, the nearest-max_hits insertion -- and each kernel keeps its own body and schedule and is assembled
// from them.  All __forceinline__: no kernel's scratch grows or occupancy drops against the piece spelled out in place
// (tools/isa_diff.py, profiles/sampling_frame/).  What is deliberately NOT here: the searches (loops in sample_pdf_body, fixed-depth
// bisections in k_sample_pdf_det), the two label loops over registers (k_sample_pdf_det, k_ray_setup phase 2), and the LDS-column
// hit lists of k_ray_setup phase 1 and k_convex_hits<true> (measured slower through the shared pieces: see "hit lists" below).
// Same operations in the same order, one rounding each: an FMA exists only where the source says fmaf.
#pragma once
#include "pnr_common.h"

#pragma clang fp contract(off)

// torch.linspace(0, 1, N)[i] as ATen's CPU kernel computes it (two-sided; the upper half from the end point with one
// rounding): oracle/pnr_oracle.c::pnro_linspace01, measured bit-exact against torch.
__device__ __forceinline__ float pnr_linspace01(int i, int N)
{
    if (N <= 1) return 0.0f;
    const float step = 1.0f / (float)(N - 1);
    if (i < N / 2) return step * (float)i;
    return fmaf(-step, (float)(N - 1 - i), 1.0f);
}

// ------------------------------------------------------------------------------------------------------------------- a3
__device__ __forceinline__ float strat_z(float nr, float fr, int i, int N, int lindisp)
{
    const float t = pnr_linspace01(i, N);
    const float omt = 1.0f - t;
    if (!lindisp) {
        const float a = nr * omt, b = fr * t;
        return a + b;
    }
    const float a = (1.0f / nr) * omt, b = (1.0f / fr) * t;
    return 1.0f / (a + b);
}

// sample i of a ray's N: the stratified depth, jittered inside its bin by *t when t is given (k_stratified, k_ray_setup)
__device__ __forceinline__ float strat_sample(float nr, float fr, int i, int N, int lindisp, const float* t)
{
    const float zi = strat_z(nr, fr, i, N, lindisp);
    if (!t) return zi;
    const float z0 = strat_z(nr, fr, 0, N, lindisp), zl = strat_z(nr, fr, N - 1, N, lindisp);
    const float lo = (i == 0) ? z0 : 0.5f * (zi + strat_z(nr, fr, i - 1, N, lindisp));
    const float up = (i == N - 1) ? zl : 0.5f * (strat_z(nr, fr, i + 1, N, lindisp) + zi);
    const float w = up - lo;
    const float m = w * *t;
    return lo + m;
}

// ------------------------------------------------------------------------------------------------------------------- a8: rays and boxes
struct RayRec { float o0, o1, o2, d0, d1, d2, nr, fr; };

// ray r of the (R, 8) record array: origin, direction, near, far (eight dword loads; hipcc merges them into two 16-byte ones)
__device__ __forceinline__ RayRec ray_load(const float* rays, int64_t r)
{
    const float* p = rays + r * 8;
    return RayRec{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
}

// the ray's interval inside one oriented box (b: centre, three axis rows, half extents -- 15 floats), starting from [near, far];
// the box is hit when *tmin <= *tmax.  pnro_bbox_hits' slab test.
__device__ __forceinline__ void slab_interval(const float* b, const RayRec& ry, float* tmin_out, float* tmax_out)
{
    const float p0 = ry.o0 - b[0], p1 = ry.o1 - b[1], p2 = ry.o2 - b[2];
    float tmin = ry.nr, tmax = ry.fr;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float r0 = b[3 + 3 * a], r1 = b[4 + 3 * a], r2 = b[5 + 3 * a];
        const float ol = (r0 * p0 + r1 * p1) + r2 * p2;
        const float dl = (r0 * ry.d0 + r1 * ry.d1) + r2 * ry.d2;
        const float inv = 1.0f / dl;
        const float e = b[12 + a];
        const float t1 = (-e - ol) * inv, t2 = (e - ol) * inv;
        tmin = fmaxf(tmin, fminf(t1, t2));
        tmax = fminf(tmax, fmaxf(t1, t2));
    }
    *tmin_out = tmin;
    *tmax_out = tmax;
}

// ------------------------------------------------------------------------------------------------------------------- hit lists
// One ray's list of kept intervals behind a small accessor: entry h is iv(h) = (t_in, t_out), box(h).  HitRows is the list in the
// ray's output rows in global memory (hit_t (R, max_hits, 2), hit_box (R, max_hits); no alignment assumed, so an interval is two
// dword accesses): k_bbox_hits, k_convex_hits<false>, k_restrict_rays.  hit_init / hit_insert / hit_hull take any such accessor.
// The second form, one thread's column of [entry][thread] LDS arrays (k_ray_setup phase 1, k_convex_hits<true>), was built and
// measured -- bit-identical, same registers and LDS, 4 % and 0.5 % slower than the lists spelled out in place, outside the
// parent's run-to-run spread -- so those two kernels keep their own copies (profiles/sampling_frame/).
template <class F, class I>
struct HitRows {
    F* t; I* b;             // the ray's own rows: hit_t + r max_hits 2, hit_box + r max_hits
    __device__ __forceinline__ float t_in(int h) const { return t[h * 2]; }
    __device__ __forceinline__ float2 iv(int h) const { return make_float2(t[h * 2], t[h * 2 + 1]); }
    __device__ __forceinline__ int box(int h) const { return b[h]; }
    __device__ __forceinline__ void set(int h, float2 v, int m) const { t[h * 2] = v.x; t[h * 2 + 1] = v.y; b[h] = m; }
};
template <class F, class I>
__device__ __forceinline__ HitRows<F, I> hit_rows(F* hit_t, I* hit_box, int64_t r, int max_hits)
{
    return HitRows<F, I>{hit_t + r * max_hits * 2, hit_box + r * max_hits};
}

// n empty entries: box -1, interval (0, 0)
template <class L>
__device__ __forceinline__ void hit_init(const L& l, int n)
{
    for (int h = 0; h < n; ++h) l.set(h, make_float2(0.0f, 0.0f), -1);
}

// Keep the max_hits NEAREST intervals, ascending (t_in, index m): a street-scene ray crosses more boxes than max_hits, and the near
// ones are the ones its samples fall in.  Insertion from the back; the farthest entry falls off the end.  cnt is the TRUE number of
// hits so far: > max_hits reports the overflow.  (Same op order as pnro_bbox_hits: bit-exact.)
template <class L>
__device__ __forceinline__ void hit_insert(const L& l, int& cnt, int max_hits, float tmin, float tmax, int m)
{
    const int n = cnt < max_hits ? cnt : max_hits;
    int pos = n;
    while (pos > 0 && l.t_in(pos - 1) > tmin) --pos;
    if (pos < max_hits) {
        for (int k = (n < max_hits ? n : max_hits - 1); k > pos; --k) l.set(k, l.iv(k - 1), l.box(k - 1));
        l.set(pos, make_float2(tmin, tmax), m);
    }
    ++cnt;
}

// the hull [min t_in, max t_out] of the kept > 0 first entries (pnr_restrict_rays: it replaces [near, far])
template <class L>
__device__ __forceinline__ void hit_hull(const L& l, int kept, float* near_out, float* far_out)
{
    float2 v = l.iv(0);
    float lo = v.x, hi = v.y;
    for (int h = 1; h < kept; ++h) {
        v = l.iv(h);
        lo = fminf(lo, v.x);
        hi = fmaxf(hi, v.y);
    }
    *near_out = lo;
    *far_out = hi;
}

// the kept interval a sample at depth zz takes its label from: the one with the smallest t_in among those containing it (-1: none)
template <class F>
__device__ __forceinline__ int label_hit(float zz, int cnt, F interval)
{
    int best = -1;
    float bt = 0.0f;
    for (int h = 0; h < cnt; ++h) {
        float ti, to;
        interval(h, ti, to);
        if (ti <= zz && zz <= to && (best < 0 || ti < bt)) {
            best = h;
            bt = ti;
        }
    }
    return best;
}

// the ids of the winning hit: best = its entry (-1: none -> -1 / -1), *box_of_best its box index (read only when best >= 0)
__device__ __forceinline__ void hit_ids(int best, const int32_t* box_of_best, const int32_t* __restrict__ box_ids, int* ls, int* li)
{
    *ls = -1;
    *li = -1;
    if (best >= 0) {
        const int m = *box_of_best;
        *ls = box_ids[m * 2];
        *li = box_ids[m * 2 + 1];
    }
}

// ------------------------------------------------------------------------------------------------------------------- a7: one wave per ray
// the union of Nt depths is padded to a power of two for the bitonic sort
__host__ __device__ __forceinline__ int pdf_padded(int Nt)
{
    int P = 1;
    while (P < Nt) P <<= 1;
    return P;
}

// total = torch.sum(w[1:-1] + 1e-5) over the nw = Nc - 2 inner weights (s_w: the ray's Nc weights in LDS, visible) in ATen's order
// (pnro_torch_sum).  nw >= 8: 8-lane vectors, four partial vectors interleaved -> lane 8 k + l owns accumulator (k, l) and adds its
// elements in ascending order, exactly as the vector code does; then the scalar tail from 0 and the 8 lanes of partial 0.  nw < 8 (no
// whole vector) is ATen's scalar row sum with four accumulators: a[k] = x[k], k < 4 (when nw >= 4), x[4..] added in order into a[0],
// result ((a[0] + a[1]) + a[2]) + a[3].  Same code: the "tail" is then a[0] (x[0], x[4], x[5], ...), lanes 0..2 hold a[1..3] as
// partials (0, l) (+ 0 is exact), and the lane-order adds finish it.  Two barriers; every lane returns the total.
__device__ __forceinline__ float pdf_torch_total(const float* s_w, int nw, float* s_part, float* s_total, int lane)
{
    const bool short4 = nw >= 4 && nw < 8;       // a row ATen sums with four scalar accumulators
    if (lane < 32) {
        const int k = lane >> 3, l = lane & 7, nv = nw / 8, groups = nv / 4;
        float pacc = 0.0f;
        for (int g = 0; g < groups; ++g) pacc = pacc + (s_w[(g * 4 + k) * 8 + l + 1] + 1e-5f);
        if (k == 0)
            for (int v = groups * 4; v < nv; ++v) pacc = pacc + (s_w[v * 8 + l + 1] + 1e-5f);
        if (short4 && lane < 3) pacc = pacc + (s_w[lane + 2] + 1e-5f);       // a[1..3] of the scalar row sum
        s_part[lane] = pacc;
    }
    __syncthreads();
    if (lane == 0) {
        const int nv = nw / 8;
        float total = 0.0f;
        // the scalar tail, from 0 (a short row's a[0]: x[0], then x[4] onwards)
        for (int j = nv * 8; j < nw; j = (short4 && j == 0) ? 4 : j + 1) total = total + (s_w[j + 1] + 1e-5f);
        for (int l = 0; l < 8; ++l) {
            float p0 = s_part[l];
            p0 = p0 + s_part[8 + l]; p0 = p0 + s_part[16 + l]; p0 = p0 + s_part[24 + l];
            total = total + p0;
        }
        *s_total = total;
    }
    __syncthreads();
    return *s_total;
}

// pdf -> cdf[0 .. nw] in LDS.  pl: this lane's pdf[lane] (0 for lane >= nw); s_pdf: all nw of them, written by this wave (behind a
// barrier or not: the chain below brings its own); one_per_lane: nw <= 64 (a constant where the caller's shapes guarantee it).
// torch.cumsum: the running sum is kept in DOUBLE, every output rounded to fp32 -- a sequential chain of nw f64 adds (with its LDS
// traffic, half of the general body's issue cycles when one lane walks it).  The pdf values are fp32 and non-negative: when every
// one of them is 0 or >= 2^-28, each is a multiple of 2^-51, and when their sum is < 2 so is every partial sum of ANY subset -- 52
// significant bits at most: no f64 add ever rounds, and a parallel prefix scan returns the sequential chain's values bit for bit.
// (pdf_j >= 1e-5 / total and sum(pdf) ~ 1: always the case for compositing weights; the sum is checked on the scan's own result,
// which is exact whenever the true sum is < 2.)  Otherwise, and for more than 64 values, the sequential chain runs.  Ends in a barrier.
__device__ __forceinline__ void pdf_cdf(float pl, int nw, bool one_per_lane, const float* s_pdf, float* s_cdf, int lane)
{
    double c = (double)pl;
    bool exact = one_per_lane && __all(pl == 0.0f || pl >= 0x1p-28f);
    if (exact) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_up(c, d, 64);
            if (lane >= d) c += o;
        }
        exact = __shfl(c, 63, 64) < 1.999;
    }
    if (exact) {
        if (lane == 0) s_cdf[0] = 0.0f;
        if (lane < nw) s_cdf[lane + 1] = (float)c;
    } else {                            // wave-uniform: the whole block (one wave) is here
        __syncthreads();
        if (lane == 0) {
            double cc = 0.0;
            s_cdf[0] = 0.0f;
            for (int j = 0; j < nw; ++j) {
                cc += (double)s_pdf[j];
                s_cdf[j + 1] = (float)cc;
            }
        }
    }
    __syncthreads();
}

// the sample at u, given inds = the number of cdf[0 .. nb) entries <= u (the caller's search): linear inside its bin
__device__ __forceinline__ float pdf_invert(float uu, int inds, int nb, const float* s_cdf, const float* s_bins)
{
    const int below = inds - 1 > 0 ? inds - 1 : 0;
    const int above = inds < nb - 1 ? inds : nb - 1;
    const float cb = s_cdf[below];
    float denom = s_cdf[above] - cb;
    if (denom < 1e-5f) denom = 1.0f;
    const float t = (uu - cb) / denom;
    const float bb = s_bins[below];
    const float span = s_bins[above] - bb;
    const float m = t * span;
    return bb + m;
}

// ascending bitonic sort of s_sort[0 .. P) (P a power of two, the padding +inf, visible on entry); ends in a barrier
__device__ __forceinline__ void pdf_bitonic(float* s_sort, int P, int lane)
{
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const float a = s_sort[i], b = s_sort[p];
                const bool asc = (i & k) == 0;
                if ((a > b) == asc) {
                    s_sort[i] = b;
                    s_sort[p] = a;
                }
            }
            __syncthreads();
        }
    }
}
