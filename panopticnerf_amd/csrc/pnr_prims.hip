// a8b: ray / convex-polytope intersection for the 3D prior (include/pnr.h "a8b: convex bounding primitives").  gfx950 only.
// The producer of the hit lists (hit_t, hit_box, hit_count) for scenes given as half-space tables instead of the cuboid table of
// k_bbox_hits; everything downstream (pnr_sample_labels, pnr_sample_pdf_labels, pnr_restrict_rays) consumes those lists unchanged.
#include <math.h>

#include "pnr_common.h"
#include "pnr_sampling_dev.h"

// One thread per ray, 256-thread blocks, grid-stride in whole blocks (the trip structure is block-uniform; the tail's surplus
// lanes carry act = false).  The primitive loop and the plane loop are wave-uniform: offsets[] and the 16-byte plane records are
// read through scalar loads (P * 16 B: cache resident), a plane costs two 3-term dot products, one correctly rounded division
// and three selects.
//
// Early exit: a primitive is left when NO lane of the wave can still hit it (one ballot per plane).  The exit condition is
// tmin > tmax, not !(tmin <= tmax): tmin only grows and tmax only shrinks (fmaxf / fminf drop a NaN quotient), so tmin > tmax
// is final, whereas a NaN bound (a NaN near / far) could still be replaced by a later plane -- such a lane keeps the wave in
// the loop.  The hit lists therefore do not depend on which lanes share a wave.
//
// The per-ray list: LDS = true (max_hits <= CONVEX_LDS_MAXH) keeps it in LDS as [entry][thread] (k_ray_setup's layout: a thread
// touches only its own column, conflict-free, no barrier) and writes the output rows once at the end; LDS = false builds it in
// the output rows as k_bbox_hits does, through the shared hit list of pnr_sampling_dev.h (hit_init, hit_insert).  Same insertion,
// same order: the max_hits nearest, ascending (t_in, primitive index).  The LDS form is a kept copy on purpose, as in k_ray_setup:
// through the shared pieces on an LDS column the kernel measured 121.3 us against 120.7 per frame, the parent's own spread being
// 0.4 (profiles/sampling_frame/ab.txt).  Change the pieces and this together.
#define CONVEX_LDS_MAXH 8

template <bool LDS>
__global__ __launch_bounds__(256) void k_convex_hits(const float* __restrict__ rays, int64_t R, const float4* __restrict__ planes,
                                                     const int32_t* __restrict__ offsets, int M, int max_hits,
                                                     float* __restrict__ hit_t, int32_t* __restrict__ hit_box,
                                                     int32_t* __restrict__ hit_count)
{
    __shared__ float2 s_t[LDS ? CONVEX_LDS_MAXH : 1][256];      // (t_in, t_out)
    __shared__ int s_hb[LDS ? CONVEX_LDS_MAXH : 1][256];
    const int tid = threadIdx.x;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < R; base += (int64_t)gridDim.x * 256) {
        const int64_t r = base + tid;
        const bool act = r < R;
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, nr = 0.0f, fr = 0.0f;
        if (act) {
            o0 = rays[r * 8 + 0]; o1 = rays[r * 8 + 1]; o2 = rays[r * 8 + 2];
            d0 = rays[r * 8 + 3]; d1 = rays[r * 8 + 4]; d2 = rays[r * 8 + 5];
            nr = rays[r * 8 + 6]; fr = rays[r * 8 + 7];
            if constexpr (LDS) {
#pragma unroll
                for (int h = 0; h < CONVEX_LDS_MAXH; ++h) { s_hb[h][tid] = -1; s_t[h][tid] = make_float2(0.0f, 0.0f); }
            } else {
                hit_init(hit_rows(hit_t, hit_box, r, max_hits), max_hits);      // the list, in the ray's output rows
            }
        }
        int cnt = 0;
        int p = M > 0 ? offsets[0] : 0;
        for (int m = 0; m < M; ++m) {
            const int pe = offsets[m + 1];
            float tmin = nr, tmax = fr;
            for (; p < pe; ++p) {
                const float4 pl = planes[p];
                const float dn = (pl.x * d0 + pl.y * d1) + pl.z * d2;
                const float on = (pl.x * o0 + pl.y * o1) + pl.z * o2;
                const float s = pl.w - on;
                const float q = s / dn;                         // read only where dn != 0
                if (dn > 0.0f) tmax = fminf(tmax, q);           // leaving
                else if (dn < 0.0f) tmin = fmaxf(tmin, q);      // entering
                else if (dn == 0.0f && s < 0.0f) tmax = -INFINITY;      // parallel and outside (-0.0f == 0.0f)
                if (__ballot(act && !(tmin > tmax)) == 0ull) break;     // the whole wave has missed this primitive
            }
            p = pe;
            if (act && tmin <= tmax) {
                if constexpr (LDS) {            // hit_insert on the LDS column: a kept copy (see the comment above the kernel)
                    const int n = cnt < max_hits ? cnt : max_hits;
                    int pos = n;
                    while (pos > 0 && s_t[pos - 1][tid].x > tmin) --pos;
                    if (pos < max_hits) {
                        for (int k = (n < max_hits ? n : max_hits - 1); k > pos; --k) {
                            s_t[k][tid] = s_t[k - 1][tid];
                            s_hb[k][tid] = s_hb[k - 1][tid];
                        }
                        s_t[pos][tid] = make_float2(tmin, tmax);
                        s_hb[pos][tid] = m;
                    }
                    ++cnt;
                } else {
                    hit_insert(hit_rows(hit_t, hit_box, r, max_hits), cnt, max_hits, tmin, tmax, m);
                }
            }
        }
        if (act) {
            hit_count[r] = cnt;             // TRUE number of primitives hit: > max_hits reports the overflow
            if constexpr (LDS) {
                for (int h = 0; h < max_hits; ++h) {
                    *reinterpret_cast<float2*>(hit_t + (r * max_hits + h) * 2) = s_t[h][tid];
                    hit_box[r * max_hits + h] = s_hb[h][tid];
                }
            }
        }
    }
}

PNR_EXPORT int pnr_convex_hits(const float* rays, int64_t n_rays, const float* planes, const int32_t* offsets, int n_prim,
                               int max_hits, float* hit_t, int32_t* hit_box, int32_t* hit_count, void* stream)
{
    PNR_REQUIRE(n_rays <= 0 || (rays && hit_t && hit_box && hit_count), "pnr_convex_hits: null pointer");
    PNR_REQUIRE(n_prim >= 0, "pnr_convex_hits: n_prim=%d is negative", n_prim);
    PNR_REQUIRE(n_rays <= 0 || n_prim == 0 || (planes && offsets), "pnr_convex_hits: null primitive table (planes, offsets) with n_prim=%d", n_prim);
    PNR_REQUIRE(max_hits >= 1, "pnr_convex_hits: max_hits=%d must be >= 1", max_hits);
    PNR_REQUIRE((((uintptr_t)planes) & 15) == 0 && (((uintptr_t)hit_t) & 7) == 0, "pnr_convex_hits: planes must be 16-byte and hit_t 8-byte aligned");
    if (n_rays <= 0) return PNR_OK;
    const dim3 grid(pnr_grid_cap((n_rays + 255) / 256)), block(256);
    if (max_hits <= CONVEX_LDS_MAXH)
        hipLaunchKernelGGL(k_convex_hits<true>, grid, block, 0, (hipStream_t)stream, rays, n_rays, (const float4*)planes, offsets, n_prim,
                           max_hits, hit_t, hit_box, hit_count);
    else
        hipLaunchKernelGGL(k_convex_hits<false>, grid, block, 0, (hipStream_t)stream, rays, n_rays, (const float4*)planes, offsets, n_prim,
                           max_hits, hit_t, hit_box, hit_count);
    PNR_CHECK_LAUNCH("pnr_convex_hits");
    return PNR_OK;
}
