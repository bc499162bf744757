// Point splatting (include/pnr.h "point splatting"): world points are projected into a view of any camera model and scattered
// into a z-buffer of packed 64-bit keys (depth bits, point index) with one native unsigned 64-bit atomic minimum per covered
// pixel, so the nearest point wins, a depth tie goes to the lowest index and the result does not depend on arrival order; a
// second kernel unpacks the buffer into a depth and an index image; a third accumulates depth-error metrics of a predicted
// depth image against such a ground truth (its double sums in the order of DESIGN.md section 8 "Ordered reductions",
// pnr_reduce_dev.h).  Small scatter- / gather-bound kernels: one thread per point or pixel, grid-stride, the view
// (PnrView) in the kernel arguments; the key is pnr_key (both pnr_geom_dev.h).  The projection is pnr_project_point (pnr_camera_dev.h)
// and nothing else, so the arithmetic is k_project_points' bit for bit (the nearest pixel and the stored depth are k_reproject's); tests/_splat_ref.py restates the whole rule in numpy.
#include <float.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"

// -DPNR_SPLAT_PREREAD=1 (A/B builds): a plain read of the cell skips the atomic when the key cannot lower it.  A cell only ever
// decreases, so a stale read errs towards issuing the atomic.  Off by default; tools/splat_time.py is its A/B (profiles/README.md
// "Splatting").
#ifndef PNR_SPLAT_PREREAD
#define PNR_SPLAT_PREREAD 0
#endif

#define PNR_DM_MAX_BLOCKS 1024            // k_depth_metrics' grid limit: what pnr_depth_metrics_workspace_bytes sizes for

struct SplatArgs {
    PnrView view;                       // pose = w2c
    float umax, vmax, near_, far_;
    const float* points; int64_t n;
    unsigned int index_base;
    unsigned long long *zbuf, *stats;
};

template <int RADIUS>
__global__ __launch_bounds__(256) void k_splat_points(const SplatArgs a)
{
    __shared__ unsigned int h[4];
    unsigned int cnt[3] = {0, 0, 0};                    // landed / left the view / clipped
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const float X = a.points[3 * i], Y = a.points[3 * i + 1], Z = a.points[3 * i + 2];
        const PnrProj q = pnr_project_point(a.view.model, a.view.cam, a.view.pose, a.umax, X, Y, Z);
        int slot = 1;
        if (q.dom && pnr_uv_inside(q.u, q.v, a.umax, a.vmax)) {
            const int wmax = a.view.width - 1, hmax = a.view.height - 1;
            const int iu = pnr_nearest_pixel(q.u, wmax), iv = pnr_nearest_pixel(q.v, hmax);
            const float e = pnr_view_depth(a.view.model, q);
            slot = 2;
            if (e >= a.near_ && e <= a.far_) {
                slot = 0;
                const unsigned long long key = pnr_key(e, a.index_base + (unsigned int)i);
#pragma unroll
                for (int dy = -RADIUS; dy <= RADIUS; ++dy) {
#pragma unroll
                    for (int dx = -RADIUS; dx <= RADIUS; ++dx) {
                        const int x = iu + dx, y = iv + dy;
                        if (x >= 0 && x <= wmax && y >= 0 && y <= hmax) {       // clipped at the border, never wrapped
                            unsigned long long* cell = a.zbuf + ((int64_t)y * a.view.width + x);
#if PNR_SPLAT_PREREAD
                            if (key < *(volatile unsigned long long*)cell) atomicMin(cell, key);
#else
                            atomicMin(cell, key);
#endif
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) cnt[k] += slot == k ? 1u : 0u;              // (constant indices: cnt stays in registers)
    }
    if (a.stats) pnr_block_count_add(cnt, h, a.stats);  // (uniform over the block)
}

__global__ __launch_bounds__(256) void k_splat_resolve(const unsigned long long* __restrict__ zbuf, int64_t n_pix, float* __restrict__ depth,
                                                       int32_t* __restrict__ index)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_pix; q += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long c = zbuf[q];
        const bool empty = c == PNR_KEY_EMPTY;
        if (depth) depth[q] = empty ? 0.0f : pnr_key_value(c);
        if (index) index[q] = empty ? -1 : (int32_t)pnr_key_index(c);
    }
}

struct DepthMetricArgs {
    const float *pred, *gt;
    const uint8_t* mask;
    int64_t n;
    float d_min, d_max;
    double* partial;                    // [blocks][5]
    double* sums;
    unsigned long long* counts;
    int n_blocks;
};

__global__ __launch_bounds__(PNR_REDUCE_BLOCK) void k_depth_metrics(const DepthMetricArgs a)
{
    __shared__ double red[4][5];
    __shared__ unsigned int hc[5];
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned int cnt[5] = {0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        if (a.mask && a.mask[i] == 0) continue;
        const float g = a.gt[i];
        if (!(fabsf(g) <= FLT_MAX && g >= a.d_min && g <= a.d_max)) continue;
        const float p = a.pred[i];
        if (!pnr_pos_finite(p)) {
            cnt[4] += 1u;
            continue;
        }
        cnt[0] += 1u;
        const float ratio = fmaxf(p / g, g / p);
        cnt[1] += ratio < 1.25f ? 1u : 0u;
        cnt[2] += ratio < 1.5625f ? 1u : 0u;
        cnt[3] += ratio < 1.953125f ? 1u : 0u;
        const double gd = (double)g;
        const double d = (double)p - gd;
        const double ad = fabs(d), d2 = d * d;
        const double l = log((double)p) - log(gd);
        s[0] += ad;
        s[1] += d2;
        s[2] += ad / gd;
        s[3] += d2 / gd;
        s[4] += l * l;
    }
    pnr_block_sum_rows(s, red, a.partial, 5);
    pnr_block_count_add(cnt, hc, a.counts);
}

// one block: term t adds the partials of blocks 0, 1, ... in that order, then once into sums[t] (no floating atomics anywhere)
__global__ __launch_bounds__(64) void k_depth_metrics_final(const DepthMetricArgs a)
{
    if (threadIdx.x >= 5) return;
    const double v = pnr_rows_total<5>((const unsigned long long*)a.partial, a.n_blocks, threadIdx.x).sum;
    a.sums[threadIdx.x] = a.sums[threadIdx.x] + v;
}

PNR_EXPORT int pnr_splat_points(int model, const float* cam_host, const float* w2c12_host, int width, int height, const float* points,
                                int64_t n, int64_t index_base, float near_, float far_, int radius, int64_t* zbuf, int64_t* stats,
                                void* stream)
{
    SplatArgs a;
    const int rc = pnr_view_check("pnr_splat_points", nullptr, model, cam_host, w2c12_host, width, height, true, a.view);
    if (rc) return rc;
    PNR_REQUIRE(n >= 0 && (int64_t)width * height <= INT32_MAX, "pnr_splat_points: bad size (n >= 0, the image holds at most 2^31 - 1 pixels)");
    PNR_REQUIRE(radius >= 0 && radius <= 2, "pnr_splat_points: radius must be 0, 1 or 2 (got %d)", radius);
    PNR_REQUIRE(near_ >= 0.0f && far_ >= near_, "pnr_splat_points: near and far must satisfy 0 <= near <= far (far may be +inf)");
    PNR_REQUIRE(index_base >= 0 && index_base + n <= (int64_t)INT32_MAX, "pnr_splat_points: index_base + n must stay within 0 .. 2^31 - 1");
    if (n == 0) return PNR_OK;                  // before the pointer checks: an empty cloud has a null pointer
    PNR_REQUIRE(points && zbuf, "pnr_splat_points: null points or zbuf");
    a.umax = pnr_view_umax(a.view); a.vmax = pnr_view_vmax(a.view); a.near_ = near_; a.far_ = far_;
    a.points = points; a.n = n; a.index_base = (unsigned int)index_base;
    a.zbuf = (unsigned long long*)zbuf; a.stats = (unsigned long long*)stats;
    const int grid = pnr_grid_cap((n + 255) / 256);
    if (radius == 0) hipLaunchKernelGGL(k_splat_points<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else if (radius == 1) hipLaunchKernelGGL(k_splat_points<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_splat_points<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_splat_points");
    return PNR_OK;
}

PNR_EXPORT int pnr_splat_resolve(const int64_t* zbuf, int64_t n_pix, float* depth, int32_t* index, void* stream)
{
    PNR_REQUIRE(n_pix >= 0, "pnr_splat_resolve: bad size");
    if (n_pix == 0 || (!depth && !index)) return PNR_OK;
    PNR_REQUIRE(zbuf, "pnr_splat_resolve: null zbuf");
    const int grid = pnr_grid_cap((n_pix + 255) / 256);
    hipLaunchKernelGGL(k_splat_resolve, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)zbuf, n_pix, depth, index);
    PNR_CHECK_LAUNCH("pnr_splat_resolve");
    return PNR_OK;
}

PNR_EXPORT int64_t pnr_depth_metrics_workspace_bytes(int64_t n)
{
    if (n < 0) return -1;
    return pnr_reduce_blocks(n, PNR_DM_MAX_BLOCKS) * 5 * (int64_t)sizeof(double);
}

PNR_EXPORT int pnr_depth_metrics(const float* pred, const float* gt, const uint8_t* mask, int64_t n, float d_min, float d_max,
                                 double* sums, int64_t* counts, void* workspace, void* stream)
{
    PNR_REQUIRE(n >= 0, "pnr_depth_metrics: bad size");
    PNR_REQUIRE(d_min > 0.0f && d_min <= d_max && d_max <= FLT_MAX, "pnr_depth_metrics: the range must satisfy 0 < d_min <= d_max, both finite");
    if (n == 0) return PNR_OK;
    PNR_REQUIRE(pred && gt && sums && counts && workspace, "pnr_depth_metrics: null pointer");
    PNR_REQUIRE((((uintptr_t)sums | (uintptr_t)counts | (uintptr_t)workspace) & 7) == 0, "pnr_depth_metrics: sums, counts and workspace must be 8-byte aligned");
    DepthMetricArgs a;
    a.pred = pred; a.gt = gt; a.mask = mask; a.n = n; a.d_min = d_min; a.d_max = d_max;
    a.partial = (double*)workspace; a.sums = sums; a.counts = (unsigned long long*)counts;
    const int64_t blocks = pnr_reduce_blocks(n, PNR_DM_MAX_BLOCKS);
    a.n_blocks = pnr_grid_cap(blocks, 4);               // (never above `blocks`: the workspace holds it)
    hipLaunchKernelGGL(k_depth_metrics, dim3(a.n_blocks), dim3(PNR_REDUCE_BLOCK), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(k_depth_metrics_final, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_depth_metrics");
    return PNR_OK;
}
