// Cross-view reprojection (include/pnr.h "cross-view reprojection"): a source pixel is lifted with the source depth image,
// projected into the target view, matched to the nearest target pixel and tested against the target depth image; with label
// images on both sides the visible pairs are counted into the cross-view confusion matrix of the multi-view consistency metric.
// A small gather-bound kernel: one thread per source pixel, grid-stride, the two views (PnrView, pnr_geom_dev.h) in the kernel
// arguments.  The ray is pnr_camera_ray and the projection pnr_project_point (pnr_camera_dev.h), the same functions
// the ray and projection kernels call, so the arithmetic is theirs bit for bit; the nearest pixel and the depth a view stores
// are that header's too, the reduction of the stats is pnr_reduce_dev.h's.  tests/_warp_ref.py
// restates the whole rule in float32 (tests/_pano_ref.py with a panoramic view on either side).
#include <float.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"

#define PNR_WARP_LDS_CLASSES 128        // up to here `agree` is a per-block LDS histogram (k_confusion's limit: 64 KiB)

struct ReprojectArgs {
    PnrView src, tgt;                   // src.pose = c2w of the source, tgt.pose = w2c of the target
    int64_t npix_src;
    float umax, vmax, tol_abs, tol_rel; // the bounds of tgt
    const int32_t* pix; int64_t R;
    const float *depth_src, *depth_tgt;
    const int32_t *label_src, *label_tgt;
    int n_classes;
    int32_t* match; float2* uv;
    unsigned long long *agree, *stats;
};

// HIST: agree through the per-block LDS histogram h[n_classes^2] (one global atomic per non-zero cell, as k_confusion);
// otherwise one global atomic per counted pixel (as k_confusion_big).  h holds at least 8 words in either case: after the
// histogram is flushed its first five words collect the block's stats.
template <bool HIST>
__global__ __launch_bounds__(256) void k_reproject(const ReprojectArgs a)
{
    extern __shared__ unsigned int h[];
    const bool count = a.agree != nullptr;              // (the entry point refuses agree without labels)
    const int cells = a.n_classes * a.n_classes;
    if (HIST && count) {
        for (int i = threadIdx.x; i < cells; i += blockDim.x) h[i] = 0;
        __syncthreads();
    }
    unsigned int cnt[5] = {0, 0, 0, 0, 0};
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = a.pix ? (int64_t)a.pix[r] : r;
        int code = -1;
        float u = 0.0f, v = 0.0f;
        if (p >= 0 && p < a.npix_src) {                 // an index outside the source image has nothing to reproject
            const int j = (int)(p / a.src.width), i = (int)(p - (int64_t)j * a.src.width);
            bool ok;
            const PnrRayRec ray = pnr_camera_ray(a.src.model, a.src.cam, a.src.pose, i, j, 0.0f, 0.0f, ok);
            const float t = a.depth_src[p];
            const bool have = pnr_pos_finite(t);     // (named first: called inside the chain below, the compiler lays the kernel out anew)
            if (ok && have) {
                const float X = ray.lo.x + t * ray.lo.w, Y = ray.lo.y + t * ray.hi.x, Z = ray.lo.z + t * ray.hi.y;
                const PnrProj q = pnr_project_point(a.tgt.model, a.tgt.cam, a.tgt.pose, a.umax, X, Y, Z);
                u = q.u;
                v = q.v;
                code = -2;
                if (q.dom && pnr_uv_inside(u, v, a.umax, a.vmax)) {
                    const int tq = pnr_nearest_pixel(v, a.tgt.height - 1) * a.tgt.width + pnr_nearest_pixel(u, a.tgt.width - 1);
                    code = tq;
                    if (a.depth_tgt) {
                        const float e = pnr_view_depth(a.tgt.model, q);
                        const float dt = a.depth_tgt[tq];
                        if (!pnr_pos_finite(dt)) code = -3;
                        else if (!(fabsf(e - dt) <= a.tol_abs + a.tol_rel * e)) code = -4;
                    }
                    if (code >= 0 && count) {
                        const int ls = a.label_src[p], lt = a.label_tgt[tq];
                        if (ls >= 0 && ls < a.n_classes && lt >= 0 && lt < a.n_classes) {
                            if (HIST) atomicAdd(&h[ls * a.n_classes + lt], 1u);
                            else atomicAdd(&a.agree[(int64_t)ls * a.n_classes + lt], 1ull);
                        }
                    }
                }
            }
        }
        if (a.match) a.match[r] = code;
        if (a.uv) a.uv[r] = make_float2(u, v);
        const int slot = code >= 0 ? 0 : -code;
#pragma unroll
        for (int k = 0; k < 5; ++k) cnt[k] += slot == k ? 1u : 0u;         // (constant indices: cnt stays in registers)
    }
    if (HIST && count) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += blockDim.x)
            if (h[i]) atomicAdd(&a.agree[i], (unsigned long long)h[i]);
    }
    if (a.stats) pnr_block_count_add(cnt, h, a.stats);  // (uniform over the block; h is free once the histogram is flushed)
}

PNR_EXPORT int pnr_reproject(int model_src, const float* cam_src_host, const float* c2w_src12_host, int width_src, int height_src,
                             const int32_t* pix, int64_t n, const float* depth_src,
                             int model_tgt, const float* cam_tgt_host, const float* w2c_tgt12_host, int width_tgt, int height_tgt,
                             const float* depth_tgt, float tol_abs, float tol_rel,
                             const int32_t* label_src, const int32_t* label_tgt, int n_classes,
                             int32_t* match, float* uv, int64_t* agree, int64_t* stats, void* stream)
{
    PNR_REQUIRE(pnr_camera_model_ok(model_src) && pnr_camera_model_ok(model_tgt), "pnr_reproject: unknown camera model %d -> %d", model_src, model_tgt);
    PNR_REQUIRE(cam_src_host && c2w_src12_host && cam_tgt_host && w2c_tgt12_host, "pnr_reproject: null camera or pose");
    PNR_REQUIRE(width_src >= 1 && height_src >= 1 && width_tgt >= 1 && height_tgt >= 1 && n >= 0 &&
                (int64_t)width_src * height_src <= INT32_MAX && (int64_t)width_tgt * height_tgt <= INT32_MAX,
                "pnr_reproject: bad size (each image holds at most 2^31 - 1 pixels)");
    if (n == 0) return PNR_OK;                  // before the pointer checks: an empty pixel list has a null pointer
    PNR_REQUIRE(pix || n == (int64_t)width_src * height_src, "pnr_reproject: without pixel indices n must be width_src*height_src");
    ReprojectArgs a;                            // (the cameras are checked once there is work, as ever)
    int rc = pnr_view_check("pnr_reproject", "src", model_src, cam_src_host, c2w_src12_host, width_src, height_src, true, a.src);
    if (!rc) rc = pnr_view_check("pnr_reproject", "tgt", model_tgt, cam_tgt_host, w2c_tgt12_host, width_tgt, height_tgt, true, a.tgt);
    if (rc) return rc;
    PNR_REQUIRE(depth_src, "pnr_reproject: null source depth image");
    PNR_REQUIRE(tol_abs >= 0.0f && tol_abs <= FLT_MAX && tol_rel >= 0.0f && tol_rel <= FLT_MAX,
                "pnr_reproject: tolerances must be finite and >= 0");
    const bool labels = label_src && label_tgt;
    PNR_REQUIRE(labels || (!label_src && !label_tgt), "pnr_reproject: label_src and label_tgt come together");
    PNR_REQUIRE(labels || !agree, "pnr_reproject: agree needs label images on both sides");
    PNR_REQUIRE(!labels || (n_classes >= 1 && n_classes <= 8192), "pnr_reproject: n_classes must be in 1 .. 8192 (got %d)", n_classes);
    PNR_REQUIRE((((uintptr_t)uv) & 7) == 0, "pnr_reproject: uv must be an 8-byte aligned device buffer");
    a.npix_src = (int64_t)width_src * height_src; a.umax = pnr_view_umax(a.tgt); a.vmax = pnr_view_vmax(a.tgt); a.tol_abs = tol_abs; a.tol_rel = tol_rel;
    a.pix = pix; a.R = n; a.depth_src = depth_src; a.depth_tgt = depth_tgt;
    a.label_src = labels ? label_src : nullptr; a.label_tgt = labels ? label_tgt : nullptr; a.n_classes = labels ? n_classes : 0;
    a.match = match; a.uv = reinterpret_cast<float2*>(uv);
    a.agree = (unsigned long long*)agree; a.stats = (unsigned long long*)stats;
    int grid = pnr_grid_cap((n + 255) / 256);
    if (agree && n_classes <= PNR_WARP_LDS_CLASSES) {
        const size_t lds = (size_t)n_classes * n_classes * sizeof(unsigned int);
        // a block zeroes and flushes n_classes^2 cells: give it at least as many trips over pixels (at most 16, as k_confusion)
        const int64_t trips = n_classes * n_classes / 256 < 1 ? 1 : n_classes * n_classes / 256 > 16 ? 16 : n_classes * n_classes / 256;
        const int64_t few = (n + 256 * trips - 1) / (256 * trips);
        grid = few < grid ? (int)few : grid;
        hipLaunchKernelGGL(k_reproject<true>, dim3(grid), dim3(256), lds < 32 ? 32 : lds, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(k_reproject<false>, dim3(grid), dim3(256), 32, (hipStream_t)stream, a);
    }
    PNR_CHECK_LAUNCH("pnr_reproject");
    return PNR_OK;
}
