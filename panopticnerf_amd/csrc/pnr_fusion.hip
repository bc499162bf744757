// Depth fusion (include/pnr.h "depth fusion"): posed depth frames of a device-resident pnr_frame table are fused into a truncated
// signed distance volume on the lattice of query_grid / mesh extraction, with an optional running-mean colour and an optional
// majority-vote label per lattice point.  tests/_tsdf_ref.py restates the rule in numpy; everything here equals it bit for bit.
//
// One thread per lattice point, x fastest, so the volume arrays are read and written coalesced; a block walks chunks of 256
// points grid-stride.  The point's state stays in registers across the WHOLE frame loop: the volume is read once and written
// once per call, however many frames -- the reason for taking a table, not one camera per launch.  The frame loop is
// wave-uniform (every lane runs f0 .. f1 - 1); a frame's record and its w2c row are read through uniform addresses of two
// noalias kernel arguments, so they are scalar loads.  Per (point, frame): one projection (pnr_project_point, the bits of
// k_project_points), one depth gather, and for the points inside the band a 3-byte colour gather and two label gathers.  The
// only stores are the point's own state after the loop: no atomics, no LDS, nothing waits on another workgroup, so two calls
// give the same bits.
#include <float.h>
#include <math.h>

#include "pnr_camera_dev.h"
#include "pnr_common.h"

// the launch constants PNR_TSDF_BLOCK and PNR_TSDF_BLOCKS_PER_CU are include/pnr.h's (a test sizes a lattice from them)
#define PNR_TSDF_CONF_MAX (1 << 30)

static_assert(sizeof(pnr_frame) == 144 && sizeof(pnr_frame) % 16 == 0, "pnr_frame: the layout include/pnr.h documents");

struct TsdfArgs {
    int f0, f1;
    unsigned int rx, sz;                // res_x, res_x * res_y
    int64_t n;                          // res_x * res_y * res_z <= 2^31 - 1
    float lo[3], step[3];
    float trunc, max_depth, w_max;
    float *tsdf, *weight, *rgb, *rgb_weight;
    int32_t *label, *conf;
};

__device__ __forceinline__ float tsdf_coord(unsigned int i, float lo, float step)
{
    const float m = ((float)i + 0.5f) * step;                       // a multiply, then an add: never an FMA (-ffp-contract=off)
    return m + lo;
}

template <bool RGB, bool LABEL>
__global__ __launch_bounds__(PNR_TSDF_BLOCK) void k_tsdf_integrate(const pnr_frame* __restrict__ frames, const float* __restrict__ w2c,
                                                                   const TsdfArgs a)
{
    for (int64_t n64 = (int64_t)blockIdx.x * PNR_TSDF_BLOCK + threadIdx.x; n64 < a.n; n64 += (int64_t)gridDim.x * PNR_TSDF_BLOCK) {
        const unsigned int n = (unsigned int)n64;
        const unsigned int iz = n / a.sz, r = n - iz * a.sz;
        const unsigned int iy = r / a.rx, ix = r - iy * a.rx;
        const float X = tsdf_coord(ix, a.lo[0], a.step[0]), Y = tsdf_coord(iy, a.lo[1], a.step[1]), Z = tsdf_coord(iz, a.lo[2], a.step[2]);
        const size_t at = (size_t)n;
        float t = a.tsdf[at], w = a.weight[at];
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, cw = 0.0f;
        int32_t lab = -1, cf = 0;
        if (RGB) { c0 = a.rgb[at * 3 + 0]; c1 = a.rgb[at * 3 + 1]; c2 = a.rgb[at * 3 + 2]; cw = a.rgb_weight[at]; }
        if (LABEL) { lab = a.label[at]; cf = a.conf[at]; }
        for (int f = a.f0; f < a.f1; ++f) {                         // wave-uniform: f, the record and the pose row are scalars
            const pnr_frame& fr = frames[f];
            const float* dimg = reinterpret_cast<const float*>(fr.depth);
            if (!dimg) continue;                                                                    // 1
            const float umax = (float)fr.width - 0.5f, vmax = (float)fr.height - 0.5f;
            const PnrProj q = pnr_project_point(fr.model, fr.cam, w2c + (size_t)f * 12, umax, X, Y, Z);    // 2
            if (!(q.dom && pnr_uv_inside(q.u, q.v, umax, vmax))) continue;
            const int iu = pnr_nearest_pixel(q.u, fr.width - 1), iv = pnr_nearest_pixel(q.v, fr.height - 1);  // 3
            const int64_t p = (int64_t)iv * fr.width + iu;          // inside the image: 0 <= iu < width, 0 <= iv < height
            const float d = dimg[p];                                                                // 4
            if (!(d > 0.0f && d <= FLT_MAX && d <= a.max_depth)) continue;
            const float s = pnr_view_depth(fr.model, q) - d;                                        // 5
            if (s > a.trunc) continue;
            const float phi = s < -a.trunc ? -1.0f : s / a.trunc;                                   // 6
            t = (t * w + phi) / (w + 1.0f);                                                         // 7
            w = fminf(w + 1.0f, a.w_max);
            if (!(s >= -a.trunc)) continue;                         // in front of the band: free space has no colour and no label
            if (RGB) {                                                                              // 8
                const uint8_t* px = reinterpret_cast<const uint8_t*>(fr.rgb);
                if (px) {
                    px += p * 3;
                    const float den = cw + 1.0f;
                    c0 = (c0 * cw + (float)px[0]) / den;
                    c1 = (c1 * cw + (float)px[1]) / den;
                    c2 = (c2 * cw + (float)px[2]) / den;
                    cw = fminf(den, a.w_max);
                }
            }
            if (LABEL) {                                                                            // 9
                const int16_t* simg = reinterpret_cast<const int16_t*>(fr.sem);
                const int16_t* iimg = reinterpret_cast<const int16_t*>(fr.inst);
                const int ls = simg ? (int)simg[p] : -1;
                if (ls >= 0) {
                    const int li = iimg ? (int)iimg[p] : -1;
                    const int32_t key = (int32_t)(((unsigned int)ls << 16) | ((unsigned int)li & 0xFFFFu));
                    if (lab == key) cf = cf < PNR_TSDF_CONF_MAX ? cf + 1 : PNR_TSDF_CONF_MAX;
                    else if (cf == 0) { lab = key; cf = 1; }
                    else cf -= 1;
                }
            }
        }
        a.tsdf[at] = t;
        a.weight[at] = w;
        if (RGB) { a.rgb[at * 3 + 0] = c0; a.rgb[at * 3 + 1] = c1; a.rgb[at * 3 + 2] = c2; a.rgb_weight[at] = cw; }
        if (LABEL) { a.label[at] = lab; a.conf[at] = cf; }
    }
}

PNR_EXPORT int pnr_tsdf_integrate(const pnr_frame* frames, const float* w2c, int f0, int f1, int res_x, int res_y, int res_z,
                                  const float* lo_host, const float* step_host, float trunc, float max_depth, float w_max,
                                  float* tsdf, float* weight, float* rgb, float* rgb_weight, int32_t* label, int32_t* conf, void* stream)
{
    PNR_REQUIRE(frames && w2c, "pnr_tsdf_integrate: null frames or w2c table");
    PNR_REQUIRE(tsdf && weight, "pnr_tsdf_integrate: null tsdf or weight");
    PNR_REQUIRE((rgb != nullptr) == (rgb_weight != nullptr), "pnr_tsdf_integrate: rgb and rgb_weight go together (both or neither)");
    PNR_REQUIRE((label != nullptr) == (conf != nullptr), "pnr_tsdf_integrate: label and conf go together (both or neither)");
    PNR_REQUIRE((((uintptr_t)frames) & 15) == 0 && (((uintptr_t)w2c) & 15) == 0,
                "pnr_tsdf_integrate: misaligned table (frames and w2c 16 bytes)");
    PNR_REQUIRE(((((uintptr_t)tsdf) | ((uintptr_t)weight) | ((uintptr_t)rgb) | ((uintptr_t)rgb_weight) | ((uintptr_t)label) | ((uintptr_t)conf)) & 3) == 0,
                "pnr_tsdf_integrate: misaligned volume array (4 bytes)");
    PNR_REQUIRE(f0 >= 0 && f1 >= f0, "pnr_tsdf_integrate: bad frame range [%d, %d) (0 <= f0 <= f1)", f0, f1);
    PNR_REQUIRE(res_x >= 1 && res_y >= 1 && res_z >= 1 && (int64_t)res_x * res_y <= INT32_MAX && (int64_t)res_x * res_y * res_z <= INT32_MAX,
                "pnr_tsdf_integrate: bad lattice %d x %d x %d (every res >= 1, at most 2^31 - 1 points)", res_x, res_y, res_z);
    PNR_REQUIRE(lo_host && step_host, "pnr_tsdf_integrate: null lo or step");
    for (int k = 0; k < 3; ++k)
        PNR_REQUIRE(isfinite(lo_host[k]) && isfinite(step_host[k]) && step_host[k] != 0.0f,
                    "pnr_tsdf_integrate: lo and step must be finite and step non-zero (axis %d)", k);
    PNR_REQUIRE(trunc > 0.0f && isfinite(trunc), "pnr_tsdf_integrate: trunc must be positive and finite");
    PNR_REQUIRE(max_depth > 0.0f, "pnr_tsdf_integrate: max_depth must be positive (it may be +inf)");
    PNR_REQUIRE(w_max >= 1.0f, "pnr_tsdf_integrate: w_max must be >= 1 (it may be +inf)");
    if (f0 == f1) return PNR_OK;
    TsdfArgs a;
    a.f0 = f0; a.f1 = f1;
    a.rx = (unsigned int)res_x; a.sz = (unsigned int)res_x * (unsigned int)res_y;
    a.n = (int64_t)res_x * res_y * res_z;
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo_host[k]; a.step[k] = step_host[k]; }
    a.trunc = trunc; a.max_depth = max_depth; a.w_max = w_max;
    a.tsdf = tsdf; a.weight = weight; a.rgb = rgb; a.rgb_weight = rgb_weight; a.label = label; a.conf = conf;
    const int grid = pnr_grid_cap((a.n + PNR_TSDF_BLOCK - 1) / PNR_TSDF_BLOCK, PNR_TSDF_BLOCKS_PER_CU);
    const hipStream_t st = (hipStream_t)stream;
    if (rgb && label) hipLaunchKernelGGL((k_tsdf_integrate<true, true>), dim3(grid), dim3(PNR_TSDF_BLOCK), 0, st, frames, w2c, a);
    else if (rgb) hipLaunchKernelGGL((k_tsdf_integrate<true, false>), dim3(grid), dim3(PNR_TSDF_BLOCK), 0, st, frames, w2c, a);
    else if (label) hipLaunchKernelGGL((k_tsdf_integrate<false, true>), dim3(grid), dim3(PNR_TSDF_BLOCK), 0, st, frames, w2c, a);
    else hipLaunchKernelGGL((k_tsdf_integrate<false, false>), dim3(grid), dim3(PNR_TSDF_BLOCK), 0, st, frames, w2c, a);
    PNR_CHECK_LAUNCH("pnr_tsdf_integrate");
    return PNR_OK;
}
