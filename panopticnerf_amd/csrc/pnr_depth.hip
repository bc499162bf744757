// Depth front end (include/pnr.h "depth front end"): what turns any depth image into a view that fusion.track, reprojection and
// the evaluator take.  k_depth_filter is an edge-preserving smoothing with a speckle rule: a tile of the input with its halo goes
// through LDS, every pixel walks its window row-major and weighs a neighbour by the host's spatial weights and a compact biweight
// of the depth difference -- no transcendental, so tests/_depth_ref.py restates it bit for bit.  k_depth_normals gives every pixel
// its camera-relative vector v = t d (the ray of pnr_camera_ray, pnr_camera_dev.h: the arithmetic of the ray, fusion and tracking
// kernels; the view is a PnrView, pnr_geom_dev.h), shares the tile's vectors through LDS (2-D tiles with a halo, this file's
// own), and crosses the differences along the two image axes.  Float32, one rounding
// per operation (-ffp-contract=off), no atomics: two runs give the same bits.
#include <float.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"

#define DF_R PNR_DEPTH_MAX_RADIUS
#define DF_TX PNR_DEPTH_TILE_X
#define DF_TY PNR_DEPTH_TILE_Y
#define DF_LW (DF_TX + 2 * DF_R)        // the LDS row: the widest halo on either side
#define DF_LH (DF_TY + 2 * DF_R)
#define DF_THREADS (DF_TX * DF_TY)

struct DepthFilterArgs {
    int width, height, radius, min_support;
    unsigned int tiles_x;
    float sigma_a, sigma_b;
    float g[DF_R + 1];
    const float* in;
    float* out;
    int16_t* support;
};

__global__ __launch_bounds__(DF_THREADS) void k_depth_filter(const DepthFilterArgs a)
{
    __shared__ float tile[DF_LH * DF_LW];
    __shared__ float gs[DF_R + 1];
    const int r = a.radius;
    const unsigned int tj = blockIdx.x / a.tiles_x, ti = blockIdx.x - tj * a.tiles_x;
    const int64_t i0 = (int64_t)ti * DF_TX - r, j0 = (int64_t)tj * DF_TY - r;
    const int lw = DF_TX + 2 * r, lh = DF_TY + 2 * r;
    // a pixel beyond the image is stored as 0, which is no valid depth: "inside the image" needs no test of its own below
    for (int e = threadIdx.x; e < lw * lh; e += DF_THREADS) {
        const int ly = e / lw, lx = e - ly * lw;
        const int64_t i = i0 + lx, j = j0 + ly;
        float t = 0.0f;
        if (i >= 0 && i < a.width && j >= 0 && j < a.height) t = a.in[(size_t)j * (size_t)a.width + (size_t)i];
        tile[ly * DF_LW + lx] = t;
    }
#pragma unroll
    for (int k = 0; k <= DF_R; ++k)
        if (threadIdx.x == k) gs[k] = a.g[k];
    __syncthreads();
    const int lx = threadIdx.x % DF_TX, ly = threadIdx.x / DF_TX;
    const int64_t i = (int64_t)ti * DF_TX + lx, j = (int64_t)tj * DF_TY + ly;
    if (i >= a.width || j >= a.height) return;                      // the partial tiles of the right and bottom edges
    const float c = tile[(ly + r) * DF_LW + lx + r];
    float out = 0.0f;
    int count = 0;
    if (pnr_pos_finite(c)) {
        const float sigma = a.sigma_a + a.sigma_b * c;
        float acc = 0.0f, ws = 0.0f;
        for (int dy = -r; dy <= r; ++dy) {
            const float gy = gs[dy < 0 ? -dy : dy];
            const float* row = &tile[(ly + r + dy) * DF_LW + lx + r];
            for (int dx = -r; dx <= r; ++dx) {
                const float t = row[dx];
                const float x = (t - c) / sigma;
                const float u = 1.0f - x * x;
                if (pnr_pos_finite(t) && u > 0.0f) {
                    const float w = (gy * gs[dx < 0 ? -dx : dx]) * (u * u);
                    acc = acc + w * t;
                    ws = ws + w;
                    count += 1;
                }
            }
        }
        if (count >= a.min_support) out = acc / ws;
    }
    const size_t q = (size_t)j * (size_t)a.width + (size_t)i;
    a.out[q] = out;
    if (a.support) a.support[q] = (int16_t)count;
}

PNR_EXPORT int pnr_depth_filter(int width, int height, const float* depth_in, int radius, const float* g_host, float sigma_a, float sigma_b,
                                int min_support, float* depth_out, int16_t* support, void* stream)
{
    PNR_REQUIRE(width >= 1 && height >= 1 && (int64_t)width * height <= INT32_MAX, "pnr_depth_filter: bad size (the image holds 1 .. 2^31 - 1 pixels)");
    PNR_REQUIRE(depth_in && depth_out && g_host, "pnr_depth_filter: null depth_in, depth_out or g");
    PNR_REQUIRE((((uintptr_t)depth_in | (uintptr_t)depth_out) & 3) == 0 && (((uintptr_t)support) & 1) == 0,
                "pnr_depth_filter: depth_in and depth_out must be 4-byte aligned, support 2-byte");
    PNR_REQUIRE(depth_in != depth_out, "pnr_depth_filter: depth_in and depth_out must differ (a pixel reads its neighbours)");
    PNR_REQUIRE(radius >= 0 && radius <= PNR_DEPTH_MAX_RADIUS, "pnr_depth_filter: radius must lie in 0 .. %d", PNR_DEPTH_MAX_RADIUS);
    for (int k = 0; k <= radius; ++k)
        PNR_REQUIRE(pnr_pos_finite(g_host[k]), "pnr_depth_filter: g[%d] must be positive and finite", k);
    PNR_REQUIRE(sigma_a >= 0.0f && sigma_a <= FLT_MAX && sigma_b >= 0.0f && sigma_b <= FLT_MAX && (sigma_a > 0.0f || sigma_b > 0.0f),
                "pnr_depth_filter: sigma_a and sigma_b must be non-negative and finite, not both 0");
    PNR_REQUIRE(min_support >= 1, "pnr_depth_filter: min_support must be >= 1");
    DepthFilterArgs a;
    a.width = width; a.height = height; a.radius = radius; a.min_support = min_support;
    a.sigma_a = sigma_a; a.sigma_b = sigma_b;
    for (int k = 0; k <= DF_R; ++k) a.g[k] = k <= radius ? g_host[k] : 0.0f;
    a.in = depth_in; a.out = depth_out; a.support = support;
    const int64_t tiles_x = ((int64_t)width + DF_TX - 1) / DF_TX, tiles_y = ((int64_t)height + DF_TY - 1) / DF_TY;
    a.tiles_x = (unsigned int)tiles_x;                              // tiles_x * tiles_y is at most 2^28 + 2^26: the grid fits a launch
    hipLaunchKernelGGL(k_depth_filter, dim3((unsigned int)(tiles_x * tiles_y)), dim3(DF_THREADS), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_depth_filter");
    return PNR_OK;
}

#define DN_TX PNR_NORMALS_TILE_X
#define DN_TY PNR_NORMALS_TILE_Y
#define DN_LW (DN_TX + 2)
#define DN_LH (DN_TY + 2)
#define DN_THREADS (DN_TX * DN_TY)

struct DepthNormalsArgs {
    PnrView view;                       // pose = c2w
    unsigned int tiles_x;
    float jump_a, jump_b, mc2;
    const float* depth;
    float* normal;
    float* vertex;
    uint8_t* code;
};

// step 1 of a pixel inside the image: (v, t), or all 0 where its NO_DEPTH test fails
__device__ __forceinline__ float4 dn_record(const DepthNormalsArgs& a, int i, int j)
{
    const float t = a.depth[(size_t)j * (size_t)a.view.width + (size_t)i];
    bool ok;
    const PnrRayRec ray = pnr_camera_ray(a.view.model, a.view.cam, a.view.pose, i, j, 0.0f, 0.0f, ok);
    if (!(ok && pnr_pos_finite(t))) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4(t * ray.lo.w, t * ray.hi.x, t * ray.hi.y, t);
}

__global__ __launch_bounds__(DN_THREADS) void k_depth_normals(const DepthNormalsArgs a)
{
    __shared__ float4 tile[DN_LH * DN_LW];          // .w = 0: no usable pixel there (NO_DEPTH, or beyond the image)
    const unsigned int tj = blockIdx.x / a.tiles_x, ti = blockIdx.x - tj * a.tiles_x;
    const int64_t i0 = (int64_t)ti * DN_TX - 1, j0 = (int64_t)tj * DN_TY - 1;
    for (int e = threadIdx.x; e < DN_LW * DN_LH; e += DN_THREADS) {
        const int ly = e / DN_LW, lx = e - ly * DN_LW;
        const int64_t i = i0 + lx, j = j0 + ly;
        float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i >= 0 && i < a.view.width && j >= 0 && j < a.view.height) rec = dn_record(a, (int)i, (int)j);
        tile[e] = rec;
    }
    __syncthreads();
    const int lx = threadIdx.x % DN_TX + 1, ly = threadIdx.x / DN_TX + 1;
    const int64_t i = i0 + lx, j = j0 + ly;
    if (i >= a.view.width || j >= a.view.height) return;
    const float4 p = tile[ly * DN_LW + lx];
    const float t = p.w;
    int code = PNR_NORMAL_NO_DEPTH;
    float n[3] = {0.0f, 0.0f, 0.0f}, vtx[3] = {0.0f, 0.0f, 0.0f};
    if (t != 0.0f) {
        vtx[0] = a.view.pose[3] + p.x; vtx[1] = a.view.pose[7] + p.y; vtx[2] = a.view.pose[11] + p.z;
        const float thr = a.jump_a + a.jump_b * t;
        const float4 nb[4] = {tile[ly * DN_LW + lx - 1], tile[ly * DN_LW + lx + 1], tile[(ly - 1) * DN_LW + lx], tile[(ly + 1) * DN_LW + lx]};
        bool use[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) use[k] = nb[k].w != 0.0f && fabsf(nb[k].w - t) <= thr;
        float D[2][3];
#pragma unroll
        for (int ax = 0; ax < 2; ++ax) {
            const float4 lo = use[2 * ax] ? nb[2 * ax] : p, hi = use[2 * ax + 1] ? nb[2 * ax + 1] : p;
            D[ax][0] = hi.x - lo.x; D[ax][1] = hi.y - lo.y; D[ax][2] = hi.z - lo.z;
        }
        code = PNR_NORMAL_NO_NEIGHBOUR;
        if ((use[0] || use[1]) && (use[2] || use[3])) {
            float c[3];
            pnr_cross3(D[0], D[1], c);
            const float cx = c[0], cy = c[1], cz = c[2];
            const float cc = (cx * cx + cy * cy) + cz * cz;         // (the grazing test needs the squared length too)
            const float len = sqrtf(cc);
            code = PNR_NORMAL_DEGENERATE;
            if (pnr_pos_finite(len)) {
                const float s = (cx * p.x + cy * p.y) + cz * p.z;
                const float vv = (p.x * p.x + p.y * p.y) + p.z * p.z;
                code = PNR_NORMAL_GRAZING;
                if (!(s * s < (a.mc2 * cc) * vv)) {
                    code = PNR_NORMAL_OK;
                    const float nx = cx / len, ny = cy / len, nz = cz / len;
                    n[0] = s > 0.0f ? -nx : nx; n[1] = s > 0.0f ? -ny : ny; n[2] = s > 0.0f ? -nz : nz;
                }
            }
        }
    }
    const size_t q = (size_t)j * (size_t)a.view.width + (size_t)i;
    a.normal[q * 3 + 0] = n[0]; a.normal[q * 3 + 1] = n[1]; a.normal[q * 3 + 2] = n[2];
    if (a.vertex) { a.vertex[q * 3 + 0] = vtx[0]; a.vertex[q * 3 + 1] = vtx[1]; a.vertex[q * 3 + 2] = vtx[2]; }
    if (a.code) a.code[q] = (uint8_t)code;
}

PNR_EXPORT int pnr_depth_normals(int model, const float* cam_host, const float* c2w12_host, int width, int height, const float* depth,
                                 float jump_a, float jump_b, float mc2, float* normal, float* vertex, uint8_t* code, void* stream)
{
    DepthNormalsArgs a;
    const int rc = pnr_view_check("pnr_depth_normals", nullptr, model, cam_host, c2w12_host, width, height, true, a.view);
    if (rc) return rc;
    PNR_REQUIRE((int64_t)width * height <= INT32_MAX, "pnr_depth_normals: bad size (the image holds 1 .. 2^31 - 1 pixels)");
    PNR_REQUIRE(depth && normal, "pnr_depth_normals: null depth or normal");
    PNR_REQUIRE((((uintptr_t)depth | (uintptr_t)normal | (uintptr_t)vertex) & 3) == 0, "pnr_depth_normals: depth, normal and vertex must be 4-byte aligned");
    PNR_REQUIRE(jump_a >= 0.0f && jump_b >= 0.0f, "pnr_depth_normals: jump_a and jump_b must be non-negative (they may be inf)");
    PNR_REQUIRE(mc2 >= 0.0f && mc2 <= 1.0f, "pnr_depth_normals: mc2 (the squared cosine) must lie in [0, 1]");
    a.jump_a = jump_a; a.jump_b = jump_b; a.mc2 = mc2;
    a.depth = depth; a.normal = normal; a.vertex = vertex; a.code = code;
    const int64_t tiles_x = ((int64_t)width + DN_TX - 1) / DN_TX, tiles_y = ((int64_t)height + DN_TY - 1) / DN_TY;
    a.tiles_x = (unsigned int)tiles_x;
    hipLaunchKernelGGL(k_depth_normals, dim3((unsigned int)(tiles_x * tiles_y)), dim3(DN_THREADS), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_depth_normals");
    return PNR_OK;
}
