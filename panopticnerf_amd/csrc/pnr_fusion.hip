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

#include "pnr_common.h"
#include "pnr_geom_dev.h"

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

template <bool RGB, bool LABEL>
__global__ __launch_bounds__(PNR_TSDF_BLOCK) void k_tsdf_integrate(const pnr_frame* __restrict__ frames, const float* __restrict__ w2c,
                                                                   const TsdfArgs a)
{
    for (int64_t n64 = (int64_t)blockIdx.x * PNR_TSDF_BLOCK + threadIdx.x; n64 < a.n; n64 += (int64_t)gridDim.x * PNR_TSDF_BLOCK) {
        const unsigned int n = (unsigned int)n64;
        const unsigned int iz = n / a.sz, r = n - iz * a.sz;
        const unsigned int iy = r / a.rx, ix = r - iy * a.rx;
        const float X = pnr_lattice_coord((float)ix, a.lo[0], a.step[0]), Y = pnr_lattice_coord((float)iy, a.lo[1], a.step[1]),
                    Z = pnr_lattice_coord((float)iz, a.lo[2], a.step[2]);
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
            if (!(pnr_pos_finite(d) && d <= a.max_depth)) continue;
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
    const int rc = pnr_lattice_check("pnr_tsdf_integrate", res_x, res_y, res_z, lo_host, step_host, 1, INT32_MAX, true);
    if (rc) return rc;
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

// ---------------------------------------------------------------------------------------------------------------------------
// Volume ray casting (include/pnr.h "volume ray casting"): the volume seen from any camera.  tests/_raycast_ref.py restates the
// rule in numpy; everything here equals it bit for bit.
//
// One thread per pixel; a wave is an 8 x 8 pixel TILE (pnr_tile_grid, pnr_geom_dev.h), not 64 pixels of a row, so the rays of a wave walk neighbouring cells and
// its gathers fall into few cache lines; a block is four tiles side by side, one block per four tiles (no cap: a ray's work runs
// from nothing to max_steps samples, and the hardware's dispatcher balances what a tile-stride loop would fix).  Partial tiles at
// the right and bottom edges are masked.  The ray is pnr_camera_ray's, the bits of the ray kernels.  Inside the march the eight
// corner values and the observed flag of the current cell stay in registers and are gathered again only when the cell changes,
// which cannot change a bit: the same numbers enter the same operations.  The only stores are the pixel's own outputs after the
// loop.  No atomics, no LDS, nothing waits on anything.
struct RaycastArgs {
    int model, width, height, max_steps;
    float cam[7], c2w[12];
    float near_, far_, min_weight, dt;
    int res[3];
    float lo[3], step[3];
    unsigned int tiles_x;
    int64_t n_tiles;
    const float *tsdf, *weight;
    float *depth, *normal;
    int32_t* src;
    uint8_t* code;
};

// the eight corners of a cell, index a + 2 b + 4 c for the corner (cx + a, cy + b, cz + c), and whether all eight are observed
struct RaycastCell {
    float v[8];
    bool obs;
};

__device__ __forceinline__ void raycast_load(const RaycastArgs& a, int cx, int cy, int cz, RaycastCell& cell)
{
    const size_t rx = (size_t)a.res[0], sz = rx * (size_t)a.res[1];
    const size_t base = ((size_t)cz * (size_t)a.res[1] + (size_t)cy) * rx + (size_t)cx;      // every corner < res_x res_y res_z
    bool obs = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const size_t at = base + (k & 1) + ((k >> 1) & 1) * rx + (k >> 2) * sz;
        cell.v[k] = a.tsdf[at];
        obs = obs && a.weight[at] >= a.min_weight;
    }
    cell.obs = obs;
}

// c = clamp((int)floor(g), 0, res - 2) and f = clamp(g - (float)c, 0, 1); the floor is clamped as a float first, so the
// conversion is in range whatever g is (NaN gives 0)
__device__ __forceinline__ void raycast_cell_of(float g, int res, int& c, float& f)
{
    const float fl = fminf(fmaxf(floorf(g), 0.0f), 1073741824.0f);
    const int ci = (int)fl;
    c = ci < res - 2 ? ci : res - 2;
    f = fminf(fmaxf(g - (float)c, 0.0f), 1.0f);
}

__device__ __forceinline__ float raycast_lerp(float p, float q, float f)
{
    const float d = q - p;
    const float m = f * d;                                          // a multiply, then an add: never an FMA
    return p + m;
}

__device__ __forceinline__ float raycast_value(const RaycastCell& c, float fx, float fy, float fz)
{
    const float x00 = raycast_lerp(c.v[0], c.v[1], fx), x10 = raycast_lerp(c.v[2], c.v[3], fx);
    const float x01 = raycast_lerp(c.v[4], c.v[5], fx), x11 = raycast_lerp(c.v[6], c.v[7], fx);
    return raycast_lerp(raycast_lerp(x00, x10, fy), raycast_lerp(x01, x11, fy), fz);
}

__global__ __launch_bounds__(PNR_RAYCAST_BLOCK) void k_tsdf_raycast(const RaycastArgs a)
{
    const int64_t tile = (int64_t)blockIdx.x * (PNR_RAYCAST_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    const unsigned int tj = (unsigned int)(tile / a.tiles_x), ti = (unsigned int)(tile - (int64_t)tj * a.tiles_x);
    const unsigned int lane = threadIdx.x & 63;
    const int64_t i64 = (int64_t)ti * PNR_RAYCAST_TILE + (lane & (PNR_RAYCAST_TILE - 1));
    const int64_t j64 = (int64_t)tj * PNR_RAYCAST_TILE + (lane >> 3);
    if (i64 >= a.width || j64 >= a.height) return;                  // the partial tiles of the right and bottom edges
    const int i = (int)i64, j = (int)j64;
    const size_t q = (size_t)j * (size_t)a.width + (size_t)i;

    float depth = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    int32_t src = -1;
    uint8_t code = PNR_RAYCAST_NO_RAY;
    bool ok;
    const PnrRayRec ray = pnr_camera_ray(a.model, a.cam, a.c2w, i, j, a.near_, a.far_, ok);
    if (ok) {
        const float o[3] = {ray.lo.x, ray.lo.y, ray.lo.z}, d[3] = {ray.lo.w, ray.hi.x, ray.hi.y};
        float og[3], dg[3];
        float t_in = ray.hi.z, t_out = ray.hi.w;
        bool miss = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            og[k] = (o[k] - a.lo[k]) / a.step[k] - 0.5f;
            dg[k] = d[k] / a.step[k];
            const float top = (float)(a.res[k] - 1);
            if (dg[k] == 0.0f) {
                miss = miss || og[k] < 0.0f || og[k] > top;
            } else {
                const float ta = (0.0f - og[k]) / dg[k], tb = (top - og[k]) / dg[k];
                t_in = fmaxf(t_in, fminf(ta, tb));
                t_out = fminf(t_out, fmaxf(ta, tb));
            }
        }
        code = PNR_RAYCAST_MISSED;
        if (!miss && t_in <= t_out) {
            code = PNR_RAYCAST_NO_SURFACE;
            RaycastCell cell;
            int cx = -1, cy = -1, cz = -1;                          // no cell is loaded yet
            float t_prev = 0.0f, v_prev = 0.0f;
            bool obs_prev = false;
            for (int n = 0; n < a.max_steps; ++n) {
                const float adv = (float)n * a.dt;
                const float t = t_in + adv;
                if (!(t <= t_out)) break;
                const float m0 = t * dg[0], m1 = t * dg[1], m2 = t * dg[2];
                int c0, c1, c2;
                float f0, f1, f2;
                raycast_cell_of(og[0] + m0, a.res[0], c0, f0);
                raycast_cell_of(og[1] + m1, a.res[1], c1, f1);
                raycast_cell_of(og[2] + m2, a.res[2], c2, f2);
                if (c0 != cx || c1 != cy || c2 != cz) {               // the cell changed: gather its eight corners again
                    cx = c0; cy = c1; cz = c2;
                    raycast_load(a, cx, cy, cz, cell);
                }
                const float v = raycast_value(cell, f0, f1, f2);
                if (obs_prev && cell.obs && v_prev < 0.0f && 0.0f <= v) {      // n >= 1: obs_prev is false at n = 0
                    const float r = v_prev / (v_prev - v);
                    const float w = (t - t_prev) * r;
                    depth = t_prev + w;
                    code = PNR_RAYCAST_HIT;
                    break;
                }
                t_prev = t; v_prev = v; obs_prev = cell.obs;
            }
            if (code == PNR_RAYCAST_HIT) {
                const float m0 = depth * dg[0], m1 = depth * dg[1], m2 = depth * dg[2];
                int c0, c1, c2;
                float f0, f1, f2;
                raycast_cell_of(og[0] + m0, a.res[0], c0, f0);
                raycast_cell_of(og[1] + m1, a.res[1], c1, f1);
                raycast_cell_of(og[2] + m2, a.res[2], c2, f2);
                const int64_t s0 = c0 + (f0 >= 0.5f ? 1 : 0), s1 = c1 + (f1 >= 0.5f ? 1 : 0), s2 = c2 + (f2 >= 0.5f ? 1 : 0);
                src = (int32_t)((s2 * a.res[1] + s1) * a.res[0] + s0);
                if (a.normal) {
                    if (c0 != cx || c1 != cy || c2 != cz) raycast_load(a, c0, c1, c2, cell);
                    if (cell.obs) {
                        const float* v = cell.v;
                        // the gradient of the trilinear interpolant: the differences along an axis, lerped along the other two
                        // in the order x, y, z
                        float gx = raycast_lerp(raycast_lerp(v[1] - v[0], v[3] - v[2], f1), raycast_lerp(v[5] - v[4], v[7] - v[6], f1), f2);
                        float gy = raycast_lerp(raycast_lerp(v[2] - v[0], v[3] - v[1], f0), raycast_lerp(v[6] - v[4], v[7] - v[5], f0), f2);
                        float gz = raycast_lerp(raycast_lerp(v[4] - v[0], v[5] - v[1], f0), raycast_lerp(v[6] - v[2], v[7] - v[3], f0), f1);
                        gx = gx / a.step[0]; gy = gy / a.step[1]; gz = gz / a.step[2];
                        const float xx = gx * gx, yy = gy * gy, zz = gz * gz;
                        const float len = sqrtf((xx + yy) + zz);
                        if (pnr_pos_finite(len)) { nx = -gx / len; ny = -gy / len; nz = -gz / len; }
                    }
                }
            }
        }
    }
    a.depth[q] = depth;
    a.code[q] = code;
    if (a.normal) { a.normal[q * 3 + 0] = nx; a.normal[q * 3 + 1] = ny; a.normal[q * 3 + 2] = nz; }
    if (a.src) a.src[q] = src;
}

PNR_EXPORT int pnr_tsdf_raycast(int model, const float* cam_host, const float* c2w12_host, int width, int height, float near_, float far_,
                                int res_x, int res_y, int res_z, const float* lo_host, const float* step_host, const float* tsdf,
                                const float* weight, float min_weight, float dt, int max_steps, float* depth, float* normal, int32_t* src,
                                uint8_t* code, void* stream)
{
    PNR_REQUIRE(pnr_camera_model_ok(model), "pnr_tsdf_raycast: unknown camera model %d", model);
    PNR_REQUIRE(cam_host && c2w12_host, "pnr_tsdf_raycast: null camera or pose (cam_host, c2w12_host)");
    PNR_REQUIRE(tsdf && weight, "pnr_tsdf_raycast: null tsdf or weight");
    PNR_REQUIRE(depth && code, "pnr_tsdf_raycast: null depth or code");
    PNR_REQUIRE(((((uintptr_t)tsdf) | ((uintptr_t)weight) | ((uintptr_t)depth) | ((uintptr_t)normal) | ((uintptr_t)src)) & 3) == 0,
                "pnr_tsdf_raycast: misaligned array (tsdf, weight, depth, normal, src: 4 bytes)");
    PNR_REQUIRE(width >= 1 && height >= 1 && (int64_t)width * height <= INT32_MAX,
                "pnr_tsdf_raycast: bad image %d x %d (width, height >= 1, at most 2^31 - 1 pixels)", width, height);
    int rc = pnr_camera_check(model, cam_host, width, height, "pnr_tsdf_raycast");
    if (!rc) rc = pnr_lattice_check("pnr_tsdf_raycast", res_x, res_y, res_z, lo_host, step_host, 2, INT32_MAX, true);
    if (rc) return rc;
    PNR_REQUIRE(dt > 0.0f && isfinite(dt), "pnr_tsdf_raycast: dt must be positive and finite");
    PNR_REQUIRE(max_steps >= 0, "pnr_tsdf_raycast: max_steps must be >= 0 (got %d)", max_steps);
    PNR_REQUIRE(min_weight > 0.0f, "pnr_tsdf_raycast: min_weight must be positive");
    PNR_REQUIRE(near_ >= 0.0f && far_ > near_, "pnr_tsdf_raycast: need 0 <= near < far");
    RaycastArgs a;
    a.model = model; a.width = width; a.height = height; a.max_steps = max_steps;
    pnr_camera_fill(model, cam_host, a.cam);
    pnr_pose_fill(c2w12_host, a.c2w);
    a.near_ = near_; a.far_ = far_; a.min_weight = min_weight; a.dt = dt;
    a.res[0] = res_x; a.res[1] = res_y; a.res[2] = res_z;
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo_host[k]; a.step[k] = step_host[k]; }
    int64_t blocks;
    pnr_tile_grid(width, height, &a.tiles_x, &a.n_tiles, &blocks);
    a.tsdf = tsdf; a.weight = weight; a.depth = depth; a.normal = normal; a.src = src; a.code = code;
    hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned int)blocks), dim3(PNR_RAYCAST_BLOCK), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_tsdf_raycast");
    return PNR_OK;
}
