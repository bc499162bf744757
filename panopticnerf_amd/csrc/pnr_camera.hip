// Cameras: fisheye and equirect ray generation and 3D -> 2D projection for all camera models (include/pnr.h "cameras").
// Small write-bound kernels in the style of k_gen_rays (pnr_sampling.hip): one thread per ray / point, grid-stride, camera
// and pose in the kernel arguments.  Every operation is a single + - * / sqrt in one fixed order (the build has
// -ffp-contract=off and correctly rounded divide / sqrt): tests/_camera_ref.py and tests/_pano_ref.py restate the kernels in
// float32, bit for bit.
#include <float.h>

#include "pnr_camera_dev.h"
#include "pnr_common.h"

// Un-projection: one thread per ray, two float4 stores (32 B/ray) + one byte into `valid`.
struct GenRaysFisheyeArgs { FisheyeCam c; float c2w[12]; int width; float near_, far_; const int32_t* pix; int64_t R; float* rays; uint8_t* valid; };
__global__ __launch_bounds__(256) void k_gen_rays_fisheye(const GenRaysFisheyeArgs a)
{
    const FisheyeCam c = a.c;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = a.pix ? (int64_t)a.pix[r] : r;
        const int j = (int)(p / a.width), i = (int)(p - (int64_t)j * a.width);
        bool ok;
        const PnrRayRec ray = pnr_fisheye_ray(c, a.c2w, i, j, a.near_, a.far_, ok);
        float4* o = reinterpret_cast<float4*>(a.rays + r * 8);
        o[0] = ray.lo;
        o[1] = ray.hi;
        if (a.valid) a.valid[r] = ok ? 1 : 0;
    }
}

// Panoramic un-projection: one thread per ray, two float4 stores (32 B/ray); every pixel is valid.
struct GenRaysEquirectArgs { float cam[4]; float c2w[12]; int width; float near_, far_; const int32_t* pix; int64_t R; float* rays; };
__global__ __launch_bounds__(256) void k_gen_rays_equirect(const GenRaysEquirectArgs a)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = a.pix ? (int64_t)a.pix[r] : r;
        const int j = (int)(p / a.width), i = (int)(p - (int64_t)j * a.width);
        const PnrRayRec ray = pnr_equirect_ray(a.cam[0], a.cam[1], a.cam[2], a.cam[3], a.c2w, i, j, a.near_, a.far_);
        float4* o = reinterpret_cast<float4*>(a.rays + r * 8);
        o[0] = ray.lo;
        o[1] = ray.hi;
    }
}

// Projection: one thread per point; reads 12 B, writes 8 + 4 + 1 B.  cam: pinhole {fx, fy, cx, cy}, fisheye cam7 or equirect cam4.
struct ProjectArgs { int model; float cam[7]; float w2c[12]; float umax, vmax; const float* pts; int64_t P; float2* uv; float* range; uint8_t* valid; };
__global__ __launch_bounds__(256) void k_project_points(const ProjectArgs a)
{
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.P; n += (int64_t)gridDim.x * blockDim.x) {
        const float X = a.pts[n * 3 + 0], Y = a.pts[n * 3 + 1], Z = a.pts[n * 3 + 2];
        const PnrProj q = pnr_project_point(a.model, a.cam, a.w2c, a.umax, X, Y, Z);
        const bool inside = pnr_uv_inside(q.u, q.v, a.umax, a.vmax);
        if (a.uv) a.uv[n] = make_float2(q.u, q.v);
        if (a.range) a.range[n] = q.rng;
        if (a.valid) a.valid[n] = (q.dom && inside) ? 1 : 0;
    }
}

PNR_EXPORT int pnr_gen_rays_fisheye(const float* cam7_host, const float* c2w12_host, int width, int height, float near_, float far_,
                                    const int32_t* pix, int64_t n_rays, float* rays, uint8_t* valid, void* stream)
{
    PNR_REQUIRE(cam7_host && c2w12_host, "pnr_gen_rays_fisheye: null camera");
    PNR_REQUIRE(width >= 1 && height >= 1 && n_rays >= 0, "pnr_gen_rays_fisheye: bad size");
    if (n_rays == 0) return PNR_OK;             // before the pointer checks: an empty pixel list has a null pointer
    PNR_REQUIRE(pix || n_rays == (int64_t)width * height, "pnr_gen_rays_fisheye: without pixel indices n_rays must be width*height");
    PNR_REQUIRE(cam7_host[3] != 0.0f && cam7_host[4] != 0.0f, "pnr_gen_rays_fisheye: zero gamma");
    PNR_REQUIRE(rays && (((uintptr_t)rays) & 15) == 0, "pnr_gen_rays_fisheye: rays must be a 16-byte aligned device buffer");
    GenRaysFisheyeArgs a;
    a.c = FisheyeCam{cam7_host[0], cam7_host[1], cam7_host[2], cam7_host[3], cam7_host[4], cam7_host[5], cam7_host[6]};
    for (int k = 0; k < 12; ++k) a.c2w[k] = c2w12_host[k];
    a.width = width; a.near_ = near_; a.far_ = far_; a.pix = pix; a.R = n_rays; a.rays = rays; a.valid = valid;
    hipLaunchKernelGGL(k_gen_rays_fisheye, dim3(pnr_grid_cap((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_gen_rays_fisheye");
    return PNR_OK;
}

PNR_EXPORT int pnr_gen_rays_equirect(const float* cam4_host, const float* c2w12_host, int width, int height, float near_, float far_,
                                     const int32_t* pix, int64_t n_rays, float* rays, void* stream)
{
    PNR_REQUIRE(cam4_host && c2w12_host, "pnr_gen_rays_equirect: null camera");
    PNR_REQUIRE(width >= 1 && height >= 1 && n_rays >= 0, "pnr_gen_rays_equirect: bad size");
    const int rc = pnr_equirect_check(cam4_host, width, height, "pnr_gen_rays_equirect");
    if (rc) return rc;
    if (n_rays == 0) return PNR_OK;             // before the pointer checks: an empty pixel list has a null pointer
    PNR_REQUIRE(pix || n_rays == (int64_t)width * height, "pnr_gen_rays_equirect: without pixel indices n_rays must be width*height");
    PNR_REQUIRE(rays && (((uintptr_t)rays) & 15) == 0, "pnr_gen_rays_equirect: rays must be a 16-byte aligned device buffer");
    GenRaysEquirectArgs a;
    for (int k = 0; k < 4; ++k) a.cam[k] = cam4_host[k];
    for (int k = 0; k < 12; ++k) a.c2w[k] = c2w12_host[k];
    a.width = width; a.near_ = near_; a.far_ = far_; a.pix = pix; a.R = n_rays; a.rays = rays;
    hipLaunchKernelGGL(k_gen_rays_equirect, dim3(pnr_grid_cap((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_gen_rays_equirect");
    return PNR_OK;
}

PNR_EXPORT int pnr_project_points(int model, const float* cam_host, const float* w2c12_host, int width, int height, const float* points,
                                  int64_t n, float* uv, float* range, uint8_t* valid, void* stream)
{
    PNR_REQUIRE(model == PNR_CAMERA_PINHOLE || model == PNR_CAMERA_FISHEYE || model == PNR_CAMERA_EQUIRECT,
                "pnr_project_points: unknown camera model %d", model);
    PNR_REQUIRE(cam_host && w2c12_host, "pnr_project_points: null camera");
    PNR_REQUIRE(width >= 1 && height >= 1 && n >= 0, "pnr_project_points: bad size");
    if (model == PNR_CAMERA_EQUIRECT) {
        const int rc = pnr_equirect_check(cam_host, width, height, "pnr_project_points");
        if (rc) return rc;
    }
    if (n == 0) return PNR_OK;
    PNR_REQUIRE(points, "pnr_project_points: null points");
    PNR_REQUIRE((((uintptr_t)uv) & 7) == 0, "pnr_project_points: uv must be an 8-byte aligned device buffer");
    ProjectArgs a;
    a.model = model;
    const int nc = model == PNR_CAMERA_FISHEYE ? 7 : 4;
    for (int k = 0; k < 7; ++k) a.cam[k] = k < nc ? cam_host[k] : 0.0f;
    for (int k = 0; k < 12; ++k) a.w2c[k] = w2c12_host[k];
    a.umax = (float)width - 0.5f; a.vmax = (float)height - 0.5f;
    a.pts = points; a.P = n; a.uv = reinterpret_cast<float2*>(uv); a.range = range; a.valid = valid;
    hipLaunchKernelGGL(k_project_points, dim3(pnr_grid_cap((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_project_points");
    return PNR_OK;
}
