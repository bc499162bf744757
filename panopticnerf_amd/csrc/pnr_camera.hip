// Cameras: ray generation for every camera model (k_gen_rays<model>, behind pnr_gen_rays / pnr_gen_rays_fisheye /
// pnr_gen_rays_equirect) and 3D -> 2D projection (k_project_points) (include/pnr.h "ray generation" / "cameras").  Small
// write-bound kernels: one thread per ray / point, grid-stride, camera and pose in the kernel arguments.  Every operation is a
// single + - * / sqrt in one fixed order (the build has -ffp-contract=off and correctly rounded divide / sqrt): the pinhole
// rays are bit-exact with oracle/pnr_oracle.c::pnro_gen_rays, and tests/_camera_ref.py and tests/_pano_ref.py restate the
// other kernels in float32, bit for bit.
#include <float.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"

// Ray generation: one thread per ray, two float4 stores (32 B/ray) + one byte into `valid` where wanted.
// MODEL is a constant, so an instance holds the one ray function of its model.
struct GenRaysArgs { PnrView view; float near_, far_; const int32_t* pix; int64_t R; float* rays; uint8_t* valid; };
template <int MODEL>
__global__ __launch_bounds__(256) void k_gen_rays(const GenRaysArgs a)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = a.pix ? (int64_t)a.pix[r] : r;
        const int j = (int)(p / a.view.width), i = (int)(p - (int64_t)j * a.view.width);
        bool ok;
        const PnrRayRec ray = pnr_camera_ray(MODEL, a.view.cam, a.view.pose, i, j, a.near_, a.far_, ok);
        float4* o = reinterpret_cast<float4*>(a.rays + r * 8);
        o[0] = ray.lo;
        o[1] = ray.hi;
        if (a.valid) a.valid[r] = ok ? 1 : 0;
    }
}

// the three entry points: pnr_view_check (an equirect camera in full), then, once there are rays, the focal lengths / gammas
template <int MODEL>
static int gen_rays(const char* who, const float* cam_host, const float* c2w12_host, int width, int height, float near_, float far_,
                    const int32_t* pix, int64_t n_rays, float* rays, uint8_t* valid, void* stream)
{
    GenRaysArgs a;
    const int rc = pnr_view_check(who, nullptr, MODEL, cam_host, c2w12_host, width, height, false, a.view);
    if (rc) return rc;
    PNR_REQUIRE(n_rays >= 0, "%s: bad size (n_rays must be >= 0)", who);
    if (n_rays == 0) return PNR_OK;             // before the pointer checks: an empty pixel list has a null pointer
    const int f = MODEL == PNR_CAMERA_FISHEYE ? 3 : 0;
    PNR_REQUIRE(MODEL == PNR_CAMERA_EQUIRECT || (cam_host[f] != 0.0f && cam_host[f + 1] != 0.0f), "%s: zero %s", who,
                MODEL == PNR_CAMERA_FISHEYE ? "gamma" : "focal length");
    PNR_REQUIRE(pix || n_rays == (int64_t)width * height, "%s: without pixel indices n_rays must be width*height", who);
    PNR_REQUIRE(rays && (((uintptr_t)rays) & 15) == 0, "%s: rays must be a 16-byte aligned device buffer", who);
    a.near_ = near_; a.far_ = far_; a.pix = pix; a.R = n_rays; a.rays = rays; a.valid = valid;
    hipLaunchKernelGGL(k_gen_rays<MODEL>, dim3(pnr_grid_cap((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH(who);
    return PNR_OK;
}

// Projection: one thread per point; reads 12 B, writes 8 + 4 + 1 B.  cam: pinhole {fx, fy, cx, cy}, fisheye cam7 or equirect cam4.
struct ProjectArgs { PnrView view; float umax, vmax; const float* pts; int64_t P; float2* uv; float* range; uint8_t* valid; };
__global__ __launch_bounds__(256) void k_project_points(const ProjectArgs a)
{
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.P; n += (int64_t)gridDim.x * blockDim.x) {
        const float X = a.pts[n * 3 + 0], Y = a.pts[n * 3 + 1], Z = a.pts[n * 3 + 2];
        const PnrProj q = pnr_project_point(a.view.model, a.view.cam, a.view.pose, a.umax, X, Y, Z);
        const bool inside = pnr_uv_inside(q.u, q.v, a.umax, a.vmax);
        if (a.uv) a.uv[n] = make_float2(q.u, q.v);
        if (a.range) a.range[n] = q.rng;
        if (a.valid) a.valid[n] = (q.dom && inside) ? 1 : 0;
    }
}

PNR_EXPORT int pnr_gen_rays(const float* intr4_host, const float* c2w12_host, int width, int height, float near_, float far_,
                            const int32_t* pix, int64_t n_rays, float* rays, void* stream)
{
    return gen_rays<PNR_CAMERA_PINHOLE>("pnr_gen_rays", intr4_host, c2w12_host, width, height, near_, far_, pix, n_rays, rays, nullptr, stream);
}

PNR_EXPORT int pnr_gen_rays_fisheye(const float* cam7_host, const float* c2w12_host, int width, int height, float near_, float far_,
                                    const int32_t* pix, int64_t n_rays, float* rays, uint8_t* valid, void* stream)
{
    return gen_rays<PNR_CAMERA_FISHEYE>("pnr_gen_rays_fisheye", cam7_host, c2w12_host, width, height, near_, far_, pix, n_rays, rays, valid, stream);
}

PNR_EXPORT int pnr_gen_rays_equirect(const float* cam4_host, const float* c2w12_host, int width, int height, float near_, float far_,
                                     const int32_t* pix, int64_t n_rays, float* rays, void* stream)
{
    return gen_rays<PNR_CAMERA_EQUIRECT>("pnr_gen_rays_equirect", cam4_host, c2w12_host, width, height, near_, far_, pix, n_rays, rays, nullptr, stream);
}

PNR_EXPORT int pnr_project_points(int model, const float* cam_host, const float* w2c12_host, int width, int height, const float* points,
                                  int64_t n, float* uv, float* range, uint8_t* valid, void* stream)
{
    ProjectArgs a;
    const int rc = pnr_view_check("pnr_project_points", nullptr, model, cam_host, w2c12_host, width, height, false, a.view);    // (a zero focal length is not refused here)
    if (rc) return rc;
    PNR_REQUIRE(n >= 0, "pnr_project_points: bad size (n must be >= 0)");
    if (n == 0) return PNR_OK;
    PNR_REQUIRE(points, "pnr_project_points: null points");
    PNR_REQUIRE((((uintptr_t)uv) & 7) == 0, "pnr_project_points: uv must be an 8-byte aligned device buffer");
    a.umax = pnr_view_umax(a.view); a.vmax = pnr_view_vmax(a.view);
    a.pts = points; a.P = n; a.uv = reinterpret_cast<float2*>(uv); a.range = range; a.valid = valid;
    hipLaunchKernelGGL(k_project_points, dim3(pnr_grid_cap((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_project_points");
    return PNR_OK;
}
