// "A camera" in one place (include/pnr.h "ray generation" / "cameras"): the per-pixel ray arithmetic of the three models and
// pnr_camera_ray, which picks among them by model word; the projection of a world point of any model; the rules a view adds to
// it (nearest pixel, stored depth); and the host side of a camera argument (its
// checks, its cam[7] and pose fill).  Callers: k_gen_rays<model> and k_project_points (pnr_camera.hip), k_sample_batch
// (pnr_batch.hip), k_reproject (pnr_warp.hip) and k_splat_points (pnr_splat.hip), which must write the same bits for the same
// camera, pose and pixel or point -- no other file branches on the model word.  Every operation is a single + - * / sqrt in one
// fixed order (the build has -ffp-contract=off and correctly rounded divide / sqrt); c2w may live in kernel arguments or in
// device memory.  The panoramic model's sine, cosine and arctangent are pnr_sincospi / pnr_atan2pi below -- the same kind of
// arithmetic, written out, never the device library's -- and are called from this file only.
#pragma once
#include <float.h>

#include "pnr_common.h"

struct FisheyeCam { float xi, k1, k2, g1, g2, u0, v0; };

// the (8) ray record as the two float4 a kernel stores
struct PnrRayRec { float4 lo, hi; };

// pinhole pixel (i = column, j = row): d = R ((i - cx)/fx, (j - cy)/fy, 1), o = t; d is not normalised
__device__ __forceinline__ PnrRayRec pnr_pinhole_ray(float fx, float fy, float cx, float cy, const float* c2w, int i, int j,
                                                     float near_, float far_)
{
    const float x = ((float)i - cx) / fx;
    const float y = ((float)j - cy) / fy;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = c2w[k * 4 + 0] * x, v = c2w[k * 4 + 1] * y;
        d[k] = (u + v) + c2w[k * 4 + 2];
    }
    return PnrRayRec{make_float4(c2w[3], c2w[7], c2w[11], d[0]), make_float4(d[1], d[2], near_, far_)};
}

// fisheye pixel: the un-projection of include/pnr.h "cameras"; ok = the pixel sees anything (otherwise d = 0, near = far = 0)
__device__ __forceinline__ PnrRayRec pnr_fisheye_ray(const FisheyeCam& c, const float* c2w, int i, int j, float near_, float far_, bool& ok)
{
    float x = ((float)i - c.u0) / c.g1;
    float y = ((float)j - c.v0) / c.g2;
    const float rd = sqrtf(x * x + y * y);
    // r (1 + k1 r^2 + k2 r^4) = rd: a fixed number of Newton steps from r = rd (a converged r is a fixed point of the step)
    float rr = rd;
#pragma unroll
    for (int s = 0; s < PNR_FISHEYE_NEWTON_STEPS; ++s) {
        const float r2 = rr * rr;
        const float r4 = r2 * r2;
        const float ka = c.k1 * r2, kb = c.k2 * r4;
        const float f = rr * ((1.0f + ka) + kb) - rd;
        const float fp = (1.0f + 3.0f * ka) + 5.0f * kb;
        rr = rr - f / fp;
    }
    const float sc = rd > 0.0f ? rr / rd : 1.0f;
    x = x * sc;
    y = y * sc;
    const float r2 = x * x + y * y;
    const float disc = 1.0f + (1.0f - c.xi * c.xi) * r2;
    ok = disc >= 0.0f && r2 <= FLT_MAX;           // (both false for NaN)
    const float lam = (c.xi + sqrtf(disc)) / (r2 + 1.0f);
    const float dx = lam * x, dy = lam * y, dz = lam - c.xi;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = c2w[k * 4 + 0] * dx, v = c2w[k * 4 + 1] * dy, w = c2w[k * 4 + 2] * dz;
        d[k] = ok ? (u + v) + w : 0.0f;
    }
    return PnrRayRec{make_float4(c2w[3], c2w[7], c2w[11], d[0]), make_float4(d[1], d[2], ok ? near_ : 0.0f, ok ? far_ : 0.0f)};
}

// sin(pi x), cos(pi x) by the rule of include/pnr.h "cameras": x in half-turns, finite
struct PnrSinCos { float s, c; };
__device__ __forceinline__ PnrSinCos pnr_sincospi(float x)
{
    const float k = __builtin_rintf(2.0f * x);          // ties to even
    const float r = x - 0.5f * k;                       // exact, |r| <= 1/4
    const float t = r * r;
    float p = PNR_SINPI_P4;
    p = p * t + PNR_SINPI_P3;
    p = p * t + PNR_SINPI_P2;
    p = p * t + PNR_SINPI_P1;
    p = p * t + PNR_SINPI_P0;
    const float s = r * p;
    float c = PNR_COSPI_Q5;
    c = c * t + PNR_COSPI_Q4;
    c = c * t + PNR_COSPI_Q3;
    c = c * t + PNR_COSPI_Q2;
    c = c * t + PNR_COSPI_Q1;
    c = c * t + PNR_COSPI_Q0;
    const int q = (int)k & 3;
    return PnrSinCos{q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c, q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s};
}

// atan2(y, x) / pi in [-1, 1] by the same rule; the sign tests are comparisons (-0 counts as +0)
__device__ __forceinline__ float pnr_atan2pi(float y, float x)
{
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const bool steep = ay > ax;
    const float mx = steep ? ay : ax, mn = steep ? ax : ay;
    const float a = mn / mx;
    const bool upper = a > PNR_TAN_PI_8;
    const float b = upper ? (a - 1.0f) / (a + 1.0f) : a;
    const float t = b * b;
    float p = PNR_ATANPI_A5;
    p = p * t + PNR_ATANPI_A4;
    p = p * t + PNR_ATANPI_A3;
    p = p * t + PNR_ATANPI_A2;
    p = p * t + PNR_ATANPI_A1;
    p = p * t + PNR_ATANPI_A0;
    float r = (upper ? 0.25f : 0.0f) + b * p;
    r = mx == 0.0f ? 0.0f : r;
    r = steep ? 0.5f - r : r;
    r = x < 0.0f ? 1.0f - r : r;
    return y < 0.0f ? -r : r;
}

// equirect pixel: cam = {lon0, dlon, lat0, dlat} in half-turns; d is unit length, every pixel sees something
__device__ __forceinline__ PnrRayRec pnr_equirect_ray(float lon0, float dlon, float lat0, float dlat, const float* c2w, int i, int j,
                                                      float near_, float far_)
{
    const float lam = lon0 + ((float)i + 0.5f) * dlon;
    const float psi = lat0 + ((float)j + 0.5f) * dlat;
    const PnrSinCos l = pnr_sincospi(lam), p = pnr_sincospi(psi);
    const float dx = p.c * l.s, dy = p.s, dz = p.c * l.c;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = c2w[k * 4 + 0] * dx, v = c2w[k * 4 + 1] * dy, w = c2w[k * 4 + 2] * dz;
        d[k] = (u + v) + w;
    }
    return PnrRayRec{make_float4(c2w[3], c2w[7], c2w[11], d[0]), make_float4(d[1], d[2], near_, far_)};
}

// the ray of any model: cam as pnr_project_point takes it; ok = the pixel sees anything (always, but for a fisheye).  With a
// constant model one ray function is left.
__device__ __forceinline__ PnrRayRec pnr_camera_ray(int model, const float* cam, const float* c2w, int i, int j, float near_, float far_, bool& ok)
{
    ok = true;
    if (model == PNR_CAMERA_PINHOLE) return pnr_pinhole_ray(cam[0], cam[1], cam[2], cam[3], c2w, i, j, near_, far_);
    if (model == PNR_CAMERA_EQUIRECT) return pnr_equirect_ray(cam[0], cam[1], cam[2], cam[3], c2w, i, j, near_, far_);
    return pnr_fisheye_ray(FisheyeCam{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6]}, c2w, i, j, near_, far_, ok);
}

// what every entry point that takes an equirect camera checks on the host, before any launch (include/pnr.h).  The two edge
// tests run in double with a slack of 1e-6 half-turns: the float32 rounding of 2/W or 1/H may carry a full range past its
// limit by W * dlon * 2^-24.
static inline int pnr_equirect_check(const float* cam, int width, int height, const char* who)
{
    for (int k = 0; k < 4; ++k) PNR_REQUIRE(fabsf(cam[k]) <= FLT_MAX, "%s: non-finite equirect parameter", who);
    PNR_REQUIRE(cam[1] != 0.0f && cam[3] != 0.0f, "%s: zero equirect step (dlon, dlat)", who);
    PNR_REQUIRE(fabsf(cam[0]) <= 1.0f, "%s: equirect lon0 must lie in [-1, 1] half-turns", who);
    PNR_REQUIRE(fabs((double)cam[1]) * width <= 2.0 + 1e-6, "%s: equirect longitudes span more than a full circle (|dlon| * width > 2)", who);
    const double e0 = cam[2], e1 = (double)cam[2] + (double)cam[3] * height;
    PNR_REQUIRE(e0 >= -0.5 - 1e-6 && e0 <= 0.5 + 1e-6 && e1 >= -0.5 - 1e-6 && e1 <= 0.5 + 1e-6,
                "%s: equirect rows leave the pitch range [-0.5, 0.5] half-turns", who);
    return PNR_OK;
}

static inline bool pnr_camera_model_ok(int model) { return model == PNR_CAMERA_PINHOLE || model == PNR_CAMERA_FISHEYE || model == PNR_CAMERA_EQUIRECT; }

// a camera of a known model, on the host before any launch: focal lengths / gammas / steps are divided by (`nonzero`: an entry
// point that never refused a zero leaves it out), and an equirect camera passes pnr_equirect_check
static inline int pnr_camera_check(int model, const float* cam, int width, int height, const char* who, bool nonzero = true)
{
    const bool nz = model == PNR_CAMERA_EQUIRECT ? (cam[1] != 0.0f && cam[3] != 0.0f)
                  : model == PNR_CAMERA_PINHOLE  ? (cam[0] != 0.0f && cam[1] != 0.0f) : (cam[3] != 0.0f && cam[4] != 0.0f);
    PNR_REQUIRE(nz || !nonzero, "%s: zero focal length or gamma", who);
    return model == PNR_CAMERA_EQUIRECT ? pnr_equirect_check(cam, width, height, who) : PNR_OK;
}

// the model's 4 or 7 camera floats into a kernel argument's zero-padded cam[7]; returns their number
static inline int pnr_camera_fill(int model, const float* cam_host, float* cam7)
{
    const int nc = model == PNR_CAMERA_FISHEYE ? 7 : 4;
    for (int k = 0; k < 7; ++k) cam7[k] = k < nc ? cam_host[k] : 0.0f;
    return nc;
}

static inline void pnr_pose_fill(const float* pose12_host, float* pose12)
{
    for (int k = 0; k < 12; ++k) pose12[k] = pose12_host[k];
}

// world point -> pixel coordinates of any model (include/pnr.h "cameras"): cam = pinhole {fx, fy, cx, cy}, fisheye cam7 or equirect
// {lon0, dlon, lat0, dlat}; umax = width - 0.5 (the equirect longitude wrap).  u, v are 0 outside the projection's domain (never
// NaN); rng = |p_cam|, z = p_cam.z.
struct PnrProj { float u, v, rng, z; bool dom; };
__device__ __forceinline__ PnrProj pnr_project_point(int model, const float* cam, const float* w2c, float umax, float X, float Y, float Z)
{
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t0 = w2c[k * 4 + 0] * X, t1 = w2c[k * 4 + 1] * Y, t2 = w2c[k * 4 + 2] * Z;
        p[k] = ((t0 + t1) + t2) + w2c[k * 4 + 3];
    }
    const float rng = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    float u, v;
    bool dom;
    if (model == PNR_CAMERA_PINHOLE) {
        dom = p[2] > 0.0f;
        const float x = p[0] / p[2], y = p[1] / p[2];
        u = cam[0] * x + cam[2];
        v = cam[1] * y + cam[3];
    } else if (model == PNR_CAMERA_EQUIRECT) {
        const float lam = pnr_atan2pi(p[0], p[2]);
        const float h = sqrtf(p[0] * p[0] + p[2] * p[2]);
        const float psi = pnr_atan2pi(p[1], h);
        dom = pnr_pos_finite(rng);
        u = (lam - cam[0]) / cam[1] - 0.5f;
        v = (psi - cam[2]) / cam[3] - 0.5f;
        const float per = 2.0f / __builtin_fabsf(cam[1]);       // the longitude period in pixels: at most one wrap
        u = u < -0.5f ? u + per : u >= umax ? u - per : u;
    } else {
        const float xi = cam[0], k1 = cam[1], k2 = cam[2];
        const float xs = p[0] / rng, ys = p[1] / rng, zs = p[2] / rng;
        const float den = zs + xi;
        dom = den > 0.0f && xi * zs + 1.0f > 0.0f && rng <= FLT_MAX;       // (a range that overflowed has lost its direction)
        const float x = xs / den, y = ys / den;
        const float r2 = x * x + y * y;
        const float s = (1.0f + k1 * r2) + k2 * (r2 * r2);
        u = (cam[3] * x) * s + cam[5];
        v = (cam[4] * y) * s + cam[6];
    }
    dom = dom && fabsf(u) <= FLT_MAX && fabsf(v) <= FLT_MAX;     // (false for NaN and Inf)
    return PnrProj{dom ? u : 0.0f, dom ? v : 0.0f, rng, p[2], dom};
}

// inside the image: pixel centres at integers, umax = width - 0.5, vmax = height - 0.5
__device__ __forceinline__ bool pnr_uv_inside(float u, float v, float umax, float vmax)
{
    return u >= -0.5f && u < umax && v >= -0.5f && v < vmax;
}

// nearest pixel of a coordinate inside the image (step 5 of include/pnr.h "cross-view reprojection"): floorf(u + 0.5f), clamped
// to nmax = size - 1 because u + 0.5f may round up to the size
__device__ __forceinline__ int pnr_nearest_pixel(float u, int nmax)
{
    const int i = (int)floorf(u + 0.5f);
    return i < nmax ? i : nmax;
}

// the depth a view of this model stores for a projected point: z-depth in a pinhole view, range otherwise
__device__ __forceinline__ float pnr_view_depth(int model, const PnrProj& q) { return model == PNR_CAMERA_PINHOLE ? q.z : q.rng; }
