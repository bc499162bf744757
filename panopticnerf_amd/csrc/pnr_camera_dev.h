// Per-pixel ray arithmetic of the two camera models (include/pnr.h "ray generation" / "cameras"), shared by the kernels that make
// rays: k_gen_rays (pnr_sampling.hip), k_gen_rays_fisheye (pnr_camera.hip) and k_sample_batch (pnr_batch.hip), which must write the
// same bits for the same camera, pose and pixel.  Every operation is a single + - * / sqrt in one fixed order (the build has
// -ffp-contract=off and correctly rounded divide / sqrt); c2w may live in kernel arguments or in device memory.
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
