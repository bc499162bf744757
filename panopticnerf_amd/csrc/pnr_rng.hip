// In-kernel RNG (include/pnr.h "in-kernel RNG"): the descriptor check every _rng entry point runs before any device work, the
// one-thread pnr_rng_begin and pnr_rng_fill, which materialises a stream as a tensor (the explicit-tensor entry points fed with
// it draw exactly what the _rng twins draw inside their kernels).
#include "pnr_common.h"
#include "pnr_philox.h"

int pnr_rng_check(const pnr_rng* r, int64_t n_rays, const char* who, PnrRngDev* out)
{
    PNR_REQUIRE(r && r->call, "%s: null rng descriptor or call", who);
    PNR_REQUIRE(r->tag >= 1 && r->tag <= 255, "%s: rng tag %d outside [1,255]", who, (int)r->tag);
    PNR_REQUIRE(r->scale >= 0.0f, "%s: rng scale must be >= 0 (got %g)", who, (double)r->scale);
    PNR_REQUIRE(r->ray_base >= 0 && n_rays >= 0 && r->ray_base + n_rays <= ((int64_t)1 << 32),
                "%s: rng ray_base %lld + n_rays %lld outside [0, 2^32]", who, (long long)r->ray_base, (long long)n_rays);
    PNR_REQUIRE((((uintptr_t)r->call) & 7) == 0, "%s: rng call must be 8-byte aligned", who);
    out->call = r->call;
    out->ray_base = (uint32_t)r->ray_base;
    out->tag = (uint32_t)r->tag;
    out->scale = r->scale;
    return PNR_OK;
}

__global__ void k_rng_begin(int64_t* __restrict__ state, int64_t* __restrict__ call)
{
    const int64_t seed = state[0], off = state[1];
    call[0] = seed;
    call[1] = off;
    state[1] = off + 1;
}

PNR_EXPORT int pnr_rng_begin(int64_t* state, int64_t* call, void* stream)
{
    PNR_REQUIRE(state && call && state != call, "pnr_rng_begin: null or aliased state / call");
    PNR_REQUIRE(((((uintptr_t)state) | ((uintptr_t)call)) & 7) == 0, "pnr_rng_begin: state / call must be 8-byte aligned");
    hipLaunchKernelGGL(k_rng_begin, dim3(1), dim3(1), 0, (hipStream_t)stream, state, call);
    PNR_CHECK_LAUNCH("pnr_rng_begin");
    return PNR_OK;
}

// one thread per 4-sample block of a ray: one Philox call, up to four stores
__global__ __launch_bounds__(256) void k_rng_fill(const PnrRngDev rng, int64_t R, int N, int normal, float* __restrict__ out)
{
    const PnrRngKey key = pnr_rng_key(rng);
    const int nb = (N + 3) >> 2;
    const int64_t total = R * nb;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / nb;
        const int b = (int)(t - r * nb);
        float v[4];
        if (normal) {
            pnr_rng_normal4(key, (uint32_t)r, (uint32_t)b, v);
        } else {
            const pnr_u4 w = pnr_rng_block(key, (uint32_t)r, (uint32_t)b);
            v[0] = pnr_uniform(w.x); v[1] = pnr_uniform(w.y); v[2] = pnr_uniform(w.z); v[3] = pnr_uniform(w.w);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * b + k < N) out[r * N + 4 * b + k] = v[k];
    }
}

PNR_EXPORT int pnr_rng_fill(const pnr_rng* rng_host, int64_t n_rays, int n_samples, int normal, float* out, void* stream)
{
    PnrRngDev rng;
    const int rc = pnr_rng_check(rng_host, n_rays, "pnr_rng_fill", &rng);
    if (rc) return rc;
    PNR_REQUIRE(n_samples >= 1 && n_samples <= (1 << 26), "pnr_rng_fill: n_samples=%d outside [1, 2^26]", n_samples);
    if (n_rays == 0) return PNR_OK;
    PNR_REQUIRE(out, "pnr_rng_fill: null pointer");
    const int64_t total = n_rays * ((n_samples + 3) / 4);
    hipLaunchKernelGGL(k_rng_fill, dim3(pnr_grid_cap((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rng, n_rays, n_samples,
                       normal, out);
    PNR_CHECK_LAUNCH("pnr_rng_fill");
    return PNR_OK;
}
