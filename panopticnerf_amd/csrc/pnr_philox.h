// In-kernel random numbers (include/pnr.h "in-kernel RNG"): Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as
// 1, 2, 3", SC'11), a counter-based generator -- no per-thread state; any draw of any stream is a pure function of (key,
// counter), so a kernel that needs a draw computes it where it is used and the backward recomputes the forward's.
// Host and device (the host copy is what a CPU build can check against the known-answer vectors).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNR_HD __host__ __device__ __forceinline__
#else
#define PNR_HD static inline
#endif

struct pnr_u4 { uint32_t x, y, z, w; };

PNR_HD uint32_t pnr_mulhi32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32 with 10 rounds; key (k0, k1), counter c
PNR_HD pnr_u4 pnr_philox4x32_10(pnr_u4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = pnr_mulhi32(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = pnr_mulhi32(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = pnr_u4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    }
    return c;
}

// One in-kernel stream as a kernel sees it (pnr_rng of include/pnr.h, validated on the host): the call's (seed, offset) are READ
// FROM DEVICE MEMORY when the kernel runs -- a captured graph's replays each draw what their own pnr_rng_begin wrote.
struct PnrRngDev {
    const int64_t* call;       // {seed, offset}
    uint32_t ray_base;         // global index of the launch's ray 0 (ray_base + n_rays <= 2^32: the host checks)
    uint32_t tag;              // 1 .. 255
    float scale;               // normal draws: noise = scale * n
};

// The per-launch half of the counter: key and the two words that do not depend on the ray or the sample.
struct PnrRngKey { uint32_t k0, k1, off_lo, off_hi, tag24, ray_base; float scale; };

#if defined(__HIPCC__)
__device__ __forceinline__ PnrRngKey pnr_rng_key(const PnrRngDev& r)
{
    const uint64_t seed = (uint64_t)r.call[0], off = (uint64_t)r.call[1];
    return PnrRngKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)off, (uint32_t)(off >> 32), r.tag << 24, r.ray_base, r.scale};
}
#endif

// the 4 words of block b (= samples 4 b .. 4 b + 3) of local ray `ray`
PNR_HD pnr_u4 pnr_rng_block(const PnrRngKey& k, uint32_t ray, uint32_t b)
{
    return pnr_philox4x32_10(pnr_u4{b | k.tag24, k.ray_base + ray, k.off_lo, k.off_hi}, k.k0, k.k1);
}

PNR_HD uint32_t pnr_u4_word(const pnr_u4& v, int i)
{
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// uniform in [0, 1): the top 24 bits (what torch.rand's float draws are: multiples of 2^-24)
PNR_HD float pnr_uniform(uint32_t w)
{
    return (float)(w >> 8) * 0x1p-24f;
}

// Box-Muller on the word pair (a, b): (n0, n1).  u1 in (0, 1] (log finite), u2 in [0, 1); sincospi on 2 u2 (exact in fp32)
// keeps the angle's rounding out of the result.
#if defined(__HIPCC__)
__device__ __forceinline__ void pnr_box_muller(uint32_t a, uint32_t b, float& n0, float& n1)
{
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f, u2 = (float)(b >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// the block as 4 normals times k.scale
__device__ __forceinline__ void pnr_rng_normal4(const PnrRngKey& k, uint32_t ray, uint32_t b, float (&n)[4])
{
    const pnr_u4 v = pnr_rng_block(k, ray, b);
    pnr_box_muller(v.x, v.y, n[0], n[1]);
    pnr_box_muller(v.z, v.w, n[2], n[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) n[i] *= k.scale;
}

// sample j of local ray `ray` as a uniform (one Philox call per draw: for kernels with one thread per sample)
__device__ __forceinline__ float pnr_rng_uniform_at(const PnrRngKey& k, uint32_t ray, int j)
{
    return pnr_uniform(pnr_u4_word(pnr_rng_block(k, ray, (uint32_t)j >> 2), j & 3));
}
#endif

#ifdef PNR_H
// host: validate a pnr_rng descriptor for a launch of n_rays rays and convert it (pnr_rng.hip; PNR_EINVAL + message otherwise)
int pnr_rng_check(const pnr_rng* r, int64_t n_rays, const char* who, PnrRngDev* out);
#endif
