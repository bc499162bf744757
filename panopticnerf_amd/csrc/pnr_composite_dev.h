// The shared frame of the compositing family: k_composite, k_composite2, k_composite_combine (pnr_composite.hip), k_composite_bwd
// (pnr_composite_bwd.hip), and the single-sample pieces the fused MLP epilogue (pnr_mlp_fuse.h) and k_ce3d (pnr_losses.hip) restate.
// Every piece exists once; each kernel keeps its own body and schedule and is assembled from them.  All __forceinline__, and
// written so that a kernel's machine code is what it was with the piece spelled out in place (tools/isa_diff.py).
// What is deliberately NOT here, because the kernels differ in it (bits would change): how alpha and the prefix become a weight
// (forward: (alpha Tl) excl; backward: alpha (Tl excl)), how a lane's weights are summed, and where an inactive lane is neutralised.
// -ffp-contract=off: an FMA exists only where the source says fmaf.
#pragma once
#include <type_traits>

#include "pnr_common.h"
#include "pnr_fuse_record.h"
#include "pnr_lane_ops.h"
#include "pnr_philox.h"

// ------------------------------------------------------------------------------------------------------------------- rows
struct f4 { float v[4]; };

// four consecutive samples of a row (16-byte aligned); an inactive lane gets zeros and touches no memory
__device__ __forceinline__ f4 ld4(const float* p, bool active)
{
    f4 o;
    if (!active) { o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f; return o; }
    const float4 t = *reinterpret_cast<const float4*>(p);
    o.v[0] = t.x; o.v[1] = t.y; o.v[2] = t.z; o.v[3] = t.w;
    return o;
}
__device__ __forceinline__ void st4(float* p, const float* v, bool active)
{
    if (active) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
// Row access as (wave-uniform row pointer) + (32-bit per-lane byte offset): hipcc then selects the scalar-base form of
// global_load / global_store (SGPR pair + one shared VGPR offset) instead of materialising a 64-bit VGPR address per row in
// flight -- two registers per row, which is what pushed k_composite_bwd past 128 VGPRs (3 waves per SIMD instead of 4).
template <class T>
__device__ __forceinline__ T* row_at(T* row, uint32_t ob)
{
    using B = std::conditional_t<std::is_const_v<T>, const char, char>;
    return reinterpret_cast<T*>(reinterpret_cast<B*>(row) + ob);
}
__device__ __forceinline__ f4 ld4o(const float* row, uint32_t ob, bool active) { return ld4(row_at(row, ob), active); }
__device__ __forceinline__ void st4o(float* row, uint32_t ob, const f4& v, bool active) { st4(row_at(row, ob), v.v, active); }

// channel c of the four samples from s0 on, in either image layout (CH_MAJOR: element (s, c) at raw[c sc + s]; else at raw[s ss + c sc])
template <bool CH_MAJOR>
__device__ __forceinline__ f4 load4(const float* __restrict__ raw, int64_t ss, int64_t sc, int64_t s0, int c, bool active)
{
    if (CH_MAJOR) return ld4(raw + (int64_t)c * sc + s0, active);
    f4 o;
    if (!active) { o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f; return o; }
    const float* p = raw + s0 * ss + (int64_t)c * sc;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.v[k] = p[k * ss];
    return o;
}

// a lane's M4 pieces of a row (base = the row's first element of this lane)
template <int M4>
__device__ __forceinline__ void ld_row(const float* base, const bool (&act)[M4], float (&v)[4 * M4])
{
#pragma unroll
    for (int j = 0; j < M4; ++j) {
        const f4 t = ld4(base + 4 * j, act[j]);
        v[4 * j] = t.v[0]; v[4 * j + 1] = t.v[1]; v[4 * j + 2] = t.v[2]; v[4 * j + 3] = t.v[3];
    }
}

// the bbox labels of four samples; -1 (no label) where the lane does not read them
__device__ __forceinline__ void ld4_labels(const int32_t* p, bool on, int (&l)[4])
{
    l[0] = l[1] = l[2] = l[3] = -1;
    if (on) { const int4 t = *reinterpret_cast<const int4*>(p); l[0] = t.x; l[1] = t.y; l[2] = t.z; l[3] = t.w; }
}

// ------------------------------------------------------------------------------------------------------ ray-group prologue
// A ray is owned by L consecutive lanes, each holding M4 float4 pieces = 4 M4 CONSECUTIVE samples (N <= 4 M4 L); a wave holds a
// group of 64 / L rays and the waves of the grid stride over the n_groups groups.  The stride's two ends -- the wave's global index and
// the number of waves -- are read in the kernel itself: blockDim.x is folded to the launch's constant only where a __global__
// function reads it; read in here it became a load and a wait at the head of every kernel.
template <int L, int M4>
struct RayLanes {
    static constexpr int RPW = 64 / L;
    int q, g, i0;                    // the lane's position in its ray, the ray's place in the wave, the lane's first sample
    int64_t n_groups;                // ray groups in all
    // of the current group:
    int64_t ray, rayc, s0;           // the lane's ray, the same clamped to a ray that exists, index of the lane's first sample in an (R, N) array
    bool valid, act[M4];             // the ray exists; piece j of the lane lies inside it (an inactive lane is pointed at its ray's sample 0)

    __device__ __forceinline__ RayLanes(int64_t R)
    {
        const int lane = threadIdx.x & 63;
        q = lane & (L - 1);
        g = lane / L;
        i0 = q * 4 * M4;
        n_groups = (R + RPW - 1) / RPW;
    }
    __device__ __forceinline__ void at(int64_t grp, int64_t R, int N)
    {
        ray = grp * RPW + g;
        valid = ray < R;
        rayc = valid ? ray : R - 1;
#pragma unroll
        for (int j = 0; j < M4; ++j) act[j] = valid && (i0 + 4 * j < N);
        s0 = rayc * N + (act[0] ? i0 : 0);
    }
};

// |d| of a ray (rays: (R, 8) = o, d, near, far)
__device__ __forceinline__ float ray_dir_norm(const float* rays, int64_t ray)
{
    const float dx = rays[ray * 8 + 3], dy = rays[ray * 8 + 4], dz = rays[ray * 8 + 5];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// ---------------------------------------------------------------------------------------------------------- sigma noise
// The noise of one float4 piece added to its sigmas: block `blk` of the ray's in-kernel stream (RNG; a piece of four consecutive
// samples is one Philox block -- WHICH block is the mapping's rule, so the kernel says it), else the tensor's four values at np
// when there is a tensor.
template <bool RNG>
__device__ __forceinline__ void add_sigma_noise4(float* sg, bool active, const PnrRngKey& key, uint32_t ray, uint32_t blk, bool have, const float* np)
{
    if constexpr (RNG) {
        if (active) {
            float n[4];
            pnr_rng_normal4(key, ray, blk, n);
#pragma unroll
            for (int k = 0; k < 4; ++k) sg[k] += n[k];
        }
    } else if (have) {
        const f4 t = ld4(np, active);
#pragma unroll
        for (int k = 0; k < 4; ++k) sg[k] += t.v[k];
    }
}

// ---------------------------------------------------------------------------------------------------------- alpha chain
// one sample: the interval (1e10 behind a ray's last sample) scaled by |d|, alpha = 1 - exp(-relu(sigma) dist), and the factor
// alpha contributes to the transmittance of everything behind it
__device__ __forceinline__ float sample_dist(bool last, float z, float znext, float dn)
{
    float dist = last ? 1e10f : (znext - z);
    dist *= dn;
    return dist;
}
__device__ __forceinline__ float sample_alpha(float sigma, float dist) { return 1.0f - expf(-(fmaxf(sigma, 0.0f) * dist)); }
__device__ __forceinline__ float alpha_factor(float alpha) { return (1.0f - alpha) + 1e-10f; }

// A lane's M consecutive samples i0 .. i0 + M - 1 (znext: z of the next lane's first sample): alpha[k], Tl[k] = the product of
// the lane's factors BEFORE sample k, dist[k] if asked for; returns the product of all M factors.
template <int M>
__device__ __forceinline__ float alpha_chain(const float (&z)[M], float znext, const float (&sg)[M], int i0, int N, float dn,
                                             float (&alpha)[M], float (&Tl)[M], float* dist = nullptr)
{
    float P = 1.0f;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const float d = sample_dist(!(i0 + k + 1 < N), z[k], (k < M - 1) ? z[k + 1] : znext, dn);
        if (dist) dist[k] = d;
        alpha[k] = sample_alpha(sg[k], d);
        Tl[k] = P;
        P *= alpha_factor(alpha[k]);
    }
    return P;
}

__device__ __forceinline__ float sigmoid_of(float v) { return 1.0f / (1.0f + expf(-v)); }

// ---------------------------------------------------------------------------------------------------------------- scans
// Segmented inclusive product scan of P over the SUB lanes of a ray (q = lane's position); returns the EXCLUSIVE value = the
// transmittance in front of the lane.  __shfl_up form: any SUB up to the wave.
template <int SUB>
__device__ __forceinline__ float scan_excl_shfl(float P, int q)
{
    float x = P;
#pragma unroll
    for (int d = 1; d < SUB; d <<= 1) {
        const float y = __shfl_up(x, d, 64);
        if (q >= d) x *= y;
    }
    float excl = __shfl_up(x, 1, 64);
    if (q == 0) excl = 1.0f;
    return excl;
}
// The same inside a 16-lane DPP row (row_shr:d; a lane without a source keeps the identity): L = 8 or 16, no LDS crossbar.
// (tile_scan of pnr_mlp_fuse.h is a different scan: 32 lanes, row_bcast15.)
template <int L>
__device__ __forceinline__ float scan_excl_dpp(float P, int q)
{
    static_assert(L == 8 || L == 16, "a ray must sit inside one 16-lane DPP row");
    float x = P;
    float y = dpp_or<0x111>(x, 1.0f); x *= (L == 16 || q >= 1) ? y : 1.0f;
    y = dpp_or<0x112>(x, 1.0f); x *= (L == 16 || q >= 2) ? y : 1.0f;
    y = dpp_or<0x114>(x, 1.0f); x *= (L == 16 || q >= 4) ? y : 1.0f;
    if constexpr (L == 16) { y = dpp_or<0x118>(x, 1.0f); x *= y; }
    float excl = dpp_or<0x111>(x, 1.0f);
    if (q == 0) excl = 1.0f;
    return excl;
}

// --------------------------------------------------------------------------------------------------- fixed-field histogram
// fix_x[c] = sum_i w_i [label_i == c] as a per-ray histogram in LDS, in 2^-30 fixed point (PNR_FUSE_FIX_SCALE; a ray's weights sum
// to <= 1) with integer adds: associative, so bit-reproducible whatever the order.  Bins: [0, C) semantic, [C, C + K) instance.
// LDS operations of one wave execute in order and only the ray's own lanes (of one wave) touch its bins: no barrier anywhere.
template <int L>
__device__ __forceinline__ void hist_zero(uint32_t* hist, int q, int CK)
{
    for (int c = q; c < CK; c += L) hist[c] = 0;
}
// (the labels by reference: a label is read only behind its field's `want`, as the kernels had it)
__device__ __forceinline__ void hist_add(uint32_t* hist, float w, bool want_s, const int& ls, int C, bool want_i, const int& li, int K)
{
    const uint32_t fx = (uint32_t)(w * PNR_FUSE_FIX_SCALE + 0.5f);
    if (want_s) { const int l = ls; if (l >= 0 && l < C) atomicAdd(&hist[l], fx); }
    if (want_i) { const int l = li; if (l >= 0 && l < K) atomicAdd(&hist[C + l], fx); }
}
__device__ __forceinline__ float hist_read(const uint32_t* hist, int c) { return (float)hist[c] * (1.0f / PNR_FUSE_FIX_SCALE); }
// the ray's L lanes write its fixed-field rows
template <int L>
__device__ __forceinline__ void hist_store(const uint32_t* hist, int q, int64_t ray, bool want_s, float* fix_sem, int C, bool want_i, float* fix_inst, int K)
{
    if (want_s) for (int c = q; c < C; c += L) fix_sem[ray * C + c] = hist_read(hist, c);
    if (want_i) for (int c = q; c < K; c += L) fix_inst[ray * K + c] = hist_read(hist, C + c);
}

// ---------------------------------------------------------------------------------------------------------- log-sum-exp
// One step of the online form, (mx, den) <- v, with ONE expf per value: of the two factors expf(mx - m2), expf(v - m2) one is
// always expf(0) = 1 (same bits as the two-expf form).  Start from mx = -inf, den = 0.
__device__ __forceinline__ void lse_step(float& mx, float& den, float v)
{
    const float d = v - mx, e = expf(-fabsf(d));
    den = d <= 0.0f ? den + e : den * e + 1.0f;
    mx = fmaxf(mx, v);
}
__device__ __forceinline__ float softmax_of(float v, float mx, float den) { return expf(v - mx) / den; }

// ------------------------------------------------------------------------------------------------------------ row store
// A batch of UB reduced rows q0 .. q0 + UB - 1 of ray `ray` (rows: 3 rgb, C semantic, K instance; nq of them in all)
template <int UB, class Args>
__device__ __forceinline__ void store_rows(const Args& a, int64_t ray, int q0, int nq, const float (&r)[UB], float accv)
{
#pragma unroll
    for (int j = 0; j < UB; ++j) {
        const int qq = q0 + j;
        if (qq >= nq) continue;
        if (qq < 3) { if (a.rgb) a.rgb[ray * 3 + qq] = a.white_bkgd ? r[j] + (1.0f - accv) : r[j]; }
        else if (qq - 3 < a.C) { if (a.sem) a.sem[ray * a.C + (qq - 3)] = r[j]; }
        else { if (a.inst) a.inst[ray * a.K + (qq - 3 - a.C)] = r[j]; }
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
// `sub` (one of SUBS...), the compositing mode, the image layout and the noise source as compile-time constants:
// launch(integral_constant<int, SUB>, bool_constant<CH_MAJOR>, bool_constant<SOFTMAX>[, the device stream]).  The in-kernel stream
// exists for channel-major images only, so no <sample-major, stream> instance is ever asked for.
template <int... SUBS, class F>
static void composite_dispatch(int sub, bool ch_major, bool softmax, const PnrRngDev* rng, F&& launch)
{
    auto one = [&](auto S) {
        auto mode = [&](auto SM) {
            if (rng) launch(S, std::true_type{}, SM, *rng);
            else if (ch_major) launch(S, std::true_type{}, SM);
            else launch(S, std::false_type{}, SM);
        };
        if (softmax) mode(std::true_type{}); else mode(std::false_type{});
    };
    ((sub == SUBS ? one(std::integral_constant<int, SUBS>{}) : void()), ...);
}
