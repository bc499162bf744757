// Block-wide reductions of the geometry kernels, one definition each (DESIGN.md section 8 "Ordered reductions"): the ordered sum
// of K doubles per workgroup and the combine of its rows (k_depth_metrics, k_cloud_metrics, k_icp_accumulate and their second
// kernels), the reduction of integer counters (those and k_splat_points, k_nn_query, k_reproject) and the exclusive block scan
// (pnr_scan_dev.h, pnr_mesh.hip).  The ORDER of the floating additions is part of those kernels' contract -- the same bits on
// every run, no floating atomics -- and tests/_reduce_ref.py restates it: a new metric kernel calls these and copies nothing.
#pragma once
#include "pnr_common.h"

#define PNR_REDUCE_BLOCK 256            // threads of a workgroup that calls pnr_block_sum_rows
#define PNR_REDUCE_BATCH 32             // rows pnr_rows_total fetches at once
#define PNR_SCAN_BLOCK 256              // threads of a workgroup that calls pnr_block_scan_excl
static_assert(PNR_REDUCE_BLOCK == 4 * 64 && PNR_SCAN_BLOCK == 4 * 64, "four waves of 64: ((w0 + w1) + w2) + w3 and the scan's 4 words of LDS");

// workgroups of PNR_REDUCE_BLOCK threads for n items, within [1, max_blocks]: what a workspace of rows is sized for
static inline int64_t pnr_reduce_blocks(int64_t n, int64_t max_blocks)
{
    const int64_t b = (n + PNR_REDUCE_BLOCK - 1) / PNR_REDUCE_BLOCK;
    return b < 1 ? 1 : b > max_blocks ? max_blocks : b;
}

#ifdef __HIPCC__
// partial[blockIdx.x * stride + k] = the workgroup's sum of s[k], k < K <= stride, in one fixed order: the wave's xor butterfly
// (m = 32 .. 1), one LDS slot per wave, then ((w0 + w1) + w2) + w3.  Called by every thread of the workgroup; what a caller
// wrote to LDS of its own before the call is visible after it (one barrier inside, after the waves' slots are written).
template <int K>
__device__ __forceinline__ void pnr_block_sum_rows(const double (&s)[K], double (&red)[4][K], double* partial, int stride)
{
    static_assert(K <= PNR_REDUCE_BLOCK, "thread k writes term k");
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = s[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K)
        partial[(int64_t)blockIdx.x * stride + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Slot `slot` of rows 0, 1, ... n_rows - 1 (rows are STRIDE words apart) added in that order from 0.0.  The additions are a
// serial chain, the loads need not be: PNR_REDUCE_BATCH rows are fetched at once (a row beyond the last counts +0.0, which
// changes no sum), then added in order.  One load per addition leaves the lane waiting a memory latency per row: measured 0.053
// against 0.008 ms for 256 rows of k_icp_solve, and 145 against 40 us for both launches of pnr_depth_metrics at 1024 rows,
// results bit-identical.  `words`: the same slots added as integers (a row's count slot); a caller that reads only one of the
// two pays for that one.
struct PnrRowsTotal { double sum; unsigned long long words; };
template <int STRIDE>
__device__ __forceinline__ PnrRowsTotal pnr_rows_total(const unsigned long long* rows, int n_rows, int slot)
{
    PnrRowsTotal t = {0.0, 0ull};
    for (int b0 = 0; b0 < n_rows; b0 += PNR_REDUCE_BATCH) {
        unsigned long long raw[PNR_REDUCE_BATCH];
#pragma unroll
        for (int k = 0; k < PNR_REDUCE_BATCH; ++k) raw[k] = b0 + k < n_rows ? rows[(int64_t)(b0 + k) * STRIDE + slot] : 0ull;
#pragma unroll
        for (int k = 0; k < PNR_REDUCE_BATCH; ++k) {
            t.sum += __longlong_as_double((long long)raw[k]);
            t.words += raw[k];
        }
    }
    return t;
}

// stats[k] += the block's sum of cnt[k], k < K: the wave's butterfly, one LDS atomic per wave, one global atomic per block and
// non-zero counter (integers: exact in any order).  Called by every thread of the block; h: K words of LDS, free to hold
// anything before the first barrier.
template <int K>
__device__ __forceinline__ void pnr_block_count_add(const unsigned int (&cnt)[K], unsigned int* h, unsigned long long* stats)
{
    __syncthreads();
    if (threadIdx.x < K) h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned int c = cnt[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&h[k], c);
    }
    __syncthreads();
    if (threadIdx.x < K && h[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// exclusive scan of v over the PNR_SCAN_BLOCK threads of the workgroup in thread order; total: the workgroup's sum.  lds: 4 words
// of T, free again on return (a caller's next trip may write them).
template <typename T>
__device__ __forceinline__ T pnr_block_scan_excl(T v, T* lds, T& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < PNR_SCAN_BLOCK / 64; ++w) {
        const T s = lds[w];
        before += w < wave ? s : (T)0;
        total += s;
    }
    __syncthreads();
    return before + incl - v;
}
#endif
