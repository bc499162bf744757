// Exclusive int32 scan of a device array, and the kernel that zeroes one (pnr_nn.hip: the bucket table of the nearest-neighbour
// index and the per-triangle counts of mesh sampling; pnr_meshcast.hip: the cell table of the ray-casting grid -- the kernels
// are `static`, each file that includes this header carries its own copy).  Three launches on one stream, no kernel waits on
// another workgroup and nothing is atomic:
//   1. k_scan_tile_sums: workgroup b adds its tile of PNR_SCAN_TILE items into sums[b];
//   2. k_scan_top:       ONE workgroup turns sums into their exclusive scan, carrying in 64 bits, and writes the 64-bit total;
//   3. k_scan_apply:     workgroup b scans its tile again and writes out[i] = sums[b] + the items before i in the tile; the
//                        thread that holds item n - 1 also writes out[n], the int32 total.
// out has n + 1 entries and MAY BE `in` itself: a workgroup reads its own tile before it writes it, and launch 1 is over.
// The int32 prefix wraps when the total passes 2^31 - 1; a caller for whom that can happen reads total64 and refuses.
// tests/test_gpu_geometry_scale.py covers k_scan_top's carry -- three to five steps of its loop at every call site, every entry
// of out compared, out[n] included -- and the 64-bit total: 2 149 548 000 from mesh sampling, which Mesh.sample refuses.
// The block primitive is pnr_block_scan_excl (pnr_reduce_dev.h), the one pnr_mesh.hip scans its packed 64-bit counts with; that
// file's multi-launch scan around it (chunk sums out of the classify kernel, 64-bit words) is a different one.
#pragma once
#include "pnr_common.h"
#include "pnr_reduce_dev.h"

#define PNR_SCAN_PER_THREAD 4
#define PNR_SCAN_TILE (PNR_SCAN_BLOCK * PNR_SCAN_PER_THREAD)

static inline int64_t pnr_scan_tiles(int64_t n) { return (n + PNR_SCAN_TILE - 1) / PNR_SCAN_TILE; }

// bytes of `ws` for a scan of n items: one int32 per tile, rounded up to 8 bytes
static inline int64_t pnr_scan_workspace_bytes(int64_t n) { return (pnr_scan_tiles(n) * 4 + 7) & ~(int64_t)7; }

#ifdef __HIPCC__
static __global__ __launch_bounds__(PNR_SCAN_BLOCK) void k_scan_tile_sums(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ sums)
{
    __shared__ int32_t lds[4];
    const int64_t base = (int64_t)blockIdx.x * PNR_SCAN_TILE + (int64_t)threadIdx.x * PNR_SCAN_PER_THREAD;
    int32_t s = 0;
#pragma unroll
    for (int i = 0; i < PNR_SCAN_PER_THREAD; ++i) s += base + i < n ? in[base + i] : 0;
    int32_t total;
    pnr_block_scan_excl<int32_t>(s, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

static __global__ __launch_bounds__(PNR_SCAN_BLOCK) void k_scan_top(int32_t* __restrict__ sums, int64_t tiles, long long* __restrict__ total64)
{
    __shared__ long long lds[4];
    long long carry = 0;
    for (int64_t c = 0; c < tiles; c += PNR_SCAN_BLOCK) {           // (uniform over the workgroup)
        const int64_t i = c + threadIdx.x;
        const long long v = i < tiles ? (long long)sums[i] : 0ll;
        long long total;
        const long long before = pnr_block_scan_excl<long long>(v, lds, total);
        if (i < tiles) sums[i] = (int32_t)(carry + before);
        carry += total;
    }
    if (threadIdx.x == 0) total64[0] = carry;
}

static __global__ __launch_bounds__(PNR_SCAN_BLOCK) void k_scan_apply(const int32_t* in, int64_t n, const int32_t* __restrict__ sums, int32_t* out)
{
    __shared__ int32_t lds[4];
    const int64_t base = (int64_t)blockIdx.x * PNR_SCAN_TILE + (int64_t)threadIdx.x * PNR_SCAN_PER_THREAD;
    int32_t v[PNR_SCAN_PER_THREAD], s = 0;
#pragma unroll
    for (int i = 0; i < PNR_SCAN_PER_THREAD; ++i) {
        v[i] = base + i < n ? in[base + i] : 0;
        s += v[i];
    }
    int32_t total;
    int32_t run = sums[blockIdx.x] + pnr_block_scan_excl<int32_t>(s, lds, total);
#pragma unroll
    for (int i = 0; i < PNR_SCAN_PER_THREAD; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
        if (base + i == n - 1) out[n] = run;
    }
}

// p[0 .. n) = 0: a kernel and not a memset, so that a captured build is a plain chain of kernel nodes
static __global__ __launch_bounds__(256) void k_zero_i32(int32_t* __restrict__ p, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0;
}

static inline void pnr_zero_i32(int32_t* p, int64_t n, hipStream_t st) { hipLaunchKernelGGL(k_zero_i32, dim3(pnr_grid_cap((n + 255) / 256)), dim3(256), 0, st, p, n); }

// out[0 .. n] = the exclusive scan of in[0 .. n) and the total; total64 (device, 8-byte aligned) receives the 64-bit total;
// ws: pnr_scan_workspace_bytes(n) bytes, 4-byte aligned.  n >= 1.  The caller checks the launches (PNR_CHECK_LAUNCH).
static inline void pnr_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, int64_t* total, hipStream_t st)
{
    const int64_t tiles = pnr_scan_tiles(n);
    long long* total64 = (long long*)total;
    int32_t* sums = (int32_t*)ws;
    hipLaunchKernelGGL(k_scan_tile_sums, dim3((unsigned)tiles), dim3(PNR_SCAN_BLOCK), 0, st, in, n, sums);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(PNR_SCAN_BLOCK), 0, st, sums, tiles, total64);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)tiles), dim3(PNR_SCAN_BLOCK), 0, st, in, n, (const int32_t*)sums, out);
}
#endif
