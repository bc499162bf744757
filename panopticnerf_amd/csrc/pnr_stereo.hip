// Stereo matching (include/pnr.h "stereo matching"): a rectified 8-bit pair -> census words -> semi-global path aggregation of the
// Hamming cost into the summed volume S (H, W, D) uint16 -> disparity in sixteenths of a pixel with the uniqueness and the
// left-right check -> depth.  Integer arithmetic up to the one float32 division of the depth; tests/_sgm_ref.py restates the rule.
//
// The aggregation is the hot path.  The matching cost is never stored: every step recomputes it from the two census images (16
// bytes per pixel, cache resident along a path), so the only volume that moves is S.  One launch per direction, in the rule's
// order on the one stream; the first STORES its path cost, the others ADD theirs (a pixel lies on exactly one path of a
// direction, so a launch never races with itself and launches are stream-ordered: no atomics).  A path is a serial chain walked
// by G lanes, each holding V CONTIGUOUS disparities (G V >= D, V a power of two): up to 48 disparities G = 16 -- one DPP row,
// four paths a wave --, above it G = 64, one path a wave with 1, 2 or 4 disparities a lane, because a wave issues one
// instruction at a time and the step is as long as its instruction count.  The minimum over d is a row butterfly (and two
// v_permlane swaps across the rows), the d - 1 / d + 1 neighbours across lanes are row_shr:1 / row_shl:1 (wave_shr:1 /
// wave_shl:1) with "absent" as the value of the lanes that have no source, and a lane's piece of an S row is one 2 V-byte
// vector access.  A step's memory is read PNR_SGM_PREFETCH steps ahead of the step.
#include <float.h>

#include "pnr_common.h"

#define PNR_SGM_ABSENT 0x10000            // a path cost that never wins a minimum (a real one is at most 63 + 192)
#define PNR_SGM_PATH_WAVES_PER_CU 8       // k_sgm_path's grid: one-wave blocks, so many per CU, grid-stride over the rest
#define PNR_SGM_ROW_PATH_MAX 48           // up to so many disparities a row of 16 lanes walks a path, above it the whole wave
// -DPNR_SGM_PREFETCH=n (A/B builds, 1 .. 4): how many steps ahead of its use a path step's memory is read.  tools/sgm_time.py is
// its A/B (profiles/README.md "Stereo").
#ifndef PNR_SGM_PREFETCH
#define PNR_SGM_PREFETCH 4
#endif

// ---- cross-lane pieces, all inside a DPP row of 16 lanes (no LDS)
template <int CTRL>
__device__ __forceinline__ int row_min_step(int x)
{
    const int y = __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, true);
    return y < x ? y : x;
}
// minimum over the 16 lanes of this lane's row; every lane of the row ends up with it (the pairings of pnr_lane_ops.h xor_add)
__device__ __forceinline__ int row_min(int x)
{
    x = row_min_step<0xB1>(x);            // quad_perm [1,0,3,2]
    x = row_min_step<0x4E>(x);            // quad_perm [2,3,0,1]
    x = row_min_step<0x141>(x);           // row_half_mirror
    x = row_min_step<0x140>(x);           // row_mirror
    return x;
}
// the value of the previous / next lane of the row; `absent` in the row's first / last lane
__device__ __forceinline__ int row_prev(int x, int absent) { return __builtin_amdgcn_update_dpp(absent, x, 0x111, 0xF, 0xF, false); }
__device__ __forceinline__ int row_next(int x, int absent) { return __builtin_amdgcn_update_dpp(absent, x, 0x101, 0xF, 0xF, false); }

// the same three over a group of G lanes, G = 16 (a row) or 64 (the wave): the minimum crosses the rows by v_permlane16_swap and
// v_permlane32_swap on two copies (pnr_lane_ops.h xor_max<16>), the neighbours by wave_shr:1 / wave_shl:1.  All VALU, no LDS.
template <int G>
__device__ __forceinline__ int group_min(int x)
{
    x = row_min(x);
    if constexpr (G == 64) {
        const auto p = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
        x = (int)p[0] < (int)p[1] ? (int)p[0] : (int)p[1];
        const auto q = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
        x = (int)q[0] < (int)q[1] ? (int)q[0] : (int)q[1];
    }
    return x;
}
template <int G>
__device__ __forceinline__ int group_prev(int x, int absent)
{
    if constexpr (G == 64) return __builtin_amdgcn_update_dpp(absent, x, 0x138, 0xF, 0xF, false);
    else return row_prev(x, absent);
}
template <int G>
__device__ __forceinline__ int group_next(int x, int absent)
{
    if constexpr (G == 64) return __builtin_amdgcn_update_dpp(absent, x, 0x130, 0xF, 0xF, false);
    else return row_next(x, absent);
}

template <int V> struct SgmVec { typedef unsigned short type __attribute__((ext_vector_type(V))); };
template <> struct SgmVec<1> { typedef unsigned short type; };
template <int V> __device__ __forceinline__ int sgm_get(const typename SgmVec<V>::type& v, int i) { return (int)v[i]; }
template <> __device__ __forceinline__ int sgm_get<1>(const unsigned short& v, int) { return (int)v; }
template <int V> __device__ __forceinline__ void sgm_set(typename SgmVec<V>::type& v, int i, int x) { v[i] = (unsigned short)x; }
template <> __device__ __forceinline__ void sgm_set<1>(unsigned short& v, int, int x) { v = (unsigned short)x; }

// ---- census: one thread per pixel
__global__ __launch_bounds__(256) void k_census(const uint8_t* __restrict__ img, int width, int height, unsigned long long* __restrict__ out)
{
    const int64_t n = (int64_t)width * height;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(q / width), x = (int)(q - (int64_t)y * width);
        const unsigned int c = img[q];
        unsigned long long w = 0;
#pragma unroll
        for (int dy = -3; dy <= 3; ++dy) {
            const int yy = min(max(y + dy, 0), height - 1);
            const uint8_t* row = img + (int64_t)yy * width;
#pragma unroll
            for (int dx = -4; dx <= 4; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const int xx = min(max(x + dx, 0), width - 1);
                w = (w << 1) | (unsigned long long)(row[xx] < c ? 1u : 0u);
            }
        }
        out[q] = w;
    }
}

// ---- path aggregation
struct SgmPathArgs {
    const unsigned long long *cl, *cr;
    unsigned short* S;
    int width, height, D, p1, p2;
    int dy, dx;
    int n_paths, n_groups;              // paths of this direction; groups of as many as a wave walks
};

// start pixel and length of path `pid` of the direction: the axis directions start on one edge, a diagonal on two
__device__ __forceinline__ int sgm_path_start(const SgmPathArgs& a, int pid, int& x0, int& y0)
{
    if (pid >= a.n_paths) {
        x0 = y0 = 0;
        return 0;
    }
    const int W = a.width, H = a.height;
    if (a.dy == 0) {
        y0 = pid;
        x0 = a.dx > 0 ? 0 : W - 1;
        return W;
    }
    if (pid < W) {                      // starts on the top (dy > 0) or bottom row
        x0 = pid;
        y0 = a.dy > 0 ? 0 : H - 1;
    } else {                            // diagonals only: the side column, below (above) the corner
        const int j = pid - W + 1;
        x0 = a.dx > 0 ? 0 : W - 1;
        y0 = a.dy > 0 ? j : H - 1 - j;
    }
    const int ny = a.dy > 0 ? H - y0 : y0 + 1;
    if (a.dx == 0) return ny;
    const int nx = a.dx > 0 ? W - x0 : x0 + 1;
    return nx < ny ? nx : ny;
}

template <int V>
struct SgmStage {                       // what one step reads: the left word, the V right words of this lane's disparities, its S piece
    unsigned long long l, r[V];
    typename SgmVec<V>::type s;
};

// A path step's memory is read PNR_SGM_PREFETCH steps before the step that uses it: a path is a serial chain, and a wave that
// waited for its own loads in every step would spend the step on memory latency.  c: the pixel's index y W + x, x: its column,
// si: the index of this lane's piece of the pixel's S row (all kept by addition along the path, not recomputed).
template <int V, bool FIRST>
__device__ __forceinline__ void sgm_fetch(const SgmPathArgs& a, int64_t c, int x, int64_t si, int d0, bool on, SgmStage<V>& st)
{
    typedef typename SgmVec<V>::type vec_t;
    if (on) {
        st.l = a.cl[c];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int d = d0 + v;
            st.r[v] = a.cr[c - (d < x ? d : x)];            // (x - d < 0: the cost is 63 whatever is read, so column 0 is)
        }
        if (!FIRST) st.s = *(const vec_t*)(a.S + si);
    }
}

// G lanes walk a path, V disparities each (G V >= D); a wave walks 64 / G paths
template <int V, int G, bool FIRST>
__global__ __launch_bounds__(64) void k_sgm_path(const SgmPathArgs a)
{
    typedef typename SgmVec<V>::type vec_t;
    constexpr int PF = PNR_SGM_PREFETCH;
    constexpr int NP = 64 / G;
    const int lane = threadIdx.x & (G - 1), sub = threadIdx.x / G;
    const int d0 = lane * V;
    const bool lane_on = d0 < a.D;      // (V divides 16 and 16 divides D: a lane is inside [0, D) whole or not at all)
    const int64_t step_c = (int64_t)a.dy * a.width + a.dx, step_s = step_c * a.D;
    for (int g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        int x, y, len, maxlen = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k) {  // the longest of the wave's paths: the loop below is wave-uniform
            int tx, ty;
            const int l = sgm_path_start(a, g * NP + k, tx, ty);
            maxlen = l > maxlen ? l : maxlen;
        }
        len = sgm_path_start(a, g * NP + sub, x, y);
        int Lp[V];
#pragma unroll
        for (int v = 0; v < V; ++v) Lp[v] = PNR_SGM_ABSENT;
        int64_t fc = (int64_t)y * a.width + x, fs = fc * a.D + d0;      // the fetch cursor, PF steps ahead of ...
        int fx = x;
        int64_t ps = fs;                                                // ... the step's own
        SgmStage<V> ring[PF] = {};
#pragma unroll
        for (int i = 0; i < PF; ++i, fc += step_c, fs += step_s, fx += a.dx) sgm_fetch<V, FIRST>(a, fc, fx, fs, d0, lane_on && i < len, ring[i]);
        for (int t0 = 0; t0 < maxlen; t0 += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i, x += a.dx, ps += step_s, fc += step_c, fs += step_s, fx += a.dx) {     // (steps past maxlen touch no memory)
                const int t = t0 + i;
                const bool act = lane_on && t < len;        // (uniform over the path's G lanes but for lane_on)
                const SgmStage<V> cur = ring[i];
                // the stage is free: the step PF ahead goes into it.  That step's S cell is another pixel's than any store
                // between here and its use, so the early load reads what the earlier directions left there
                sgm_fetch<V, FIRST>(a, fc, fx, fs, d0, lane_on && t + PF < len, ring[i]);
                int m = Lp[0];
#pragma unroll
                for (int v = 1; v < V; ++v) m = Lp[v] < m ? Lp[v] : m;
                m = group_min<G>(m);
                const int before = group_prev<G>(Lp[V - 1], PNR_SGM_ABSENT), after = group_next<G>(Lp[0], PNR_SGM_ABSENT);
                const int jump = m + a.p2;
                vec_t s = cur.s;
                if (FIRST) {
                    const vec_t zero = {};
                    s = zero;
                }
                int L[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const int c = x - d0 - v >= 0 ? (int)__popcll(cur.l ^ cur.r[v]) : 63;
                    const int lo = v > 0 ? Lp[v - 1] : before, hi = v < V - 1 ? Lp[v + 1] : after;
                    int best = lo < hi ? lo : hi;
                    best += a.p1;
                    best = Lp[v] < best ? Lp[v] : best;
                    best = jump < best ? jump : best;
                    L[v] = t == 0 ? c : c + best - m;
                }
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    Lp[v] = lane_on ? L[v] : PNR_SGM_ABSENT;
                    sgm_set<V>(s, v, sgm_get<V>(s, v) + L[v]);
                }
                if (act) *(vec_t*)(a.S + ps) = s;
            }
        }
    }
}

// ---- selection
// dR(y, xr) = argmin_k S(y, xr + k, k), the lowest k on ties: 16 lanes per pixel of the right image, a lane gathers its V
// disparities down the volume's diagonal and the row butterfly takes the minimum of the (S, k) pairs
template <int V>
__global__ __launch_bounds__(256) void k_sgm_right(const unsigned short* __restrict__ S, int width, int height, int D, int16_t* __restrict__ disp_right)
{
    const int lane = threadIdx.x & 15, sub = threadIdx.x >> 4;
    const int d0 = lane * V;
    const int64_t n = (int64_t)width * height;
    for (int64_t base = (int64_t)blockIdx.x * 16; base < n; base += (int64_t)gridDim.x * 16) {      // (uniform over the block)
        const int64_t q = base + sub;
        const bool on = q < n;
        int key = 0x7FFFFFFF;
        if (on) {
            const int xr = (int)(q % width);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int k = d0 + v;
                if (k < D && xr + k < width) {
                    const int kk = ((int)S[(q + k) * D + k] << 8) | k;
                    key = kk < key ? kk : key;
                }
            }
        }
        key = row_min(key);
        if (on && lane == 0) disp_right[q] = (int16_t)(key & 255);
    }
}

struct SgmSelectArgs {
    const unsigned short* S;
    int width, height, D, uniqueness, lr_tol;
    const int16_t* disp_right;
    int16_t* d16;
};

// 16 lanes per pixel, the aggregation's layout: a lane reads its V disparities as one vector, the row butterfly does the rest
template <int V>
__global__ __launch_bounds__(256) void k_sgm_select(const SgmSelectArgs a)
{
    typedef typename SgmVec<V>::type vec_t;
    const int lane = threadIdx.x & 15, sub = threadIdx.x >> 4;
    const int d0 = lane * V;
    const bool lane_on = d0 < a.D;
    const int64_t n = (int64_t)a.width * a.height;
    const int BIG = 0xFFFF;             // above any S (at most 2040)
    for (int64_t base = (int64_t)blockIdx.x * 16; base < n; base += (int64_t)gridDim.x * 16) {      // (uniform over the block)
        const int64_t q = base + sub;
        const bool on = q < n;
        int s[V];
        if (on && lane_on) {
            const vec_t v = *(const vec_t*)(a.S + q * a.D + d0);
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] = sgm_get<V>(v, i);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] = BIG;
        }
        int key = (s[0] << 8) | d0;     // the minimum of (S, d) pairs: the lowest d among equal S
#pragma unroll
        for (int i = 1; i < V; ++i) {
            const int k = (s[i] << 8) | (d0 + i);
            key = k < key ? k : key;
        }
        key = row_min(key);
        const int best = key >> 8, ds = key & 255;
        int second = BIG, sm = BIG, sp = BIG;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int d = d0 + i;
            second = (d < ds - 1 || d > ds + 1) && s[i] < second ? s[i] : second;
            sm = d == ds - 1 ? s[i] : sm;
            sp = d == ds + 1 ? s[i] : sp;
        }
        second = row_min(second);
        sm = row_min(sm);
        sp = row_min(sp);
        if (on && lane == 0) {
            const int y = (int)(q / a.width), x = (int)(q - (int64_t)y * a.width);
            int out;
            if (x - ds < 0) out = -1;
            else if (second != BIG && second * (100 - a.uniqueness) < best * 100) out = -2;
            else if (a.lr_tol >= 0 && abs((int)a.disp_right[q - ds] - ds) > a.lr_tol) out = -3;
            else {
                int off = 0;
                if (ds > 0 && ds < a.D - 1) {
                    const int den = sm + sp - 2 * best;
                    if (den != 0) {     // (den > 0: best is the minimum)
                        const int num = 2 * 8 * (sm - sp) + den, den2 = 2 * den;
                        off = num >= 0 ? num / den2 : -((-num + den2 - 1) / den2);      // floor, toward -inf
                    }
                }
                out = 16 * ds + off;
            }
            a.d16[q] = (int16_t)out;
        }
    }
}

// ---- depth
__global__ __launch_bounds__(256) void k_disparity_depth(const int16_t* __restrict__ d16, int64_t n, float fb, float d_min, float d_max,
                                                         float* __restrict__ depth)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int d = d16[q];
        float z = 0.0f;
        if (d > 0) {
            const float disp = (float)d * 0.0625f;
            const float t = fb / disp;
            z = t >= d_min && t <= d_max ? t : 0.0f;
        }
        depth[q] = z;
    }
}

// ---- entry points
static bool sgm_size_ok(int width, int height) { return width >= 1 && height >= 1 && (int64_t)width * height <= INT32_MAX; }
static bool sgm_disp_ok(int D) { return D >= 16 && D <= 256 && D % 16 == 0; }
static int sgm_lane_values(int D, int G = 16)       // V: the power of two with G V >= D
{
    int v = 1;
    while (G * v < D) v *= 2;
    return v;
}

PNR_EXPORT int pnr_census(const uint8_t* img, int width, int height, int64_t* out, void* stream)
{
    PNR_REQUIRE(sgm_size_ok(width, height), "pnr_census: bad size (width, height >= 1, at most 2^31 - 1 pixels)");
    PNR_REQUIRE(img && out, "pnr_census: null img or out");
    const int grid = pnr_grid_cap(((int64_t)width * height + 255) / 256);
    hipLaunchKernelGGL(k_census, dim3(grid), dim3(256), 0, (hipStream_t)stream, img, width, height, (unsigned long long*)out);
    PNR_CHECK_LAUNCH("pnr_census");
    return PNR_OK;
}

PNR_EXPORT int64_t pnr_sgm_workspace_bytes(int width, int height, int max_disp, int paths)
{
    if (!sgm_size_ok(width, height) || !sgm_disp_ok(max_disp) || (paths != 4 && paths != 8)) {
        pnr_set_error("pnr_sgm_workspace_bytes: bad size, max_disp or paths (%d x %d, %d, %d)", width, height, max_disp, paths);
        return -1;
    }
    return 0;                           // the per-direction passes add into S itself: nothing is staged
}

template <int V, int G>
static void sgm_launch_path(const SgmPathArgs& a, bool first, int grid, hipStream_t stream)
{
    if (first) hipLaunchKernelGGL((k_sgm_path<V, G, true>), dim3(grid), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((k_sgm_path<V, G, false>), dim3(grid), dim3(64), 0, stream, a);
}

PNR_EXPORT int pnr_sgm_aggregate(const int64_t* census_l, const int64_t* census_r, int width, int height, int max_disp, int p1, int p2,
                                 int paths, uint16_t* S, void* workspace, void* stream)
{
    PNR_REQUIRE(sgm_size_ok(width, height), "pnr_sgm_aggregate: bad size (width, height >= 1, at most 2^31 - 1 pixels)");
    PNR_REQUIRE(sgm_disp_ok(max_disp), "pnr_sgm_aggregate: max_disp must be a multiple of 16 in 16 .. 256 (got %d)", max_disp);
    PNR_REQUIRE(p1 > 0 && p1 <= p2 && p2 <= 192, "pnr_sgm_aggregate: the penalties must satisfy 0 < p1 <= p2 <= 192 (got %d, %d)", p1, p2);
    PNR_REQUIRE(paths == 4 || paths == 8, "pnr_sgm_aggregate: paths must be 4 or 8 (got %d)", paths);
    PNR_REQUIRE(census_l && census_r && S, "pnr_sgm_aggregate: null census or S");
    PNR_REQUIRE(((uintptr_t)S & 31) == 0 && (((uintptr_t)census_l | (uintptr_t)census_r) & 7) == 0,
                "pnr_sgm_aggregate: S must be 32-byte aligned, the census images 8-byte aligned");
    (void)workspace;                    // pnr_sgm_workspace_bytes is 0: may be NULL
    static const int dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};       // (dy, dx), the rule's order
    SgmPathArgs a;
    a.cl = (const unsigned long long*)census_l; a.cr = (const unsigned long long*)census_r; a.S = S;
    a.width = width; a.height = height; a.D = max_disp; a.p1 = p1; a.p2 = p2;
    // a path is a serial chain and a wave issues one instruction at a time: above 48 disparities the whole wave walks ONE path
    // (1, 2 or 4 disparities a lane), which shortens the step; below, a row of 16 lanes does, four paths a wave
    const int G = max_disp > PNR_SGM_ROW_PATH_MAX ? 64 : 16;
    const int V = sgm_lane_values(max_disp, G), per_wave = 64 / G;
    for (int r = 0; r < paths; ++r) {
        a.dy = dirs[r][0]; a.dx = dirs[r][1];
        a.n_paths = a.dy == 0 ? height : a.dx == 0 ? width : width + height - 1;
        a.n_groups = (a.n_paths + per_wave - 1) / per_wave;
        const int grid = pnr_grid_cap(a.n_groups, PNR_SGM_PATH_WAVES_PER_CU);
        const hipStream_t st = (hipStream_t)stream;
        if (G == 64) {
            switch (V) {
            case 1: sgm_launch_path<1, 64>(a, r == 0, grid, st); break;
            case 2: sgm_launch_path<2, 64>(a, r == 0, grid, st); break;
            default: sgm_launch_path<4, 64>(a, r == 0, grid, st); break;
            }
        } else {
            switch (V) {
            case 1: sgm_launch_path<1, 16>(a, r == 0, grid, st); break;
            case 2: sgm_launch_path<2, 16>(a, r == 0, grid, st); break;
            default: sgm_launch_path<4, 16>(a, r == 0, grid, st); break;
            }
        }
    }
    PNR_CHECK_LAUNCH("pnr_sgm_aggregate");
    return PNR_OK;
}

PNR_EXPORT int pnr_sgm_select(const uint16_t* S, int width, int height, int max_disp, int uniqueness, int lr_tol, int16_t* d16,
                              int16_t* disp_right, void* stream)
{
    PNR_REQUIRE(sgm_size_ok(width, height), "pnr_sgm_select: bad size (width, height >= 1, at most 2^31 - 1 pixels)");
    PNR_REQUIRE(sgm_disp_ok(max_disp), "pnr_sgm_select: max_disp must be a multiple of 16 in 16 .. 256 (got %d)", max_disp);
    PNR_REQUIRE(uniqueness >= 0 && uniqueness <= 99, "pnr_sgm_select: uniqueness must lie in 0 .. 99 (got %d)", uniqueness);
    PNR_REQUIRE(lr_tol >= -1, "pnr_sgm_select: lr_tol must be >= 0, or -1 for no left-right check (got %d)", lr_tol);
    PNR_REQUIRE(S && d16, "pnr_sgm_select: null S or d16");
    PNR_REQUIRE(disp_right || lr_tol < 0, "pnr_sgm_select: disp_right may be NULL only when lr_tol < 0");
    PNR_REQUIRE(((uintptr_t)S & 31) == 0, "pnr_sgm_select: S must be 32-byte aligned");
    const int64_t n = (int64_t)width * height;
    const int grid = pnr_grid_cap((n + 15) / 16);
    const hipStream_t st = (hipStream_t)stream;
    if (disp_right) {
        switch (sgm_lane_values(max_disp)) {
        case 1: hipLaunchKernelGGL(k_sgm_right<1>, dim3(grid), dim3(256), 0, st, S, width, height, max_disp, disp_right); break;
        case 2: hipLaunchKernelGGL(k_sgm_right<2>, dim3(grid), dim3(256), 0, st, S, width, height, max_disp, disp_right); break;
        case 4: hipLaunchKernelGGL(k_sgm_right<4>, dim3(grid), dim3(256), 0, st, S, width, height, max_disp, disp_right); break;
        case 8: hipLaunchKernelGGL(k_sgm_right<8>, dim3(grid), dim3(256), 0, st, S, width, height, max_disp, disp_right); break;
        default: hipLaunchKernelGGL(k_sgm_right<16>, dim3(grid), dim3(256), 0, st, S, width, height, max_disp, disp_right); break;
        }
    }
    SgmSelectArgs a;
    a.S = S; a.width = width; a.height = height; a.D = max_disp; a.uniqueness = uniqueness; a.lr_tol = lr_tol;
    a.disp_right = disp_right; a.d16 = d16;
    switch (sgm_lane_values(max_disp)) {
    case 1: hipLaunchKernelGGL(k_sgm_select<1>, dim3(grid), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(k_sgm_select<2>, dim3(grid), dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_sgm_select<4>, dim3(grid), dim3(256), 0, st, a); break;
    case 8: hipLaunchKernelGGL(k_sgm_select<8>, dim3(grid), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(k_sgm_select<16>, dim3(grid), dim3(256), 0, st, a); break;
    }
    PNR_CHECK_LAUNCH("pnr_sgm_select");
    return PNR_OK;
}

PNR_EXPORT int pnr_disparity_depth(const int16_t* d16, int64_t n, float fb, float d_min, float d_max, float* depth, void* stream)
{
    PNR_REQUIRE(n >= 0, "pnr_disparity_depth: bad size");
    PNR_REQUIRE(pnr_pos_finite(fb), "pnr_disparity_depth: fb = fx * baseline must be positive and finite");
    PNR_REQUIRE(d_min > 0.0f && d_min <= d_max, "pnr_disparity_depth: the range must satisfy 0 < d_min <= d_max (d_max may be +inf)");
    if (n == 0) return PNR_OK;
    PNR_REQUIRE(d16 && depth, "pnr_disparity_depth: null d16 or depth");
    hipLaunchKernelGGL(k_disparity_depth, dim3(pnr_grid_cap((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d16, n, fb, d_min, d_max, depth);
    PNR_CHECK_LAUNCH("pnr_disparity_depth");
    return PNR_OK;
}
