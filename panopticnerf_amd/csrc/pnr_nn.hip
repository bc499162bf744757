// Nearest neighbours and geometry metrics (include/pnr.h "nearest neighbours"): an exact fixed-radius nearest-neighbour search
// between two clouds through a spatial hash, the reconstruction metrics accumulated from its answers, and surface points of a
// triangle mesh at a given density.  The search's answer is brute force's, bit for bit, whatever the table does: pnr_key
// (distance bits, index; pnr_geom_dev.h) under a minimum, so collisions and a bucket visited twice cost time and nothing else.
// Small gather-bound kernels: one thread per point, query or output point, grid-stride; the only
// LDS is the few words of the block-wide counters and sums (pnr_reduce_dev.h; the metric sums take the order of DESIGN.md
// section 8 "Ordered reductions").  tests/_nn_ref.py restates every rule in numpy.
#include <float.h>
#include <math.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"
#include "pnr_philox.h"

#define PNR_CM_MAX_BLOCKS 1024            // k_cloud_metrics' grid limit: what pnr_cloud_metrics_workspace_bytes sizes for
#define PNR_CM_COUNTS (2 + PNR_CLOUD_MAX_TAU)

struct NnGrid {
    const float* ref; int64_t n;          // ref[0] is the origin, read on the device (a captured build follows the data)
    float inv;                            // 1 / h, h = 2 Dp
    unsigned int mask;                    // T - 1
};

__device__ __forceinline__ void nn_origin(const NnGrid& g, float& ox, float& oy, float& oz)
{
    ox = oy = oz = 0.0f;
    if (g.n > 0) {
        const float x = g.ref[0], y = g.ref[1], z = g.ref[2];
        if (pnr_finite3(x, y, z)) { ox = x; oy = y; oz = z; }
    }
}

// the cell coordinate of p on one axis: clamped as a float, then converted
__device__ __forceinline__ int nn_cell(float p, float o, float inv)
{
    const float c = floorf((p - o) * inv);
    return (int)fminf(fmaxf(c, -PNR_NN_CELL_CLAMP), PNR_NN_CELL_CLAMP);
}

__device__ __forceinline__ unsigned int nn_bucket(int cx, int cy, int cz, unsigned int mask)
{
    return (((unsigned int)cx * PNR_NN_HASH_X) ^ ((unsigned int)cy * PNR_NN_HASH_Y) ^ ((unsigned int)cz * PNR_NN_HASH_Z)) & mask;
}

// FILL = false: count[bucket] += 1 per finite reference point.  FILL = true: the point's record goes to
// start[bucket] + (the value the bucket's cursor had) - 1, the cursor counting down from the bucket's count.
template <bool FILL>
__device__ __forceinline__ void nn_scatter(const NnGrid& g, int32_t* __restrict__ cursor, const int32_t* __restrict__ start,
                                           float4* __restrict__ records)
{
    float ox, oy, oz;
    nn_origin(g, ox, oy, oz);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < g.n; j += (int64_t)gridDim.x * blockDim.x) {
        const float x = g.ref[3 * j], y = g.ref[3 * j + 1], z = g.ref[3 * j + 2];
        if (!pnr_finite3(x, y, z)) continue;
        const unsigned int b = nn_bucket(nn_cell(x, ox, g.inv), nn_cell(y, oy, g.inv), nn_cell(z, oz, g.inv), g.mask);
        if (!FILL) {
            atomicAdd(&cursor[b], 1);
        } else {
            const int64_t at = (int64_t)start[b] + (int64_t)atomicSub(&cursor[b], 1) - 1;
            if (at >= 0 && at < g.n) records[at] = make_float4(x, y, z, __int_as_float((int)j));
        }
    }
}

__global__ __launch_bounds__(256) void k_nn_count(const NnGrid g, int32_t* __restrict__ cursor) { nn_scatter<false>(g, cursor, nullptr, nullptr); }

__global__ __launch_bounds__(256) void k_nn_fill(const NnGrid g, int32_t* __restrict__ cursor, const int32_t* __restrict__ start, float4* __restrict__ records)
{
    nn_scatter<true>(g, cursor, start, records);
}

struct NnQueryArgs {
    NnGrid g;
    float dp, r2;
    const int32_t* start;
    const float4* records;
    const float* q; int64_t m;
    int32_t* index; float* dist2;
    unsigned long long* stats;
};

__global__ __launch_bounds__(256) void k_nn_query(const NnQueryArgs a)
{
    __shared__ unsigned int h[4];
    unsigned int cnt[3] = {0, 0, 0};                    // found / none in radius / invalid
    float ox, oy, oz;
    nn_origin(a.g, ox, oy, oz);
    const int n32 = (int)a.g.n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += (int64_t)gridDim.x * blockDim.x) {
        const float qx = a.q[3 * i], qy = a.q[3 * i + 1], qz = a.q[3 * i + 2];
        unsigned long long best = PNR_KEY_EMPTY;
        int slot = 2;
        if (pnr_finite3(qx, qy, qz)) {
            const int x0 = nn_cell(qx - a.dp, ox, a.g.inv), x1 = nn_cell(qx + a.dp, ox, a.g.inv);
            const int y0 = nn_cell(qy - a.dp, oy, a.g.inv), y1 = nn_cell(qy + a.dp, oy, a.g.inv);
            const int z0 = nn_cell(qz - a.dp, oz, a.g.inv), z1 = nn_cell(qz + a.dp, oz, a.g.inv);
            for (int cz = z0; cz <= z1; ++cz)
                for (int cy = y0; cy <= y1; ++cy)
                    for (int cx = x0; cx <= x1; ++cx) {
                        const unsigned int b = nn_bucket(cx, cy, cz, a.g.mask);
                        const PnrRange rg = pnr_table_range(a.start, b, n32);
                        for (int r = rg.s; r < rg.e; ++r) {
                            const float4 p = a.records[r];
                            const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
                            const float d2 = (dx * dx + dy * dy) + dz * dz;
                            if (d2 <= a.r2) {
                                const unsigned long long key = pnr_key(d2, __float_as_uint(p.w));
                                best = key < best ? key : best;
                            }
                        }
                    }
            slot = best == PNR_KEY_EMPTY ? 1 : 0;
        }
        a.index[i] = best == PNR_KEY_EMPTY ? -1 : (int32_t)pnr_key_index(best);
        a.dist2[i] = best == PNR_KEY_EMPTY ? INFINITY : pnr_key_value(best);
#pragma unroll
        for (int k = 0; k < 3; ++k) cnt[k] += slot == k ? 1u : 0u;
    }
    if (a.stats) pnr_block_count_add(cnt, h, a.stats);  // (uniform over the block)
}

struct CloudMetricArgs {
    const int32_t* index;
    const float* dist2;
    const float* query;                 // (m, 3) or NULL: a query with a non-finite coordinate does not count
    int64_t m;
    double dmax;
    float tau2[PNR_CLOUD_MAX_TAU];
    int n_tau;
    double* partial;                    // [blocks][2]
    double* sums;
    unsigned long long* counts;
    int n_blocks;
};

__global__ __launch_bounds__(PNR_REDUCE_BLOCK) void k_cloud_metrics(const CloudMetricArgs a)
{
    __shared__ double red[4][2];
    __shared__ unsigned int hc[PNR_CM_COUNTS];
    double s[2] = {0.0, 0.0};
    unsigned int cnt[PNR_CM_COUNTS];
#pragma unroll
    for (int k = 0; k < PNR_CM_COUNTS; ++k) cnt[k] = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += (int64_t)gridDim.x * blockDim.x) {
        const float d2 = a.dist2[i];
        if (d2 != d2) continue;
        if (a.query && !pnr_finite3(a.query[3 * i], a.query[3 * i + 1], a.query[3 * i + 2])) continue;
        const bool found = a.index[i] >= 0;
        const double d = found ? sqrt((double)d2) : a.dmax;
        cnt[0] += 1u;
        cnt[1] += found ? 0u : 1u;
#pragma unroll
        for (int k = 0; k < PNR_CLOUD_MAX_TAU; ++k) cnt[2 + k] += (k < a.n_tau && found && d2 <= a.tau2[k]) ? 1u : 0u;
        s[0] += d;
        s[1] += d * d;
    }
    pnr_block_sum_rows(s, red, a.partial, 2);
    pnr_block_count_add(cnt, hc, a.counts);
}

// one block: term t adds the partials of blocks 0, 1, ... in that order, then once into sums[t] (no floating atomics anywhere)
__global__ __launch_bounds__(64) void k_cloud_metrics_final(const CloudMetricArgs a)
{
    if (threadIdx.x >= 2) return;
    const double v = pnr_rows_total<2>((const unsigned long long*)a.partial, a.n_blocks, threadIdx.x).sum;
    a.sums[threadIdx.x] = a.sums[threadIdx.x] + v;
}

struct SampleArgs {
    PnrMesh m;
    float rho;
    uint32_t seed_lo, seed_hi;
    int32_t* start;                     // count: the counts, in place of their scan; emit: the scan
    int64_t n_points;
    float* points; int32_t* face;
};

struct SampleTri { float p0[3], e1[3], e2[3]; bool ok; };

__device__ __forceinline__ SampleTri sample_tri(const PnrMesh& m, int64_t t)
{
    SampleTri r;
    const int32_t i0 = m.faces[3 * t], i1 = m.faces[3 * t + 1], i2 = m.faces[3 * t + 2];
    r.ok = i0 >= 0 && i0 < m.n_vertices && i1 >= 0 && i1 < m.n_vertices && i2 >= 0 && i2 < m.n_vertices;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.p0[c] = r.ok ? m.vertices[3 * (int64_t)i0 + c] : 0.0f;
        r.e1[c] = r.ok ? m.vertices[3 * (int64_t)i1 + c] - r.p0[c] : 0.0f;
        r.e2[c] = r.ok ? m.vertices[3 * (int64_t)i2 + c] - r.p0[c] : 0.0f;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_mesh_sample_count(const SampleArgs a)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.m.n_faces; t += (int64_t)gridDim.x * blockDim.x) {
        const SampleTri r = sample_tri(a.m, t);
        float n[3];
        pnr_cross3(r.e1, r.e2, n);
        const float s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        int k = 0;
        if (r.ok && s <= FLT_MAX) {                     // (a NaN or infinite s: the area is not finite)
            const float area = 0.5f * sqrtf(s);
            const float u = pnr_uniform(pnr_philox4x32_10(pnr_u4{(uint32_t)t, 0u, 0u, 0u}, a.seed_lo, a.seed_hi).x);
            const float x = floorf(area * a.rho + u);
            k = x >= (float)PNR_SAMPLE_MAX_PER_FACE ? PNR_SAMPLE_MAX_PER_FACE : (int)x;   // (x >= 0: compared as a float, no conversion of +inf)
        }
        a.start[t] = k;
    }
}

__global__ __launch_bounds__(256) void k_mesh_sample_emit(const SampleArgs a)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_points; i += (int64_t)gridDim.x * blockDim.x) {
        // the triangle t with start[t] <= i < start[t + 1]: the last t whose start is <= i
        int64_t lo = 0, hi = a.m.n_faces - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if ((int64_t)a.start[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const int64_t t = lo;
        const uint32_t j = (uint32_t)(i - (int64_t)a.start[t]);
        const SampleTri r = sample_tri(a.m, t);
        const pnr_u4 w = pnr_philox4x32_10(pnr_u4{(uint32_t)t, 1u + j, 0u, 0u}, a.seed_lo, a.seed_hi);
        float u = pnr_uniform(w.x), v = pnr_uniform(w.y);
        if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
#pragma unroll
        for (int c = 0; c < 3; ++c) a.points[3 * i + c] = (r.p0[c] + u * r.e1[c]) + v * r.e2[c];
        a.face[i] = (int32_t)t;
    }
}

// ---- entry points

// the cell size h = 2 Dp and its inverse are both finite: a denormal max_dist whose 1 / h is +inf would send the two corners of
// a query's box to the two clamp cells, 2^21 cells per axis
static bool nn_cell_ok(float d) { return pnr_pos_finite(d * PNR_NN_PAD * 2.0f) && pnr_pos_finite(1.0f / (d * PNR_NN_PAD * 2.0f)); }
static bool nn_table_ok(int64_t T) { return T >= 2 && T <= PNR_NN_MAX_TABLE && (T & (T - 1)) == 0; }

static NnGrid nn_grid(const float* ref, int64_t n, float max_dist, int64_t T, float* dp_out)
{
    const float dp = max_dist * PNR_NN_PAD, h = 2.0f * dp;
    NnGrid g;
    g.ref = ref; g.n = n; g.inv = 1.0f / h; g.mask = (unsigned int)(T - 1);
    if (dp_out) *dp_out = dp;
    return g;
}

PNR_EXPORT int64_t pnr_nn_workspace_bytes(int64_t n, int64_t table_size)
{
    if (n < 0 || n > (int64_t)INT32_MAX || !nn_table_ok(table_size)) return -1;
    return pnr_table_carve(8, table_size, true).bytes;      // the scan's total, its tile sums, the cursors
}

PNR_EXPORT int pnr_nn_build(const float* ref, int64_t n, float max_dist, int64_t table_size, int32_t* start, float* records,
                            void* workspace, void* stream)
{
    PNR_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "pnr_nn_build: n must be within 0 .. 2^31 - 1");
    PNR_REQUIRE(pnr_pos_finite(max_dist), "pnr_nn_build: max_dist must be positive and finite (got %g)", (double)max_dist);
    PNR_REQUIRE(nn_table_ok(table_size), "pnr_nn_build: table_size must be a power of two in 2 .. 2^28 (got %lld)", (long long)table_size);
    PNR_REQUIRE(pnr_pos_finite(max_dist * PNR_NN_PAD * 2.0f), "pnr_nn_build: max_dist is too large: the cell size 2 max_dist overflows");
    PNR_REQUIRE(nn_cell_ok(max_dist), "pnr_nn_build: max_dist is too small: 1 / (2 max_dist) overflows (got %g)", (double)max_dist);
    PNR_REQUIRE(((uintptr_t)start & 3) == 0, "pnr_nn_build: start must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                               // an empty cloud: an all-zero table (a null start: nothing to fill)
        if (start) {
            pnr_zero_i32(start, table_size + 1, st);
            PNR_CHECK_LAUNCH("pnr_nn_build");
        }
        return PNR_OK;
    }
    PNR_REQUIRE(start, "pnr_nn_build: null start");
    PNR_REQUIRE(ref && records && workspace, "pnr_nn_build: null ref, records or workspace");
    PNR_REQUIRE(((uintptr_t)ref & 3) == 0, "pnr_nn_build: ref must be 4-byte aligned");
    PNR_REQUIRE(((uintptr_t)records & 15) == 0, "pnr_nn_build: records must be 16-byte aligned");
    PNR_REQUIRE(((uintptr_t)workspace & 7) == 0, "pnr_nn_build: workspace must be 8-byte aligned");
    const NnGrid g = nn_grid(ref, n, max_dist, table_size, nullptr);
    const PnrTableWs w = pnr_table_carve(8, table_size, true);
    int32_t* cursor = (int32_t*)((char*)workspace + w.cursor);
    const int grid = pnr_grid_cap((n + 255) / 256);
    pnr_zero_i32(cursor, table_size, st);
    hipLaunchKernelGGL(k_nn_count, dim3(grid), dim3(256), 0, st, g, cursor);
    pnr_scan_i32(cursor, start, table_size, (char*)workspace + w.sums, (int64_t*)workspace, st);
    hipLaunchKernelGGL(k_nn_fill, dim3(grid), dim3(256), 0, st, g, cursor, (const int32_t*)start, (float4*)records);
    PNR_CHECK_LAUNCH("pnr_nn_build");
    return PNR_OK;
}

PNR_EXPORT int pnr_nn_query(const float* ref, int64_t n, float max_dist, int64_t table_size, const int32_t* start, const float* records,
                            const float* query, int64_t m, int32_t* index, float* dist2, int64_t* stats, void* stream)
{
    PNR_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "pnr_nn_query: n must be within 0 .. 2^31 - 1");
    PNR_REQUIRE(m >= 0 && m <= (int64_t)INT32_MAX, "pnr_nn_query: m must be within 0 .. 2^31 - 1");
    PNR_REQUIRE(pnr_pos_finite(max_dist), "pnr_nn_query: max_dist must be positive and finite (got %g)", (double)max_dist);
    PNR_REQUIRE(nn_table_ok(table_size), "pnr_nn_query: table_size must be a power of two in 2 .. 2^28 (got %lld)", (long long)table_size);
    PNR_REQUIRE(pnr_pos_finite(max_dist * PNR_NN_PAD * 2.0f), "pnr_nn_query: max_dist is too large: the cell size 2 max_dist overflows");
    PNR_REQUIRE(nn_cell_ok(max_dist), "pnr_nn_query: max_dist is too small: 1 / (2 max_dist) overflows (got %g)", (double)max_dist);
    if (m == 0) return PNR_OK;
    PNR_REQUIRE(start && query && index && dist2, "pnr_nn_query: null start, query, index or dist2");
    PNR_REQUIRE(n == 0 || (ref && records), "pnr_nn_query: null ref or records");
    PNR_REQUIRE((((uintptr_t)ref | (uintptr_t)start | (uintptr_t)query | (uintptr_t)index | (uintptr_t)dist2) & 3) == 0,
                "pnr_nn_query: ref, start, query, index and dist2 must be 4-byte aligned");
    PNR_REQUIRE(((uintptr_t)records & 15) == 0, "pnr_nn_query: records must be 16-byte aligned");
    PNR_REQUIRE(((uintptr_t)stats & 7) == 0, "pnr_nn_query: stats must be 8-byte aligned");
    NnQueryArgs a;
    a.g = nn_grid(ref, n, max_dist, table_size, &a.dp);
    a.r2 = max_dist * max_dist;
    a.start = start; a.records = (const float4*)records; a.q = query; a.m = m;
    a.index = index; a.dist2 = dist2; a.stats = (unsigned long long*)stats;
    const int grid = pnr_grid_cap((m + 255) / 256);
    hipLaunchKernelGGL(k_nn_query, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_nn_query");
    return PNR_OK;
}

PNR_EXPORT int64_t pnr_cloud_metrics_workspace_bytes(int64_t m)
{
    if (m < 0 || m > (int64_t)INT32_MAX) return -1;
    return pnr_reduce_blocks(m, PNR_CM_MAX_BLOCKS) * 2 * (int64_t)sizeof(double);
}

PNR_EXPORT int pnr_cloud_metrics(const int32_t* index, const float* dist2, const float* query, int64_t m, float max_dist,
                                 const float* tau_host, int n_tau, double* sums, int64_t* counts, void* workspace, void* stream)
{
    PNR_REQUIRE(m >= 0 && m <= (int64_t)INT32_MAX, "pnr_cloud_metrics: m must be within 0 .. 2^31 - 1");
    PNR_REQUIRE(pnr_pos_finite(max_dist), "pnr_cloud_metrics: max_dist must be positive and finite (got %g)", (double)max_dist);
    PNR_REQUIRE(n_tau >= 0 && n_tau <= PNR_CLOUD_MAX_TAU, "pnr_cloud_metrics: n_tau must be within 0 .. %d thresholds (got %d)", PNR_CLOUD_MAX_TAU, n_tau);
    PNR_REQUIRE(n_tau == 0 || tau_host, "pnr_cloud_metrics: null tau_host");
    CloudMetricArgs a;
    for (int k = 0; k < PNR_CLOUD_MAX_TAU; ++k) {
        const float t = k < n_tau ? tau_host[k] : 0.0f;
        PNR_REQUIRE(k >= n_tau || (t > 0.0f && t <= max_dist), "pnr_cloud_metrics: tau[%d] = %g must satisfy 0 < tau <= max_dist = %g", k, (double)t,
                    (double)max_dist);
        a.tau2[k] = t * t;
    }
    if (m == 0) return PNR_OK;
    PNR_REQUIRE(index && dist2 && sums && counts && workspace, "pnr_cloud_metrics: null index, dist2, sums, counts or workspace");
    PNR_REQUIRE((((uintptr_t)index | (uintptr_t)dist2 | (uintptr_t)query) & 3) == 0, "pnr_cloud_metrics: index, dist2 and query must be 4-byte aligned");
    PNR_REQUIRE((((uintptr_t)sums | (uintptr_t)counts | (uintptr_t)workspace) & 7) == 0, "pnr_cloud_metrics: sums, counts and workspace must be 8-byte aligned");
    a.index = index; a.dist2 = dist2; a.query = query; a.m = m; a.dmax = (double)max_dist; a.n_tau = n_tau;
    a.partial = (double*)workspace; a.sums = sums; a.counts = (unsigned long long*)counts;
    a.n_blocks = pnr_grid_cap(pnr_reduce_blocks(m, PNR_CM_MAX_BLOCKS), 4);       // (never above that: the workspace holds it)
    hipLaunchKernelGGL(k_cloud_metrics, dim3(a.n_blocks), dim3(PNR_REDUCE_BLOCK), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(k_cloud_metrics_final, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_cloud_metrics");
    return PNR_OK;
}

#define SAMPLE_MAX_FACES ((int64_t)INT32_MAX - 1)             // the scan writes n_faces + 1 int32 entries
PNR_EXPORT int64_t pnr_mesh_sample_workspace_bytes(int64_t n_faces)
{
    if (n_faces < 0 || n_faces > SAMPLE_MAX_FACES) return -1;
    return pnr_table_carve(0, n_faces, false).bytes;
}

PNR_EXPORT int pnr_mesh_sample_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, float rho, int64_t seed,
                                     int32_t* start, int64_t* total, void* workspace, void* stream)
{
    SampleArgs a;
    const int rc = pnr_mesh_check("pnr_mesh_sample_count", vertices, n_vertices, faces, n_faces, SAMPLE_MAX_FACES, a.m);
    if (rc) return rc;
    PNR_REQUIRE(rho >= 0.0f && rho <= FLT_MAX, "pnr_mesh_sample_count: rho must be finite and >= 0 (got %g)", (double)rho);
    PNR_REQUIRE(((uintptr_t)start & 3) == 0 && ((uintptr_t)total & 7) == 0, "pnr_mesh_sample_count: start must be 4-byte and total 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n_faces == 0) {                         // no faces: start[0] = 0 and total = 0 (a null one: nothing to fill)
        if (start) pnr_zero_i32(start, 1, st);
        if (total) pnr_zero_i32((int32_t*)total, 2, st);
        if (start || total) PNR_CHECK_LAUNCH("pnr_mesh_sample_count");
        return PNR_OK;
    }
    PNR_REQUIRE(start && total, "pnr_mesh_sample_count: null start or total");
    PNR_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0, "pnr_mesh_sample_count: workspace must be non-null and 4-byte aligned");
    a.rho = rho;
    a.seed_lo = (uint32_t)(uint64_t)seed; a.seed_hi = (uint32_t)((uint64_t)seed >> 32);
    a.start = start; a.n_points = 0; a.points = nullptr; a.face = nullptr;
    hipLaunchKernelGGL(k_mesh_sample_count, dim3(pnr_grid_cap((n_faces + 255) / 256)), dim3(256), 0, st, a);
    pnr_scan_i32(start, start, n_faces, workspace, total, st);
    PNR_CHECK_LAUNCH("pnr_mesh_sample_count");
    return PNR_OK;
}

PNR_EXPORT int pnr_mesh_sample_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t seed,
                                    const int32_t* start, int64_t n_points, float* points, int32_t* face, void* stream)
{
    SampleArgs a;
    const int rc = pnr_mesh_check("pnr_mesh_sample_emit", vertices, n_vertices, faces, n_faces, SAMPLE_MAX_FACES, a.m);
    if (rc) return rc;
    PNR_REQUIRE(n_points >= 0 && n_points <= (int64_t)INT32_MAX, "pnr_mesh_sample_emit: n_points must be within 0 .. 2^31 - 1");
    if (n_points == 0) return PNR_OK;
    PNR_REQUIRE(n_faces >= 1, "pnr_mesh_sample_emit: n_points > 0 on a mesh without faces");
    PNR_REQUIRE(start && points && face, "pnr_mesh_sample_emit: null start, points or face");
    PNR_REQUIRE((((uintptr_t)start | (uintptr_t)points | (uintptr_t)face) & 3) == 0, "pnr_mesh_sample_emit: start, points and face must be 4-byte aligned");
    a.rho = 0.0f;
    a.seed_lo = (uint32_t)(uint64_t)seed; a.seed_hi = (uint32_t)((uint64_t)seed >> 32);
    a.start = (int32_t*)start; a.n_points = n_points; a.points = points; a.face = face;
    hipLaunchKernelGGL(k_mesh_sample_emit, dim3(pnr_grid_cap((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_mesh_sample_emit");
    return PNR_OK;
}
