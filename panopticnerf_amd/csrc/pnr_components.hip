// Connected components (include/pnr.h "connected components"): the components of an image, a lattice or a mesh by lock-free
// union-find on a parent array P with P[i] <= i, the labels numbered by the lowest member.  Integer atomics at agent scope are
// the only communication between workgroups (the XCDs have separate L2s: every read and write of P while it is being linked is
// an agent-scope operation); no kernel waits on another workgroup or wave, and every pointer chase steps only to a strictly
// smaller non-negative index, so each kernel terminates on any memory content.  The root of a finished component is its lowest
// index whatever the interleaving: the result does not depend on the schedule.  tests/_cc_ref.py restates the rule in numpy.
// Two forms of the lattice's link step, chosen at build time.  TILED (the default): a workgroup labels a tile of PNR_CC_TILE_*
// elements in LDS first, with the same union-find on tile-local indices and LDS atomics, writes P[i] = the global index of the
// tile-local root (the tile's lowest member: the local order is the flat order, so P[i] <= i holds), and the link kernel then
// unites only across tile borders.  FLAT (-DPNR_CC_FLAT): P[i] = i and every link goes to global memory; the baseline the tiled
// form is measured against (profiles/README.md).  Both give the same bits.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"

#define CC_MAX_ELEMENTS ((int64_t)INT32_MAX - 1)               // the scan writes n + 1 int32 entries

#define CC_GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// SCOPE: agent for the parent array in global memory, workgroup for a tile's in LDS
#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT
#define CC_WG __HIP_MEMORY_SCOPE_WORKGROUP
template <int SCOPE = CC_AGENT> __device__ __forceinline__ int32_t cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE = CC_AGENT> __device__ __forceinline__ int32_t cc_min(int32_t* p, int32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE); }
__device__ __forceinline__ void cc_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, CC_AGENT); }

// the root of a: steps only to a strictly smaller non-negative parent, so at most a steps on any content.  A stale parent is an
// older ancestor, still a member of the set.
template <int SCOPE = CC_AGENT>
__device__ __forceinline__ int32_t cc_find(const int32_t* P, int32_t a)
{
    for (;;) {
        const int32_t p = cc_load<SCOPE>(P + a);
        if (!(p < a && p >= 0)) return a;
        a = p;
    }
}

// join the sets of a and b: the larger root takes the smaller as its parent under a minimum; where another thread was first, the
// value that minimum returns is a smaller member of the same set and the round repeats from it.  The larger root strictly
// decreases each round.
template <int SCOPE = CC_AGENT>
__device__ __forceinline__ void cc_unite(int32_t* P, int32_t a, int32_t b)
{
    a = cc_find<SCOPE>(P, a);
    b = cc_find<SCOPE>(P, b);
    while (a != b) {
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = cc_min<SCOPE>(P + a, b);
        if (!(old < a && old >= 0)) break;              // old == a: a was a root and is linked now
        a = cc_find<SCOPE>(P, old);
        b = cc_find<SCOPE>(P, b);
    }
}

// counter[r] += 1 for the root r of every thread of the block (r < 0: none), with one atomic per distinct root and wave, and
// one per block for the root of thread 0: the elements of one large component would otherwise queue on a single address
// (cdna_hip_programming.md Guideline 12).  Called by every thread of a block of 256, in uniform control flow.  The loop clears
// at least one lane a round and waits for nobody.
__device__ __forceinline__ void cc_block_count(int32_t* counter, int32_t r)
{
    __shared__ int32_t s_lead, s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_lead = r;
    __syncthreads();
    const int32_t lead = s_lead;
    const bool mine = r >= 0 && r == lead;
    const unsigned long long b = __ballot(mine);
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0 && lead >= 0) atomicAdd(counter + lead, (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]));
    bool pending = r >= 0 && !mine;
    for (;;) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;                               // (uniform over the wave)
        const int first = __ffsll((long long)todo) - 1;
        const int32_t v = __shfl(r, first);
        const unsigned long long same = __ballot(pending && r == v);
        if (lane == first) atomicAdd(counter + v, __popcll(same));
        pending = pending && r != v;
    }
}

#define CC_BLOCK_STRIDE(base, n) for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < (n); base += (int64_t)gridDim.x * blockDim.x)

// ---- lattices

struct CcLattice {
    const void* data; int mode; float tol;
    int rx, ry, rz; int64_t n;
    int32_t* P;                     // the labels buffer
    int32_t* rank;                  // (n + 1): the root flags, then their scan
    int32_t* counter;               // (n): elements per root; NULL where size is not wanted
    int32_t* size;
};

template <int MODE> struct CcElem;
template <> struct CcElem<PNR_CC_KEYS> {
    typedef int32_t T;
    static __device__ __forceinline__ bool fg(int32_t k) { return k >= 0; }
    static __device__ __forceinline__ bool linked(int32_t a, int32_t b, float) { return a == b; }
};
template <> struct CcElem<PNR_CC_VALUES> {
    typedef float T;
    static __device__ __forceinline__ bool fg(float v) { return pnr_pos_finite(v); }
    static __device__ __forceinline__ bool linked(float a, float b, float tol) { return fabsf(a - b) <= tol; }
};

template <int MODE>
__global__ __launch_bounds__(256) void k_cc_init(const CcLattice a)
{
    const typename CcElem<MODE>::T* d = (const typename CcElem<MODE>::T*)a.data;
    CC_GRID_STRIDE(i, a.n) {
        a.P[i] = CcElem<MODE>::fg(d[i]) ? (int32_t)i : -1;
        if (a.counter) a.counter[i] = 0;
    }
}

// is (dz, dy, dx) a backward neighbour (a smaller flat index) of the neighbourhood: 3 or 13 in a volume, 2 or 4 in an image
template <int FULL>
__device__ __forceinline__ bool cc_backward(int dz, int dy, int dx)
{
    return (dz < 0 || dy < 0 || (dy == 0 && dx < 0)) && (FULL || (dz != 0) + (dy != 0) + (dx != 0) == 1);
}

// One tile of TX x TY x TZ elements a workgroup, one thread each, tiles taken block-stride: the tile's own union-find in LDS on
// the local index l = (lz TY + ly) TX + lx, whose order is the flat order; then P[i] = the global index of the local root.
template <int MODE, int FULL, int TX, int TY, int TZ>
__global__ __launch_bounds__(256) void k_cc_tile(const CcLattice a)
{
    static_assert(TX * TY * TZ == 256, "one thread per element of the tile");
    typedef CcElem<MODE> E;
    __shared__ int32_t lp[256];
    __shared__ typename E::T val[256];
    const typename E::T* d = (const typename E::T*)a.data;
    const int ntx = (a.rx + TX - 1) / TX, nty = (a.ry + TY - 1) / TY, ntz = (a.rz + TZ - 1) / TZ;
    const int64_t tiles = (int64_t)ntx * nty * ntz;
    const int l = threadIdx.x, lx = l % TX, ly = (l / TX) % TY, lz = l / (TX * TY);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {               // (uniform over the workgroup)
        const int x0 = (int)(t % ntx) * TX, y0 = (int)((t / ntx) % nty) * TY, z0 = (int)(t / ((int64_t)ntx * nty)) * TZ;
        const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
        const bool in = gx < a.rx && gy < a.ry && gz < a.rz;
        const int64_t i = ((int64_t)gz * a.ry + gy) * a.rx + gx;
        typename E::T v = typename E::T();
        if (in) v = d[i];
        const bool fg = in && E::fg(v);
        val[l] = v;
        lp[l] = fg ? l : -1;
        __syncthreads();
        if (fg) {
#pragma unroll
            for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!cc_backward<FULL>(dz, dy, dx)) continue;
                        const int jx = lx + dx, jy = ly + dy, jz = lz + dz;
                        if (jx < 0 || jx >= TX || jy < 0 || jy >= TY || jz < 0) continue;
                        const int j = (jz * TY + jy) * TX + jx;
                        if (lp[j] >= 0 && E::linked(v, val[j], a.tol)) cc_unite<CC_WG>(lp, l, j);      // lp[j] >= 0: foreground, never undone
                    }
        }
        __syncthreads();
        if (in) {
            int32_t root = -1;
            if (fg) {
                const int r = cc_find<CC_WG>(lp, l);
                root = (int32_t)((((int64_t)(z0 + r / (TX * TY))) * a.ry + (y0 + (r / TX) % TY)) * a.rx + (x0 + r % TX));
            }
            a.P[i] = root;
            if (a.counter) a.counter[i] = 0;
        }
        __syncthreads();                                                    // lp and val are the next tile's
    }
}

// every foreground element unites with its backward neighbours that pass the mode's test; with TX > 0 only with those in
// another tile (k_cc_tile has joined the rest)
template <int MODE, int FULL, int TX, int TY, int TZ>
__global__ __launch_bounds__(256) void k_cc_link(const CcLattice a)
{
    typedef CcElem<MODE> E;
    const typename E::T* d = (const typename E::T*)a.data;
    CC_GRID_STRIDE(i, a.n) {
        const typename E::T v = d[i];
        if (!E::fg(v)) continue;
        const int ix = (int)(i % a.rx), iy = (int)((i / a.rx) % a.ry), iz = (int)(i / ((int64_t)a.rx * a.ry));
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_backward<FULL>(dz, dy, dx)) continue;
                    const int jx = ix + dx, jy = iy + dy, jz = iz + dz;
                    if (jx < 0 || jx >= a.rx || jy < 0 || jy >= a.ry || jz < 0) continue;
                    if (TX > 0 && jx / (TX > 0 ? TX : 1) == ix / (TX > 0 ? TX : 1) && jy / (TY > 0 ? TY : 1) == iy / (TY > 0 ? TY : 1) &&
                        jz / (TZ > 0 ? TZ : 1) == iz / (TZ > 0 ? TZ : 1))
                        continue;
                    const int64_t j = ((int64_t)jz * a.ry + jy) * a.rx + jx;
                    const typename E::T w = d[j];
                    if (E::fg(w) && E::linked(v, w, a.tol)) cc_unite(a.P, (int32_t)i, (int32_t)j);
                }
    }
}

// P[i] = its root, rank[i] = whether i is one, counter[root] += 1.  The links are over: a root found here is final.
__global__ __launch_bounds__(256) void k_cc_flatten(const CcLattice a)
{
    CC_BLOCK_STRIDE(base, a.n) {                        // (uniform over the block: cc_block_count has barriers)
        const int64_t i = base + threadIdx.x;
        int32_t r = -1;
        if (i < a.n) {
            if (cc_load(a.P + i) >= 0) {
                r = cc_find(a.P, (int32_t)i);
                cc_store(a.P + i, r);
            }
            a.rank[i] = r == (int32_t)i ? 1 : 0;
        }
        if (a.counter) cc_block_count(a.counter, r);
    }
}

__global__ __launch_bounds__(256) void k_cc_relabel(const CcLattice a)
{
    CC_GRID_STRIDE(i, a.n) {
        const int32_t r = a.P[i];
        const bool fg = r >= 0 && r <= (int32_t)i;
        a.P[i] = fg ? a.rank[r] : -1;
        if (a.size) a.size[i] = fg ? a.counter[r] : 0;
    }
}

// ---- meshes: the elements are the vertices, a face links its three

struct CcMesh {
    const int32_t* faces; int64_t n_faces, n_vertices;
    int32_t* P;                     // vertex_label
    int32_t* rank;                  // (V + 1)
    int32_t* counter;               // (V): valid faces per root
    int32_t* face_label; int32_t* face_size;
};

__device__ __forceinline__ bool cc_face(const CcMesh& a, int64_t f, int32_t& v0, int32_t& v1, int32_t& v2)
{
    v0 = a.faces[3 * f]; v1 = a.faces[3 * f + 1]; v2 = a.faces[3 * f + 2];
    return v0 >= 0 && v0 < a.n_vertices && v1 >= 0 && v1 < a.n_vertices && v2 >= 0 && v2 < a.n_vertices;
}

__global__ __launch_bounds__(256) void k_cc_mesh_init(const CcMesh a)
{
    CC_GRID_STRIDE(i, a.n_vertices) { a.P[i] = (int32_t)i; a.counter[i] = 0; }
}

__global__ __launch_bounds__(256) void k_cc_mesh_link(const CcMesh a)
{
    CC_GRID_STRIDE(f, a.n_faces) {
        int32_t v0, v1, v2;
        if (!cc_face(a, f, v0, v1, v2)) continue;
        cc_unite(a.P, v0, v1);
        cc_unite(a.P, v1, v2);
    }
}

__global__ __launch_bounds__(256) void k_cc_mesh_flatten(const CcMesh a)
{
    CC_GRID_STRIDE(i, a.n_vertices) cc_store(a.P + i, cc_find(a.P, (int32_t)i));
}

// the vertices are flat: a valid face adds itself to its root's counter
__global__ __launch_bounds__(256) void k_cc_mesh_count(const CcMesh a)
{
    CC_BLOCK_STRIDE(base, a.n_faces) {
        const int64_t f = base + threadIdx.x;
        int32_t v0, v1, v2, r = -1;
        if (f < a.n_faces && cc_face(a, f, v0, v1, v2)) r = a.P[v0];
        cc_block_count(a.counter, r >= 0 && r <= v0 ? r : -1);
    }
}

// a root counts iff a valid face uses its component: a vertex no valid face uses is a root alone with a counter of 0
__global__ __launch_bounds__(256) void k_cc_mesh_flag(const CcMesh a)
{
    CC_GRID_STRIDE(i, a.n_vertices) a.rank[i] = a.P[i] == (int32_t)i && a.counter[i] > 0 ? 1 : 0;
}

// the faces first, from the roots, then (a second launch) the vertices in place
template <bool FACES>
__global__ __launch_bounds__(256) void k_cc_mesh_relabel(const CcMesh a)
{
    if (FACES) {
        CC_GRID_STRIDE(f, a.n_faces) {
            int32_t v0, v1, v2;
            const bool ok = cc_face(a, f, v0, v1, v2);
            const int32_t r = ok ? a.P[v0] : -1;
            const bool in = r >= 0 && r <= v0;
            a.face_label[f] = in ? a.rank[r] : -1;
            if (a.face_size) a.face_size[f] = in ? a.counter[r] : 0;
        }
    } else {
        CC_GRID_STRIDE(i, a.n_vertices) {
            const int32_t r = a.P[i];
            const bool in = r >= 0 && r <= (int32_t)i;
            a.P[i] = in && a.counter[r] > 0 ? a.rank[r] : -1;
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_fill_faces(int32_t* __restrict__ face_label, int32_t* __restrict__ face_size, int64_t n)
{
    CC_GRID_STRIDE(f, n) {
        if (face_label) face_label[f] = -1;
        if (face_size) face_size[f] = 0;
    }
}

// ---- per-component statistics

struct CcStats {
    const int32_t* labels; const int32_t* size;
    int rx, ry; int64_t n, n_components;
    int32_t* sizes; int32_t* boxes;
};

__global__ __launch_bounds__(256) void k_cc_stats_init(const CcStats a)
{
    CC_GRID_STRIDE(c, a.n_components) {
        a.sizes[c] = 0;
        if (a.boxes) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { a.boxes[6 * c + k] = INT32_MAX; a.boxes[6 * c + 3 + k] = -1; }
        }
    }
}

// sizes: every member stores its component's size, the same value; boxes: integer minima and maxima
__global__ __launch_bounds__(256) void k_cc_stats(const CcStats a)
{
    CC_GRID_STRIDE(i, a.n) {
        const int32_t c = a.labels[i];
        if (c < 0 || c >= a.n_components) continue;
        a.sizes[c] = a.size[i];
        if (a.boxes) {
            const int ix = (int)(i % a.rx), iy = (int)((i / a.rx) % a.ry), iz = (int)(i / ((int64_t)a.rx * a.ry));
            int32_t* b = a.boxes + 6 * (int64_t)c;
            // an atomic only where the box as read just now does not hold the point: a bound only ever widens, so a stale read
            // costs an atomic that changes nothing and never skips one that was needed
            if (ix < cc_load(b + 0)) atomicMin(b + 0, ix);
            if (iy < cc_load(b + 1)) atomicMin(b + 1, iy);
            if (iz < cc_load(b + 2)) atomicMin(b + 2, iz);
            if (ix > cc_load(b + 3)) atomicMax(b + 3, ix);
            if (iy > cc_load(b + 4)) atomicMax(b + 4, iy);
            if (iz > cc_load(b + 5)) atomicMax(b + 5, iz);
        }
    }
}

// ---- entry points

// {rank (n + 1) | counter (n) | the scan's tile sums}, each part rounded to 8 bytes
struct CcWs { int64_t counter; PnrTableWs t; };
static CcWs cc_carve(int64_t n)
{
    CcWs w;
    w.counter = ((n + 1) * 4 + 7) & ~(int64_t)7;
    w.t = pnr_table_carve(w.counter + ((n * 4 + 7) & ~(int64_t)7), n, false);
    return w;
}

PNR_EXPORT int64_t pnr_cc_workspace_bytes(int64_t n_elements)
{
    if (n_elements < 0 || n_elements > CC_MAX_ELEMENTS) return -1;
    return cc_carve(n_elements).t.bytes;
}

static bool cc_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + (uintptr_t)b_bytes && y < x + (uintptr_t)a_bytes;
}

// steps 1 and 2 of a lattice: P and the links
template <int MODE, int FULL, int TX, int TY, int TZ>
static void cc_launch_links(const CcLattice& a, int grid, hipStream_t st)
{
#ifdef PNR_CC_FLAT
    hipLaunchKernelGGL(k_cc_init<MODE>, dim3(grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_cc_link<MODE, FULL, 0, 0, 0>), dim3(grid), dim3(256), 0, st, a);
#else
    const int64_t tiles = (((int64_t)a.rx + TX - 1) / TX) * (((int64_t)a.ry + TY - 1) / TY) * (((int64_t)a.rz + TZ - 1) / TZ);
    hipLaunchKernelGGL((k_cc_tile<MODE, FULL, TX, TY, TZ>), dim3(pnr_grid_cap(tiles)), dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_cc_link<MODE, FULL, TX, TY, TZ>), dim3(grid), dim3(256), 0, st, a);
#endif
}

template <int MODE>
static void cc_launch_lattice(const CcLattice& a, int full, int grid, hipStream_t st)
{
    if (a.rz == 1) {                                    // an image
        if (full) cc_launch_links<MODE, 1, PNR_CC_TILE_X, PNR_CC_TILE_Y, 1>(a, grid, st);
        else cc_launch_links<MODE, 0, PNR_CC_TILE_X, PNR_CC_TILE_Y, 1>(a, grid, st);
    } else {
        if (full) cc_launch_links<MODE, 1, PNR_CC_TILE3_X, PNR_CC_TILE3_Y, PNR_CC_TILE3_Z>(a, grid, st);
        else cc_launch_links<MODE, 0, PNR_CC_TILE3_X, PNR_CC_TILE3_Y, PNR_CC_TILE3_Z>(a, grid, st);
    }
}

PNR_EXPORT int pnr_cc_label(const void* data, int mode, float tol, int res_x, int res_y, int res_z, int full, int32_t* labels, int32_t* size,
                            int64_t* count, void* workspace, void* stream)
{
    PNR_REQUIRE(mode == PNR_CC_KEYS || mode == PNR_CC_VALUES, "pnr_cc_label: unknown mode %d", mode);
    PNR_REQUIRE(full == 0 || full == 1, "pnr_cc_label: full must be 0 or 1 (got %d)", full);
    PNR_REQUIRE(mode != PNR_CC_VALUES || tol >= 0.0f, "pnr_cc_label: tol must be >= 0 and not NaN (got %g)", (double)tol);
    PNR_REQUIRE(count && ((uintptr_t)count & 7) == 0, "pnr_cc_label: count must be non-null and 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (res_x >= 0 && res_y >= 0 && res_z >= 0 && (res_x == 0 || res_y == 0 || res_z == 0)) {     // no elements: count = 0
        pnr_zero_i32((int32_t*)count, 2, st);
        PNR_CHECK_LAUNCH("pnr_cc_label");
        return PNR_OK;
    }
    const float zero3[3] = {0.0f, 0.0f, 0.0f};
    const int rc = pnr_lattice_check("pnr_cc_label", res_x, res_y, res_z, zero3, zero3, 1, CC_MAX_ELEMENTS, false);
    if (rc) return rc;
    PNR_REQUIRE(data && labels && workspace, "pnr_cc_label: null data, labels or workspace");
    PNR_REQUIRE((((uintptr_t)data | (uintptr_t)labels | (uintptr_t)size) & 3) == 0, "pnr_cc_label: data, labels and size must be 4-byte aligned");
    PNR_REQUIRE(((uintptr_t)workspace & 7) == 0, "pnr_cc_label: workspace must be 8-byte aligned");
    CcLattice a;
    a.data = data; a.mode = mode; a.tol = tol; a.rx = res_x; a.ry = res_y; a.rz = res_z; a.n = (int64_t)res_x * res_y * res_z;
    PNR_REQUIRE(!cc_overlap(data, a.n * 4, labels, a.n * 4) && !cc_overlap(data, a.n * 4, size, a.n * 4) && !cc_overlap(labels, a.n * 4, size, a.n * 4),
                "pnr_cc_label: data, labels and size may not overlap");
    const CcWs w = cc_carve(a.n);
    a.P = labels; a.rank = (int32_t*)workspace; a.counter = size ? (int32_t*)((char*)workspace + w.counter) : nullptr; a.size = size;
    const int grid = pnr_grid_cap((a.n + 255) / 256);
    if (mode == PNR_CC_KEYS) cc_launch_lattice<PNR_CC_KEYS>(a, full, grid, st);
    else cc_launch_lattice<PNR_CC_VALUES>(a, full, grid, st);
    hipLaunchKernelGGL(k_cc_flatten, dim3(grid), dim3(256), 0, st, a);
    pnr_scan_i32(a.rank, a.rank, a.n, (char*)workspace + w.t.sums, count, st);
    hipLaunchKernelGGL(k_cc_relabel, dim3(grid), dim3(256), 0, st, a);
    PNR_CHECK_LAUNCH("pnr_cc_label");
    return PNR_OK;
}

PNR_EXPORT int pnr_cc_mesh(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* vertex_label, int32_t* face_label, int32_t* face_size,
                           int64_t* count, void* workspace, void* stream)
{
    PnrMesh m;
    const int rc = pnr_mesh_check("pnr_cc_mesh", nullptr, 0, faces, n_faces, (int64_t)INT32_MAX, m);
    if (rc) return rc;
    PNR_REQUIRE(n_vertices >= 0 && n_vertices <= CC_MAX_ELEMENTS, "pnr_cc_mesh: n_vertices must be within 0 .. 2^31 - 2");
    PNR_REQUIRE(count && ((uintptr_t)count & 7) == 0, "pnr_cc_mesh: count must be non-null and 8-byte aligned");
    PNR_REQUIRE((n_vertices == 0 || vertex_label) && (n_faces == 0 || face_label), "pnr_cc_mesh: null vertex_label or face_label");
    PNR_REQUIRE((((uintptr_t)vertex_label | (uintptr_t)face_label | (uintptr_t)face_size) & 3) == 0,
                "pnr_cc_mesh: vertex_label, face_label and face_size must be 4-byte aligned");
    PNR_REQUIRE(!cc_overlap(faces, n_faces * 12, face_label, n_faces * 4) && !cc_overlap(faces, n_faces * 12, face_size, n_faces * 4) &&
                    !cc_overlap(faces, n_faces * 12, vertex_label, n_vertices * 4),
                "pnr_cc_mesh: the outputs may not overlap faces");
    hipStream_t st = (hipStream_t)stream;
    if (n_vertices == 0) {                      // no elements: every face is out of range, count = 0
        if (n_faces) hipLaunchKernelGGL(k_cc_fill_faces, dim3(pnr_grid_cap((n_faces + 255) / 256)), dim3(256), 0, st, face_label, face_size, n_faces);
        pnr_zero_i32((int32_t*)count, 2, st);
        PNR_CHECK_LAUNCH("pnr_cc_mesh");
        return PNR_OK;
    }
    PNR_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "pnr_cc_mesh: workspace must be non-null and 8-byte aligned");
    const CcWs w = cc_carve(n_vertices);
    CcMesh a;
    a.faces = faces; a.n_faces = n_faces; a.n_vertices = n_vertices;
    a.P = vertex_label; a.rank = (int32_t*)workspace; a.counter = (int32_t*)((char*)workspace + w.counter);
    a.face_label = face_label; a.face_size = face_size;
    const int gv = pnr_grid_cap((n_vertices + 255) / 256), gf = pnr_grid_cap((n_faces + 255) / 256);
    hipLaunchKernelGGL(k_cc_mesh_init, dim3(gv), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cc_mesh_link, dim3(gf), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cc_mesh_flatten, dim3(gv), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cc_mesh_count, dim3(gf), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cc_mesh_flag, dim3(gv), dim3(256), 0, st, a);
    pnr_scan_i32(a.rank, a.rank, n_vertices, (char*)workspace + w.t.sums, count, st);
    hipLaunchKernelGGL(k_cc_mesh_relabel<true>, dim3(gf), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cc_mesh_relabel<false>, dim3(gv), dim3(256), 0, st, a);
    PNR_CHECK_LAUNCH("pnr_cc_mesh");
    return PNR_OK;
}

PNR_EXPORT int pnr_cc_stats(const int32_t* labels, const int32_t* size, int res_x, int res_y, int res_z, int64_t n_components, int32_t* sizes,
                            int32_t* boxes, void* stream)
{
    const float zero3[3] = {0.0f, 0.0f, 0.0f};
    const int rc = pnr_lattice_check("pnr_cc_stats", res_x, res_y, res_z, zero3, zero3, 1, CC_MAX_ELEMENTS, false);
    if (rc) return rc;
    PNR_REQUIRE(n_components >= 0 && n_components <= CC_MAX_ELEMENTS, "pnr_cc_stats: n_components must be within 0 .. 2^31 - 2");
    if (n_components == 0) return PNR_OK;
    PNR_REQUIRE(labels && size && sizes, "pnr_cc_stats: null labels, size or sizes");
    PNR_REQUIRE((((uintptr_t)labels | (uintptr_t)size | (uintptr_t)sizes | (uintptr_t)boxes) & 3) == 0,
                "pnr_cc_stats: labels, size, sizes and boxes must be 4-byte aligned");
    CcStats a;
    a.labels = labels; a.size = size; a.rx = res_x; a.ry = res_y; a.n = (int64_t)res_x * res_y * res_z; a.n_components = n_components;
    a.sizes = sizes; a.boxes = boxes;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cc_stats_init, dim3(pnr_grid_cap((n_components + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cc_stats, dim3(pnr_grid_cap((a.n + 255) / 256)), dim3(256), 0, st, a);
    PNR_CHECK_LAUNCH("pnr_cc_stats");
    return PNR_OK;
}
