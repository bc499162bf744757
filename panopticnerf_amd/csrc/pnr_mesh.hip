// Mesh extraction (include/pnr.h "mesh extraction"): marching tetrahedra on the Kuhn split of a (res_z, res_y, res_x) float32
// lattice -> vertices, int32 faces and, per vertex, the lattice point its label comes from.  tests/_mesh_ref.py restates the
// rule twice; everything here equals it bit for bit, so the numbering is part of the contract: no atomics anywhere.
//
// pnr_mesh_count: k_mesh_classify (a point's eight values p + {0,1}^3 are its cube's corners AND the far ends of the seven
// edges it owns: one load set gives the 7-bit crossing mask and the cube's triangle count) -> a reduce-then-scan of the two
// counts carried as one 64-bit add (vertices low, triangles high; both totals stay below 2^31): per-chunk sums out of the
// classify blocks, ONE block over the chunk sums (k_mesh_scan_sums, which also writes the totals), then k_mesh_scan_add scans
// inside each chunk and adds the chunk's base.  No kernel waits on another workgroup: the stream orders the three launches.
// pnr_mesh_emit: k_mesh_emit, one thread per point, writes the point's vertices at its scanned base and its cube's triangles at
// theirs; a triangle corner is base_v[owner] + popcount(mask[owner] & ((1 << kind) - 1)) with the owner one of the cube's corners.
//
// All four are memory bound.  A point's x neighbour is the next lane's point (coalesced); its y and z neighbours are other
// rows of the same launch, read again from L2.  A chunk is PNR_MESH_CHUNK consecutive points; a block walks chunks grid-stride.
// The lattice's check and points are pnr_geom_dev.h's; the 64-bit scan over chunk sums is this file's own, not pnr_scan_dev.h's.
#include <math.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"

#define PNR_MESH_BLOCK 256
static_assert(PNR_MESH_BLOCK == PNR_SCAN_BLOCK, "the three scan kernels call pnr_block_scan_excl");
#define PNR_MESH_ITEMS 4                                    // points a thread handles per chunk
#define PNR_MESH_CHUNK (PNR_MESH_BLOCK * PNR_MESH_ITEMS)    // 1024 points: one entry of the chunk-sum level
// -DPNR_MESH_BLOCKS_PER_CU=n (A/B builds): the capped grid of the per-point kernels.  Measured at 256^3 (profiles/README.md "Mesh"):
// 4 -> 8 -> 16 blocks a compute unit take a sphere's count + emit from 307 to 250 to 229 us and noise's from 1.73 to 1.82 to 1.83 ms.
#ifndef PNR_MESH_BLOCKS_PER_CU
#define PNR_MESH_BLOCKS_PER_CU 8
#endif
#define PNR_MESH_MAX_POINTS ((int64_t)(INT32_MAX / 12))     // 12 triangles a cube at most: every count fits an int32 scan

typedef unsigned long long mesh_u64;

// ---- the tables.  Tetrahedron pi (xyz xzy yxz yzx zxy zyx) has the corner codes 0, C1, C2, 7 (code = x + 2 y + 4 z of the
// offset from the cube's corner).  MESH_FLIP[case][parity of pi] is the header's 16 x 2 table.  From them, per (tetrahedron,
// case), the up to two triangles as six 6-bit fields (owner code | kind << 3), winding applied: built at compile time.
constexpr int MESH_C1[6] = {1, 1, 2, 2, 4, 4};
constexpr int MESH_C2[6] = {3, 5, 3, 6, 5, 6};
constexpr int MESH_PARITY[6] = {0, 1, 1, 0, 0, 1};
constexpr int MESH_FLIP[16][2] = {{0, 0}, {0, 1}, {1, 0}, {0, 1}, {0, 1}, {1, 0}, {0, 1}, {0, 1},
                                  {1, 0}, {0, 1}, {1, 0}, {1, 0}, {0, 1}, {0, 1}, {1, 0}, {0, 0}};
struct MeshTable {
    mesh_u64 tri[6 * 16];
};
constexpr MeshTable mesh_make_table()
{
    MeshTable t{};
    for (int tet = 0; tet < 6; ++tet) {
        const int c[4] = {0, MESH_C1[tet], MESH_C2[tet], 7};
        for (int cs = 0; cs < 16; ++cs) {
            int I[4] = {0, 0, 0, 0}, O[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int k = 0; k < 4; ++k) {
                if ((cs >> k) & 1) I[ni++] = k;
                else O[no++] = k;
            }
            int v[6][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}}, nv = 0;      // (inside corner, outside corner)
            if (ni == 1) {
                for (int k = 0; k < 3; ++k) { v[k][0] = I[0]; v[k][1] = O[k]; }
                nv = 3;
            } else if (ni == 3) {
                for (int k = 0; k < 3; ++k) { v[k][0] = I[k]; v[k][1] = O[0]; }
                nv = 3;
            } else if (ni == 2) {
                const int q[4][2] = {{I[0], O[0]}, {I[0], O[1]}, {I[1], O[1]}, {I[1], O[0]}};
                const int order[6] = {0, 1, 2, 0, 2, 3};
                for (int k = 0; k < 6; ++k) { v[k][0] = q[order[k]][0]; v[k][1] = q[order[k]][1]; }
                nv = 6;
            }
            if (MESH_FLIP[cs][MESH_PARITY[tet]]) {
                for (int b = 0; b < nv; b += 3) {
                    const int s0 = v[b + 1][0], s1 = v[b + 1][1];
                    v[b + 1][0] = v[b + 2][0]; v[b + 1][1] = v[b + 2][1];
                    v[b + 2][0] = s0; v[b + 2][1] = s1;
                }
            }
            mesh_u64 e = 0;
            for (int k = 0; k < nv; ++k) {
                const int a = v[k][0] < v[k][1] ? v[k][0] : v[k][1], b = v[k][0] < v[k][1] ? v[k][1] : v[k][0];
                const int owner = c[a], kind = (c[b] ^ c[a]) - 1;      // the lower end owns the edge; its code is a subset of the upper's
                e |= (mesh_u64)(owner | (kind << 3)) << (6 * k);
            }
            t.tri[tet * 16 + cs] = e;
        }
    }
    return t;
}
__constant__ MeshTable d_mesh_table = mesh_make_table();

struct MeshDims {
    int rx, ry, rz;
    int sz;                 // rx * ry
    int n;                  // rx * ry * rz
    int n_chunks;
};

// the eight values p + {0,1}^3 (index = corner code); a corner outside the lattice reads as NaN, which is never inside
__device__ __forceinline__ void mesh_load8(const float* __restrict__ f, const MeshDims& d, int n, int& ix, int& iy, int& iz, bool& ex, bool& ey, bool& ez, float v[8])
{
    iz = n / d.sz;
    const int r = n - iz * d.sz;
    iy = r / d.rx;
    ix = r - iy * d.rx;
    ex = ix + 1 < d.rx; ey = iy + 1 < d.ry; ez = iz + 1 < d.rz;
    const float absent = __builtin_nanf("");
    v[0] = f[n];
    v[1] = ex ? f[n + 1] : absent;
    v[2] = ey ? f[n + d.rx] : absent;
    v[3] = ex && ey ? f[n + d.rx + 1] : absent;
    v[4] = ez ? f[n + d.sz] : absent;
    v[5] = ex && ez ? f[n + d.sz + 1] : absent;
    v[6] = ey && ez ? f[n + d.sz + d.rx] : absent;
    v[7] = ex && ey && ez ? f[n + d.sz + d.rx + 1] : absent;
}

__device__ __forceinline__ unsigned mesh_inside_bits(const float v[8], float level)
{
    unsigned cm = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) cm |= (v[c] > level ? 1u : 0u) << c;
    return cm;
}

// the 7-bit crossing mask of the edges a point owns (bit = kind = code - 1) | the triangle count of its cube << 8
__device__ __forceinline__ unsigned mesh_info(unsigned cm, bool ex, bool ey, bool ez)
{
    const unsigned exist = (ex ? 0xAAu : 0u) | 0x55u, eyist = (ey ? 0xCCu : 0u) | 0x33u, ezist = (ez ? 0xF0u : 0u) | 0x0Fu;
    const unsigned there = exist & eyist & ezist;                   // corners inside the lattice
    const unsigned differs = (cm & 1u) ? ~cm : cm;                  // corners whose side is not the point's
    const unsigned mask = ((differs & there) >> 1) & 0x7Fu;
    unsigned ntri = 0;
    if (ex && ey && ez) {
#pragma unroll
        for (int tet = 0; tet < 6; ++tet) {
            const unsigned pc = (cm & 1u) + ((cm >> MESH_C1[tet]) & 1u) + ((cm >> MESH_C2[tet]) & 1u) + (cm >> 7);
            ntri += pc == 2u ? 2u : ((pc == 1u || pc == 3u) ? 1u : 0u);
        }
    }
    return mask | (ntri << 8);
}

__device__ __forceinline__ mesh_u64 mesh_counts(unsigned info) { return (mesh_u64)__popc(info & 0x7Fu) | ((mesh_u64)(info >> 8) << 32); }

// ---- count, step 1: info per point (zeros in the last chunk's padding) and the chunk's sum
__global__ __launch_bounds__(PNR_MESH_BLOCK) void k_mesh_classify(const float* __restrict__ field, MeshDims d, float level,
                                                                  unsigned short* __restrict__ info, mesh_u64* __restrict__ sums)
{
    __shared__ mesh_u64 lds[4];
    for (int chunk = blockIdx.x; chunk < d.n_chunks; chunk += gridDim.x) {
        mesh_u64 mine = 0;
#pragma unroll
        for (int j = 0; j < PNR_MESH_ITEMS; ++j) {
            const int n = chunk * PNR_MESH_CHUNK + j * PNR_MESH_BLOCK + (int)threadIdx.x;
            unsigned w = 0;
            if (n < d.n) {
                int ix, iy, iz;
                bool ex, ey, ez;
                float v[8];
                mesh_load8(field, d, n, ix, iy, iz, ex, ey, ez, v);
                w = mesh_info(mesh_inside_bits(v, level), ex, ey, ez);
            }
            info[n] = (unsigned short)w;                            // n < n_chunks * PNR_MESH_CHUNK, the array's padded length
            mine += mesh_counts(w);
        }
        mesh_u64 total;
        pnr_block_scan_excl<mesh_u64>(mine, lds, total);
        if (threadIdx.x == 0) sums[chunk] = total;
    }
}

// ---- count, step 2: ONE block turns the chunk sums into their exclusive prefix, in place, and writes the totals
#define PNR_MESH_SCAN_ITEMS 4
__global__ __launch_bounds__(PNR_MESH_BLOCK) void k_mesh_scan_sums(mesh_u64* __restrict__ sums, int n_chunks, int64_t* __restrict__ totals)
{
    __shared__ mesh_u64 lds[4];
    mesh_u64 carry = 0;
    for (int base = 0; base < n_chunks; base += PNR_MESH_BLOCK * PNR_MESH_SCAN_ITEMS) {
        const int i0 = base + (int)threadIdx.x * PNR_MESH_SCAN_ITEMS;
        mesh_u64 v[PNR_MESH_SCAN_ITEMS], s = 0;
#pragma unroll
        for (int j = 0; j < PNR_MESH_SCAN_ITEMS; ++j) {
            v[j] = i0 + j < n_chunks ? sums[i0 + j] : 0;
            s += v[j];
        }
        mesh_u64 total;
        mesh_u64 run = pnr_block_scan_excl<mesh_u64>(s, lds, total) + carry;
#pragma unroll
        for (int j = 0; j < PNR_MESH_SCAN_ITEMS; ++j) {
            if (i0 + j < n_chunks) sums[i0 + j] = run;
            run += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        totals[0] = (int64_t)(carry & 0xFFFFFFFFull);
        totals[1] = (int64_t)(carry >> 32);
    }
}

// ---- count, step 3: scan inside each chunk (a thread holds PNR_MESH_ITEMS CONSECUTIVE points here) and add the chunk's base:
// rec[n] = base_v | info << 32 (mask in bits 32 .. 38, the triangle count in 40 .. 43), base_t[n]
__global__ __launch_bounds__(PNR_MESH_BLOCK) void k_mesh_scan_add(const unsigned short* __restrict__ info, const mesh_u64* __restrict__ sums,
                                                                  int n_chunks, mesh_u64* __restrict__ rec, int* __restrict__ base_t)
{
    __shared__ mesh_u64 lds[4];
    typedef unsigned short us4 __attribute__((ext_vector_type(4)));
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int n0 = chunk * PNR_MESH_CHUNK + (int)threadIdx.x * PNR_MESH_ITEMS;
        const us4 w = *reinterpret_cast<const us4*>(info + n0);
        mesh_u64 s = 0;
#pragma unroll
        for (int j = 0; j < PNR_MESH_ITEMS; ++j) s += mesh_counts(w[j]);
        mesh_u64 total;
        mesh_u64 run = pnr_block_scan_excl<mesh_u64>(s, lds, total) + sums[chunk];
#pragma unroll
        for (int j = 0; j < PNR_MESH_ITEMS; ++j) {
            rec[n0 + j] = (run & 0xFFFFFFFFull) | ((mesh_u64)w[j] << 32);
            base_t[n0 + j] = (int)(run >> 32);
            run += mesh_counts(w[j]);
        }
    }
}

// ---- emit
struct MeshEmitArgs {
    const float* field;
    const mesh_u64* rec;
    const int* base_t;
    float* vertices;
    int* faces;
    int64_t* src;
    MeshDims d;
    float level;
    float lo[3], step[3];
};

__global__ __launch_bounds__(PNR_MESH_BLOCK) void k_mesh_emit(MeshEmitArgs a)
{
    // a thread's copy of the records of its cube's corners 0 .. 6 (corner 7 owns no edge of the cube): the triangle table
    // names owners at run time, and a run-time index into registers would go to scratch.  Each thread reads only its own column.
    __shared__ mesh_u64 s_rec[7][PNR_MESH_BLOCK];
    const MeshDims& d = a.d;
    for (int chunk = blockIdx.x; chunk < d.n_chunks; chunk += gridDim.x) {
#pragma unroll 1
        for (int j = 0; j < PNR_MESH_ITEMS; ++j) {
            const int n = chunk * PNR_MESH_CHUNK + j * PNR_MESH_BLOCK + (int)threadIdx.x;
            if (n >= d.n) continue;
            const mesh_u64 own = a.rec[n];
            const unsigned mask = (unsigned)(own >> 32) & 0x7Fu, ntri = (unsigned)(own >> 40) & 0xFu;
            if (mask == 0 && ntri == 0) continue;
            int ix, iy, iz;
            bool ex, ey, ez;
            float v[8];
            mesh_load8(a.field, d, n, ix, iy, iz, ex, ey, ez, v);
            if (mask != 0 && a.vertices) {
                const float pa[3] = {pnr_lattice_coord((float)ix, a.lo[0], a.step[0]), pnr_lattice_coord((float)iy, a.lo[1], a.step[1]),
                                     pnr_lattice_coord((float)iz, a.lo[2], a.step[2])};
                const float pb[3] = {pnr_lattice_coord((float)(ix + 1), a.lo[0], a.step[0]), pnr_lattice_coord((float)(iy + 1), a.lo[1], a.step[1]),
                                     pnr_lattice_coord((float)(iz + 1), a.lo[2], a.step[2])};
                const bool in0 = v[0] > a.level;
                size_t vi = (size_t)(unsigned)own;
#pragma unroll
                for (int code = 1; code < 8; ++code) {
                    if (!((mask >> (code - 1)) & 1u)) continue;
                    float t = (a.level - v[0]) / (v[code] - v[0]);
                    t = t != t ? 0.5f : (t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t));
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float pe = ((code >> k) & 1) ? pb[k] : pa[k];
                        const float dlt = pe - pa[k];
                        const float m = t * dlt;
                        a.vertices[vi * 3 + k] = pa[k] + m;
                    }
                    if (a.src) a.src[vi] = in0 ? (int64_t)n : (int64_t)(n + (code & 1) + ((code >> 1) & 1) * d.rx + ((code >> 2) & 1) * d.sz);
                    ++vi;
                }
            }
            if (ntri != 0 && a.faces) {                             // the cube exists: all eight corners are lattice points
                s_rec[0][threadIdx.x] = own;
#pragma unroll
                for (int c = 1; c < 7; ++c) s_rec[c][threadIdx.x] = a.rec[n + (c & 1) + ((c >> 1) & 1) * d.rx + ((c >> 2) & 1) * d.sz];
                const unsigned cm = mesh_inside_bits(v, a.level);
                size_t ti = (size_t)a.base_t[n];
                const size_t t_end = ti + ntri;                     // what pnr_mesh_count counted: a field edited since cannot write past it
#pragma unroll
                for (int tet = 0; tet < 6; ++tet) {
                    const unsigned cs = (cm & 1u) | (((cm >> MESH_C1[tet]) & 1u) << 1) | (((cm >> MESH_C2[tet]) & 1u) << 2) | ((cm >> 7) << 3);
                    const unsigned pc = __popc(cs);
                    const int nt = pc == 2u ? 2 : ((pc == 1u || pc == 3u) ? 1 : 0);
                    mesh_u64 e = d_mesh_table.tri[tet * 16 + (int)cs];
                    for (int q = 0; q < nt && ti < t_end; ++q) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const unsigned owner = (unsigned)e & 7u, kind = ((unsigned)e >> 3) & 7u;
                            const mesh_u64 orec = s_rec[owner][threadIdx.x];
                            a.faces[ti * 3 + k] = (int)((unsigned)orec + __popc((unsigned)(orec >> 32) & ((1u << kind) - 1u)));
                            e >>= 6;
                        }
                        ++ti;
                    }
                }
            }
        }
    }
}

// ---- entry points
static bool mesh_res_ok(int rx, int ry, int rz)
{
    return rx >= 1 && ry >= 1 && rz >= 1 && (int64_t)rx * ry <= PNR_MESH_MAX_POINTS && (int64_t)rx * ry * rz <= PNR_MESH_MAX_POINTS;
}
static MeshDims mesh_dims(int rx, int ry, int rz)
{
    MeshDims d;
    d.rx = rx; d.ry = ry; d.rz = rz; d.sz = rx * ry; d.n = rx * ry * rz;
    d.n_chunks = (d.n + PNR_MESH_CHUNK - 1) / PNR_MESH_CHUNK;
    return d;
}
// the workspace: rec (8 bytes a point), base_t (4), info (2), each padded to whole chunks, then the chunk sums (8 a chunk)
struct MeshWorkspace {
    mesh_u64* rec;
    int* base_t;
    unsigned short* info;
    mesh_u64* sums;
};
static MeshWorkspace mesh_carve(void* workspace, const MeshDims& d)
{
    const size_t np = (size_t)d.n_chunks * PNR_MESH_CHUNK;
    char* p = (char*)workspace;
    MeshWorkspace w;
    w.rec = (mesh_u64*)p;
    w.base_t = (int*)(p + 8 * np);
    w.info = (unsigned short*)(p + 12 * np);
    w.sums = (mesh_u64*)(p + 14 * np);
    return w;
}

PNR_EXPORT int64_t pnr_mesh_workspace_bytes(int res_x, int res_y, int res_z)
{
    if (!mesh_res_ok(res_x, res_y, res_z)) {
        pnr_set_error("pnr_mesh_workspace_bytes: bad lattice %d x %d x %d (every res >= 1, at most (2^31 - 1) / 12 points)", res_x, res_y, res_z);
        return -1;
    }
    const MeshDims d = mesh_dims(res_x, res_y, res_z);
    return (int64_t)d.n_chunks * (14 * PNR_MESH_CHUNK + 8);
}

PNR_EXPORT int pnr_mesh_count(const float* field, int res_x, int res_y, int res_z, float level, void* workspace, int64_t* totals,
                              void* stream)
{
    PNR_REQUIRE(mesh_res_ok(res_x, res_y, res_z), "pnr_mesh_count: bad lattice %d x %d x %d (every res >= 1, at most (2^31 - 1) / 12 points)",
                res_x, res_y, res_z);
    PNR_REQUIRE(isfinite(level), "pnr_mesh_count: level must be finite");
    PNR_REQUIRE(field && workspace && totals, "pnr_mesh_count: null field, workspace or totals");
    PNR_REQUIRE(((uintptr_t)field & 3) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)totals & 7) == 0,
                "pnr_mesh_count: misaligned pointer (field 4, workspace 16, totals 8 bytes)");
    const MeshDims d = mesh_dims(res_x, res_y, res_z);
    const MeshWorkspace w = mesh_carve(workspace, d);
    const hipStream_t st = (hipStream_t)stream;
    if (res_x < 2 || res_y < 2 || res_z < 2) {                      // no cube: the mesh is empty, and pnr_mesh_emit launches nothing
        PNR_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
        return PNR_OK;
    }
    const int grid = pnr_grid_cap(d.n_chunks, PNR_MESH_BLOCKS_PER_CU);
    hipLaunchKernelGGL(k_mesh_classify, dim3(grid), dim3(PNR_MESH_BLOCK), 0, st, field, d, level, w.info, w.sums);
    hipLaunchKernelGGL(k_mesh_scan_sums, dim3(1), dim3(PNR_MESH_BLOCK), 0, st, w.sums, d.n_chunks, totals);
    hipLaunchKernelGGL(k_mesh_scan_add, dim3(grid), dim3(PNR_MESH_BLOCK), 0, st, (const unsigned short*)w.info, (const mesh_u64*)w.sums,
                       d.n_chunks, w.rec, w.base_t);
    PNR_CHECK_LAUNCH("pnr_mesh_count");
    return PNR_OK;
}

PNR_EXPORT int pnr_mesh_emit(const float* field, int res_x, int res_y, int res_z, float level, const float* lo_host, const float* step_host,
                             const void* workspace, float* vertices, int32_t* faces, int64_t* src, void* stream)
{
    const int rc = pnr_lattice_check("pnr_mesh_emit", res_x, res_y, res_z, lo_host, step_host, 1, PNR_MESH_MAX_POINTS, false);
    if (rc) return rc;
    PNR_REQUIRE(isfinite(level), "pnr_mesh_emit: level must be finite");
    PNR_REQUIRE(field && workspace, "pnr_mesh_emit: null field or workspace");
    PNR_REQUIRE(((uintptr_t)field & 3) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)vertices & 3) == 0 &&
                    ((uintptr_t)faces & 3) == 0 && ((uintptr_t)src & 7) == 0,
                "pnr_mesh_emit: misaligned pointer (field, vertices, faces 4, src 8, workspace 16 bytes)");
    if (res_x < 2 || res_y < 2 || res_z < 2) return PNR_OK;
    MeshEmitArgs a;
    a.d = mesh_dims(res_x, res_y, res_z);
    const MeshWorkspace w = mesh_carve(const_cast<void*>(workspace), a.d);
    a.field = field; a.rec = w.rec; a.base_t = w.base_t; a.vertices = vertices; a.faces = faces; a.src = src; a.level = level;
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo_host[k]; a.step[k] = step_host[k]; }
    const int grid = pnr_grid_cap(a.d.n_chunks, PNR_MESH_BLOCKS_PER_CU);
    hipLaunchKernelGGL(k_mesh_emit, dim3(grid), dim3(PNR_MESH_BLOCK), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_mesh_emit");
    return PNR_OK;
}
