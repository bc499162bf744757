// Mesh ray casting (include/pnr.h "mesh ray casting"): the first hit of a ray with a triangle mesh, for the pixels of any camera
// or a list of rays -- the way back from a Mesh to an image.  The answer is DEFINED by brute force over all faces: the watertight
// ray-triangle test of Woop, Benthin and Wald in float32, two-sided, under pnr_key(t, face) and a minimum (pnr_geom_dev.h, as
// everything shared below).  The uniform grid built here only prunes: whatever its resolution, the outputs are brute force's
// bit for bit (DESIGN.md section 8 "Mesh ray casting" has the argument; tests/_meshcast_ref.py restates rule and walk).
// Build: bounds (integer atomics on order-preserving keys), per-face cell counts, the shared scan, fill (pnr_table_carve,
// pnr_table_range).  Cast: one thread per ray, a wave an 8 x 8 pixel tile (pnr_tile_grid) or 64 consecutive rays; one device
// body for both.  The mesh is a PnrMesh.  A cell entry is a 48-byte record of the three corners and the face index: a candidate
// is three 16-byte loads and no dependent gather.  No LDS, no floating atomics, nothing waits on anything.
#include <float.h>
#include <math.h>

#include "pnr_common.h"
#include "pnr_geom_dev.h"

#define MC_BOUNDS_WORDS 8                   // workspace words of the bounds: 3 min keys, 3 max keys, the usable faces, one spare

struct McGrid {
    int res[3];
    float lo[3], inv[3], cell[3];
    const int32_t* start;                   // (cells + 1)
    const float4* records;                  // (n_entries, 3)
    int64_t n_entries;
};

struct McTri { float v[3][3]; bool ok; };

// the corners of face t; ok = every index in range and every coordinate finite (a face that is not ok never hits)
__device__ __forceinline__ McTri mc_tri(const PnrMesh& m, int64_t t)
{
    McTri r;
    const int32_t i[3] = {m.faces[3 * t], m.faces[3 * t + 1], m.faces[3 * t + 2]};
    r.ok = i[0] >= 0 && i[0] < m.n_vertices && i[1] >= 0 && i[1] < m.n_vertices && i[2] >= 0 && i[2] < m.n_vertices;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) r.v[c][k] = r.ok ? m.vertices[3 * (int64_t)i[c] + k] : 0.0f;
    r.ok = r.ok && pnr_finite3(r.v[0][0], r.v[0][1], r.v[0][2]) && pnr_finite3(r.v[1][0], r.v[1][1], r.v[1][2]) &&
           pnr_finite3(r.v[2][0], r.v[2][1], r.v[2][2]);
    return r;
}

// ---- the index

// order-preserving key of a float (-0 below +0; no NaN reaches it)
__device__ __forceinline__ unsigned int mc_key(float x)
{
    const unsigned int u = __float_as_uint(x);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mc_unkey(unsigned int k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ __launch_bounds__(64) void k_meshcast_bounds_init(unsigned int* __restrict__ w)
{
    if (threadIdx.x < MC_BOUNDS_WORDS) w[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
}

__global__ __launch_bounds__(256) void k_meshcast_bounds(const PnrMesh m, unsigned int* __restrict__ w)
{
    unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, n = 0u;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m.n_faces; t += (int64_t)gridDim.x * blockDim.x) {
        const McTri r = mc_tri(m, t);
        if (!r.ok) continue;
        n += 1u;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned int key = mc_key(r.v[c][k]);
                lo[k] = key < lo[k] ? key : lo[k];
                hi[k] = key > hi[k] ? key : hi[k];
            }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned int a = __shfl_xor(lo[k], s, 64), b = __shfl_xor(hi[k], s, 64);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
        n += __shfl_xor(n, s, 64);
    }
    if ((threadIdx.x & 63) == 0 && n) {             // integer atomics: exact in any order
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&w[k], lo[k]); atomicMax(&w[3 + k], hi[k]); }
        atomicAdd(&w[6], n);
    }
}

// bounds[0..2] = lo, [3..5] = hi (+inf / -inf without a usable face), [6] = the bits of the usable-face count, [7] = 0
__global__ __launch_bounds__(64) void k_meshcast_bounds_final(const unsigned int* __restrict__ w, float* __restrict__ bounds)
{
    const int k = threadIdx.x;
    if (k >= MC_BOUNDS_WORDS) return;
    const bool any = w[6] != 0u;
    bounds[k] = k < 3 ? (any ? mc_unkey(w[k]) : INFINITY) : k < 6 ? (any ? mc_unkey(w[k]) : -INFINITY) : __uint_as_float(k == 6 ? w[6] : 0u);
}

// the grid coordinate of p on one axis, and a cell index clamped as a float before the conversion (NaN gives 0)
__device__ __forceinline__ float mc_g(float p, float lo, float inv) { return (p - lo) * inv; }
__device__ __forceinline__ int mc_cell(float g, int res) { return (int)fminf(fmaxf(floorf(g), 0.0f), (float)(res - 1)); }

// FILL = false: cursor[cell] += 1 for every cell of the face's padded box.  FILL = true: the face's record goes to
// start[cell] + (the value the cell's cursor had) - 1, the cursor counting down from the cell's count.
template <bool FILL>
__device__ __forceinline__ void mc_scatter(const PnrMesh& m, const McGrid& g, int32_t* __restrict__ cursor, float4* __restrict__ records)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m.n_faces; t += (int64_t)gridDim.x * blockDim.x) {
        const McTri r = mc_tri(m, t);
        if (!r.ok) continue;
        int c0[3], c1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = mc_g(r.v[0][k], g.lo[k], g.inv[k]), b = mc_g(r.v[1][k], g.lo[k], g.inv[k]), c = mc_g(r.v[2][k], g.lo[k], g.inv[k]);
            c0[k] = mc_cell(fminf(fminf(a, b), c) - PNR_MESHCAST_PAD, g.res[k]);
            c1[k] = mc_cell(fmaxf(fmaxf(a, b), c) + PNR_MESHCAST_PAD, g.res[k]);
        }
        for (int cz = c0[2]; cz <= c1[2]; ++cz)
            for (int cy = c0[1]; cy <= c1[1]; ++cy)
                for (int cx = c0[0]; cx <= c1[0]; ++cx) {
                    const int64_t cell = ((int64_t)cz * g.res[1] + cy) * g.res[0] + cx;
                    if (!FILL) {
                        atomicAdd(&cursor[cell], 1);
                    } else {
                        const int64_t at = (int64_t)g.start[cell] + (int64_t)atomicSub(&cursor[cell], 1) - 1;
                        if (at >= 0 && at < g.n_entries) {                 // (a damaged table never writes outside)
                            records[3 * at + 0] = make_float4(r.v[0][0], r.v[0][1], r.v[0][2], r.v[1][0]);
                            records[3 * at + 1] = make_float4(r.v[1][1], r.v[1][2], r.v[2][0], r.v[2][1]);
                            records[3 * at + 2] = make_float4(r.v[2][2], __int_as_float((int)t), 0.0f, 0.0f);
                        }
                    }
                }
    }
}

__global__ __launch_bounds__(256) void k_meshcast_count(const PnrMesh m, const McGrid g, int32_t* __restrict__ cursor) { mc_scatter<false>(m, g, cursor, nullptr); }

__global__ __launch_bounds__(256) void k_meshcast_fill(const PnrMesh m, const McGrid g, int32_t* __restrict__ cursor, float4* __restrict__ records)
{
    mc_scatter<true>(m, g, cursor, records);
}

// ---- the cast

struct McRay {
    float o[3], d[3], near_, far_;
    int kx, ky, kz;
    float Sx, Sy, Sz;
};

struct McHit { bool hit; float t, U, V, W, det; };

__device__ __forceinline__ float mc_pick(const float (&v)[3], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : v[2]; }

// the watertight test of one face (include/pnr.h "mesh ray casting", RAY-TRIANGLE TEST): every operation rounded, never an FMA
__device__ __forceinline__ McHit mc_test(const McRay& r, const float (&v0)[3], const float (&v1)[3], const float (&v2)[3])
{
    float A[3], B[3], C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { A[k] = v0[k] - r.o[k]; B[k] = v1[k] - r.o[k]; C[k] = v2[k] - r.o[k]; }
    const float Akz = mc_pick(A, r.kz), Bkz = mc_pick(B, r.kz), Ckz = mc_pick(C, r.kz);
    const float Ax = mc_pick(A, r.kx) - r.Sx * Akz, Ay = mc_pick(A, r.ky) - r.Sy * Akz, Az = r.Sz * Akz;
    const float Bx = mc_pick(B, r.kx) - r.Sx * Bkz, By = mc_pick(B, r.ky) - r.Sy * Bkz, Bz = r.Sz * Bkz;
    const float Cx = mc_pick(C, r.kx) - r.Sx * Ckz, Cy = mc_pick(C, r.ky) - r.Sy * Ckz, Cz = r.Sz * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {          // on an edge or a vertex: exact products, one subtraction, one rounding
        U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
        V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
        W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
    }
    McHit h;
    h.U = U; h.V = V; h.W = W;
    h.det = (U + V) + W;
    const bool mixed = (U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f);
    const float T = (U * Az + V * Bz) + W * Cz;
    h.t = T / h.det + 0.0f;                                               // (-0 becomes +0: the key orders as the value does)
    // the hit point t d, relative to the origin, lies in the box of the three corners A, B, C widened by a relative tolerance: a
    // ray nearly in the plane of a face, whose t is cancellation noise, does not hit that face somewhere it is not
    float M = 0.0f;                                                       // the largest |component| of the three corners: what bounds the error of t d_k
#pragma unroll
    for (int k = 0; k < 3; ++k) M = fmaxf(M, fmaxf(fmaxf(fabsf(A[k]), fabsf(B[k])), fabsf(C[k])));
    const float e = PNR_MESHCAST_BOX_TOL * M;
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float q = h.t * r.d[k];
        const float lo = fminf(fminf(A[k], B[k]), C[k]), hi = fmaxf(fmaxf(A[k], B[k]), C[k]);
        inside = inside && q >= lo - e && q <= hi + e;
    }
    h.hit = !mixed && h.det != 0.0f && h.t >= r.near_ && h.t <= r.far_ && inside;     // (a NaN misses)
    return h;
}

__device__ __forceinline__ void mc_keep(const McHit& h, int face, unsigned long long& best)
{
    if (h.hit) {
        const unsigned long long key = pnr_key(h.t, (unsigned int)face);
        best = key < best ? key : best;
    }
}

// the plain loop over all faces: what the rule says, and the path of a ray whose grid coordinates are too large for the walk
__device__ __forceinline__ unsigned long long mc_brute(const PnrMesh& m, const McRay& r)
{
    unsigned long long best = PNR_KEY_EMPTY;
    for (int64_t t = 0; t < m.n_faces; ++t) {
        const McTri tri = mc_tri(m, t);
        if (tri.ok) mc_keep(mc_test(r, tri.v[0], tri.v[1], tri.v[2]), (int)t, best);
    }
    return best;
}

// the slab walk (include/pnr.h, THE INDEX): false = the ray's reach is not within the bound of the exactness argument
__device__ __forceinline__ bool mc_walk(const McGrid& g, const McRay& r, unsigned long long& best)
{
    float og[3], dg[3];
    // the ray's reach: a bound, in world units, on every |component| of a corner relative to the origin; the walk is exact while
    // the box test's tolerance at that reach is half a pad of the SMALLEST cell, else the plain loop
    float reach = 0.0f;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        og[k] = (r.o[k] - g.lo[k]) * g.inv[k];
        dg[k] = r.d[k] * g.inv[k];
        finite = finite && fabsf(og[k]) <= FLT_MAX && fabsf(dg[k]) <= FLT_MAX;
        reach = fmaxf(reach, (fabsf(og[k]) + (float)(g.res[k] + 1)) * g.cell[k]);
    }
    if (!finite || !(reach <= PNR_MESHCAST_MAX_REACH * fminf(fminf(g.cell[0], g.cell[1]), g.cell[2]))) return false;
    int kz = 0;
    if (fabsf(dg[1]) > fabsf(dg[0])) kz = 1;
    if (fabsf(dg[2]) > fabsf(mc_pick(dg, kz))) kz = 2;
    const int kx = kz == 0 ? 1 : 0, ky = kz == 2 ? 1 : 2;
    const float dz = mc_pick(dg, kz), oz = mc_pick(og, kz);
    if (dz == 0.0f) return false;                                   // (d != 0 but d * inv underflowed)
    float t_in = r.near_, t_out = r.far_;
    best = PNR_KEY_EMPTY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = -PNR_MESHCAST_PAD, b = (float)g.res[k] + PNR_MESHCAST_PAD;
        if (dg[k] == 0.0f) {
            if (og[k] < a || og[k] > b) return true;                // outside the padded box for good: no candidate
        } else {
            const float ta = (a - og[k]) / dg[k], tb = (b - og[k]) / dg[k];
            t_in = fmaxf(t_in, fminf(ta, tb));
            t_out = fminf(t_out, fmaxf(ta, tb));
        }
    }
    if (!(fabsf(t_in) <= FLT_MAX && fabsf(t_out) <= FLT_MAX)) return false;       // an overflowed or NaN clip: the plain loop
    if (!(t_in <= t_out)) return true;
    const int rz = kz == 0 ? g.res[0] : kz == 1 ? g.res[1] : g.res[2];
    const int rx = kx == 0 ? g.res[0] : g.res[1], ry = ky == 1 ? g.res[1] : g.res[2];
    const int64_t sx = kx == 0 ? 1 : g.res[0], sy = ky == 1 ? g.res[0] : (int64_t)g.res[0] * g.res[1];
    const int64_t sz = kz == 0 ? 1 : kz == 1 ? g.res[0] : (int64_t)g.res[0] * g.res[1];
    const float ox = mc_pick(og, kx), oy = mc_pick(og, ky), dx = mc_pick(dg, kx), dy = mc_pick(dg, ky);
    const bool up = dz > 0.0f;
    const float gz_in = oz + t_in * dz;
    int L = mc_cell(up ? gz_in - PNR_MESHCAST_PAD : gz_in + PNR_MESHCAST_PAD, rz);
    const int64_t n_cells = (int64_t)g.res[0] * g.res[1] * g.res[2];
    const int n32 = (int)g.n_entries;
    while (L >= 0 && L < rz) {
        const float za = up ? (float)L : (float)(L + 1), zb = up ? (float)(L + 1) : (float)L;
        float ta = (za - oz) / dz, tb = (zb - oz) / dz;
        ta = fminf(fmaxf(ta, t_in), t_out);
        tb = fminf(fmaxf(tb, t_in), t_out);
        const float m0 = ta * dx, m1 = tb * dx, m2 = ta * dy, m3 = tb * dy;
        const float xa = ox + m0, xb = ox + m1, ya = oy + m2, yb = oy + m3;
        const int x0 = mc_cell(fminf(xa, xb) - PNR_MESHCAST_PAD, rx), x1 = mc_cell(fmaxf(xa, xb) + PNR_MESHCAST_PAD, rx);
        const int y0 = mc_cell(fminf(ya, yb) - PNR_MESHCAST_PAD, ry), y1 = mc_cell(fmaxf(ya, yb) + PNR_MESHCAST_PAD, ry);
        for (int cy = y0; cy <= y1; ++cy)
            for (int cx = x0; cx <= x1; ++cx) {
                const int64_t cell = (int64_t)L * sz + (int64_t)cy * sy + (int64_t)cx * sx;
                if (cell < 0 || cell >= n_cells) continue;
                const PnrRange rg = pnr_table_range(g.start, cell, n32);
                for (int q = rg.s; q < rg.e; ++q) {
                    const float4 p0 = g.records[3 * (int64_t)q], p1 = g.records[3 * (int64_t)q + 1], p2 = g.records[3 * (int64_t)q + 2];
                    const float v0[3] = {p0.x, p0.y, p0.z}, v1[3] = {p0.w, p1.x, p1.y}, v2[3] = {p1.z, p1.w, p2.x};
                    mc_keep(mc_test(r, v0, v1, v2), __float_as_int(p2.y), best);
                }
            }
        if (best != PNR_KEY_EMPTY) {                                     // the best hit lies more than PAD short of this layer's far face
            const float tb_ = pnr_key_value(best);
            const float gzb = oz + tb_ * dz;
            if ((up ? zb - gzb : gzb - zb) > PNR_MESHCAST_PAD) break;
        }
        if (tb >= t_out) break;
        L += up ? 1 : -1;
    }
    return true;
}

struct McArgs {
    PnrMesh m;
    McGrid g;
    int model, width, height;
    float cam[7], c2w[12], near_, far_;
    unsigned int tiles_x;
    int64_t n_tiles;
    const float* rays; int64_t n_rays;
    float *depth, *bary, *normal;
    int32_t *face, *vertex;
    uint8_t* code;
    int8_t* side;
};

// one ray, whatever its source: the outputs of element q
__device__ __forceinline__ void mc_cast(const McArgs& a, size_t q, const PnrRayRec& rec, bool ok)
{
    McRay r;
    r.o[0] = rec.lo.x; r.o[1] = rec.lo.y; r.o[2] = rec.lo.z;
    r.d[0] = rec.lo.w; r.d[1] = rec.hi.x; r.d[2] = rec.hi.y;
    r.near_ = rec.hi.z; r.far_ = rec.hi.w;
    ok = ok && pnr_finite3(r.o[0], r.o[1], r.o[2]) && pnr_finite3(r.d[0], r.d[1], r.d[2]) &&
         (r.d[0] != 0.0f || r.d[1] != 0.0f || r.d[2] != 0.0f) && r.near_ >= 0.0f && r.near_ <= r.far_;      // (false for a NaN near or far)
    float depth = 0.0f, b[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
    int32_t face = -1, vertex = -1;
    int8_t side = 0;
    uint8_t code = PNR_RAYCAST_NO_RAY;
    if (ok) {
        int kz = 0;
        if (fabsf(r.d[1]) > fabsf(r.d[0])) kz = 1;
        if (fabsf(r.d[2]) > fabsf(mc_pick(r.d, kz))) kz = 2;
        int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
        const float dz = mc_pick(r.d, kz);
        if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
        r.kx = kx; r.ky = ky; r.kz = kz;
        r.Sx = mc_pick(r.d, kx) / dz; r.Sy = mc_pick(r.d, ky) / dz; r.Sz = 1.0f / dz;
        unsigned long long best = PNR_KEY_EMPTY;
        if (!mc_walk(a.g, r, best)) best = mc_brute(a.m, r);
        code = PNR_RAYCAST_MISSED;
        if (best != PNR_KEY_EMPTY && (int64_t)pnr_key_index(best) < a.m.n_faces) {       // (a damaged table never reads outside)
            code = PNR_RAYCAST_HIT;
            face = (int32_t)pnr_key_index(best);
            depth = pnr_key_value(best);
            const McTri tri = mc_tri(a.m, face);                    // (the winner is a usable face: its record was made from these)
            const McHit h = mc_test(r, tri.v[0], tri.v[1], tri.v[2]);
            b[0] = h.U / h.det; b[1] = h.V / h.det; b[2] = h.W / h.det;
            int kb = 0;
            if (b[1] > b[0]) kb = 1;
            if (b[2] > mc_pick(b, kb)) kb = 2;
            vertex = a.m.faces[3 * (int64_t)face + kb];
            float e1[3], e2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { e1[k] = tri.v[1][k] - tri.v[0][k]; e2[k] = tri.v[2][k] - tri.v[0][k]; }
            const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
            const float dot = (nx * r.d[0] + ny * r.d[1]) + nz * r.d[2];
            side = dot < 0.0f ? 1 : -1;
            const float xx = nx * nx, yy = ny * ny, zz = nz * nz;
            const float len = sqrtf((xx + yy) + zz);
            if (pnr_pos_finite(len)) {
                const float ux = nx / len, uy = ny / len, uz = nz / len;
                n[0] = side > 0 ? ux : -ux; n[1] = side > 0 ? uy : -uy; n[2] = side > 0 ? uz : -uz;
            }
        }
    }
    a.depth[q] = depth;
    a.face[q] = face;
    a.code[q] = code;
    if (a.bary) { a.bary[3 * q] = b[0]; a.bary[3 * q + 1] = b[1]; a.bary[3 * q + 2] = b[2]; }
    if (a.vertex) a.vertex[q] = vertex;
    if (a.normal) { a.normal[3 * q] = n[0]; a.normal[3 * q + 1] = n[1]; a.normal[3 * q + 2] = n[2]; }
    if (a.side) a.side[q] = side;
}

template <bool IMAGE>
__global__ __launch_bounds__(PNR_RAYCAST_BLOCK) void k_mesh_cast(const McArgs a)
{
    if (IMAGE) {
        const int64_t tile = (int64_t)blockIdx.x * (PNR_RAYCAST_BLOCK / 64) + (threadIdx.x >> 6);
        if (tile >= a.n_tiles) return;
        const unsigned int tj = (unsigned int)(tile / a.tiles_x), ti = (unsigned int)(tile - (int64_t)tj * a.tiles_x);
        const unsigned int lane = threadIdx.x & 63;
        const int64_t i64 = (int64_t)ti * PNR_RAYCAST_TILE + (lane & (PNR_RAYCAST_TILE - 1));
        const int64_t j64 = (int64_t)tj * PNR_RAYCAST_TILE + (lane >> 3);
        if (i64 >= a.width || j64 >= a.height) return;              // the partial tiles of the right and bottom edges
        bool ok;
        const PnrRayRec rec = pnr_camera_ray(a.model, a.cam, a.c2w, (int)i64, (int)j64, a.near_, a.far_, ok);
        mc_cast(a, (size_t)j64 * (size_t)a.width + (size_t)i64, rec, ok);
    } else {
        const int64_t q = (int64_t)blockIdx.x * PNR_RAYCAST_BLOCK + threadIdx.x;
        if (q >= a.n_rays) return;
        const float4* p = (const float4*)(a.rays + 8 * q);
        mc_cast(a, (size_t)q, PnrRayRec{p[0], p[1]}, true);
    }
}

// ---- entry points

static bool mc_res_ok(int rx, int ry, int rz)
{
    return rx >= 1 && ry >= 1 && rz >= 1 && rx <= PNR_MESHCAST_MAX_RES && ry <= PNR_MESHCAST_MAX_RES && rz <= PNR_MESHCAST_MAX_RES;
}

static int mc_grid_check(const char* who, int rx, int ry, int rz, const float* lo_host, const float* cell_host, McGrid& g)
{
    PNR_REQUIRE(mc_res_ok(rx, ry, rz), "%s: bad grid %d x %d x %d (every res within 1 .. %d)", who, rx, ry, rz, PNR_MESHCAST_MAX_RES);
    PNR_REQUIRE(lo_host && cell_host, "%s: null lo_host or cell_host", who);
    g.res[0] = rx; g.res[1] = ry; g.res[2] = rz;
    for (int k = 0; k < 3; ++k) {
        PNR_REQUIRE(fabsf(lo_host[k]) <= FLT_MAX, "%s: lo must be finite (axis %d)", who, k);
        PNR_REQUIRE(pnr_pos_finite(cell_host[k]) && pnr_pos_finite(1.0f / cell_host[k]),
                    "%s: cell must be positive and finite, with a finite inverse (axis %d: %g)", who, k, (double)cell_host[k]);
        g.lo[k] = lo_host[k];
        g.inv[k] = 1.0f / cell_host[k];
        g.cell[k] = cell_host[k];
    }
    g.start = nullptr; g.records = nullptr; g.n_entries = 0;
    return PNR_OK;
}

static int64_t mc_cells(const McGrid& g) { return (int64_t)g.res[0] * g.res[1] * g.res[2]; }

PNR_EXPORT int64_t pnr_mesh_grid_workspace_bytes(int res_x, int res_y, int res_z)
{
    if (!mc_res_ok(res_x, res_y, res_z)) return -1;
    const int64_t cells = (int64_t)res_x * res_y * res_z;
    return pnr_table_carve(MC_BOUNDS_WORDS * 4, cells, true).bytes;      // the bounds' keys, the scan's tile sums, the cursors
}

PNR_EXPORT int pnr_mesh_grid_bounds(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, float* bounds,
                                    void* workspace, void* stream)
{
    PnrMesh m;
    const int rc = pnr_mesh_check("pnr_mesh_grid_bounds", vertices, n_vertices, faces, n_faces, INT32_MAX, m);
    if (rc) return rc;
    PNR_REQUIRE(bounds && workspace, "pnr_mesh_grid_bounds: null bounds or workspace");
    PNR_REQUIRE(((uintptr_t)bounds & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "pnr_mesh_grid_bounds: bounds must be 4-byte and workspace 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned int* w = (unsigned int*)workspace;
    hipLaunchKernelGGL(k_meshcast_bounds_init, dim3(1), dim3(64), 0, st, w);
    if (n_faces > 0) hipLaunchKernelGGL(k_meshcast_bounds, dim3(pnr_grid_cap((n_faces + 255) / 256)), dim3(256), 0, st, m, w);
    hipLaunchKernelGGL(k_meshcast_bounds_final, dim3(1), dim3(64), 0, st, (const unsigned int*)w, bounds);
    PNR_CHECK_LAUNCH("pnr_mesh_grid_bounds");
    return PNR_OK;
}

PNR_EXPORT int pnr_mesh_grid_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int res_x, int res_y,
                                   int res_z, const float* lo_host, const float* cell_host, int32_t* start, int64_t* total, void* workspace,
                                   void* stream)
{
    PnrMesh m;
    McGrid g;
    int rc = pnr_mesh_check("pnr_mesh_grid_count", vertices, n_vertices, faces, n_faces, INT32_MAX, m);
    if (rc) return rc;
    rc = mc_grid_check("pnr_mesh_grid_count", res_x, res_y, res_z, lo_host, cell_host, g);
    if (rc) return rc;
    PNR_REQUIRE(start && total && workspace, "pnr_mesh_grid_count: null start, total or workspace");
    PNR_REQUIRE(((uintptr_t)start & 3) == 0 && (((uintptr_t)total | (uintptr_t)workspace) & 7) == 0,
                "pnr_mesh_grid_count: start must be 4-byte, total and workspace 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t cells = mc_cells(g);
    const PnrTableWs w = pnr_table_carve(MC_BOUNDS_WORDS * 4, cells, true);
    int32_t* cursor = (int32_t*)((char*)workspace + w.cursor);
    pnr_zero_i32(cursor, cells, st);
    if (n_faces > 0) hipLaunchKernelGGL(k_meshcast_count, dim3(pnr_grid_cap((n_faces + 255) / 256)), dim3(256), 0, st, m, g, cursor);
    pnr_scan_i32(cursor, start, cells, (char*)workspace + w.sums, total, st);
    PNR_CHECK_LAUNCH("pnr_mesh_grid_count");
    return PNR_OK;
}

PNR_EXPORT int pnr_mesh_grid_fill(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int res_x, int res_y,
                                  int res_z, const float* lo_host, const float* cell_host, const int32_t* start, int64_t n_entries,
                                  float* records, void* workspace, void* stream)
{
    PnrMesh m;
    McGrid g;
    int rc = pnr_mesh_check("pnr_mesh_grid_fill", vertices, n_vertices, faces, n_faces, INT32_MAX, m);
    if (rc) return rc;
    rc = mc_grid_check("pnr_mesh_grid_fill", res_x, res_y, res_z, lo_host, cell_host, g);
    if (rc) return rc;
    PNR_REQUIRE(n_entries >= 0 && n_entries <= (int64_t)INT32_MAX, "pnr_mesh_grid_fill: n_entries must be within 0 .. 2^31 - 1 (got %lld)", (long long)n_entries);
    if (n_entries == 0 || n_faces == 0) return PNR_OK;
    PNR_REQUIRE(start && records && workspace, "pnr_mesh_grid_fill: null start, records or workspace");
    PNR_REQUIRE(((uintptr_t)start & 3) == 0 && ((uintptr_t)records & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
                "pnr_mesh_grid_fill: start must be 4-byte, records 16-byte and workspace 8-byte aligned");
    g.start = start; g.n_entries = n_entries;
    int32_t* cursor = (int32_t*)((char*)workspace + pnr_table_carve(MC_BOUNDS_WORDS * 4, mc_cells(g), true).cursor);
    hipLaunchKernelGGL(k_meshcast_fill, dim3(pnr_grid_cap((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, g, cursor, (float4*)records);
    PNR_CHECK_LAUNCH("pnr_mesh_grid_fill");
    return PNR_OK;
}

// what both casts check of the mesh, the index and the outputs, and their fill of the launch's arguments
static int mc_cast_check(const char* who, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int res_x, int res_y,
                         int res_z, const float* lo_host, const float* cell_host, const int32_t* start, const float* records, int64_t n_entries,
                         float* depth, int32_t* face, uint8_t* code, float* bary, int32_t* vertex, float* normal, int8_t* side, McArgs& a)
{
    int rc = pnr_mesh_check(who, vertices, n_vertices, faces, n_faces, INT32_MAX, a.m);
    if (rc) return rc;
    rc = mc_grid_check(who, res_x, res_y, res_z, lo_host, cell_host, a.g);
    if (rc) return rc;
    PNR_REQUIRE(n_entries >= 0 && n_entries <= (int64_t)INT32_MAX, "%s: n_entries must be within 0 .. 2^31 - 1 (got %lld)", who, (long long)n_entries);
    PNR_REQUIRE(start, "%s: null start", who);
    PNR_REQUIRE(n_entries == 0 || records, "%s: null records", who);
    PNR_REQUIRE(((uintptr_t)start & 3) == 0 && ((uintptr_t)records & 15) == 0, "%s: start must be 4-byte and records 16-byte aligned", who);
    PNR_REQUIRE(depth && face && code, "%s: null depth, face or code", who);
    PNR_REQUIRE((((uintptr_t)depth | (uintptr_t)face | (uintptr_t)bary | (uintptr_t)vertex | (uintptr_t)normal) & 3) == 0,
                "%s: misaligned array (depth, face, bary, vertex, normal: 4 bytes)", who);
    a.g.start = start; a.g.records = (const float4*)records; a.g.n_entries = n_entries;
    a.depth = depth; a.face = face; a.code = code; a.bary = bary; a.vertex = vertex; a.normal = normal; a.side = side;
    a.model = 0; a.width = a.height = 0; a.near_ = a.far_ = 0.0f; a.tiles_x = 1; a.n_tiles = 0; a.rays = nullptr; a.n_rays = 0;
    for (int k = 0; k < 7; ++k) a.cam[k] = 0.0f;
    for (int k = 0; k < 12; ++k) a.c2w[k] = 0.0f;
    return PNR_OK;
}

PNR_EXPORT int pnr_mesh_raycast(int model, const float* cam_host, const float* c2w12_host, int width, int height, float near_, float far_,
                                const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int res_x, int res_y,
                                int res_z, const float* lo_host, const float* cell_host, const int32_t* start, const float* records,
                                int64_t n_entries, float* depth, int32_t* face, uint8_t* code, float* bary, int32_t* vertex, float* normal,
                                int8_t* side, void* stream)
{
    PNR_REQUIRE(pnr_camera_model_ok(model), "pnr_mesh_raycast: unknown camera model %d", model);
    PNR_REQUIRE(cam_host && c2w12_host, "pnr_mesh_raycast: null camera or pose (cam_host, c2w12_host)");
    PNR_REQUIRE(width >= 1 && height >= 1 && (int64_t)width * height <= INT32_MAX,
                "pnr_mesh_raycast: bad image %d x %d (width, height >= 1, at most 2^31 - 1 pixels)", width, height);
    int rc = pnr_camera_check(model, cam_host, width, height, "pnr_mesh_raycast");
    if (rc) return rc;
    PNR_REQUIRE(near_ >= 0.0f && far_ > near_, "pnr_mesh_raycast: need 0 <= near < far");
    McArgs a;
    rc = mc_cast_check("pnr_mesh_raycast", vertices, n_vertices, faces, n_faces, res_x, res_y, res_z, lo_host, cell_host, start, records, n_entries,
                       depth, face, code, bary, vertex, normal, side, a);
    if (rc) return rc;
    a.model = model; a.width = width; a.height = height; a.near_ = near_; a.far_ = far_;
    pnr_camera_fill(model, cam_host, a.cam);
    pnr_pose_fill(c2w12_host, a.c2w);
    int64_t blocks;
    pnr_tile_grid(width, height, &a.tiles_x, &a.n_tiles, &blocks);
    hipLaunchKernelGGL(k_mesh_cast<true>, dim3((unsigned int)blocks), dim3(PNR_RAYCAST_BLOCK), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_mesh_raycast");
    return PNR_OK;
}

PNR_EXPORT int pnr_mesh_cast_rays(const float* rays, int64_t n_rays, const float* vertices, int64_t n_vertices, const int32_t* faces,
                                  int64_t n_faces, int res_x, int res_y, int res_z, const float* lo_host, const float* cell_host,
                                  const int32_t* start, const float* records, int64_t n_entries, float* depth, int32_t* face, uint8_t* code,
                                  float* bary, int32_t* vertex, float* normal, int8_t* side, void* stream)
{
    PNR_REQUIRE(n_rays >= 0 && n_rays <= (int64_t)INT32_MAX, "pnr_mesh_cast_rays: n_rays must be within 0 .. 2^31 - 1");
    if (n_rays == 0) return PNR_OK;
    PNR_REQUIRE(rays && ((uintptr_t)rays & 15) == 0, "pnr_mesh_cast_rays: rays must be non-null and 16-byte aligned");
    McArgs a;
    const int rc = mc_cast_check("pnr_mesh_cast_rays", vertices, n_vertices, faces, n_faces, res_x, res_y, res_z, lo_host, cell_host, start, records,
                                 n_entries, depth, face, code, bary, vertex, normal, side, a);
    if (rc) return rc;
    a.rays = rays; a.n_rays = n_rays;
    const int64_t blocks = (n_rays + PNR_RAYCAST_BLOCK - 1) / PNR_RAYCAST_BLOCK;
    hipLaunchKernelGGL(k_mesh_cast<false>, dim3((unsigned int)blocks), dim3(PNR_RAYCAST_BLOCK), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_mesh_cast_rays");
    return PNR_OK;
}
