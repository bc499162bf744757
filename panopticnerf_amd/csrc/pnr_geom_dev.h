// What the geometry kernels share beyond pnr_camera_dev.h, pnr_reduce_dev.h and pnr_scan_dev.h, each rule written once.  Host
// parts first, device parts under __HIPCC__: single + - * / operations in the order written (-ffp-contract=off).
#pragma once
#include "pnr_camera_dev.h"
#include "pnr_reduce_dev.h"
#include "pnr_scan_dev.h"

// ---- a view: model word, image size, the model's camera floats zero-padded, ONE pose (c2w to make rays, w2c to project)
struct PnrView { int model, width, height; float cam[7], pose[12]; };

// umax, vmax of pnr_uv_inside, called on the host: converted in the kernel, each holds a VGPR where it held an SGPR
static inline float pnr_view_umax(const PnrView& v) { return (float)v.width - 0.5f; }
static inline float pnr_view_vmax(const PnrView& v) { return (float)v.height - 0.5f; }

// a camera argument on the host: model word, pointers, image size, pnr_camera_check (`nonzero` is its switch), the fill of v;
// `side` ("src", "tgt", or NULL) follows `who` in the messages of a two-view entry point
static inline int pnr_view_check(const char* who, const char* side, int model, const float* cam_host, const float* pose_host, int width, int height,
                                 bool nonzero, PnrView& v)
{
    char label[96];
    snprintf(label, sizeof label, "%s%s%s", who, side ? ": " : "", side ? side : "");
    PNR_REQUIRE(pnr_camera_model_ok(model), "%s: unknown camera model %d", label, model);
    PNR_REQUIRE(cam_host && pose_host, "%s: null camera or pose", label);
    PNR_REQUIRE(width >= 1 && height >= 1, "%s: bad size: image %d x %d (width, height >= 1)", label, width, height);
    const int rc = pnr_camera_check(model, cam_host, width, height, label, nonzero);
    if (rc) return rc;
    v.model = model; v.width = width; v.height = height;
    pnr_camera_fill(model, cam_host, v.cam); pnr_pose_fill(pose_host, v.pose);
    return PNR_OK;
}

// ---- the ray casters' grid: a wave is an 8 x 8 pixel tile, a block PNR_RAYCAST_BLOCK / 64 tiles (at most 2^28 + 2^25 tiles)
static inline void pnr_tile_grid(int width, int height, unsigned int* tiles_x, int64_t* n_tiles, int64_t* blocks)
{
    const int64_t tx = ((int64_t)width + PNR_RAYCAST_TILE - 1) / PNR_RAYCAST_TILE, ty = ((int64_t)height + PNR_RAYCAST_TILE - 1) / PNR_RAYCAST_TILE;
    *tiles_x = (unsigned int)tx; *n_tiles = tx * ty;
    *blocks = (*n_tiles + PNR_RAYCAST_BLOCK / 64 - 1) / (PNR_RAYCAST_BLOCK / 64);
}

// ---- a table's workspace {header bytes | the scan's tile sums | an int32 cursor per cell, if any}: offsets, total rounded to 8
struct PnrTableWs { int64_t sums, cursor, bytes; };
static inline PnrTableWs pnr_table_carve(int64_t header_bytes, int64_t n_cells, bool cursors)
{
    const int64_t cursor = header_bytes + pnr_scan_workspace_bytes(n_cells);
    return PnrTableWs{header_bytes, cursor, (cursor + (cursors ? n_cells * 4 : 0) + 7) & ~(int64_t)7};
}

// ---- a mesh, and its host check; max_faces is 2^31 - 1, or 2^31 - 2 where n_faces + 1 int32 entries are scanned
struct PnrMesh { const float* vertices; int64_t n_vertices; const int32_t* faces; int64_t n_faces; };
static inline int pnr_mesh_check(const char* who, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t max_faces,
                                 PnrMesh& m)
{
    PNR_REQUIRE(n_vertices >= 0 && n_vertices <= (int64_t)INT32_MAX, "%s: n_vertices must be within 0 .. 2^31 - 1", who);
    PNR_REQUIRE(n_faces >= 0 && n_faces <= max_faces, "%s: n_faces must be within 0 .. 2^31 - %d", who, (int)(((int64_t)1 << 31) - max_faces));
    PNR_REQUIRE(n_faces == 0 || faces, "%s: null faces", who);
    PNR_REQUIRE(n_faces == 0 || n_vertices == 0 || vertices, "%s: null vertices", who);
    PNR_REQUIRE((((uintptr_t)vertices | (uintptr_t)faces) & 3) == 0, "%s: vertices and faces must be 4-byte aligned", who);
    m.vertices = vertices; m.n_vertices = n_vertices; m.faces = faces; m.n_faces = n_faces;
    return PNR_OK;
}

// ---- a lattice: every res >= min_res, at most max_points points, lo and step finite, step non-zero where it is divided by
static inline int pnr_lattice_check(const char* who, int res_x, int res_y, int res_z, const float* lo_host, const float* step_host, int min_res,
                                    int64_t max_points, bool nonzero_step)
{
    PNR_REQUIRE(res_x >= min_res && res_y >= min_res && res_z >= min_res && (int64_t)res_x * res_y <= max_points && (int64_t)res_x * res_y * res_z <= max_points,
                "%s: bad lattice %d x %d x %d (every res >= %d, at most %lld points)", who, res_x, res_y, res_z, min_res, (long long)max_points);
    PNR_REQUIRE(lo_host && step_host, "%s: null lo or step", who);
    for (int k = 0; k < 3; ++k)
        PNR_REQUIRE(isfinite(lo_host[k]) && isfinite(step_host[k]) && (step_host[k] != 0.0f || !nonzero_step),
                    "%s: lo and step must be finite%s (axis %d)", who, nonzero_step ? " and step non-zero" : "", k);
    return PNR_OK;
}

#ifdef __HIPCC__
// ---- keys under a 64-bit minimum: the value is not negative and not NaN, so its bits order as it does; a tie goes to the index
#define PNR_KEY_EMPTY 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ unsigned long long pnr_key(float value, unsigned int index) { return ((unsigned long long)__float_as_uint(value) << 32) | index; }
__device__ __forceinline__ float pnr_key_value(unsigned long long key) { return __uint_as_float((unsigned int)(key >> 32)); }
__device__ __forceinline__ unsigned int pnr_key_index(unsigned long long key) { return (unsigned int)key; }

// ---- the entries [s, e) of `cell` (a hash bucket or a grid cell, in the caller's index type) of a scanned table, clamped to
// [0, n32]: a damaged table reads inside
struct PnrRange { int s, e; };
template <class Cell>
__device__ __forceinline__ PnrRange pnr_table_range(const int32_t* start, Cell cell, int n32)
{
    const int s = min(max(start[cell], 0), n32);
    return PnrRange{s, min(max(start[cell + 1], s), n32)};
}

// ---- lattice point i (converted by the caller from its own index type) on one axis: a multiply, then an add, never an FMA
__device__ __forceinline__ float pnr_lattice_coord(float i, float lo, float step) { return (i + 0.5f) * step + lo; }

// ---- c = a x b
__device__ __forceinline__ void pnr_cross3(const float (&a)[3], const float (&b)[3], float (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
#endif
