// Pose tracking (include/pnr.h "pose tracking"): point-to-plane ICP of a live depth frame against a model view with depth and
// world-space normals, as k_tsdf_raycast writes them.  k_icp_accumulate is one linearisation: per live pixel the projective
// association (the ray of pnr_camera_ray, the projection of pnr_project_point -- pnr_camera_dev.h, the functions the ray,
// reprojection and fusion kernels call, so the arithmetic is theirs bit for bit), the gates and the Jacobian row in float32, and
// the 28 sums of the normal equations in double, reduced in the one stated order (pnr_reduce_dev.h; DESIGN.md section 8 "Ordered
// reductions"): one row of partials per workgroup, no floating atomics.  k_icp_solve is one workgroup: it adds the rows in block
// order, factorises, and updates the pose where it lives, in device memory, so K iterations are 2K launches with no host read
// between them.  tests/_icp_ref.py restates both.
#include <float.h>

#include "pnr_camera_dev.h"
#include "pnr_common.h"
#include "pnr_reduce_dev.h"

struct IcpArgs {
    int model_l, model_m;
    float cam_l[7], cam_m[7];
    float c2w_m[12], w2c_m[12];
    int width_l, width_m, height_m;
    int64_t npix;
    float umax, vmax, dist2;
    const float *depth_l, *pose, *depth_m, *normal_m;
    uint8_t* code;
    float* residual;
    unsigned long long* ws;             // slot 0: the rows written; then [blocks][PNR_ICP_ROW]
};

__global__ __launch_bounds__(PNR_REDUCE_BLOCK) void k_icp_accumulate(const IcpArgs a)
{
    __shared__ double red[4][PNR_ICP_SUMS];
    __shared__ unsigned int redc[4];
    const float ident[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    float P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = a.pose[k];
    double s[PNR_ICP_SUMS];
#pragma unroll
    for (int k = 0; k < PNR_ICP_SUMS; ++k) s[k] = 0.0;
    unsigned int cnt = 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.npix; q += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(q / a.width_l), i = (int)(q - (int64_t)j * a.width_l);
        int code = PNR_ICP_NO_DEPTH;
        float r = 0.0f;
        bool ok;
        const PnrRayRec ray = pnr_camera_ray(a.model_l, a.cam_l, ident, i, j, 0.0f, 0.0f, ok);
        const float t = a.depth_l[q];
        if (ok && pnr_pos_finite(t)) {
            const float x = t * ray.lo.w, y = t * ray.hi.x, z = t * ray.hi.y;
            float qv[3], p[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float u = P[k * 4 + 0] * x, v = P[k * 4 + 1] * y, w = P[k * 4 + 2] * z;
                qv[k] = (u + v) + w;
                p[k] = qv[k] + P[k * 4 + 3];
            }
            const PnrProj pr = pnr_project_point(a.model_m, a.cam_m, a.w2c_m, a.umax, p[0], p[1], p[2]);
            code = PNR_ICP_OUTSIDE;
            if (pr.dom && pnr_uv_inside(pr.u, pr.v, a.umax, a.vmax)) {
                const int ia = pnr_nearest_pixel(pr.u, a.width_m - 1), ib = pnr_nearest_pixel(pr.v, a.height_m - 1);
                const int64_t mq = (int64_t)ib * a.width_m + ia;
                const float dm = a.depth_m[mq];
                const float nx = a.normal_m[mq * 3 + 0], ny = a.normal_m[mq * 3 + 1], nz = a.normal_m[mq * 3 + 2];
                // pnr_finite3's test written out: called here, the same test holds four more registers (95 -> 99 VGPRs, a wave
                // less per SIMD) and the launch measures 1 us (5 %) slower
                const bool nfin = fabsf(nx) <= FLT_MAX && fabsf(ny) <= FLT_MAX && fabsf(nz) <= FLT_MAX;
                code = PNR_ICP_NO_MODEL;
                if (pnr_pos_finite(dm) && nfin && (nx != 0.0f || ny != 0.0f || nz != 0.0f)) {
                    bool okm;
                    const PnrRayRec rm = pnr_camera_ray(a.model_m, a.cam_m, a.c2w_m, ia, ib, 0.0f, 0.0f, okm);
                    if (okm) {
                        const float mx = rm.lo.x + dm * rm.lo.w, my = rm.lo.y + dm * rm.hi.x, mz = rm.lo.z + dm * rm.hi.y;
                        const float ex = mx - p[0], ey = my - p[1], ez = mz - p[2];
                        const float e2 = (ex * ex + ey * ey) + ez * ez;
                        code = PNR_ICP_TOO_FAR;
                        if (e2 <= a.dist2) {
                            const float facing = (nx * qv[0] + ny * qv[1]) + nz * qv[2];
                            code = PNR_ICP_BACK_FACING;
                            if (!(facing >= 0.0f)) {
                                code = PNR_ICP_MATCH;
                                r = (nx * ex + ny * ey) + nz * ez;
                                const float cx = qv[1] * nz - qv[2] * ny;
                                const float cy = qv[2] * nx - qv[0] * nz;
                                const float cz = qv[0] * ny - qv[1] * nx;
                                const double J[6] = {(double)cx, (double)cy, (double)cz, (double)nx, (double)ny, (double)nz};
                                const double rd = (double)r;
                                int n = 0;
#pragma unroll
                                for (int c0 = 0; c0 < 6; ++c0)
#pragma unroll
                                    for (int c1 = c0; c1 < 6; ++c1) s[n++] += J[c0] * J[c1];
#pragma unroll
                                for (int c0 = 0; c0 < 6; ++c0) s[21 + c0] += J[c0] * rd;
                                s[27] += rd * rd;
                                cnt += 1u;
                            }
                        }
                    }
                }
            }
        }
        if (a.code) a.code[q] = (uint8_t)code;
        if (a.residual) a.residual[q] = r;
    }
    // the row: 28 sums, then the count, whose four wave sums go to LDS before the sums' barrier, which covers them
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = cnt;
    pnr_block_sum_rows(s, red, (double*)(a.ws + 1), PNR_ICP_ROW);
    if (threadIdx.x == PNR_ICP_SUMS) a.ws[1 + (int64_t)blockIdx.x * PNR_ICP_ROW + PNR_ICP_SUMS] = (unsigned long long)redc[0] + redc[1] + redc[2] + redc[3];
    if (blockIdx.x == 0 && threadIdx.x == PNR_ICP_SUMS + 1) a.ws[0] = (unsigned long long)gridDim.x;
}

struct IcpSolveArgs {
    const unsigned long long* ws;
    int max_rows;
    long long min_matches;
    double max_rot2, max_trans2;
    int update;
    float* pose;
    double* hist;
};

// (-1)^k / (2k + 1)! and (-1)^k / (2k + 2)!: quotients of 1.0 and an exact integer, folded by the compiler (correctly rounded)
#define ICP_CA(k, f) ((k) % 2 ? -1.0 : 1.0) / (f)
__device__ __forceinline__ double icp_series_a(double s)
{
    double a = ICP_CA(7, 1307674368000.0);
    a = a * s + ICP_CA(6, 6227020800.0);
    a = a * s + ICP_CA(5, 39916800.0);
    a = a * s + ICP_CA(4, 362880.0);
    a = a * s + ICP_CA(3, 5040.0);
    a = a * s + ICP_CA(2, 120.0);
    a = a * s + ICP_CA(1, 6.0);
    a = a * s + ICP_CA(0, 1.0);
    return a;
}

__device__ __forceinline__ double icp_series_b(double s)
{
    double b = ICP_CA(7, 20922789888000.0);
    b = b * s + ICP_CA(6, 87178291200.0);
    b = b * s + ICP_CA(5, 479001600.0);
    b = b * s + ICP_CA(4, 3628800.0);
    b = b * s + ICP_CA(3, 40320.0);
    b = b * s + ICP_CA(2, 720.0);
    b = b * s + ICP_CA(1, 24.0);
    b = b * s + ICP_CA(0, 2.0);
    return b;
}

__global__ __launch_bounds__(64) void k_icp_solve(const IcpSolveArgs a)
{
    __shared__ double tot[PNR_ICP_SUMS];
    __shared__ unsigned long long totc;
    const unsigned long long stored = a.ws[0];
    const int rows = stored < (unsigned long long)a.max_rows ? (int)stored : a.max_rows;      // (never past the workspace)
    // lane s adds slot s of the rows in block order: the sums' lanes as doubles, the count's lane as integers
    if (threadIdx.x < PNR_ICP_ROW) {
        const PnrRowsTotal t = pnr_rows_total<PNR_ICP_ROW>(a.ws + 1, rows, threadIdx.x);
        if (threadIdx.x < PNR_ICP_SUMS) tot[threadIdx.x] = t.sum;
        else totc = t.words;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long count = (long long)totc;
    double w2 = 0.0, v2 = 0.0;
    int status = PNR_ICP_OK;
    if (count < a.min_matches) {
        status = PNR_ICP_TOO_FEW;
    } else if (a.update) {
        double A[6][6], L[6][6], g[6], y[6], x[6];
        int n = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                A[i][j] = tot[n];
                A[j][i] = tot[n];
                ++n;
            }
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = tot[21 + i];
        bool degenerate = false;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double t = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - L[j][k] * L[j][k];
            if (!(t > 0x1p-30 * A[j][j])) degenerate = true;
            L[j][j] = sqrt(t);
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double u = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) u = u - L[i][k] * L[j][k];
                L[i][j] = u / L[j][j];
            }
        }
        if (degenerate) {
            status = PNR_ICP_DEGENERATE;
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double t = g[i];
#pragma unroll
                for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
                y[i] = t / L[i][i];
            }
#pragma unroll
            for (int i = 5; i >= 0; --i) {
                double t = y[i];
#pragma unroll
                for (int k = i + 1; k < 6; ++k) t = t - L[k][i] * x[k];
                x[i] = t / L[i][i];
            }
            w2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
            v2 = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5];
            if (!(w2 <= a.max_rot2 && v2 <= a.max_trans2)) {
                status = PNR_ICP_STEP_TOO_LARGE;
            } else {
                const double sa = icp_series_a(w2), sb = icp_series_b(w2);
                const double K[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
                double D[3][3], R[3][4];
#pragma unroll
                for (int k = 0; k < 12; ++k) R[k / 4][k % 4] = (double)a.pose[k];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        D[i][j] = i == j ? 1.0 + sb * (x[i] * x[i] - w2) : sa * K[i][j] + sb * (x[i] * x[j]);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) a.pose[i * 4 + j] = (float)((D[i][0] * R[0][j] + D[i][1] * R[1][j]) + D[i][2] * R[2][j]);
                    a.pose[i * 4 + 3] = (float)(R[i][3] + x[3 + i]);
                }
            }
        }
    }
    a.hist[0] = (double)count;
    a.hist[1] = tot[27];
    a.hist[2] = w2;
    a.hist[3] = v2;
    a.hist[4] = (double)status;
}

static int64_t icp_blocks(int64_t n_pix) { return pnr_reduce_blocks(n_pix, PNR_ICP_MAX_BLOCKS); }

PNR_EXPORT int64_t pnr_icp_workspace_bytes(int64_t n_pix)
{
    if (n_pix < 1 || n_pix > (int64_t)INT32_MAX) return -1;
    return (1 + icp_blocks(n_pix) * PNR_ICP_ROW) * (int64_t)sizeof(double);
}

PNR_EXPORT int pnr_icp_accumulate(int model_l, const float* cam_l_host, int width_l, int height_l, const float* depth_l, const float* pose12,
                                  int model_m, const float* cam_m_host, const float* c2w_m12_host, const float* w2c_m12_host, int width_m,
                                  int height_m, const float* depth_m, const float* normal_m, float dist_max, void* workspace, uint8_t* code,
                                  float* residual, void* stream)
{
    PNR_REQUIRE(pnr_camera_model_ok(model_l) && pnr_camera_model_ok(model_m), "pnr_icp_accumulate: unknown camera model %d -> %d", model_l, model_m);
    PNR_REQUIRE(cam_l_host && cam_m_host && c2w_m12_host && w2c_m12_host, "pnr_icp_accumulate: null camera or model pose");
    PNR_REQUIRE(width_l >= 1 && height_l >= 1 && width_m >= 1 && height_m >= 1 && (int64_t)width_l * height_l <= INT32_MAX &&
                (int64_t)width_m * height_m <= INT32_MAX, "pnr_icp_accumulate: bad size (each image holds 1 .. 2^31 - 1 pixels)");
    int rc = pnr_camera_check(model_l, cam_l_host, width_l, height_l, "pnr_icp_accumulate: live");
    if (!rc) rc = pnr_camera_check(model_m, cam_m_host, width_m, height_m, "pnr_icp_accumulate: model");
    if (rc) return rc;
    PNR_REQUIRE(depth_l && pose12 && depth_m && normal_m && workspace, "pnr_icp_accumulate: null depth_l, pose12, depth_m, normal_m or workspace");
    PNR_REQUIRE((((uintptr_t)depth_l | (uintptr_t)pose12 | (uintptr_t)depth_m | (uintptr_t)normal_m | (uintptr_t)residual) & 3) == 0,
                "pnr_icp_accumulate: depth_l, pose12, depth_m, normal_m and residual must be 4-byte aligned");
    PNR_REQUIRE((((uintptr_t)workspace) & 7) == 0, "pnr_icp_accumulate: workspace must be 8-byte aligned");
    const float dist2 = dist_max * dist_max;
    PNR_REQUIRE(dist_max > 0.0f && dist2 <= FLT_MAX, "pnr_icp_accumulate: dist_max must be positive with a finite square");
    IcpArgs a;
    a.model_l = model_l; a.model_m = model_m;
    pnr_camera_fill(model_l, cam_l_host, a.cam_l);
    pnr_camera_fill(model_m, cam_m_host, a.cam_m);
    pnr_pose_fill(c2w_m12_host, a.c2w_m);
    pnr_pose_fill(w2c_m12_host, a.w2c_m);
    a.width_l = width_l; a.width_m = width_m; a.height_m = height_m; a.npix = (int64_t)width_l * height_l;
    a.umax = (float)width_m - 0.5f; a.vmax = (float)height_m - 0.5f; a.dist2 = dist2;
    a.depth_l = depth_l; a.pose = pose12; a.depth_m = depth_m; a.normal_m = normal_m;
    a.code = code; a.residual = residual; a.ws = (unsigned long long*)workspace;
    const int grid = pnr_grid_cap(icp_blocks(a.npix), 1);         // (never above icp_blocks: the workspace holds it)
    hipLaunchKernelGGL(k_icp_accumulate, dim3(grid), dim3(PNR_REDUCE_BLOCK), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_icp_accumulate");
    return PNR_OK;
}

PNR_EXPORT int pnr_icp_solve(const void* workspace, int64_t n_pix, int64_t min_matches, float max_rot, float max_trans, int update,
                             float* pose12, double* history_row, void* stream)
{
    PNR_REQUIRE(workspace && pose12 && history_row, "pnr_icp_solve: null workspace, pose12 or history row");
    PNR_REQUIRE((((uintptr_t)workspace | (uintptr_t)history_row) & 7) == 0 && (((uintptr_t)pose12) & 3) == 0,
                "pnr_icp_solve: workspace and history must be 8-byte aligned, pose12 4-byte");
    PNR_REQUIRE(n_pix >= 1 && n_pix <= (int64_t)INT32_MAX, "pnr_icp_solve: bad size (n_pix in 1 .. 2^31 - 1)");
    PNR_REQUIRE(min_matches >= 1, "pnr_icp_solve: min_matches must be >= 1");
    PNR_REQUIRE(max_rot > 0.0f && max_rot <= PNR_ICP_MAX_ROT, "pnr_icp_solve: max_rot must lie in (0, %g] radians", (double)PNR_ICP_MAX_ROT);
    PNR_REQUIRE(max_trans > 0.0f, "pnr_icp_solve: max_trans must be positive (it may be inf)");
    IcpSolveArgs a;
    a.ws = (const unsigned long long*)workspace; a.max_rows = (int)icp_blocks(n_pix); a.min_matches = min_matches;
    a.max_rot2 = (double)max_rot * (double)max_rot; a.max_trans2 = (double)max_trans * (double)max_trans;
    a.update = update; a.pose = pose12; a.hist = history_row;
    hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_icp_solve");
    return PNR_OK;
}
