// Training frames (include/pnr.h "training frames"): one kernel draws a ray batch from a device-resident table of posed images --
// the (frame, pixel) draw from the in-kernel Philox stream, the ray of that camera and pixel (pnr_camera_ray of
// pnr_camera_dev.h: the bits of k_gen_rays<model>, pnr_camera.hip) and the gathered targets.  One thread per ray, grid-stride; per ray one Philox call, a binary
// search over the frame prefix sums, a 144-byte record read and up to five dependent gathers: latency- and gather-bound at the
// few thousand rays of a training step.  The table (records, prefix sums, frame count) is read when the kernel runs.
#include "pnr_camera_dev.h"
#include "pnr_common.h"
#include "pnr_philox.h"

static_assert(sizeof(pnr_frame) == 144 && sizeof(pnr_frame) % 16 == 0, "pnr_frame: the layout include/pnr.h documents");

struct SampleBatchArgs {
    const pnr_frame* frames; const int64_t* cum; const int32_t* n_frames; int mode; PnrRngDev rng; int64_t R;
    float* rays; float* rgb; float* depth; int32_t* sem; int32_t* inst; int32_t* frame_out; int32_t* pix_out;
};

__device__ __forceinline__ uint64_t pnr_word64(const pnr_u4& v) { return ((uint64_t)v.x << 32) | v.y; }

__global__ __launch_bounds__(256) void k_sample_batch(const SampleBatchArgs a)
{
    const PnrRngKey key = pnr_rng_key(a.rng);
    const int F = a.n_frames[0];
    // mode 1: the call's frame, from global ray 0 of the frame stream (PNR_TAG_FRAME) whatever ray_base is
    int f1 = -1;
    if (a.mode == PNR_SAMPLE_FRAME && F > 0) {
        const pnr_u4 v = pnr_philox4x32_10(pnr_u4{(uint32_t)PNR_TAG_FRAME << 24, 0u, key.off_lo, key.off_hi}, key.k0, key.k1);
        f1 = (int)__umul64hi(pnr_word64(v), (uint64_t)F);
    }
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t W = pnr_word64(pnr_rng_block(key, (uint32_t)r, 0u));
        int f = -1;
        int64_t k = 0;
        if (a.mode == PNR_SAMPLE_FRAME) {
            const int64_t n = f1 >= 0 ? a.frames[f1].n_valid : 0;
            if (n > 0) { f = f1; k = (int64_t)__umul64hi(W, (uint64_t)n); }
        } else {
            const int64_t n = F > 0 ? a.cum[F] : 0;
            if (n > 0) {
                const int64_t idx = (int64_t)__umul64hi(W, (uint64_t)n);
                int lo = 0, hi = F;                   // the last f in [0, F) with cum[f] <= idx (cum[0] = 0 <= idx < cum[F])
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (a.cum[mid] <= idx) lo = mid; else hi = mid;
                }
                f = lo;
                k = idx - a.cum[f];
            }
        }
        PnrRayRec ray{make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, dep = 0.0f;
        int32_t ls = -1, li = -1, p = -1;
        if (f >= 0) {
            const pnr_frame& fr = a.frames[f];
            const int32_t* vp = reinterpret_cast<const int32_t*>(fr.valid_pix);
            p = vp ? vp[k] : (int32_t)k;
            const int j = p / fr.width, i = p - j * fr.width;
            bool ok;                                // (a frame's valid_pix holds no pixel outside the lens)
            ray = pnr_camera_ray(fr.model, fr.cam, fr.c2w, i, j, fr.near_, fr.far_, ok);
            if (a.rgb) {
                const uint8_t* px = reinterpret_cast<const uint8_t*>(fr.rgb) + (int64_t)p * 3;
                c0 = (float)px[0] / 255.0f; c1 = (float)px[1] / 255.0f; c2 = (float)px[2] / 255.0f;
            }
            if (a.depth && fr.depth) dep = reinterpret_cast<const float*>(fr.depth)[p];
            if (a.sem && fr.sem) ls = reinterpret_cast<const int16_t*>(fr.sem)[p];
            if (a.inst && fr.inst) li = reinterpret_cast<const int16_t*>(fr.inst)[p];
        }
        if (a.rays) {
            float4* o = reinterpret_cast<float4*>(a.rays + r * 8);
            o[0] = ray.lo;
            o[1] = ray.hi;
        }
        if (a.rgb) { a.rgb[r * 3 + 0] = c0; a.rgb[r * 3 + 1] = c1; a.rgb[r * 3 + 2] = c2; }
        if (a.depth) a.depth[r] = dep;
        if (a.sem) a.sem[r] = ls;
        if (a.inst) a.inst[r] = li;
        if (a.frame_out) a.frame_out[r] = f;
        if (a.pix_out) a.pix_out[r] = p;
    }
}

PNR_EXPORT int pnr_sample_batch(const pnr_frame* frames, const int64_t* cum, const int32_t* n_frames, int mode, const pnr_rng* rng_host,
                                int64_t n_rays, float* rays, float* rgb, float* depth, int32_t* sem, int32_t* inst, int32_t* frame_out,
                                int32_t* pix_out, void* stream)
{
    PNR_REQUIRE(frames && cum && n_frames, "pnr_sample_batch: null frame table");
    PNR_REQUIRE((((uintptr_t)frames) & 15) == 0 && (((uintptr_t)cum) & 7) == 0 && (((uintptr_t)n_frames) & 3) == 0,
                "pnr_sample_batch: misaligned frame table (frames 16, cum 8, n_frames 4 bytes)");
    PNR_REQUIRE(mode == PNR_SAMPLE_POOLED || mode == PNR_SAMPLE_FRAME, "pnr_sample_batch: unknown mode %d", mode);
    PnrRngDev rng;
    const int rc = pnr_rng_check(rng_host, n_rays, "pnr_sample_batch", &rng);
    if (rc) return rc;
    PNR_REQUIRE(rng_host->tag == PNR_TAG_PIXEL, "pnr_sample_batch: tag clash: the pixel stream is tag %d (the frame stream %d; 1 .. 15 are the render streams'), got %d",
                PNR_TAG_PIXEL, PNR_TAG_FRAME, (int)rng_host->tag);
    if (n_rays == 0) return PNR_OK;
    PNR_REQUIRE((((uintptr_t)rays) & 15) == 0, "pnr_sample_batch: rays must be a 16-byte aligned device buffer");
    SampleBatchArgs a;
    a.frames = frames; a.cum = cum; a.n_frames = n_frames; a.mode = mode; a.rng = rng; a.R = n_rays;
    a.rays = rays; a.rgb = rgb; a.depth = depth; a.sem = sem; a.inst = inst; a.frame_out = frame_out; a.pix_out = pix_out;
    hipLaunchKernelGGL(k_sample_batch, dim3(pnr_grid_cap((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PNR_CHECK_LAUNCH("pnr_sample_batch");
    return PNR_OK;
}
