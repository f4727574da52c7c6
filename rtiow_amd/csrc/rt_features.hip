// rt_features.hip -- first-hit feature buffers: albedo, normal, depth, hit count and object id (rtiow_hip.h, "feature buffers";
// DESIGN.md section 14).
//
// The third translation unit of librtiow_hip.so.  It owns ONE kernel of its own, rt::features_kernel, which traces the camera rays of a
// dense render -- bounce 0 of ray_color, main.rs:131-134 + HittableList::hit mod.rs:54-70 -- and keeps the hit record the render
// kernel throws away, and the small kernel that turns the exact sums into what a denoiser takes.  It reads the tables rt_upload_scene
// built (rt_host::set_scene_params); the first-hit scan itself is rt_first_hit.hpp, which the ray queries of rt_trace.hip share.
// rt_kernels.hpp, rt_device.hpp, rt_api.hip and rt_diag.hpp are untouched, so every render kernel keeps its machine code.
//
// Shape of the kernel (simple on purpose): one wave covers an 8 x 8 pixel tile, a lane owns one pixel and loops over its samples
// with the eight sums in registers; no atomics, no LDS sums, no work queue.  Per sample: the camera ray, the shared scan in its `wave`
// scheme with t_max = +inf (first_hit_wave: the 64 rays of a pixel tile are coherent, which keeps its superset small;
// -DRT_FEATURES_COUNT counts it), the quantised sums of the winner's record.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_host.hpp"
#ifdef RT_FEATURES_COUNT
#define RT_SCAN_COUNT               // rt_first_hit.hpp: the scan's diagnostic counters (tools/features_bench.py --counts)
#endif
#include "rt_first_hit.hpp"

using namespace rt_host;

namespace rt {

constexpr int kFeatBlock = 256;                     // four waves, each on pixel tiles of its own
constexpr int kFeatWaves = kFeatBlock / 64;

struct FeatArgs {
    unsigned long long *feat;       // [height][width][8] exact sums
    int32_t *ids;                   // [height][width] list index of the first sample's hit, or NULL
    int32_t accumulate;             // 1: add to feat (RT_FLAG_ACCUMULATE)
    uint32_t tiles_x;               // pixel tiles per row of tiles: ceil(width / 8)
    uint32_t n_wtiles;              // tiles_x * ceil(height / 8)
};

// a normal's component on the 2^-32 grid, signed: 0 for a NaN, else floor(clamp(x, -2^16, 2^16) * 2^32) as a two's-complement
// integer (the product with 2^32 is exact; |value| <= 2^48)
__device__ __forceinline__ unsigned long long quantize_signed(double x)
{
    if (x != x) return 0ull;
    x = __builtin_fmin(__builtin_fmax(x, -65536.0), 65536.0);
    return (unsigned long long)(long long)__builtin_floor(x * 4294967296.0);
}

__global__ __launch_bounds__(kFeatBlock) void features_kernel(const KParams P, const FeatArgs F)
{
    __shared__ uint4 s_stage[kFeatWaves][64 * 4];
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const double wm1 = (double)(P.width - 1), hm1 = (double)(P.height - 1);
    const uint32_t n_waves = gridDim.x * (uint32_t)kFeatWaves;

    for (uint32_t wt = blockIdx.x * (uint32_t)kFeatWaves + (uint32_t)wave; wt < F.n_wtiles; wt += n_waves) {
        const uint32_t ty = wt / F.tiles_x, tx = wt - ty * F.tiles_x;
        const int i = (int)(tx * 8u) + (lane & 7), j = (int)(ty * 8u) + (lane >> 3);
        // lanes past the right or top edge stay in the wave: rows that keep nothing, nothing written
        const bool valid = i < P.width && j < P.height;
        const uint32_t g_pix = (uint32_t)j * (uint32_t)P.width + (uint32_t)i;
        unsigned long long sum[RT_FEATURE_WORDS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
        int first_id = -1;
        ScanCounts cnt = {false};

        for (int s = 0; s < P.spp; ++s) {
            // ---- the camera ray of (pixel, sample): main.rs:131-134, camera.rs:47-54 -- the render kernel's own start of a sample
            D3 o = mk(0.0, 0.0, 0.0), d = mk(0.0, 0.0, 0.0);
            if (valid) {
                const uint32_t g_s = (uint32_t)P.sample_begin + (uint32_t)s;
                U4 w = philox4x32_10(g_pix, g_s, 0u, 0u, P.k0, P.k1);
                uint32_t ev = 1u;
                const double cu = ((double)i + u01(w.x)) / wm1;                 // main.rs:131
                const double cv = ((double)j + u01(w.y)) / hm1;                 // main.rs:132
                // vec3.rs:59-68: block 0 = (u jitter, v jitter, lens x, lens y); every further block holds two tries
                uint32_t wx = w.z, wy = w.w;
                while (!unit_disk_accepts(wx, wy)) {
                    w = philox4x32_10(g_pix, g_s, ev, 0u, P.k0, P.k1);
                    ev++;
                    wx = w.x; wy = w.y;
                    if (!unit_disk_accepts(wx, wy)) { wx = w.z; wy = w.w; }
                }
                const D3 cam_origin = ld3(P.cam.origin);
                const D3 rd = mk(u11(wx), u11(wy), 0.0) * P.cam.lens_radius;
                const D3 offset = ld3(P.cam.u) * rd.x + ld3(P.cam.v) * rd.y;
                o = cam_origin + offset;
                d = (((ld3(P.cam.llc) + ld3(P.cam.horizontal) * cu) + ld3(P.cam.vertical) * cv) - cam_origin) - offset;
            }

            // ---- HittableList::hit, mod.rs:54-70, with t_max = +inf
            FirstHit fh = {__builtin_inf(), -1};
            first_hit_wave<false>(P, s_stage[wave], lane, o, d, valid, fh, cnt);

            // ---- the hit record: sphere.rs:36-37 + mod.rs:20-30; the material only for the winner
            if (valid && fh.hit >= 0) {
                const HitRecord rec = hit_record(P, o, d, fh);
                // by KIND: a Dialectric's attenuation is (1, 1, 1) (materials.rs:103), whatever the flat scene's albedo field holds
                const bool glass = (int)rec.mrec[5] == RT_KIND_DIALECTRIC;
                sum[0] += quantize(glass ? 1.0 : rec.mrec[2]);
                sum[1] += quantize(glass ? 1.0 : rec.mrec[3]);
                sum[2] += quantize(glass ? 1.0 : rec.mrec[4]);
                sum[3] += quantize_signed(rec.normal.x);
                sum[4] += quantize_signed(rec.normal.y);
                sum[5] += quantize_signed(rec.normal.z);
                sum[6] += quantize(fh.closest);
                sum[7] += 1ull;
            }
            if (s == 0) first_id = fh.hit;
        }

        if (valid) {
            unsigned long long *out = F.feat + (size_t)g_pix * RT_FEATURE_WORDS;
#pragma unroll
            for (int k = 0; k < RT_FEATURE_WORDS; ++k) out[k] = F.accumulate ? out[k] + sum[k] : sum[k];
            if (F.ids) F.ids[g_pix] = first_id;
        }
        flush_counts(cnt);
    }
}

// exact sum -> f64 value, hi/lo form (rt_api.hip, fix_to_f64)
__device__ __forceinline__ double feat_fix_to_f64(unsigned long long q)
{
    return ((double)(uint32_t)(q >> 32) * 4294967296.0 + (double)(uint32_t)q) * (1.0 / 4294967296.0);
}

__global__ void features_to_f32_kernel(const unsigned long long *__restrict__ feat, float *__restrict__ out, long long npix, double spp)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; k < npix; k += stride) {
        const unsigned long long *q = feat + RT_FEATURE_WORDS * k;
        float *o = out + RT_FEATURE_WORDS * k;
        for (int c = 0; c < 3; ++c) o[c] = (float)(feat_fix_to_f64(q[c]) / spp);
        for (int c = 3; c < 6; ++c) {
            const bool neg = (long long)q[c] < 0;
            const double v = feat_fix_to_f64(neg ? 0ull - q[c] : q[c]);
            o[c] = (float)((neg ? -v : v) / spp);
        }
        const unsigned long long hits = q[7];
        o[6] = hits ? (float)(feat_fix_to_f64(q[6]) / (double)hits) : 0.0f;
        o[7] = (float)((double)hits / spp);
    }
}

} // namespace rt

namespace {

// The start of both forms of a feature launch.  What it accepts beyond validate_params is checked before anything is touched: the checks
// that need no context come first (a caller without a device still gets the precise message), then the context's own; then the device.
int begin_features(const rt_context *ctx, const rt_camera *cam, const rt_params *p, const void *feat)
{
    int rc = validate_params(p);
    if (rc) return rc;
    if (p->flags & (RT_FLAG_UNIFORM53 | RT_FLAG_DIAG_STATS | RT_FLAG_NO_FILTER))
        return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers come from a kernel of their own: RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS and "
                    "RT_FLAG_NO_FILTER are not available on them (flags 0x%x)", p->flags);
    if (p->shard_count != 1)
        return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers are not sharded: shard_count must be 1 (is %d)", p->shard_count);
    if (p->spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers need spp >= 1 (is %d)", p->spp);
    if (!cam) return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers: cam is NULL");
    if (!feat) return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers: the feature buffer is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->scan_mode != 5)
        return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers need the shipped scan mode 5; this context was created under RTIOW_SCAN_MODE=%d", ctx->scan_mode);
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    RT_HIP(hipSetDevice(ctx->device));
    return RT_OK;
}

int validate_to_f32(const rt_context *ctx, const void *feat, int32_t width, int32_t rows, int64_t spp, const void *out)
{
    if (width < 1 || rows < 0 || spp < 1)
        return fail(RT_ERR_INVALID_ARGUMENT, "features to f32: bad width/rows/spp (%d, %d, %lld)", width, rows, (long long)spp);
    if (rows > 0 && (!feat || !out)) return fail(RT_ERR_INVALID_ARGUMENT, "features to f32: a buffer is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return RT_OK;
}

} // namespace

extern "C" {

// bounce 0 of main.rs:122-136: the first hit of every camera ray
int rt_render_features_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, void *d_feat, void *d_ids, void *stream_v)
{
    int rc = begin_features(ctx, cam, p, d_feat);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_v;

    rt::KParams kp;
    memset(&kp, 0, sizeof(kp));
    static_assert(sizeof(kp.cam) == sizeof(rt_camera), "camera layouts must match");
    memcpy(&kp.cam, cam, sizeof(rt_camera));
    kp.width = p->width; kp.height = p->height;
    kp.spp = p->spp; kp.sample_begin = p->sample_begin;
    kp.t_min = p->t_min;
    kp.k0 = (uint32_t)p->seed; kp.k1 = (uint32_t)(p->seed >> 32);
    kp.rows = p->height; kp.n_spheres = ctx->n_spheres;
    set_scene_params(ctx, kp);
    // (no launch slot: the kernel has no work counter and no statistics words, and rt_last_stats does not report on it)
    rt::FeatArgs fa;
    fa.feat = (unsigned long long *)d_feat;
    fa.ids = (int32_t *)d_ids;
    fa.accumulate = (p->flags & RT_FLAG_ACCUMULATE) ? 1 : 0;
    fa.tiles_x = ((uint32_t)p->width + 7u) / 8u;
    fa.n_wtiles = fa.tiles_x * (((uint32_t)p->height + 7u) / 8u);
    // one wave per pixel tile (tiles of sky are cheap, tiles of spheres are not)
    const long long grid = rt::wave_grid(fa.n_wtiles, rt::kFeatWaves);
    hipLaunchKernelGGL(rt::features_kernel, dim3((unsigned)grid), dim3(rt::kFeatBlock), 0, stream, kp, fa);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_render_features(rt_context *ctx, const rt_camera *cam, const rt_params *p, uint64_t *out_feat, int32_t *out_ids, float *kernel_ms)
{
    int rc = begin_features(ctx, cam, p, out_feat);
    if (rc) return rc;
    const size_t npix = (size_t)p->width * p->height;
    Stage st(ctx);
    const auto feat = st.out(out_feat, npix * RT_FEATURE_WORDS);
    const auto ids = st.out(out_ids, npix);
    if ((rc = st.commit())) return rc;
    rt_params q = *p;
    q.flags &= ~RT_FLAG_ACCUMULATE;                     // host form always starts from zero
    return timed_section(ctx, "rt_render_features", kernel_ms, st,
        [&] { return rt_render_features_device(ctx, cam, &q, st.ptr(feat), st.ptr(ids), ctx->own_stream); });
}

#ifdef RT_FEATURES_COUNT
int rt_debug_features_counts(rt_context *ctx, unsigned long long out[8]) { return rt::read_and_zero_counts(ctx, out); }
#endif

int rt_features_to_f32_device(rt_context *ctx, const void *d_feat, int32_t width, int32_t rows, int64_t spp, void *d_out, void *stream_v)
{
    int rc = validate_to_f32(ctx, d_feat, width, rows, spp, d_out);
    if (rc) return rc;
    if (rows == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const long long npix = (long long)width * rows;
    hipLaunchKernelGGL(rt::features_to_f32_kernel, dim3(grid_256(npix)), dim3(256), 0, (hipStream_t)stream_v,
                       (const unsigned long long *)d_feat, (float *)d_out, npix, (double)spp);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_features_to_f32(rt_context *ctx, const uint64_t *feat, int32_t width, int32_t rows, int64_t spp, float *out)
{
    int rc = validate_to_f32(ctx, feat, width, rows, spp, out);
    if (rc) return rc;
    if (rows == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const size_t count = (size_t)width * rows * RT_FEATURE_WORDS;
    Stage st(ctx);
    const auto words = st.in(feat, count);
    const auto f32 = st.out(out, count);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    rc = rt_features_to_f32_device(ctx, st.ptr(words), width, rows, spp, st.ptr(f32), ctx->own_stream);
    if (rc) return rc;
    RT_HIP(st.finish());
    return RT_OK;
}

} // extern "C"
