// rt_temporal.hip -- temporal accumulation across the frames of an animation by first-hit reprojection (rtiow_hip.h, "temporal
// accumulation").
//
// The sixth translation unit of librtiow_hip.so.  Like the denoiser it sits wholly beside the render kernels: it reads the exact sums a
// render and a feature launch left on the device, and the one-sample frame the previous call wrote, and writes a one-sample frame of exact
// sums plus a history length per pixel.  rt_kernels.hpp, rt_device.hpp, rt_api.hip and the other translation units are untouched, so every
// existing kernel keeps its machine code.  The arithmetic lives in rt_temporal_core.hpp, once, for the kernel here, for rt_temporal_host
// and for the stand-alone sanitizer program of the tests.
//
// One launch, one lane per pixel: a wave covers an 8 x 8 pixel tile and a workgroup four of them (as features_kernel does), so the four
// taps of neighbouring lanes and their 3 x 3 boxes fall into the same cache lines; a grid-stride loop over the tiles.  The constants of the
// call -- both cameras among them -- are computed on the host by rt_tp::constants and arrive as a kernel argument (wave-uniform).  No LDS,
// no atomics; a lane stores its three sums and its length once.  There is ONE form of the kernel: profiles/temporal.txt has the
// measurement that says a staged form is not worth building.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "rt_host.hpp"
#include "rt_temporal_core.hpp"
#include "rt_temporal_shared.hpp"

using namespace rt_host;

namespace rt {

__global__ __launch_bounds__(kTpBlock) void temporal_kernel(const rt_tp::Const K, const rt_tp::Buffers B, const TpTiling T,
                                                            unsigned long long *__restrict__ out_fix, uint32_t *__restrict__ out_len)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_waves = gridDim.x * (uint32_t)kTpWaves;
    for (uint32_t wt = blockIdx.x * (uint32_t)kTpWaves + wave; wt < T.n_tiles; wt += n_waves) {
        const uint32_t ty = wt / T.tiles_x, tx = wt - ty * T.tiles_x;
        const long long i = (long long)(tx * 8u + (lane & 7u)), j = (long long)(ty * 8u + (lane >> 3));
        if (i >= K.width || j >= K.height) continue;            // lanes past the right or top edge: nothing computed, nothing stored
        uint64_t q[3];
        const uint32_t len = rt_tp::pixel_at(i, j, K, B, q);
        const unsigned long long p = (unsigned long long)(j * K.width + i);
        out_fix[3 * p + 0] = q[0]; out_fix[3 * p + 1] = q[1]; out_fix[3 * p + 2] = q[2];
        out_len[p] = len;
    }
}

} // namespace rt

namespace {

// What every form checks, before anything is touched; none of it needs a context.  *K: the constants of the call.
int validate_temporal(const struct rt_temporal *tp, const void *fix, bool has_count, int64_t spp, const void *feat, int64_t feat_spp,
                      const rt_camera *cam, const void *prev_fix, const void *prev_len, const void *prev_feat, int64_t prev_feat_spp,
                      const rt_camera *prev_cam, int32_t width, int32_t height, const void *out_fix, const void *out_len, rt_tp::Const *K)
{
    if (!tp) return fail(RT_ERR_INVALID_ARGUMENT, "temporal: the options are NULL");
    if (!fix || !feat || !cam || !out_fix || !out_len)
        return fail(RT_ERR_INVALID_ARGUMENT, "temporal: a buffer is NULL (fix, feat, cam, out_fix or out_len)");
    const int n_hist = (prev_fix ? 1 : 0) + (prev_len ? 1 : 0) + (prev_feat ? 1 : 0) + (prev_cam ? 1 : 0);
    if (n_hist != 0 && n_hist != 4)
        return fail(RT_ERR_INVALID_ARGUMENT, "temporal: a partial history (%d of prev_fix, prev_len, prev_feat, prev_cam): all four or none", n_hist);
    return rt::tp_check_settings("temporal", tp, has_count, spp, feat_spp, cam, n_hist != 0, prev_feat_spp, prev_cam, width, height, K);
}

rt_tp::Buffers buffers_of(const void *fix, const void *count, const void *feat, const void *prev_fix, const void *prev_len, const void *prev_feat)
{
    rt_tp::Buffers B;
    B.fix = (const uint64_t *)fix; B.count = (const uint32_t *)count; B.feat = (const uint64_t *)feat;
    B.prev_fix = (const uint64_t *)prev_fix; B.prev_len = (const uint32_t *)prev_len; B.prev_feat = (const uint64_t *)prev_feat;
    return B;
}

} // namespace

extern "C" {

int rt_temporal_device(rt_context *ctx, const void *d_fix, const void *d_count, int64_t spp, const void *d_feat, int64_t feat_spp,
                       const rt_camera *cam, const void *d_prev_fix, const void *d_prev_len, const void *d_prev_feat, int64_t prev_feat_spp,
                       const rt_camera *prev_cam, int32_t width, int32_t height, const struct rt_temporal *tp, void *d_out_fix, void *d_out_len,
                       void *stream_v)
{
    rt_tp::Const K;
    int rc = validate_temporal(tp, d_fix, d_count != nullptr, spp, d_feat, feat_spp, cam, d_prev_fix, d_prev_len, d_prev_feat, prev_feat_spp,
                               prev_cam, width, height, d_out_fix, d_out_len, &K);
    if (rc) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    // (no launch slot: rt_last_stats does not report on an accumulation; no scene needed)
    rt::TpTiling T;
    const unsigned grid = rt::tp_grid(width, height, &T);
    hipLaunchKernelGGL(rt::temporal_kernel, dim3(grid), dim3(rt::kTpBlock), 0, (hipStream_t)stream_v, K,
                       buffers_of(d_fix, d_count, d_feat, d_prev_fix, d_prev_len, d_prev_feat), T, (unsigned long long *)d_out_fix,
                       (uint32_t *)d_out_len);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_temporal(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp,
                const rt_camera *cam, const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp,
                const rt_camera *prev_cam, int32_t width, int32_t height, const struct rt_temporal *tp, uint64_t *out_fix, uint32_t *out_len,
                float *kernel_ms)
{
    rt_tp::Const K;
    int rc = validate_temporal(tp, fix, count != nullptr, spp, feat, feat_spp, cam, prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam, width,
                               height, out_fix, out_len, &K);
    if (rc) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    const bool hist = prev_cam != nullptr;              // no history: its three buffers are left out whatever the caller passed
    const size_t npix = (size_t)width * height;
    Stage st(ctx);                                      // (the order of the blocks: tests/stage_layout_table.cpp, temporal_blocks)
    const auto sums = st.in(fix, npix * 3), guides = st.in(feat, npix * RT_FEATURE_WORDS);
    const auto counts = st.in(count, npix);
    const auto psums = st.in(hist ? prev_fix : nullptr, npix * 3), pguides = st.in(hist ? prev_feat : nullptr, npix * RT_FEATURE_WORDS);
    const auto plen = st.in(hist ? prev_len : nullptr, npix);
    const auto out = st.out(out_fix, npix * 3);
    const auto olen = st.out(out_len, npix);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    return timed_section(ctx, "rt_temporal", kernel_ms, st, [&] {
        return rt_temporal_device(ctx, st.ptr(sums), st.ptr(counts), spp, st.ptr(guides), feat_spp, cam, st.ptr(psums), st.ptr(plen), st.ptr(pguides),
                                  prev_feat_spp, prev_cam, width, height, tp, st.ptr(out), st.ptr(olen), ctx->own_stream);
    });
}

// the library's own CPU statement: the very functions the kernel compiles, one pixel after the other
int rt_temporal_host(const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp, const rt_camera *cam,
                     const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp, const rt_camera *prev_cam,
                     int32_t width, int32_t height, const struct rt_temporal *tp, uint64_t *out_fix, uint32_t *out_len)
{
    rt_tp::Const K;
    int rc = validate_temporal(tp, fix, count != nullptr, spp, feat, feat_spp, cam, prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam, width,
                               height, out_fix, out_len, &K);
    if (rc) return rc;
    rt_tp::accumulate_host(K, buffers_of(fix, count, feat, prev_fix, prev_len, prev_feat), out_fix, out_len);
    return RT_OK;
}

} // extern "C"
