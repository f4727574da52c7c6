// rt_temporal_var.hip -- temporal accumulation with second moments, and the variance-guided denoiser fed by a variance the caller gives
// (rtiow_hip.h, "temporal accumulation with second moments"): the temporal half of SVGF and the one entry of the
// filter that takes its result.
//
// The thirteenth translation unit of librtiow_hip.so.  (It lives in denoise/ for the reason rt_denoise_var.hip does: tools/isa_fingerprint.py
// --all is pinned to the kernels of rtiow_amd/csrc/rt_*.hip; its own two kernels are pinned by --temporal-var,
// profiles/isa_fingerprint_temporal_var.txt.)  The arithmetic lives in rt_temporal_var_core.hpp and rt_denoise_var_core.hpp, once, for the
// kernels here, for the two host statements and for the stand-alone sanitizer program of the tests.  No existing kernel is touched: the
// checks and the tiling rt_temporal shares are rt_temporal_shared.hpp's, and the launches behind the filter's prepare are
// rt::dn_var_levels_device of rt_denoise_var.hip.
//
// temporal_var_kernel has temporal_kernel's shape: one lane per pixel, a wave on an 8 x 8 pixel tile, four waves a workgroup, a grid-stride
// loop over the tiles; the constants of the call, both cameras among them, arrive as ONE kernel argument (wave-uniform).  No LDS, no atomics.
// The 3 x 3 neighbourhood of the current frame is walked once, for the spatial moments and the clamp's box together.  A lane stores its
// three sums, its length, three moments and three variances once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_host.hpp"
#include "rt_temporal_var_core.hpp"
#include "rt_temporal_shared.hpp"
#include "rt_denoise_var_core.hpp"
#include "rt_denoise_shared.hpp"

using namespace rt_host;

namespace rt {

__global__ __launch_bounds__(kTpBlock) void temporal_var_kernel(const rt_tp::Const K, const rt_tp::BuffersVar B, const TpTiling T,
                                                                unsigned long long *__restrict__ out_fix, uint32_t *__restrict__ out_len,
                                                                double *__restrict__ out_m2, double *__restrict__ out_var)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_waves = gridDim.x * (uint32_t)kTpWaves;
    for (uint32_t wt = blockIdx.x * (uint32_t)kTpWaves + wave; wt < T.n_tiles; wt += n_waves) {
        const uint32_t ty = wt / T.tiles_x, tx = wt - ty * T.tiles_x;
        const long long i = (long long)(tx * 8u + (lane & 7u)), j = (long long)(ty * 8u + (lane >> 3));
        if (i >= K.width || j >= K.height) continue;            // lanes past the right or top edge: nothing computed, nothing stored
        uint64_t q[3];
        double m2[3], var[3];
        const uint32_t len = rt_tp::pixel_var_at(i, j, K, B, q, m2, var);
        const unsigned long long p = (unsigned long long)(j * K.width + i);
        out_fix[3 * p + 0] = q[0]; out_fix[3 * p + 1] = q[1]; out_fix[3 * p + 2] = q[2];
        out_len[p] = len;
        out_m2[3 * p + 0] = m2[0]; out_m2[3 * p + 1] = m2[1]; out_m2[3 * p + 2] = m2[2];
        out_var[3 * p + 0] = var[0]; out_var[3 * p + 1] = var[1]; out_var[3 * p + 2] = var[2];
    }
}

// rt_denoise_var's prepare with the variance given: one lane per pixel
__global__ __launch_bounds__(kDnBlock) void denoise_var_given_prepare_kernel(const unsigned long long *__restrict__ fix,
                                                                             const double *__restrict__ var,
                                                                             const uint32_t *__restrict__ count, double spp,
                                                                             const unsigned long long *__restrict__ feat, double feat_spp,
                                                                             int demodulate, unsigned long long npix, double *__restrict__ guide,
                                                                             double *__restrict__ mod, double *__restrict__ c0,
                                                                             double *__restrict__ var0)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < npix; p += stride) {
        double c[3], m[3], n[3], z;
        rt_dn::prepare((const uint64_t *)fix + 3 * p, count ? (double)count[p] : spp, (const uint64_t *)feat + 8 * p, feat_spp, demodulate != 0, c, m,
                       n, &z);
        const double v[3] = {var[3 * p + 0], var[3 * p + 1], var[3 * p + 2]};
        var0[p] = rt_dn::prepare_var_given(v, m);
        c0[3 * p + 0] = c[0]; c0[3 * p + 1] = c[1]; c0[3 * p + 2] = c[2];
        mod[3 * p + 0] = m[0]; mod[3 * p + 1] = m[1]; mod[3 * p + 2] = m[2];
        guide[4 * p + 0] = n[0]; guide[4 * p + 1] = n[1]; guide[4 * p + 2] = n[2]; guide[4 * p + 3] = z;
    }
}

} // namespace rt

namespace {

// What every form checks, before anything is touched, in rt_temporal's order: the two new outputs join the NULL check and prev_m2 the
// history count; none of it needs a context.  *K: the constants of the call.
int validate_temporal_var(const struct rt_temporal *tp, const void *fix, bool has_count, int64_t spp, const void *feat, int64_t feat_spp,
                          const rt_camera *cam, const void *prev_fix, const void *prev_len, const void *prev_feat, int64_t prev_feat_spp,
                          const rt_camera *prev_cam, const void *prev_m2, int32_t width, int32_t height, const void *out_fix, const void *out_len,
                          const void *out_m2, const void *out_var, rt_tp::Const *K)
{
    if (!tp) return fail(RT_ERR_INVALID_ARGUMENT, "temporal_var: the options are NULL");
    if (!fix || !feat || !cam || !out_fix || !out_len || !out_m2 || !out_var)
        return fail(RT_ERR_INVALID_ARGUMENT, "temporal_var: a buffer is NULL (fix, feat, cam, out_fix, out_len, out_m2 or out_var)");
    const int n_hist = (prev_fix ? 1 : 0) + (prev_len ? 1 : 0) + (prev_feat ? 1 : 0) + (prev_cam ? 1 : 0) + (prev_m2 ? 1 : 0);
    if (n_hist != 0 && n_hist != 5)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "temporal_var: a partial history (%d of prev_fix, prev_len, prev_feat, prev_cam, prev_m2): all five or none", n_hist);
    return rt::tp_check_settings("temporal_var", tp, has_count, spp, feat_spp, cam, n_hist != 0, prev_feat_spp, prev_cam, width, height, K);
}

rt_tp::BuffersVar buffers_of(const void *fix, const void *count, const void *feat, const void *prev_fix, const void *prev_len, const void *prev_feat,
                             const void *prev_m2)
{
    rt_tp::BuffersVar B;
    B.fix = (const uint64_t *)fix; B.count = (const uint32_t *)count; B.feat = (const uint64_t *)feat;
    B.prev_fix = (const uint64_t *)prev_fix; B.prev_len = (const uint32_t *)prev_len; B.prev_feat = (const uint64_t *)prev_feat;
    B.prev_m2 = (const double *)prev_m2;
    return B;
}

// rt_denoise_var's checks in its order, with var in half's place
int validate_denoise_var_given(const struct rt_denoise *dn, const void *fix, const void *var, int64_t spp, bool has_count, const void *feat,
                               int64_t feat_spp, int32_t width, int32_t height, const void *out)
{
    if (!dn) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var_given: dn is NULL");
    if (!fix) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var_given: a buffer is NULL (fix)");
    if (!var) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var_given: the variance is NULL (var)");
    if (!feat || !out) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var_given: a buffer is NULL (feat or out)");
    return rt::dn_check_settings("denoise_var_given", dn, spp, has_count, feat_spp, width, height);
}

} // namespace

extern "C" {

int rt_temporal_var_device(rt_context *ctx, const void *d_fix, const void *d_count, int64_t spp, const void *d_feat, int64_t feat_spp,
                           const rt_camera *cam, const void *d_prev_fix, const void *d_prev_len, const void *d_prev_feat, int64_t prev_feat_spp,
                           const rt_camera *prev_cam, const void *d_prev_m2, int32_t width, int32_t height, const struct rt_temporal *tp,
                           void *d_out_fix, void *d_out_len, void *d_out_m2, void *d_out_var, void *stream_v)
{
    rt_tp::Const K;
    int rc = validate_temporal_var(tp, d_fix, d_count != nullptr, spp, d_feat, feat_spp, cam, d_prev_fix, d_prev_len, d_prev_feat, prev_feat_spp,
                                   prev_cam, d_prev_m2, width, height, d_out_fix, d_out_len, d_out_m2, d_out_var, &K);
    if (rc) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    // (no launch slot: rt_last_stats does not report on an accumulation; no scene needed)
    rt::TpTiling T;
    const unsigned grid = rt::tp_grid(width, height, &T);
    hipLaunchKernelGGL(rt::temporal_var_kernel, dim3(grid), dim3(rt::kTpBlock), 0, (hipStream_t)stream_v, K,
                       buffers_of(d_fix, d_count, d_feat, d_prev_fix, d_prev_len, d_prev_feat, d_prev_m2), T, (unsigned long long *)d_out_fix,
                       (uint32_t *)d_out_len, (double *)d_out_m2, (double *)d_out_var);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_temporal_var(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp,
                    const rt_camera *cam, const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp,
                    const rt_camera *prev_cam, const double *prev_m2, int32_t width, int32_t height, const struct rt_temporal *tp,
                    uint64_t *out_fix, uint32_t *out_len, double *out_m2, double *out_var, float *kernel_ms)
{
    rt_tp::Const K;
    int rc = validate_temporal_var(tp, fix, count != nullptr, spp, feat, feat_spp, cam, prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam,
                                   prev_m2, width, height, out_fix, out_len, out_m2, out_var, &K);
    if (rc) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)width * height;
    Stage st(ctx);                                      // (a history is all five or none: validated above)
    const auto sums = st.in(fix, npix * 3), guides = st.in(feat, npix * RT_FEATURE_WORDS);
    const auto counts = st.in(count, npix);
    const auto psums = st.in(prev_fix, npix * 3), pguides = st.in(prev_feat, npix * RT_FEATURE_WORDS);
    const auto plen = st.in(prev_len, npix);
    const auto pm2 = st.in(prev_m2, npix * 3);
    const auto out = st.out(out_fix, npix * 3);
    const auto olen = st.out(out_len, npix);
    const auto om2 = st.out(out_m2, npix * 3), ovar = st.out(out_var, npix * 3);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    return timed_section(ctx, "rt_temporal_var", kernel_ms, st, [&] {
        return rt_temporal_var_device(ctx, st.ptr(sums), st.ptr(counts), spp, st.ptr(guides), feat_spp, cam, st.ptr(psums), st.ptr(plen),
                                      st.ptr(pguides), prev_feat_spp, prev_cam, st.ptr(pm2), width, height, tp, st.ptr(out), st.ptr(olen),
                                      st.ptr(om2), st.ptr(ovar), ctx->own_stream);
    });
}

// the library's own CPU statement: the very functions the kernel compiles, one pixel after the other
int rt_temporal_var_host(const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp, const rt_camera *cam,
                         const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp,
                         const rt_camera *prev_cam, const double *prev_m2, int32_t width, int32_t height, const struct rt_temporal *tp,
                         uint64_t *out_fix, uint32_t *out_len, double *out_m2, double *out_var)
{
    rt_tp::Const K;
    int rc = validate_temporal_var(tp, fix, count != nullptr, spp, feat, feat_spp, cam, prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam,
                                   prev_m2, width, height, out_fix, out_len, out_m2, out_var, &K);
    if (rc) return rc;
    rt_tp::accumulate_var_host(K, buffers_of(fix, count, feat, prev_fix, prev_len, prev_feat, prev_m2), out_fix, out_len, out_m2, out_var);
    return RT_OK;
}

int rt_denoise_var_given_device(rt_context *ctx, const void *d_fix, const void *d_var, const void *d_count, int64_t spp, const void *d_feat,
                                int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, void *d_work, void *d_out_fix,
                                void *stream_v)
{
    int rc = validate_denoise_var_given(dn, d_fix, d_var, spp, d_count != nullptr, d_feat, feat_spp, width, height, d_out_fix);
    if (rc) return rc;
    if (!d_work) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var_given: the workspace is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    // (no launch slot: rt_last_stats does not report on a denoise; no scene needed)
    const unsigned long long npix = (unsigned long long)width * (unsigned long long)height;
    const rt_dn::Work k = rt_dn::partition((double *)d_work, npix, true);
    hipLaunchKernelGGL(rt::denoise_var_given_prepare_kernel, dim3(rt::dn_blocks_for(npix)), dim3(rt::kDnBlock), 0, stream,
                       (const unsigned long long *)d_fix, (const double *)d_var, (const uint32_t *)d_count, (double)spp,
                       (const unsigned long long *)d_feat, (double)feat_spp, (dn->flags & RT_DENOISE_DEMODULATE) ? 1 : 0, npix, k.guide, k.mod, k.ca,
                       k.va);
    RT_HIP(hipGetLastError());
    return rt::dn_var_levels_device(dn, k, width, height, d_out_fix, stream);
}

int rt_denoise_var_given(rt_context *ctx, const uint64_t *fix, const double *var, const uint32_t *count, int64_t spp, const uint64_t *feat,
                         int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix, float *kernel_ms)
{
    int rc = validate_denoise_var_given(dn, fix, var, spp, count != nullptr, feat, feat_spp, width, height, out_fix);
    if (rc) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)width * height;
    Stage st(ctx);
    const auto sums = st.in(fix, npix * 3);
    const auto vars = st.in(var, npix * 3);
    const auto guides = st.in(feat, npix * RT_FEATURE_WORDS);
    const auto out = st.out(out_fix, npix * 3);
    const auto work = st.scratch<double>(npix * rt_dn::kVarWorkDoubles);
    const auto counts = st.in(count, npix);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    return timed_section(ctx, "rt_denoise_var_given", kernel_ms, st, [&] {
        return rt_denoise_var_given_device(ctx, st.ptr(sums), st.ptr(vars), st.ptr(counts), spp, st.ptr(guides), feat_spp, width, height, dn,
                                           st.ptr(work), st.ptr(out), ctx->own_stream);
    });
}

// the library's own CPU statement of the filter: the very functions the kernels compile, one pixel after the other
int rt_denoise_var_given_host(const uint64_t *fix, const double *var, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp,
                              int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix)
{
    int rc = validate_denoise_var_given(dn, fix, var, spp, count != nullptr, feat, feat_spp, width, height, out_fix);
    if (rc) return rc;
    std::vector<double> work;
    try {
        work.resize((size_t)width * height * rt_dn::kVarWorkDoubles);
    } catch (...) {
        return fail(RT_ERR_OUT_OF_MEMORY, "rt_denoise_var_given_host: no memory for the workspace");
    }
    rt_dn::filter_var_given_host(fix, var, count, (long long)spp, feat, (long long)feat_spp, width, height, dn->levels,
                                 (dn->flags & RT_DENOISE_DEMODULATE) != 0, dn->sigma_color, dn->sigma_normal, dn->sigma_depth, work.data(), out_fix);
    return RT_OK;
}

} // extern "C"
