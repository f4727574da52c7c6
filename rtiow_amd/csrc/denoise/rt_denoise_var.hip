// rt_denoise_var.hip -- the variance-guided a-trous denoiser fed by the half-sample sums (rtiow_hip.h, "variance-guided denoiser";
// DESIGN.md section 25).
//
// The twelfth translation unit of librtiow_hip.so, a sibling of rt_denoise.hip.  (It lives in a folder of its own for the reason
// wavefront/ does: tools/isa_fingerprint.py --all is pinned to the kernels of rtiow_amd/csrc/rt_*.hip; its own five kernels are pinned by
// --denoise-var, profiles/isa_fingerprint_denoise_var.txt.)  The arithmetic lives in rt_denoise_var_core.hpp, once, for the kernels here,
// for rt_denoise_var_host and for the stand-alone sanitizer program of the tests.  What the two denoisers share lives in
// rt_denoise_shared.hpp and rt_denoise_tile.inc (see rt_denoise.hip); here stay the kernels under their names, the record's eleventh
// plane, the NULL checks and the measured defaults.
//
// Launches of one denoise, 2 + 2 levels: prepare (one lane per pixel: rt_denoise's prepare and the variance of the two half means), then
// per level the statistics (the 3x3 box mean of the colour and the 3x3 Gaussian of the variance, one pass) and the 5x5 a-trous taps, then
// finish.  The workspace holds 19 doubles per pixel: rt_denoise's 16, two variance planes (a level reads one and writes the other) and
// the variance's Gaussian.  The level kernel -- the hot path, 25 taps of a record of 11 doubles -- exists in rt_denoise's two forms, which
// give identical bits (the tap order is fixed by rt_dn::level_pixel_var):
//   gather  one lane per pixel, the 25 records straight from global memory;
//   tile    a workgroup takes a 16 x 16 tile of ONE residue class modulo the hole step s, stages its (16 + 4)^2 records in LDS as eleven
//           planes of 400 doubles (35 200 bytes; plane-major: a wave's lanes read consecutive doubles of one plane) and reads the taps
//           from there.
// Which one a level takes: kDnVarTileDefault below, or RTIOW_DENOISE_LEVEL_KERNEL=gather|tile (rt_denoise's diagnostic knob, read per call).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_host.hpp"
#include "rt_denoise_var_core.hpp"
#include "rt_denoise_shared.hpp"

using namespace rt_host;

namespace rt {

// Which form of the level kernel ships for hole step 2^l: the one with the lower SUM of the two measured frames' times, 1200x675 and
// 1920x1080 (profiles/denoise_var.txt, tools/denoise_var_bench.py; statistics pass + level kernel in ms, gather / tile):
//   level 0 (with prepare and finish)  0.167 / 0.114   0.402 / 0.278   tile
//   level 1                            0.118 / 0.083   0.277 / 0.160   tile
//   level 2                            0.120 / 0.105   0.276 / 0.236   tile
//   level 3                            0.117 / 0.112   0.254 / 0.285   gather (0.371 against 0.397)
//   level 4                            0.114 / 0.128   0.230 / 0.166   tile   (0.344 against 0.294)
//   level 5                            0.110 / 0.138   0.228 / 0.188   tile   (0.338 against 0.326)
// Levels 6 and 7 were not measured and take level 5's form.
constexpr bool kDnVarTileDefault[rt_dn::kMaxLevels] = {true, true, true, false, true, true, true, true};

struct DvFrame {
    using Rec = rt_dn::TapVar;
    const double *guide;            // [npix][4] normal xyz, depth
    const double *cin;              // [npix][3] the level's input colour
    const double *box;              // [npix][3] its 3x3 box mean
    const double *vin;              // [npix] the level's input variance
    const double *gv;               // [npix] its 3x3 Gaussian
    double *cout;                   // [npix][3] the level's output colour
    double *vout;                   // [npix] ... and variance
    uint32_t width, height;
    unsigned long long npix;
    rt_dn::LevelConst L;
    double sc2;                     // sigma_color^2
};

__global__ __launch_bounds__(kDnBlock) void denoise_var_prepare_kernel(const unsigned long long *__restrict__ fix,
                                                                       const unsigned long long *__restrict__ half,
                                                                       const uint32_t *__restrict__ count, double spp,
                                                                       const unsigned long long *__restrict__ feat, double feat_spp,
                                                                       int demodulate, unsigned long long npix, double *__restrict__ guide,
                                                                       double *__restrict__ mod, double *__restrict__ c0,
                                                                       double *__restrict__ var0)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < npix; p += stride) {
        double c[3], m[3], n[3], z;
        const double samples = count ? (double)count[p] : spp;
        rt_dn::prepare((const uint64_t *)fix + 3 * p, samples, (const uint64_t *)feat + 8 * p, feat_spp, demodulate != 0, c, m, n, &z);
        var0[p] = rt_dn::prepare_var((const uint64_t *)fix + 3 * p, (const uint64_t *)half + 3 * p, samples, m);
        c0[3 * p + 0] = c[0]; c0[3 * p + 1] = c[1]; c0[3 * p + 2] = c[2];
        mod[3 * p + 0] = m[0]; mod[3 * p + 1] = m[1]; mod[3 * p + 2] = m[2];
        guide[4 * p + 0] = n[0]; guide[4 * p + 1] = n[1]; guide[4 * p + 2] = n[2]; guide[4 * p + 3] = z;
    }
}

// the level's statistics in one pass: the 3x3 box mean of the colour and the 3x3 Gaussian of the variance
__global__ __launch_bounds__(kDnBlock) void denoise_var_stats_kernel(const double *__restrict__ cin, const double *__restrict__ vin,
                                                                     uint32_t width, uint32_t height, unsigned long long npix,
                                                                     double *__restrict__ box, double *__restrict__ gv)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < npix; p += stride) {
        const uint32_t j = (uint32_t)p / width, i = (uint32_t)p - j * width;        // npix <= 2^31: p fits 32 bits
        double g[3];
        rt_dn::box_mean((long long)i, (long long)j, (long long)width, (long long)height,
                        [cin, width](long long ii, long long jj, double c[3]) {
                            const double *s = cin + 3 * ((unsigned long long)jj * width + (unsigned long long)ii);
                            c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
                        }, g);
        box[3 * p + 0] = g[0]; box[3 * p + 1] = g[1]; box[3 * p + 2] = g[2];
        gv[p] = rt_dn::gauss_var((long long)i, (long long)j, (long long)width, (long long)height, [vin, width](long long ii, long long jj) {
            return vin[(unsigned long long)jj * width + (unsigned long long)ii];
        });
    }
}

// form (a): one lane per pixel, every tap from global memory
__global__ __launch_bounds__(kDnBlock) void denoise_var_level_gather_kernel(const DvFrame F) { dn_gather_body(F); }

// form (b): a workgroup per 16 x 16 tile of one sub-lattice, the records staged in LDS (DnTiling; the body is rt_denoise_tile.inc); this
// is the pixel it filters from its staged taps
template <class TapAt>
__device__ __forceinline__ void dn_tile_pixel(const DvFrame &F, long long i, long long j, long long W, long long H, const rt_dn::TapVar &centre,
                                              TapAt staged)
{
    const unsigned long long p = (unsigned long long)(j * W + i);
    double out[3], var;
    rt_dn::level_pixel_var(i, j, W, H, F.L, F.sc2, F.gv[p], centre, staged, out, &var);
    F.cout[3 * p + 0] = out[0]; F.cout[3 * p + 1] = out[1]; F.cout[3 * p + 2] = out[2];
    F.vout[p] = var;
}

__global__ __launch_bounds__(kDnBlock) void denoise_var_level_tile_kernel(const DvFrame F, const DnTiling T)
{
#include "rt_denoise_tile.inc"
}

__global__ __launch_bounds__(kDnBlock) void denoise_var_finish_kernel(const double *__restrict__ c, const double *__restrict__ mod,
                                                                      unsigned long long npix, unsigned long long *__restrict__ out)
{
    dn_finish_body(c, mod, npix, out);
}

// What follows prepare, for rt_denoise_var_device and rt_denoise_var_given_device (denoise/rt_temporal_var.hip): per level the statistics
// and the taps, then finish into d_out_fix, on `stream`.  k: the partitioned workspace, prepared (guide, mod, ca, va).
int dn_var_levels_device(const struct rt_denoise *dn, rt_dn::Work k, int32_t width, int32_t height, void *d_out_fix, hipStream_t stream)
{
    const unsigned long long npix = (unsigned long long)width * (unsigned long long)height;
    const unsigned grid = dn_blocks_for(npix);
    const int knob = dn_level_kernel_knob();
    for (int l = 0; l < dn->levels; ++l) {
        hipLaunchKernelGGL(denoise_var_stats_kernel, dim3(grid), dim3(kDnBlock), 0, stream, (const double *)k.ca, (const double *)k.va,
                           (uint32_t)width, (uint32_t)height, npix, k.box, k.gv);
        RT_HIP(hipGetLastError());
        DvFrame F;
        F.guide = k.guide; F.cin = k.ca; F.box = k.box; F.vin = k.va; F.gv = k.gv; F.cout = k.cb; F.vout = k.vb;
        F.width = (uint32_t)width; F.height = (uint32_t)height; F.npix = npix;
        F.L = rt_dn::level_const(dn->sigma_color, dn->sigma_normal, dn->sigma_depth, l);
        F.sc2 = dn->sigma_color * dn->sigma_color;
        dn_launch_level(F, knob < 0 ? kDnVarTileDefault[l] : knob == 1, denoise_var_level_tile_kernel, denoise_var_level_gather_kernel, stream);
        RT_HIP(hipGetLastError());
        double *t = k.ca; k.ca = k.cb; k.cb = t;
        t = k.va; k.va = k.vb; k.vb = t;
    }
    hipLaunchKernelGGL(denoise_var_finish_kernel, dim3(grid), dim3(kDnBlock), 0, stream, (const double *)k.ca, (const double *)k.mod, npix,
                       (unsigned long long *)d_out_fix);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

} // namespace rt

namespace {

// What every form checks, before anything is touched, in rt_denoise's order with the NULL half behind the NULL fix; none of it needs a
// context.
int validate_denoise_var(const struct rt_denoise *dn, const void *fix, const void *half, int64_t spp, bool has_count, const void *feat,
                         int64_t feat_spp, int32_t width, int32_t height, const void *out)
{
    if (!dn) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var: dn is NULL");
    if (!fix) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var: a buffer is NULL (fix)");
    if (!half) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var: the half-sample sums are NULL (half)");
    if (!feat || !out) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var: a buffer is NULL (feat or out)");
    return rt::dn_check_settings("denoise_var", dn, spp, has_count, feat_spp, width, height);
}

} // namespace

extern "C" {

int rt_denoise_var_workspace_bytes(int32_t width, int32_t height, int64_t *out_bytes)
{
    return rt::dn_workspace_bytes("denoise_var workspace", width, height, rt_dn::kVarWorkDoubles, out_bytes);
}

int rt_denoise_var_device(rt_context *ctx, const void *d_fix, const void *d_half, const void *d_count, int64_t spp, const void *d_feat,
                          int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, void *d_work, void *d_out_fix,
                          void *stream_v)
{
    int rc = validate_denoise_var(dn, d_fix, d_half, spp, d_count != nullptr, d_feat, feat_spp, width, height, d_out_fix);
    if (rc) return rc;
    if (!d_work) return fail(RT_ERR_INVALID_ARGUMENT, "denoise_var: the workspace is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    // (no launch slot: rt_last_stats does not report on a denoise; no scene needed)
    const unsigned long long npix = (unsigned long long)width * (unsigned long long)height;
    rt_dn::Work k = rt_dn::partition((double *)d_work, npix, true);
    const unsigned grid = rt::dn_blocks_for(npix);
    hipLaunchKernelGGL(rt::denoise_var_prepare_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, (const unsigned long long *)d_fix,
                       (const unsigned long long *)d_half, (const uint32_t *)d_count, (double)spp, (const unsigned long long *)d_feat,
                       (double)feat_spp, (dn->flags & RT_DENOISE_DEMODULATE) ? 1 : 0, npix, k.guide, k.mod, k.ca, k.va);
    RT_HIP(hipGetLastError());
    return rt::dn_var_levels_device(dn, k, width, height, d_out_fix, stream);
}

int rt_denoise_var(rt_context *ctx, const uint64_t *fix, const uint64_t *half, const uint32_t *count, int64_t spp, const uint64_t *feat,
                   int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix, float *kernel_ms)
{
    int rc = validate_denoise_var(dn, fix, half, spp, count != nullptr, feat, feat_spp, width, height, out_fix);
    if (rc) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)width * height;
    Stage st(ctx);
    const auto sums = st.in(fix, npix * 3), halves = st.in(half, npix * 3), guides = st.in(feat, npix * RT_FEATURE_WORDS);
    const auto out = st.out(out_fix, npix * 3);
    const auto work = st.scratch<double>(npix * rt_dn::kVarWorkDoubles);
    const auto counts = st.in(count, npix);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    return timed_section(ctx, "rt_denoise_var", kernel_ms, st, [&] {
        return rt_denoise_var_device(ctx, st.ptr(sums), st.ptr(halves), st.ptr(counts), spp, st.ptr(guides), feat_spp, width, height, dn,
                                     st.ptr(work), st.ptr(out), ctx->own_stream);
    });
}

// the library's own CPU statement of the filter: the very functions the kernels compile, one pixel after the other
int rt_denoise_var_host(const uint64_t *fix, const uint64_t *half, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp,
                        int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix)
{
    int rc = validate_denoise_var(dn, fix, half, spp, count != nullptr, feat, feat_spp, width, height, out_fix);
    if (rc) return rc;
    std::vector<double> work;
    try {
        work.resize((size_t)width * height * rt_dn::kVarWorkDoubles);
    } catch (...) {
        return fail(RT_ERR_OUT_OF_MEMORY, "rt_denoise_var_host: no memory for the workspace");
    }
    rt_dn::filter_var_host(fix, half, count, (long long)spp, feat, (long long)feat_spp, width, height, dn->levels,
                           (dn->flags & RT_DENOISE_DEMODULATE) != 0, dn->sigma_color, dn->sigma_normal, dn->sigma_depth, work.data(), out_fix);
    return RT_OK;
}

} // extern "C"
