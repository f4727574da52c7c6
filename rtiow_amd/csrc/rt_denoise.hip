// rt_denoise.hip -- the edge-avoiding a-trous denoiser driven by the first-hit guides (rtiow_hip.h, "denoiser").
//
// The fifth translation unit of librtiow_hip.so.  It sits wholly beside the render kernels: it reads the exact sums a render and a
// feature launch left on the device, and writes a one-sample frame of exact sums.  It reads neither rt_kernels.hpp nor rt_device.hpp.
// The arithmetic lives in rt_denoise_core.hpp, once, for the kernels here, for rt_denoise_host and for the stand-alone sanitizer program
// of the tests.  What this unit shares with the variance-guided denoiser (denoise/rt_denoise_var.hip) lives in rt_denoise_shared.hpp --
// the tile geometry, the load of a record, the gather body, the checks of the settings, the tiling arithmetic, a level's launch -- and
// in rt_denoise_tile.inc, the body of the tile form; here stay the kernels under their names, the NULL checks and the measured defaults.
//
// Launches of one denoise: prepare (one lane per pixel), then per level a 3x3 box mean and the 5x5 a-trous taps, then finish (one lane
// per pixel).  The workspace holds 16 doubles per pixel: the guides (normal, depth), the modulation, two colour frames (a level reads one
// and writes the other) and the box mean.  The level kernel -- the hot path, 25 taps of a record of 10 doubles -- exists in two forms
// that give identical bits (the tap order is fixed by rt_dn::level_pixel, not by where the records come from):
//   gather  one lane per pixel, the 25 records straight from global memory (L2 / Infinity-Cache resident at frame sizes);
//   tile    pixels with equal residues modulo the hole step s form an independent dense 5x5 convolution: a workgroup takes a 16 x 16
//           tile of ONE such sub-lattice, stages its (16 + 4)^2 records in LDS once (32 000 bytes) and reads the taps from there.
// Which one a level takes: kDnTileDefault below, or RTIOW_DENOISE_LEVEL_KERNEL=gather|tile (a diagnostic knob; the same frame either way).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_host.hpp"
#include "rt_denoise_core.hpp"
#include "rt_denoise_shared.hpp"

using namespace rt_host;

namespace rt {

// Which form of the level kernel ships for hole step 2^l.  Measured per level at 1200x675 and 1920x1080 (profiles/denoise.txt): the tile form
// takes 0.54 .. 0.97 of the gather's time at levels 0-4 on both frames; at level 5 it is 0.75 (1920x1080) and 1.04 (1200x675, inside the
// gather's 7 % spread) -- no level where the gather is worth a switch.
constexpr bool kDnTileDefault[rt_dn::kMaxLevels] = {true, true, true, true, true, true, true, true};

struct DnFrame {
    using Rec = rt_dn::Tap;
    const double *guide;            // [npix][4] normal xyz, depth
    const double *cin;              // [npix][3] the level's input colour
    const double *box;              // [npix][3] its 3x3 box mean
    double *cout;                   // [npix][3] the level's output
    uint32_t width, height;
    unsigned long long npix;
    rt_dn::LevelConst L;
};

__global__ __launch_bounds__(kDnBlock) void denoise_prepare_kernel(const unsigned long long *__restrict__ fix, const uint32_t *__restrict__ count,
                                                                   double spp, const unsigned long long *__restrict__ feat, double feat_spp,
                                                                   int demodulate, unsigned long long npix, double *__restrict__ guide,
                                                                   double *__restrict__ mod, double *__restrict__ c0)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < npix; p += stride) {
        double c[3], m[3], n[3], z;
        rt_dn::prepare((const uint64_t *)fix + 3 * p, count ? (double)count[p] : spp, (const uint64_t *)feat + 8 * p, feat_spp, demodulate != 0,
                       c, m, n, &z);
        c0[3 * p + 0] = c[0]; c0[3 * p + 1] = c[1]; c0[3 * p + 2] = c[2];
        mod[3 * p + 0] = m[0]; mod[3 * p + 1] = m[1]; mod[3 * p + 2] = m[2];
        guide[4 * p + 0] = n[0]; guide[4 * p + 1] = n[1]; guide[4 * p + 2] = n[2]; guide[4 * p + 3] = z;
    }
}

__global__ __launch_bounds__(kDnBlock) void denoise_box_kernel(const double *__restrict__ cin, uint32_t width, uint32_t height,
                                                               unsigned long long npix, double *__restrict__ box)
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
    }
}

// form (a): one lane per pixel, every tap from global memory
__global__ __launch_bounds__(kDnBlock) void denoise_level_gather_kernel(const DnFrame F) { dn_gather_body(F); }

// form (b): a workgroup per 16 x 16 tile of one sub-lattice, the records staged in LDS (DnTiling; the body is rt_denoise_tile.inc); this
// is the pixel it filters from its staged taps
template <class TapAt>
__device__ __forceinline__ void dn_tile_pixel(const DnFrame &F, long long i, long long j, long long W, long long H, const rt_dn::Tap &centre,
                                              TapAt staged)
{
    double out[3];
    rt_dn::level_pixel(i, j, W, H, F.L, centre, staged, out);
    const unsigned long long p = (unsigned long long)(j * W + i);
    F.cout[3 * p + 0] = out[0]; F.cout[3 * p + 1] = out[1]; F.cout[3 * p + 2] = out[2];
}

__global__ __launch_bounds__(kDnBlock) void denoise_level_tile_kernel(const DnFrame F, const DnTiling T)
{
#include "rt_denoise_tile.inc"
}

__global__ __launch_bounds__(kDnBlock) void denoise_finish_kernel(const double *__restrict__ c, const double *__restrict__ mod,
                                                                  unsigned long long npix, unsigned long long *__restrict__ out)
{
    dn_finish_body(c, mod, npix, out);
}

} // namespace rt

namespace {

// What every form of the denoiser checks, before anything is touched; none of it needs a context.
int validate_denoise(const struct rt_denoise *dn, const void *fix, int64_t spp, bool has_count, const void *feat, int64_t feat_spp,
                     int32_t width, int32_t height, const void *out)
{
    if (!dn) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: dn is NULL");
    if (!fix || !feat || !out) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: a buffer is NULL (fix, feat or out)");
    return rt::dn_check_settings("denoise", dn, spp, has_count, feat_spp, width, height);
}

} // namespace

extern "C" {

int rt_denoise_workspace_bytes(int32_t width, int32_t height, int64_t *out_bytes)
{
    return rt::dn_workspace_bytes("denoise workspace", width, height, rt_dn::kWorkDoubles, out_bytes);
}

int rt_denoise_device(rt_context *ctx, const void *d_fix, const void *d_count, int64_t spp, const void *d_feat, int64_t feat_spp, int32_t width,
                      int32_t height, const struct rt_denoise *dn, void *d_work, void *d_out_fix, void *stream_v)
{
    int rc = validate_denoise(dn, d_fix, spp, d_count != nullptr, d_feat, feat_spp, width, height, d_out_fix);
    if (rc) return rc;
    if (!d_work) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: the workspace is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    // (no launch slot: rt_last_stats does not report on a denoise; no scene needed)
    const unsigned long long npix = (unsigned long long)width * (unsigned long long)height;
    rt_dn::Work k = rt_dn::partition((double *)d_work, npix, false);
    const unsigned grid = rt::dn_blocks_for(npix);
    hipLaunchKernelGGL(rt::denoise_prepare_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, (const unsigned long long *)d_fix,
                       (const uint32_t *)d_count, (double)spp, (const unsigned long long *)d_feat, (double)feat_spp,
                       (dn->flags & RT_DENOISE_DEMODULATE) ? 1 : 0, npix, k.guide, k.mod, k.ca);
    RT_HIP(hipGetLastError());
    const int knob = rt::dn_level_kernel_knob();
    for (int l = 0; l < dn->levels; ++l) {
        hipLaunchKernelGGL(rt::denoise_box_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, (const double *)k.ca, (uint32_t)width,
                           (uint32_t)height, npix, k.box);
        RT_HIP(hipGetLastError());
        rt::DnFrame F;
        F.guide = k.guide; F.cin = k.ca; F.box = k.box; F.cout = k.cb;
        F.width = (uint32_t)width; F.height = (uint32_t)height; F.npix = npix;
        F.L = rt_dn::level_const(dn->sigma_color, dn->sigma_normal, dn->sigma_depth, l);
        rt::dn_launch_level(F, knob < 0 ? rt::kDnTileDefault[l] : knob == 1, rt::denoise_level_tile_kernel, rt::denoise_level_gather_kernel, stream);
        RT_HIP(hipGetLastError());
        double *t = k.ca; k.ca = k.cb; k.cb = t;
    }
    hipLaunchKernelGGL(rt::denoise_finish_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, (const double *)k.ca, (const double *)k.mod, npix,
                       (unsigned long long *)d_out_fix);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_denoise(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp, int32_t width,
               int32_t height, const struct rt_denoise *dn, uint64_t *out_fix, float *kernel_ms)
{
    int rc = validate_denoise(dn, fix, spp, count != nullptr, feat, feat_spp, width, height, out_fix);
    if (rc) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)width * height;
    Stage st(ctx);                                      // (the order of the blocks: tests/stage_layout_table.cpp, denoise_blocks)
    const auto sums = st.in(fix, npix * 3), guides = st.in(feat, npix * RT_FEATURE_WORDS);
    const auto out = st.out(out_fix, npix * 3);
    const auto work = st.scratch<double>(npix * rt_dn::kWorkDoubles);
    const auto counts = st.in(count, npix);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    return timed_section(ctx, "rt_denoise", kernel_ms, st, [&] {
        return rt_denoise_device(ctx, st.ptr(sums), st.ptr(counts), spp, st.ptr(guides), feat_spp, width, height, dn, st.ptr(work), st.ptr(out),
                                 ctx->own_stream);
    });
}

// the library's own CPU statement of the filter: the very functions the kernels compile, one pixel after the other
int rt_denoise_host(const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp, int32_t width,
                    int32_t height, const struct rt_denoise *dn, uint64_t *out_fix)
{
    int rc = validate_denoise(dn, fix, spp, count != nullptr, feat, feat_spp, width, height, out_fix);
    if (rc) return rc;
    std::vector<double> work;
    try {
        work.resize((size_t)width * height * rt_dn::kWorkDoubles);
    } catch (...) {
        return fail(RT_ERR_OUT_OF_MEMORY, "rt_denoise_host: no memory for the workspace");
    }
    rt_dn::filter_host(fix, count, (long long)spp, feat, (long long)feat_spp, width, height, dn->levels, (dn->flags & RT_DENOISE_DEMODULATE) != 0,
                       dn->sigma_color, dn->sigma_normal, dn->sigma_depth, work.data(), out_fix);
    return RT_OK;
}

} // extern "C"
