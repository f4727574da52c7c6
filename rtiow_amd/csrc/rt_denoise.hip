// rt_denoise.hip -- the edge-avoiding a-trous denoiser driven by the first-hit guides (rtiow_hip.h, "denoiser").
//
// The fifth translation unit of librtiow_hip.so.  It sits wholly beside the render kernels: it reads the exact sums a render and a
// feature launch left on the device, and writes a one-sample frame of exact sums.  rt_kernels.hpp, rt_device.hpp, rt_api.hip and the
// other translation units are untouched, so every existing kernel keeps its machine code.  The arithmetic lives in rt_denoise_core.hpp,
// once, for the kernels here, for rt_denoise_host and for the stand-alone sanitizer program of the tests.
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

using namespace rt_host;

namespace rt {

constexpr int kDnBlock = 256;
constexpr int kDnTile = 16;                         // a workgroup's tile of one sub-lattice: 16 x 16 pixels
constexpr int kDnSide = kDnTile + 4;                // ... and its halo of two taps on every side
constexpr int kDnCells = kDnSide * kDnSide;
constexpr int kDnWorkDoubles = 16;                  // per pixel: guides 4, modulation 3, colour in 3, colour out 3, box mean 3
constexpr long long kDnMaxBlocks = 1 << 20;         // grid-stride loops beyond (a launch's work-items fit 32 bits)

// Which form of the level kernel ships for hole step 2^l.  Measured per level at 1200x675 and 1920x1080 (profiles/denoise.txt): the tile form
// takes 0.54 .. 0.97 of the gather's time at levels 0-4 on both frames; at level 5 it is 0.75 (1920x1080) and 1.04 (1200x675, inside the
// gather's 7 % spread) -- no level where the gather is worth a switch.
constexpr bool kDnTileDefault[rt_dn::kMaxLevels] = {true, true, true, true, true, true, true, true};

struct DnFrame {
    const double *guide;            // [npix][4] normal xyz, depth
    const double *cin;              // [npix][3] the level's input colour
    const double *box;              // [npix][3] its 3x3 box mean
    double *cout;                   // [npix][3] the level's output
    uint32_t width, height;
    unsigned long long npix;
    rt_dn::LevelConst L;
};

__device__ __forceinline__ void dn_load_tap(const DnFrame &F, unsigned long long p, rt_dn::Tap *t)
{
    const double *c = F.cin + 3 * p, *g = F.box + 3 * p, *q = F.guide + 4 * p;
    t->c[0] = c[0]; t->c[1] = c[1]; t->c[2] = c[2];
    t->g[0] = g[0]; t->g[1] = g[1]; t->g[2] = g[2];
    t->n[0] = q[0]; t->n[1] = q[1]; t->n[2] = q[2];
    t->z = q[3];
}

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
__global__ __launch_bounds__(kDnBlock) void denoise_level_gather_kernel(const DnFrame F)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < F.npix; p += stride) {
        const uint32_t j = (uint32_t)p / F.width, i = (uint32_t)p - j * F.width;
        rt_dn::Tap centre;
        dn_load_tap(F, p, &centre);
        const long long s = F.L.step;
        double out[3];
        rt_dn::level_pixel((long long)i, (long long)j, (long long)F.width, (long long)F.height, F.L, centre,
                           [&](int dx, int dy, rt_dn::Tap *t) {
                               // (in-frame: level_pixel asks for no other tap)
                               const long long q = (long long)p + (s * dy) * (long long)F.width + s * dx;
                               dn_load_tap(F, (unsigned long long)q, t);
                           }, out);
        F.cout[3 * p + 0] = out[0]; F.cout[3 * p + 1] = out[1]; F.cout[3 * p + 2] = out[2];
    }
}

// form (b): a workgroup per 16 x 16 tile of one sub-lattice (pixels with i % s == ri, j % s == rj), the records staged in LDS.
// tiles_x, tiles_y: tiles per sub-lattice (of the widest one; narrower ones have empty tiles); nri = min(s, width) residues in x.
struct DnTiling {
    uint32_t tiles_x, tiles_y, nri, n_tiles;
};

__global__ __launch_bounds__(kDnBlock) void denoise_level_tile_kernel(const DnFrame F, const DnTiling T)
{
    __shared__ double s_rec[10][kDnCells];
    const long long s = F.L.step;
    const long long W = (long long)F.width, H = (long long)F.height;
    const int lx = (int)threadIdx.x & (kDnTile - 1), ly = (int)threadIdx.x >> 4;
    const uint32_t gx = T.nri * T.tiles_x;
    for (uint32_t t = blockIdx.x; t < T.n_tiles; t += gridDim.x) {
        const uint32_t by = t / gx, bx = t - by * gx;
        const uint32_t ri = bx / T.tiles_x, tx = bx - ri * T.tiles_x;
        const uint32_t rj = by / T.tiles_y, ty = by - rj * T.tiles_y;
        // sub-lattice coordinates (u, v) -> pixel (ri + s u, rj + s v); the tile's first cell is (16 tx - 2, 16 ty - 2)
        const long long u0 = (long long)tx * kDnTile - 2, v0 = (long long)ty * kDnTile - 2;
        for (int cell = (int)threadIdx.x; cell < kDnCells; cell += kDnBlock) {
            const int cy = cell / kDnSide, cx = cell - cy * kDnSide;
            const long long ii = (long long)ri + s * (u0 + cx), jj = (long long)rj + s * (v0 + cy);
            if (ii < 0 || ii >= W || jj < 0 || jj >= H) continue;           // never read: level_pixel skips taps outside the frame
            rt_dn::Tap r;
            dn_load_tap(F, (unsigned long long)(jj * W + ii), &r);
            s_rec[0][cell] = r.c[0]; s_rec[1][cell] = r.c[1]; s_rec[2][cell] = r.c[2];
            s_rec[3][cell] = r.g[0]; s_rec[4][cell] = r.g[1]; s_rec[5][cell] = r.g[2];
            s_rec[6][cell] = r.n[0]; s_rec[7][cell] = r.n[1]; s_rec[8][cell] = r.n[2];
            s_rec[9][cell] = r.z;
        }
        __syncthreads();
        const long long i = (long long)ri + s * (u0 + 2 + lx), j = (long long)rj + s * (v0 + 2 + ly);
        if (i < W && j < H) {
            auto staged = [&](int dx, int dy, rt_dn::Tap *q) {
                const int cell = (ly + 2 + dy) * kDnSide + (lx + 2 + dx);
                q->c[0] = s_rec[0][cell]; q->c[1] = s_rec[1][cell]; q->c[2] = s_rec[2][cell];
                q->g[0] = s_rec[3][cell]; q->g[1] = s_rec[4][cell]; q->g[2] = s_rec[5][cell];
                q->n[0] = s_rec[6][cell]; q->n[1] = s_rec[7][cell]; q->n[2] = s_rec[8][cell];
                q->z = s_rec[9][cell];
            };
            rt_dn::Tap centre;
            staged(0, 0, &centre);
            double out[3];
            rt_dn::level_pixel(i, j, W, H, F.L, centre, staged, out);
            const unsigned long long p = (unsigned long long)(j * W + i);
            F.cout[3 * p + 0] = out[0]; F.cout[3 * p + 1] = out[1]; F.cout[3 * p + 2] = out[2];
        }
        __syncthreads();                                                    // the next tile overwrites the records
    }
}

__global__ __launch_bounds__(kDnBlock) void denoise_finish_kernel(const double *__restrict__ c, const double *__restrict__ mod,
                                                                  unsigned long long npix, unsigned long long *__restrict__ out)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < npix; p += stride) {
        uint64_t q[3];
        rt_dn::finish(c + 3 * p, mod + 3 * p, q);
        out[3 * p + 0] = q[0]; out[3 * p + 1] = q[1]; out[3 * p + 2] = q[2];
    }
}

} // namespace rt

namespace {

// What every form of the denoiser checks, before anything is touched; none of it needs a context.
int validate_denoise(const struct rt_denoise *dn, const void *fix, int64_t spp, bool has_count, const void *feat, int64_t feat_spp,
                     int32_t width, int32_t height, const void *out)
{
    if (!dn) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: dn is NULL");
    if (!fix || !feat || !out) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: a buffer is NULL (fix, feat or out)");
    if (dn->levels < 1 || dn->levels > RT_DENOISE_MAX_LEVELS)
        return fail(RT_ERR_INVALID_ARGUMENT, "denoise: levels must be 1..%d (is %d)", RT_DENOISE_MAX_LEVELS, dn->levels);
    if (dn->flags & ~RT_DENOISE_DEMODULATE) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: unknown flags 0x%x", dn->flags);
    if (!(dn->sigma_color > 0.0) || !(dn->sigma_normal > 0.0) || !(dn->sigma_depth > 0.0) || !std::isfinite(dn->sigma_color) ||
        !std::isfinite(dn->sigma_normal) || !std::isfinite(dn->sigma_depth))
        return fail(RT_ERR_INVALID_ARGUMENT, "denoise: every sigma must be > 0 and finite (%g, %g, %g)", dn->sigma_color, dn->sigma_normal,
                    dn->sigma_depth);
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: bad width/height (%d, %d)", width, height);
    if ((long long)width * height > (1ll << 31))
        return fail(RT_ERR_INVALID_ARGUMENT, "denoise: width * height must be <= 2^31 (is %lld)", (long long)width * height);
    if (!has_count && spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: spp >= 1 without a count buffer (is %lld)", (long long)spp);
    if (feat_spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "denoise: feat_spp >= 1 (is %lld)", (long long)feat_spp);
    return RT_OK;
}

// RTIOW_DENOISE_LEVEL_KERNEL (diagnostic): -1 not set, 0 gather, 1 tile
int level_kernel_knob()
{
    const char *e = getenv("RTIOW_DENOISE_LEVEL_KERNEL");
    if (!e || !*e) return -1;
    if (!strcmp(e, "gather")) return 0;
    if (!strcmp(e, "tile")) return 1;
    return -1;
}

unsigned blocks_for(unsigned long long items)
{
    unsigned long long b = (items + rt::kDnBlock - 1) / rt::kDnBlock;
    if (b > (unsigned long long)rt::kDnMaxBlocks) b = (unsigned long long)rt::kDnMaxBlocks;
    return (unsigned)(b < 1 ? 1 : b);
}

} // namespace

extern "C" {

int rt_denoise_workspace_bytes(int32_t width, int32_t height, int64_t *out_bytes)
{
    if (!out_bytes) return fail(RT_ERR_INVALID_ARGUMENT, "denoise workspace: out_bytes is NULL");
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARGUMENT, "denoise workspace: bad width/height (%d, %d)", width, height);
    if ((long long)width * height > (1ll << 31))
        return fail(RT_ERR_INVALID_ARGUMENT, "denoise workspace: width * height must be <= 2^31 (is %lld)", (long long)width * height);
    *out_bytes = (int64_t)width * height * rt::kDnWorkDoubles * (int64_t)sizeof(double);
    return RT_OK;
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
    double *guide = (double *)d_work, *mod = guide + 4 * npix, *ca = mod + 3 * npix, *cb = ca + 3 * npix, *box = cb + 3 * npix;
    const unsigned grid = blocks_for(npix);
    hipLaunchKernelGGL(rt::denoise_prepare_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, (const unsigned long long *)d_fix,
                       (const uint32_t *)d_count, (double)spp, (const unsigned long long *)d_feat, (double)feat_spp,
                       (dn->flags & RT_DENOISE_DEMODULATE) ? 1 : 0, npix, guide, mod, ca);
    RT_HIP(hipGetLastError());
    const int knob = level_kernel_knob();
    for (int l = 0; l < dn->levels; ++l) {
        hipLaunchKernelGGL(rt::denoise_box_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, (const double *)ca, (uint32_t)width,
                           (uint32_t)height, npix, box);
        RT_HIP(hipGetLastError());
        rt::DnFrame F;
        F.guide = guide; F.cin = ca; F.box = box; F.cout = cb;
        F.width = (uint32_t)width; F.height = (uint32_t)height; F.npix = npix;
        F.L = rt_dn::level_const(dn->sigma_color, dn->sigma_normal, dn->sigma_depth, l);
        // the tiling of the sub-lattices: min(s, width) x min(s, height) of them, each ceil(ceil(width / s) / 16) tiles wide
        const unsigned long long s = (unsigned long long)F.L.step;
        const unsigned long long nri = s < (unsigned long long)width ? s : (unsigned long long)width;
        const unsigned long long nrj = s < (unsigned long long)height ? s : (unsigned long long)height;
        const unsigned long long tiles_x = (((unsigned long long)width + s - 1) / s + rt::kDnTile - 1) / rt::kDnTile;
        const unsigned long long tiles_y = (((unsigned long long)height + s - 1) / s + rt::kDnTile - 1) / rt::kDnTile;
        const unsigned long long n_tiles = nri * tiles_x * nrj * tiles_y;
        bool tile = knob < 0 ? rt::kDnTileDefault[l] : knob == 1;
        if (n_tiles >= (1ull << 31)) tile = false;                          // (the tile number is a 32-bit integer)
        if (tile) {
            rt::DnTiling T;
            T.tiles_x = (uint32_t)tiles_x; T.tiles_y = (uint32_t)tiles_y; T.nri = (uint32_t)nri; T.n_tiles = (uint32_t)n_tiles;
            const unsigned tgrid = (unsigned)(n_tiles > (unsigned long long)rt::kDnMaxBlocks ? (unsigned long long)rt::kDnMaxBlocks : n_tiles);
            hipLaunchKernelGGL(rt::denoise_level_tile_kernel, dim3(tgrid), dim3(rt::kDnBlock), 0, stream, F, T);
        } else {
            hipLaunchKernelGGL(rt::denoise_level_gather_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, F);
        }
        RT_HIP(hipGetLastError());
        double *t = ca; ca = cb; cb = t;
    }
    hipLaunchKernelGGL(rt::denoise_finish_kernel, dim3(grid), dim3(rt::kDnBlock), 0, stream, (const double *)ca, (const double *)mod, npix,
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
    const auto work = st.scratch<double>(npix * rt::kDnWorkDoubles);
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
        work.resize((size_t)width * height * rt::kDnWorkDoubles);
    } catch (...) {
        return fail(RT_ERR_OUT_OF_MEMORY, "rt_denoise_host: no memory for the workspace");
    }
    rt_dn::filter_host(fix, count, (long long)spp, feat, (long long)feat_spp, width, height, dn->levels, (dn->flags & RT_DENOISE_DEMODULATE) != 0,
                       dn->sigma_color, dn->sigma_normal, dn->sigma_depth, work.data(), out_fix);
    return RT_OK;
}

} // extern "C"
