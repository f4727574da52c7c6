// rt_api.hip -- host runtime behind include/rtiow_hip.h (C ABI of librtiow_hip.so).
//
// Owns the device-side scene, the work counter, the statistics words and the
// HIP events of one context; validates parameters; launches the persistent
// render kernel.  No CPU fallback: every entry point needs a gfx950 device.
//
// This file holds the context's life cycle, the scene upload and the host forms of the scene's tables, the shard helpers, the dense and the
// pixel-list launches with their statistics, and the conversions of the exact sums (rt_fix_to_f32_device, the two resolves) with their
// kernels.  It defines what rt_host.hpp and rt_launch.hpp declare.  The other kernel families are translation units of their own beside it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_launch.hpp"        // rt_host.hpp (rtiow_hip.h, rt_context), rt_kernels.hpp, launch_render: what rt_frames.hip and rt_dense.hip share with this file

namespace {

thread_local char g_err[512] = "";

int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    if (!v || !*v) return dflt;
    return atoi(v);
}

} // namespace

int rt_host::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

using namespace rt_host;

int rt_host::validate_params(const rt_params *p)
{
    if (!p) return fail(RT_ERR_INVALID_ARGUMENT, "params is NULL");
    if (p->width < 2 || p->height < 2)
        return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be >= 2 (u,v divide by W-1,H-1; main.rs:131-132)");
    if (p->width > 65535 || p->height > 65535)
        return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be <= 65535");
    if ((long long)p->width * p->height > 0x7fffffffLL)
        return fail(RT_ERR_INVALID_ARGUMENT, "width*height does not fit the 32-bit Philox pixel counter");
    if (p->spp < 0 || p->sample_begin < 0 || (long long)p->spp + p->sample_begin > 0x7fffffffLL)
        return fail(RT_ERR_INVALID_ARGUMENT, "spp/sample_begin out of range");
    if (p->max_depth < 0) return fail(RT_ERR_INVALID_ARGUMENT, "max_depth must be >= 0");
    if (!(p->t_min > 0.0)) return fail(RT_ERR_INVALID_ARGUMENT, "t_min must be > 0 (reference: 1e-4, main.rs:44)");
    if (p->tile_rows < 1) return fail(RT_ERR_INVALID_ARGUMENT, "tile_rows must be >= 1");
    if (p->shard_count < 1 || p->shard_index < 0 || p->shard_index >= p->shard_count)
        return fail(RT_ERR_INVALID_ARGUMENT, "need 0 <= shard_index < shard_count");
    // (a bit this library does not know would be a request it silently ignores: a caller built against a newer header finds out here)
    if (p->flags & ~RT_FLAG_KNOWN)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown flags 0x%x (this library knows 0x%x)", p->flags & ~RT_FLAG_KNOWN, RT_FLAG_KNOWN);
    return RT_OK;
}

namespace {

// rows owned by a shard: tiles t = shard_index, shard_index+shard_count, ...
int shard_rows(const rt_params *p)
{
    const long long T = p->tile_rows, H = p->height;
    const long long ntiles = (H + T - 1) / T;
    long long rows = 0;
    for (long long t = p->shard_index; t < ntiles; t += p->shard_count) {
        const long long lo = t * T;
        rows += (lo + T <= H) ? T : (H - lo);
    }
    return (int)rows;
}

} // namespace

int rt_host::ensure(DeviceBlock &block, size_t need)
{
    if (block.bytes >= need && block.ptr) return RT_OK;
    if (block.ptr) { (void)hipFree(block.ptr); block.ptr = nullptr; block.bytes = 0; }
    RT_HIP(hipMalloc(&block.ptr, need ? need : 16));
    block.bytes = need;
    return RT_OK;
}

namespace {

// What rt_scene_core.hpp states on its own of the device side, pinned here: the one file that sees both.
static_assert(rt_scene::kTablesVersion == 1, "the scene tables changed: bump kTablesVersion in rt_scene_core.hpp AND this assert, so that "
              "this file -- a hashed kernel source (bench.py, kernel_source_sha) -- changes with them");
static_assert(rt_scene::kTubeBasisErr == rt::kTubeBasisErr && rt_scene::kTubeCenterErr == rt::kTubeCenterErr && rt_scene::kFilterKU == rt::kFilterKU,
              "rt_scene_core.hpp and rt_device.hpp disagree on a filter constant");
static_assert(rt_scene::kMatStride == rt::kMatStride, "rt_scene_core.hpp and rt_params.hpp disagree on the material record");
static_assert(sizeof(rt_scene::Word4) == sizeof(uint4) && offsetof(rt_scene::Word4, x) == offsetof(uint4, x) && offsetof(rt_scene::Word4, y) == offsetof(uint4, y) &&
              offsetof(rt_scene::Word4, z) == offsetof(uint4, z) && offsetof(rt_scene::Word4, w) == offsetof(uint4, w), "Word4 must have uint4's layout");

// the two diagnostic knobs of the scene build, read at upload (rt_scene_core.hpp, tile_layout), and the context's scan mode
rt_scene::Knobs scene_knobs(int scan_mode)
{
    rt_scene::Knobs k;
    k.scan_mode = scan_mode; k.no_grid = env_int("RTIOW_NO_GRID", 0); k.grid_dim = env_int("RTIOW_GRID_DIM", 0);
    return k;
}

// releases every device table of the scene and marks the context as having none
void free_scene(rt_context *ctx)
{
    (void)hipFree(ctx->d_filt); (void)hipFree(ctx->d_geo); (void)hipFree(ctx->d_mat);
    (void)hipFree(ctx->d_btube); (void)hipFree(ctx->d_geo_slot); (void)hipFree(ctx->d_slot_orig);
    ctx->d_filt = nullptr; ctx->d_geo = ctx->d_mat = nullptr; ctx->d_btube = nullptr; ctx->d_geo_slot = nullptr; ctx->d_slot_orig = nullptr;
#ifdef RTIOW_CROSSCHECK_MODES
    ctx->x.release();
#endif
    ctx->n_spheres = -1;
}

// one table: allocate + copy; on failure the caller frees the whole scene
template <typename T>
int upload_table(T **dst, const T *src, size_t count)
{
    RT_HIP(hipMalloc((void **)dst, (count ? count : 1) * sizeof(T)));
    if (count) RT_HIP(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

} // namespace

// the scene's tables and grid, as every render kernel reads them
void rt_host::set_scene_params(const rt_context *ctx, rt::KParams &kp)
{
    kp.filt = ctx->d_filt; kp.geo = ctx->d_geo; kp.mat = ctx->d_mat;
    const rt_scene::Header &sc = ctx->scene;
    kp.n_tiles = sc.n_tiles;
#ifdef RTIOW_CROSSCHECK_MODES
    kp.x.bmat = ctx->x.d_bmat; kp.x.kpt = ctx->x.d_kpt;
    kp.x.bmat16 = ctx->x.d_bmat16; kp.x.kpt16 = ctx->x.d_kpt16; kp.x.bmatL = ctx->x.d_bmatL;
#endif
    kp.btube = ctx->d_btube; kp.tube_rho = sc.tube_rho;
    kp.geo_slot = ctx->d_geo_slot; kp.slot_orig = ctx->d_slot_orig;
    kp.n_global = sc.n_global; kp.grid_dim = sc.grid_dim;
    kp.grid_rows = 0ull;
    for (int k = 0; sc.grid_dim > 0 && (k + 1) * sc.grid_dim <= 64; ++k) kp.grid_rows |= 1ull << (k * sc.grid_dim);
    for (int k = 0; k < 8; ++k) kp.grid[k] = sc.grid[k];
    kp.scene_scale = sc.scene_scale;
    kp.n_always = sc.n_always;
    for (int e = 0; e < 8; ++e) kp.always_idx[e] = sc.always_idx[e];
}

void rt_host::fill_common_params(const rt_context *ctx, const rt_params *p, const LaunchPlan &plan, unsigned long long npix,
                                 unsigned long long total_items, unsigned long long n_blocks, void *d_fix, rt::KParams &kp)
{
    memset(&kp, 0, sizeof(kp));
    kp.width = p->width; kp.height = p->height;
    kp.spp = p->spp; kp.sample_begin = p->sample_begin; kp.max_depth = p->max_depth;
    kp.t_min = p->t_min;
    kp.k0 = (uint32_t)p->seed; kp.k1 = (uint32_t)(p->seed >> 32);
    rt_keys::fill_round_keys(kp.k0, kp.k1, kp.round_keys);          // (what the capped dense kernels read instead of rebuilding it from k0, k1)
    kp.tile_rows = 1; kp.shard_index = 0; kp.shard_count = 1;
    kp.n_spheres = ctx->n_spheres;
    kp.npix = (uint32_t)npix; kp.total_items = total_items; kp.n_blocks = (uint32_t)n_blocks;
    kp.inv_spp = p->spp > 0 ? 1.0 / (double)p->spp : 0.0;
    kp.inv_width = 1.0 / (double)p->width;
    kp.magic_spp = magic_for(p->spp);
    kp.use_ring = plan.use_ring ? 1 : 0;
    kp.block_items = plan.block_items;
    set_scene_params(ctx, kp);
    kp.fix = (unsigned long long *)d_fix;
}

int rt_host::begin_launch(rt_context *ctx, hipStream_t stream, rt::KParams &kp, int max_depth, size_t clear_bytes, int untraced_scan_mode, bool *trace)
{
    ctx->cur = (ctx->cur + 1) % rt_context::kSlots;
    ctx->d_queue = ctx->q_slots[ctx->cur]; ctx->d_stats = ctx->s_slots[ctx->cur];
    ctx->ev0 = ctx->e0_slots[ctx->cur]; ctx->ev1 = ctx->e1_slots[ctx->cur];
    if (ctx->slot_used[ctx->cur]) RT_HIP(hipStreamWaitEvent(stream, ctx->ev1, 0));
    ctx->slot_used[ctx->cur] = true;
    kp.queue = ctx->d_queue; kp.stats = ctx->d_stats;

    if (clear_bytes) RT_HIP(hipMemsetAsync(kp.fix, 0, clear_bytes, stream));
    RT_HIP(hipMemsetAsync(ctx->d_queue, 0, 64, stream));
    RT_HIP(hipMemsetAsync(ctx->d_stats, 0, 1024, stream));
    memset(&ctx->last, 0, sizeof(ctx->last));
    ctx->last.n_spheres = ctx->n_spheres;
    ctx->last.block_threads = rt::kBlock;
    ctx->zero_depth_samples = 0;
    *trace = max_depth != 0 && kp.total_items != 0;
    if (*trace) return RT_OK;
    RT_HIP(hipEventRecord(ctx->ev0, stream));
    RT_HIP(hipEventRecord(ctx->ev1, stream));
    ctx->zero_depth_samples = kp.total_items;
    ctx->last.scan_mode = untraced_scan_mode;
    ctx->launched = true;
    return RT_OK;
}

// what a pixel-list render accepts beyond validate_params: checked before anything is touched.  The checks that need no context come
// first (so a caller -- and a test -- without a device still gets the precise message), then the context's own.
int rt_host::validate_pixel_list(const rt_context *ctx, const rt_camera *cam, const rt_params *p, int64_t n_pixels)
{
    int rc = validate_params(p);
    if (rc) return rc;
    if (p->flags & (RT_FLAG_UNIFORM53 | RT_FLAG_DIAG_STATS | RT_FLAG_NO_FILTER))
        return fail(RT_ERR_INVALID_ARGUMENT, "pixel-list renders run the shipped kernel only: RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS and "
                    "RT_FLAG_NO_FILTER are not available on them (flags 0x%x)", p->flags);
    if (p->shard_count != 1)
        return fail(RT_ERR_INVALID_ARGUMENT, "pixel-list renders are not sharded: shard_count must be 1 (is %d)", p->shard_count);
    if (n_pixels < 0 || n_pixels > 0x7fffffffLL)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_pixels %lld out of range [0, 2^31)", (long long)n_pixels);
    if (!ctx || !cam) return fail(RT_ERR_INVALID_ARGUMENT, "ctx/cam is NULL");
    if (ctx->scan_mode != 5)
        return fail(RT_ERR_INVALID_ARGUMENT, "pixel-list renders need the shipped scan mode 5; this context was created under RTIOW_SCAN_MODE=%d", ctx->scan_mode);
    return RT_OK;
}

#ifdef RTIOW_CROSSCHECK_MODES
namespace rt_host {
#include "xcheck/rt_xcheck_host.inc"       // B operands of scan modes 2-4
}
#endif

namespace {

// The dense launch's kernel: the one place that maps (mode, diag, u53, small grid, blocks of 1 024) to an instantiation, and says
// which one ran (rt_stats::kernel_variant: 1 small grid, 2 U53, 4 blocks of 1 024; rt_last_dense_body).  The shipped kernel has a leaner
// instantiation for scenes whose tile grid has <= 64 cells, and a second body with the capped unit-sphere redraw (rt_dense.hip;
// RTIOW_DENSE_BODY=classic: the instantiations below): kernel_variant says the same for both.
int launch_dense(rt_context *ctx, const rt::KParams &kp, hipStream_t stream, int mode, bool diag, bool u53, bool small_grid, bool large_blocks, int *grid)
{
    const bool shipped = mode == 5 && !diag;
    ctx->last.kernel_variant = (shipped && small_grid ? 1 : 0) | (u53 ? 2 : 0) | (shipped && large_blocks ? 4 : 0);
    ctx->last_dense_body = shipped && !u53 && dense_body_is_capped(small_grid, large_blocks) ? 1 : 0;
    if (ctx->last_dense_body) return launch_dense_capped(ctx, kp, stream, small_grid, large_blocks, grid);
    if (u53) {
        if (mode == 0) return launch_render<0, false, false, true>(ctx, kp, stream, grid);
        if (small_grid) return large_blocks ? launch_render<5, false, true, true, rt::kItemBlockLarge>(ctx, kp, stream, grid)
                                            : launch_render<5, false, true, true>(ctx, kp, stream, grid);
        return large_blocks ? launch_render<5, false, false, true, rt::kItemBlockLarge>(ctx, kp, stream, grid)
                            : launch_render<5, false, false, true>(ctx, kp, stream, grid);
    }
    if (shipped) {
        if (small_grid) return large_blocks ? launch_render<5, false, true, false, rt::kItemBlockLarge>(ctx, kp, stream, grid)
                                            : launch_render<5, false, true>(ctx, kp, stream, grid);
        return large_blocks ? launch_render<5, false, false, false, rt::kItemBlockLarge>(ctx, kp, stream, grid)
                            : launch_render<5, false>(ctx, kp, stream, grid);
    }
    switch (mode * 2 + (diag ? 1 : 0)) {
    case 0: return launch_render<0, false>(ctx, kp, stream, grid);
    case 1: return launch_render<0, true>(ctx, kp, stream, grid);
    case 2: return launch_render<1, false>(ctx, kp, stream, grid);
    case 3: return launch_render<1, true>(ctx, kp, stream, grid);
#ifdef RTIOW_CROSSCHECK_MODES
    case 4: return launch_render<2, false>(ctx, kp, stream, grid);
    case 5: return launch_render<2, true>(ctx, kp, stream, grid);
    case 6: return launch_render<3, false>(ctx, kp, stream, grid);
    case 7: return launch_render<3, true>(ctx, kp, stream, grid);
    case 8: return launch_render<4, false>(ctx, kp, stream, grid);
    case 9: return launch_render<4, true>(ctx, kp, stream, grid);
#endif
    default: return launch_render<5, true>(ctx, kp, stream, grid);
    }
}

} // namespace

// ---- the exact sums' conversions: the kernels of rt_fix_to_f32_device, rt_resolve_rgba8_device and rt_resolve_rgba8_counts_device ----
namespace rt {

// exact sum -> f64 value (one rounding above 2^53)
__device__ __forceinline__ double fix_to_f64(unsigned long long q)
{
    return ((double)(uint32_t)(q >> 32) * 4294967296.0 + (double)(uint32_t)q) * (1.0 / 4294967296.0);
}

__global__ void fix_to_f32_kernel(const unsigned long long *__restrict__ fix, float *__restrict__ out, long long count)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; k < count; k += stride) out[k] = (float)fix_to_f64(fix[k]);
}

// Color::to_rgba, vec3.rs:403-421, in f64, + the row flip of main.rs:141-145.
__device__ __forceinline__ uint8_t as_u8(double x)
{   // Rust `as u8`: saturating, NaN -> 0
    if (!(x == x)) return 0;
    if (x <= 0.0) return 0;
    if (x >= 255.0) return 255;
    return (uint8_t)x;
}
__device__ __forceinline__ double clamp_r(double x, double lo, double hi)
{   // f64::clamp: NaN stays NaN
    if (x < lo) return lo;
    if (x > hi) return hi;
    return x;
}
__global__ void resolve_rgba8_kernel(const unsigned long long *__restrict__ fix, uint8_t *__restrict__ out,
                                     int width, int rows, double scale, int flip)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)width * rows;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; k < npix; k += stride) {
        const int r = (int)(k / width);
        const int i = (int)(k - (long long)r * width);
        const int dst = flip ? rows - 1 - r : r;
        const unsigned long long *q = fix + k * 3;
        uchar4 px;
        px.x = as_u8(256.0 * clamp_r(__builtin_sqrt(scale * fix_to_f64(q[0])), 0.0, 0.999));
        px.y = as_u8(256.0 * clamp_r(__builtin_sqrt(scale * fix_to_f64(q[1])), 0.0, 0.999));
        px.z = as_u8(256.0 * clamp_r(__builtin_sqrt(scale * fix_to_f64(q[2])), 0.0, 0.999));
        px.w = 255;
        reinterpret_cast<uchar4 *>(out)[(long long)dst * width + i] = px;
    }
}

// Color::to_rgba with each pixel's OWN sample count (vec3.rs:403-421 with samples_per_pixel = count[p]) + the row flip: the resolve of
// an adaptive frame.  A pixel without samples (count 0) divides by zero as the reference would: 0 * inf = NaN -> byte 0.
__global__ void resolve_rgba8_counts_kernel(const unsigned long long *__restrict__ fix, const uint32_t *__restrict__ count,
                                            uint8_t *__restrict__ out, int width, int rows, int flip)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)width * rows;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; k < npix; k += stride) {
        const int r = (int)(k / width);
        const int i = (int)(k - (long long)r * width);
        const int dst = flip ? rows - 1 - r : r;
        const unsigned long long *q = fix + k * 3;
        const double scale = 1.0 / (double)count[k];            // vec3.rs:409
        uchar4 px;
        px.x = as_u8(256.0 * clamp_r(__builtin_sqrt(scale * fix_to_f64(q[0])), 0.0, 0.999));
        px.y = as_u8(256.0 * clamp_r(__builtin_sqrt(scale * fix_to_f64(q[1])), 0.0, 0.999));
        px.z = as_u8(256.0 * clamp_r(__builtin_sqrt(scale * fix_to_f64(q[2])), 0.0, 0.999));
        px.w = 255;
        reinterpret_cast<uchar4 *>(out)[(long long)dst * width + i] = px;
    }
}

// ---- the tube filter's known-answer kernel (rt_filter_tube_device, beside rt_tube_tile_host below) ----
// The one known-answer kernel that is NOT in rt_selftest.hip: it stages its operands in LDS through the very helpers the render kernel
// calls, and compiled in a translation unit without a render kernel its address arithmetic comes out in another order (304 instructions
// instead of 308, tools/isa_fingerprint.py --all).  It is there to run the kernel's own code, so it stays in the kernel's unit.
// One tile of the MODE 5 (tube) filter exactly as the render kernel evaluates it: 64 rays against
// the 32 columns of `tile`.  h_out[ray][column][k] = lambda u_k.(c - o) as the matrix pipe returns it;
// rows_out[ray] = (lambda u_1, lambda u_2, t_1, t_2, sane).
__global__ __launch_bounds__(64) void tube_products_kernel(const double *o, const double *d, const uint4 *tile, float rho,
                                                         float *h_out, float *rows_out)
{
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    __shared__ uint4 stage[64 * 4];
    const int lane = threadIdx.x, col = lane & 31, hh = lane >> 5;
    const TubeRay T = make_tube(mk(o[3 * lane], o[3 * lane + 1], o[3 * lane + 2]),
                                mk(d[3 * lane], d[3 * lane + 1], d[3 * lane + 2]), rho);
    for (int k = 0; k < 2; ++k) for (int i = 0; i < 3; ++i) rows_out[lane * 9 + 3 * k + i] = T.u[k][i];
    rows_out[lane * 9 + 6] = T.t[0]; rows_out[lane * 9 + 7] = T.t[1]; rows_out[lane * 9 + 8] = T.sane ? 1.0f : 0.0f;
    bf16x8 A[4];
    uint32_t w[2][8];
    tube_a_words(T, w);
    tube_stage_operands(stage, lane, w, A);
    const bf16x8 b = __builtin_bit_cast(bf16x8, tile[lane]);
    const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int G = 0; G < 4; ++G) {
        const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[G], b, zero16, 0, 0, 0);
        for (int bb = 0; bb < 2; ++bb)
            for (int j = 0; j < 4; ++j) {
                const int ray = 16 * G + 8 * bb + 4 * hh + j;
                h_out[(ray * 32 + col) * 2 + 0] = acc[8 * bb + j];
                h_out[(ray * 32 + col) * 2 + 1] = acc[8 * bb + 4 + j];
            }
    }
}

} // namespace rt

extern "C" {

const char *rt_last_error(void) { return g_err; }
const char *rt_backend_name(void) { return "hip-gfx950"; }
int32_t rt_abi_version(void) { return RTIOW_HIP_ABI_VERSION; }
#ifndef RT_SOURCE_SHA
#define RT_SOURCE_SHA "unknown"
#endif
const char *rt_build_source_sha(void) { return RT_SOURCE_SHA; }

int rt_create(int32_t device_id, rt_context **out)
{
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(RT_ERR_NO_DEVICE, "no HIP device visible (%s); librtiow_hip has no CPU fallback",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= count)
        return fail(RT_ERR_INVALID_ARGUMENT, "device_id %d out of range [0,%d)", device_id, count);
    RT_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    RT_HIP(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RT_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only",
                    device_id, prop.gcnArchName);
    rt_context *ctx = new (std::nothrow) rt_context();
    if (!ctx) return fail(RT_ERR_OUT_OF_MEMORY, "host allocation failed");
    ctx->device = device_id;
    ctx->cu_count = prop.multiProcessorCount;
    ctx->blocks_per_cu = env_int("RTIOW_BLOCKS_PER_CU", 0);
    ctx->ring_min_spp = env_int("RTIOW_RING_MIN_SPP", 0);                             // (raised to the kernel's own minimum per launch)
    ctx->scan_mode = env_int("RTIOW_SCAN_MODE", 5);
#ifdef RTIOW_CROSSCHECK_MODES
    if (ctx->scan_mode < 1 || ctx->scan_mode > 5) ctx->scan_mode = 5;
#else
    if (ctx->scan_mode != 1 && ctx->scan_mode != 5) {
        const int asked = ctx->scan_mode;
        rt_destroy(ctx);
        return fail(RT_ERR_INVALID_ARGUMENT, "RTIOW_SCAN_MODE=%d: this build carries scan modes 1 and 5 (modes 2-4 need "
                    "a -DRTIOW_CROSSCHECK_MODES build)", asked);
    }
#endif
    hipError_t e1 = hipSuccess, e2 = hipSuccess, e3 = hipSuccess, e4 = hipSuccess;
    for (int k = 0; k < rt_context::kSlots; ++k) {
        hipError_t a = hipMalloc((void **)&ctx->q_slots[k], 64), b = hipMalloc((void **)&ctx->s_slots[k], 1024);
        hipError_t c = hipEventCreate(&ctx->e0_slots[k]), d = hipEventCreate(&ctx->e1_slots[k]);
        if (a != hipSuccess) e1 = a;
        if (b != hipSuccess) e2 = b;
        if (c != hipSuccess) e3 = c;
        if (d != hipSuccess) e4 = d;
    }
    ctx->d_queue = ctx->q_slots[0]; ctx->d_stats = ctx->s_slots[0]; ctx->ev0 = ctx->e0_slots[0]; ctx->ev1 = ctx->e1_slots[0];
    hipError_t e5 = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess) {
        rt_destroy(ctx);
        return fail(RT_ERR_HIP, "context setup failed on device %d", device_id);
    }
    *out = ctx;
    return RT_OK;
}

int rt_destroy(rt_context *ctx)
{
    if (!ctx) return RT_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    free_scene(ctx);
    for (int k = 0; k < rt_context::kSlots; ++k) {
        (void)hipFree(ctx->q_slots[k]); (void)hipFree(ctx->s_slots[k]);
        if (ctx->e0_slots[k]) (void)hipEventDestroy(ctx->e0_slots[k]);
        if (ctx->e1_slots[k]) (void)hipEventDestroy(ctx->e1_slots[k]);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;                                         // (the arena, the selection scratch and the path queues: DeviceBlock members)
    return RT_OK;
}

int rt_upload_scene(rt_context *ctx, const rt_sphere *spheres, int32_t n)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n < 0 || (n > 0 && !spheres)) return fail(RT_ERR_INVALID_ARGUMENT, "bad sphere list");
    if (n > RT_MAX_SPHERES) return fail(RT_ERR_INVALID_ARGUMENT, "at most %d spheres (RT_MAX_SPHERES)", RT_MAX_SPHERES);
    // (scan mode 1, the VALU cross-check filter, keeps 16-bit candidate lists in LDS)
    if (ctx->scan_mode == 1 && n > 65535) return fail(RT_ERR_INVALID_ARGUMENT, "RTIOW_SCAN_MODE=1 (the cross-check filter) takes at most 65535 spheres");
    for (int i = 0; i < n; ++i) {
        const rt_sphere &s = spheres[i];
        if (s.kind < RT_LAMBERTIAN || s.kind > RT_DIALECTRIC)
            return fail(RT_ERR_INVALID_ARGUMENT, "sphere %d: unknown material kind %d", i, s.kind);
        const double mags[4] = { s.center[0], s.center[1], s.center[2], s.radius };
        for (double v : mags)
            if (!(std::fabs(v) < 1e15))
                return fail(RT_ERR_INVALID_ARGUMENT, "sphere %d: coordinates/radius must be finite and below 1e15", i);
        // sphere.rs:37 divides by the radius: a zero radius makes every normal inf/NaN in the reference too
        if (s.radius == 0.0) return fail(RT_ERR_INVALID_ARGUMENT, "sphere %d: radius must not be zero", i);
    }
    RT_HIP(hipSetDevice(ctx->device));
    // the previous scene may still be in use by a launch on any stream
    RT_HIP(hipDeviceSynchronize());
    free_scene(ctx);
    const rt_scene::Tables T = rt_scene::build(spheres, n, scene_knobs(ctx->scan_mode));
    int rc = RT_OK;
    if (!rc && !T.btube.empty()) rc = upload_table(&ctx->d_btube, reinterpret_cast<const uint4 *>(T.btube.data()), T.btube.size());
    if (!rc && !T.geo_slot.empty()) rc = upload_table(&ctx->d_geo_slot, T.geo_slot.data(), T.geo_slot.size());
    if (!rc && !T.slot_orig.empty()) rc = upload_table(&ctx->d_slot_orig, T.slot_orig.data(), T.slot_orig.size());
    if (!rc && ctx->scan_mode == 1) rc = upload_table(&ctx->d_filt, T.filt.data(), T.filt.size());
#ifdef RTIOW_CROSSCHECK_MODES
    if (!rc) rc = xcheck_upload_tables(ctx, spheres, n, T);
#endif
    if (!rc) rc = upload_table(&ctx->d_geo, T.geo.data(), T.geo.size());
    if (!rc) rc = upload_table(&ctx->d_mat, T.mat.data(), T.mat.size());
    if (rc) {                       // a failed upload leaves NO scene behind (message of the failing call kept)
        free_scene(ctx);
        return rc;
    }
    ctx->scene = T.header;
    ctx->n_spheres = n;
    return RT_OK;
}

int rt_shard_rows(const rt_params *p, int32_t *out_rows)
{
    if (!out_rows) return fail(RT_ERR_INVALID_ARGUMENT, "out_rows is NULL");
    int rc = validate_params(p);
    if (rc) return rc;
    *out_rows = shard_rows(p);
    return RT_OK;
}

int rt_shard_row_index(const rt_params *p, int32_t compact_row, int32_t *out_j)
{
    if (!out_j) return fail(RT_ERR_INVALID_ARGUMENT, "out_j is NULL");
    int rc = validate_params(p);
    if (rc) return rc;
    if (compact_row < 0 || compact_row >= shard_rows(p))
        return fail(RT_ERR_INVALID_ARGUMENT, "compact_row out of range");
    const int lt = compact_row / p->tile_rows;
    *out_j = (lt * p->shard_count + p->shard_index) * p->tile_rows + (compact_row - lt * p->tile_rows);
    return RT_OK;
}

int rt_render_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, void *d_fix, void *stream_v)
{
    if (!ctx || !cam) return fail(RT_ERR_INVALID_ARGUMENT, "ctx/cam is NULL");
    int rc = validate_params(p);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    const int rows = shard_rows(p);
    if (rows > 0 && !d_fix) return fail(RT_ERR_INVALID_ARGUMENT, "d_fix is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;

    const long long npix = (long long)rows * p->width;
    // Work items are single pixel-samples in pixel-major order (item w = pixel * spp + sample), handed out in
    // blocks of consecutive items (plan_launch, rt_launch.hpp); the work counter counts blocks.
    const unsigned long long total_items = (unsigned long long)npix * (unsigned long long)p->spp;
    const int mode = (p->flags & RT_FLAG_NO_FILTER) ? 0 : ctx->scan_mode;
    const bool diag = (p->flags & RT_FLAG_DIAG_STATS) != 0, u53 = (p->flags & RT_FLAG_UNIFORM53) != 0;
    const bool small_grid = small_grid_scene(ctx);
    // RTIOW_LARGE_BLOCK_MIN_ITEMS moves the blocks of 1 024's last threshold (tests: 0 = every launch that qualifies otherwise; a huge value = never)
    const char *lb_env = getenv("RTIOW_LARGE_BLOCK_MIN_ITEMS");
    const unsigned long long lb_min = (lb_env && *lb_env) ? strtoull(lb_env, nullptr, 0)
                                    : (p->flags & RT_FLAG_OVERLAPPED) ? 0ull : rt::kLargeMinItems;   // (overlapped passes: the next pass fills the tail)
    const LaunchPlan plan = plan_launch(p->spp, ctx->ring_min_spp, mode == 5 && !diag, small_grid, true, total_items, lb_min);
    const unsigned long long n_blocks = (total_items + plan.block_items - 1) / plan.block_items;
    if (n_blocks > 0x7fffffffULL)
        return fail(RT_ERR_INVALID_ARGUMENT, "rows*width*spp = %llu pixel-samples in one launch: at most 2^31 blocks of %d "
                    "(split the samples over several launches with sample_begin and RT_FLAG_ACCUMULATE)", total_items, (int)plan.block_items);
    // 53-bit uniforms: instantiated for the shipped scan mode (both grid variants) and for RT_FLAG_NO_FILTER
    if (u53 && (diag || (mode != 0 && mode != 5)))
        return fail(RT_ERR_INVALID_ARGUMENT, "RT_FLAG_UNIFORM53 runs with scan mode 5 (the default) or RT_FLAG_NO_FILTER, without RT_FLAG_DIAG_STATS");
    rt::KParams kp;
    fill_common_params(ctx, p, plan, (unsigned long long)npix, total_items, n_blocks, d_fix, kp);
    static_assert(sizeof(rt::KCamera) == sizeof(rt_camera), "camera layouts must match");
    memcpy(&kp.cam, cam, sizeof(rt_camera));
    kp.tile_rows = p->tile_rows; kp.shard_index = p->shard_index; kp.shard_count = p->shard_count;
    kp.rows = rows;
    kp.magic_width = magic_for(p->width); kp.magic_tile = magic_for(p->tile_rows);
    const size_t clear_bytes = (p->flags & RT_FLAG_ACCUMULATE) ? 0 : (size_t)npix * 3 * sizeof(unsigned long long);
    return run_launch(ctx, stream, kp, p->max_depth, clear_bytes, 0, [&](int *grid) {
        ctx->last.scan_mode = mode;
        return launch_dense(ctx, kp, stream, mode, diag, u53, small_grid, plan.large_blocks, grid);
    });
}

int rt_last_stats(rt_context *ctx, rt_stats *stats)
{
    if (!ctx || !stats) return fail(RT_ERR_INVALID_ARGUMENT, "ctx/stats is NULL");
    if (!ctx->launched) return fail(RT_ERR_INVALID_ARGUMENT, "no launch to report on");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.0f;
    RT_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    unsigned long long h[80];
    RT_HIP(hipMemcpy(h, ctx->d_stats, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 64; ++k) ctx->last.live_per_bounce[k] = h[16 + k];
    ctx->last.rays_traced = h[0];
    ctx->last.samples = h[1] + ctx->zero_depth_samples;
    ctx->last.candidates = h[2];
    ctx->last.exact_roots = h[3];
    ctx->last.direct_samples = h[4];
    ctx->last.sphere_tests = h[0] * (unsigned long long)(ctx->last.n_spheres > 0 ? ctx->last.n_spheres : 0);
    ctx->last.kernel_ms = ms;
    *stats = ctx->last;
    return RT_OK;
}

#if defined(RT_PHASE_STAMPS) || defined(RT_BLOCK_COUNTS) || defined(RT_EXIT_TIMES) || defined(RT_LDS_CONFLICTS)
extern "C" int rt_debug_phase_cycles(rt_context *ctx, unsigned long long out[8])
{
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipEventSynchronize(ctx->ev1));
    RT_HIP(hipMemcpy(out, ctx->d_stats + 8, 64, hipMemcpyDeviceToHost));
    return RT_OK;
}
extern "C" int rt_debug_phase_cycles16(rt_context *ctx, unsigned long long out[16])      // the 8 above + the finer split at stats[80..87]
{
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipEventSynchronize(ctx->ev1));
    RT_HIP(hipMemcpy(out, ctx->d_stats + 8, 64, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(out + 8, ctx->d_stats + 80, 64, hipMemcpyDeviceToHost));
    return RT_OK;
}
#endif

int rt_fix_to_f32_device(rt_context *ctx, const void *d_fix, int64_t count, void *d_out_f32, void *stream_v)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (count < 0 || (count > 0 && (!d_fix || !d_out_f32))) return fail(RT_ERR_INVALID_ARGUMENT, "bad buffers");
    if (count == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rt::fix_to_f32_kernel, dim3(grid_256(count)), dim3(256), 0, (hipStream_t)stream_v,
                       (const unsigned long long *)d_fix, (float *)d_out_f32, (long long)count);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_resolve_rgba8_device(rt_context *ctx, const void *d_fix, int32_t width, int32_t rows,
                            int64_t spp, int32_t flip, void *d_rgba, void *stream_v)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (width < 1 || rows < 0 || spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "bad width/rows/spp");
    if (rows == 0) return RT_OK;
    if (!d_fix || !d_rgba) return fail(RT_ERR_INVALID_ARGUMENT, "bad buffers");
    RT_HIP(hipSetDevice(ctx->device));
    const double scale = 1.0 / (double)spp;            // vec3.rs:409
    hipLaunchKernelGGL(rt::resolve_rgba8_kernel, dim3(grid_256((long long)width * rows)), dim3(256), 0, (hipStream_t)stream_v,
                       (const unsigned long long *)d_fix, (uint8_t *)d_rgba, (int)width, (int)rows, scale, (int)flip);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_render(rt_context *ctx, const rt_camera *cam, const rt_params *p,
              float *out_sum, uint64_t *out_fix, rt_stats *stats)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    int rc = validate_params(p);
    if (rc) return rc;
    const int rows = shard_rows(p);
    const size_t count = (size_t)rows * p->width * 3;
    if (count > 0 && !out_sum && !out_fix) return fail(RT_ERR_INVALID_ARGUMENT, "no output buffer");
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const auto sums = out_fix ? st.out(out_fix, count) : st.scratch<uint64_t>(count);      // (rendered whether or not the caller asks)
    const auto f32 = st.out(out_sum, count);
    if ((rc = st.commit())) return rc;
    rt_params q = *p;
    q.flags &= ~RT_FLAG_ACCUMULATE;                     // host form always starts from zero
    rc = rt_render_device(ctx, cam, &q, st.ptr(sums), ctx->own_stream);
    if (rc) return rc;
    if (out_sum) {
        rc = rt_fix_to_f32_device(ctx, st.ptr(sums), (int64_t)count, st.ptr(f32), ctx->own_stream);
        if (rc) return rc;
    }
    RT_HIP(st.finish());
    if (stats) return rt_last_stats(ctx, stats);
    return RT_OK;
}

int rt_resolve_rgba8(rt_context *ctx, const uint64_t *fix, int32_t width, int32_t rows,
                     int64_t spp, int32_t flip, uint8_t *out_rgba)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (width < 1 || rows < 0 || spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "bad width/rows/spp");
    if (rows == 0) return RT_OK;
    if (!fix || !out_rgba) return fail(RT_ERR_INVALID_ARGUMENT, "bad buffers");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)width * rows;
    Stage st(ctx);
    const auto sums = st.in(fix, npix * 3);
    const auto rgba = st.out(out_rgba, npix * 4);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    rc = rt_resolve_rgba8_device(ctx, st.ptr(sums), width, rows, spp, flip, st.ptr(rgba), ctx->own_stream);
    if (rc) return rc;
    RT_HIP(st.finish());
    return RT_OK;
}

// main.rs:122-145 in one call: the exact sums never leave the device; 4 bytes per pixel come back, straight into the caller's
// (pageable) buffer.  Measured at 1200x675 (profiles/r05_end_to_end.txt): wall - kernel = 0.16 ms with this plain copy, 0.27 ms
// through a pinned landing buffer + memcpy, 0.88 ms for rt_render + rt_resolve_rgba8 (the sums out and in again).
int rt_render_rgba8(rt_context *ctx, const rt_camera *cam, const rt_params *p, int32_t flip,
                    uint8_t *out_rgba, rt_stats *stats)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    int rc = validate_params(p);
    if (rc) return rc;
    if (p->spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_rgba8 needs spp >= 1 (to_rgba divides by the sample count, vec3.rs:409)");
    const int rows = shard_rows(p);
    const size_t npix = (size_t)rows * p->width;
    if (npix > 0 && !out_rgba) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgba is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const auto sums = st.scratch<uint64_t>(npix * 3);
    const auto rgba = st.out(out_rgba, npix * 4);
    if ((rc = st.commit())) return rc;
    rt_params q = *p;
    q.flags &= ~RT_FLAG_ACCUMULATE;                     // host form always starts from zero
    rc = rt_render_device(ctx, cam, &q, st.ptr(sums), ctx->own_stream);
    if (rc) return rc;
    if (npix > 0) {
        rc = rt_resolve_rgba8_device(ctx, st.ptr(sums), p->width, rows, (int64_t)p->spp, flip, st.ptr(rgba), ctx->own_stream);
        if (rc) return rc;
    }
    RT_HIP(st.finish());
    if (stats) return rt_last_stats(ctx, stats);
    return RT_OK;
}

// ---- pixel lists -------------------------------------------------------------------------------------------------------------
int rt_render_pixels_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const uint32_t *d_pixels,
                            int64_t n_pixels, void *d_fix, void *stream_v)
{
    int rc = validate_pixel_list(ctx, cam, p, n_pixels);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (n_pixels == 0) return RT_OK;
    if (!d_pixels || !d_fix) return fail(RT_ERR_INVALID_ARGUMENT, "d_pixels/d_fix is NULL");
    const unsigned long long total_items = (unsigned long long)n_pixels * (unsigned long long)p->spp;
    // work blocks as the shipped kernel's ring of 2 x 16 pixel slots takes them (plan_launch), never the blocks of 1 024
    const LaunchPlan plan = plan_launch(p->spp, ctx->ring_min_spp, true, false, false, total_items, 0);
    const unsigned long long n_blocks = (total_items + plan.block_items - 1) / plan.block_items;
    if (n_blocks > 0x7fffffffULL)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_pixels*spp = %llu pixel-samples in one launch: at most 2^31 blocks of %d", total_items, (int)plan.block_items);
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;

    rt::KParams kp;
    fill_common_params(ctx, p, plan, (unsigned long long)n_pixels, total_items, n_blocks, d_fix, kp);
    memcpy(&kp.cam, cam, sizeof(rt_camera));
    kp.rows = 1;                                                         // (rows and the sharding fields are unused by the variant; no magic_width)
    kp.pix_list = d_pixels;
    const size_t clear_bytes = (p->flags & RT_FLAG_ACCUMULATE) ? 0 : (size_t)n_pixels * 3 * sizeof(unsigned long long);
    return run_launch(ctx, stream, kp, p->max_depth, clear_bytes, 0, [&](int *grid) {
        const bool small_grid = small_grid_scene(ctx);
        ctx->last.scan_mode = 5;
        ctx->last.kernel_variant = 8 | (small_grid ? 1 : 0);
        return small_grid ? launch_render<5, false, true, false, rt::kItemBlockList>(ctx, kp, stream, grid)      // (the pixel-list instantiations)
                          : launch_render<5, false, false, false, rt::kItemBlockList>(ctx, kp, stream, grid);
    });
}

int rt_render_pixels(rt_context *ctx, const rt_camera *cam, const rt_params *p, const uint32_t *pixels, int64_t n_pixels,
                     uint64_t *out_fix, rt_stats *stats)
{
    int rc = validate_pixel_list(ctx, cam, p, n_pixels);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (n_pixels == 0) return RT_OK;
    if (!pixels || !out_fix) return fail(RT_ERR_INVALID_ARGUMENT, "pixels/out_fix is NULL");
    const long long npix_frame = (long long)p->width * p->height;
    for (int64_t k = 0; k < n_pixels; ++k)
        if ((long long)pixels[k] >= npix_frame)
            return fail(RT_ERR_INVALID_ARGUMENT, "pixels[%lld] = %u is not a pixel of a %d x %d frame", (long long)k, pixels[k], p->width, p->height);
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const auto sums = st.out(out_fix, (size_t)n_pixels * 3);
    const auto list = st.in(pixels, (size_t)n_pixels);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    rt_params q = *p;
    q.flags &= ~RT_FLAG_ACCUMULATE;                     // host form always starts from zero
    rc = rt_render_pixels_device(ctx, cam, &q, st.ptr(list), n_pixels, st.ptr(sums), ctx->own_stream);
    if (rc) return rc;
    RT_HIP(st.finish());
    if (stats) return rt_last_stats(ctx, stats);
    return RT_OK;
}

int rt_resolve_rgba8_counts_device(rt_context *ctx, const void *d_fix, const void *d_count, int32_t width, int32_t rows,
                                   int32_t flip, void *d_rgba, void *stream_v)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (width < 1 || rows < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad width/rows");
    if (rows == 0) return RT_OK;
    if (!d_fix || !d_count || !d_rgba) return fail(RT_ERR_INVALID_ARGUMENT, "bad buffers");
    RT_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rt::resolve_rgba8_counts_kernel, dim3(grid_256((long long)width * rows)), dim3(256), 0, (hipStream_t)stream_v,
                       (const unsigned long long *)d_fix, (const uint32_t *)d_count, (uint8_t *)d_rgba, (int)width, (int)rows, (int)flip);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_resolve_rgba8_counts(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int32_t width, int32_t rows,
                            int32_t flip, uint8_t *out_rgba)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (width < 1 || rows < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad width/rows");
    if (rows == 0) return RT_OK;
    if (!fix || !count || !out_rgba) return fail(RT_ERR_INVALID_ARGUMENT, "bad buffers");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)width * rows;
    Stage st(ctx);
    const auto sums = st.in(fix, npix * 3);
    const auto rgba = st.out(out_rgba, npix * 4);
    const auto counts = st.in(count, npix);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    rc = rt_resolve_rgba8_counts_device(ctx, st.ptr(sums), st.ptr(counts), width, rows, flip, st.ptr(rgba), ctx->own_stream);
    if (rc) return rc;
    RT_HIP(st.finish());
    return RT_OK;
}

int rt_tube_tile_host(const rt_sphere *spheres32, uint32_t *out_words, float *out_bound, float *out_rho)
{
    if (!spheres32 || !out_words || !out_bound || !out_rho) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    rt_scene::Word4 tile[64];
    *out_rho = rt_scene::full_tile(spheres32, tile, out_bound);
    memcpy(out_words, tile, sizeof(tile));
    return RT_OK;
}

int rt_filter_tube_device(rt_context *ctx, const double *o, const double *d, const rt_sphere *spheres32,
                          float *out_h, float *out_rows, float *out_bound, float *out_rho)
{
    if (!ctx || !o || !d || !spheres32 || !out_h || !out_rows || !out_bound || !out_rho)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_HIP(hipSetDevice(ctx->device));
    rt_scene::Word4 tile[64];
    const float rho = *out_rho = rt_scene::full_tile(spheres32, tile, out_bound);
    Stage st(ctx);                                      // 64 rays, one tile of 64 operand words, 32 columns x 2 products and 9 row values per ray
    const auto ro = st.in(o, 64 * 3), rd = st.in(d, 64 * 3);
    const auto words = st.in(reinterpret_cast<const uint4 *>(tile), 64);
    const auto h = st.out(out_h, 64 * 32 * 2), rows = st.out(out_rows, 64 * 9);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    hipLaunchKernelGGL(rt::tube_products_kernel, dim3(1), dim3(64), 0, ctx->own_stream,
                       st.ptr(ro), st.ptr(rd), st.ptr(words), rho, st.ptr(h), st.ptr(rows));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
    return RT_OK;
}

int rt_tile_layout_host(const rt_sphere *spheres, int32_t n, int32_t out_dims[2], float out_grid[8], int32_t *out_slot_of, int32_t cap)
{
    if (!spheres || n < 0 || n > RT_MAX_SPHERES || !out_dims || !out_grid || (!out_slot_of && cap > 0)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_tile_layout_host: bad argument");
    const rt_scene::TileLayout L = rt_scene::list_layout(spheres, n, scene_knobs(5));
    out_dims[0] = L.grid_dim; out_dims[1] = L.n_global;
    for (int k = 0; k < 8; ++k) out_grid[k] = L.grid[k];
    if ((size_t)cap < L.slot_of.size()) return fail(RT_ERR_INVALID_ARGUMENT, "rt_tile_layout_host: out_slot_of too small");
    for (size_t k = 0; k < L.slot_of.size(); ++k) out_slot_of[k] = L.slot_of[k];
    return (int)L.slot_of.size();
}

} // extern "C"
