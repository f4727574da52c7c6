// rt_host.hpp -- what the translation units of librtiow_hip.so share: the context, the error path, parameter validation and the ONE
// launch path of the render kernel, which the dense, the pixel-list and the frame-batch entry points all take: plan_launch (work-block
// size, ring, blocks of 1 024: a pure function of a few integers), magic_for, fill_common_params, run_launch (slot, clears, the
// "nothing to trace" exit, the kernel, the tail) and launch_render (one instantiation).  An entry point keeps its own validation, its
// own few KParams fields and its kernel choice.  rt_api.hip defines the functions declared here (and every kernel but the frame-batch
// instantiations of render_kernel, which rt_frames.hip owns, and the capped dense ones, which rt_dense.hip owns).
// The host-buffer entry points share their plumbing here as well: StageLayout / Stage (one device arena per context, laid out per call),
// timed_section (a pair of events of the call's own around its kernels) and grid_256.
// rt_scene_core.hpp (included here for rt_context's Header) builds the scene's tables on the host, pure and HIP-free; a change to what a
// table holds bumps its kTablesVersion and the static_assert on it in rt_api.hip, so that the hashed sources change with it.
#pragma once
#include <hip/hip_runtime.h>

#include "rtiow_hip.h"
#include "rt_kernels.hpp"
#include "rt_scene_core.hpp"
#include "rt_round_keys.hpp"
#ifdef RTIOW_CROSSCHECK_MODES
#include "xcheck/rt_xcheck_host_ctx.hpp"
#endif

namespace rt_host {
int fail(int code, const char *fmt, ...);          // records the thread's rt_last_error message, returns `code`
}

#define RT_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return rt_host::fail(e_ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP,        \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct rt_context {
    int device = 0;
    int cu_count = 0;
    float *d_filt = nullptr;       // [n][4] f32 filter records (MODE 1)
    double *d_geo = nullptr;       // [n][4] exact geometry
    double *d_mat = nullptr;       // [n][kMatStride] exact materials
    uint4 *d_btube = nullptr;      // [tiles/2 + 1][64] MODE 5 (tube filter) B operands
    double *d_geo_slot = nullptr;  // MODE 5: [slots][4] exact geometry in table (slot) order
    uint32_t *d_slot_orig = nullptr;   // MODE 5: [slots] list index of the sphere in each column of the table
    rt_scene::Header scene;        // the scene's scalars: tile counts, the grid, the radius floor, the always-exact list (rt_scene_core.hpp)
#ifdef RTIOW_CROSSCHECK_MODES
    XcheckScene x;                 // device tables of scan modes 2-4 (xcheck/rt_xcheck_host_ctx.hpp)
#endif
    int scan_mode = 5;             // filter: 5 tube bf16x2 MFMA (default, shipped), 1 VALU + scalar loads (cross-check);
                                   // with -DRTIOW_CROSSCHECK_MODES also 2 f32 MFMA, 3 bf16x3 MFMA, 4 lifted bf16x3 MFMA
    int n_spheres = -1;
    // Per-launch state -- the work counter, the statistics words and the two events -- exists kSlots times, used in turn: a context
    // may have kSlots renders in flight (on different streams: the second fills the first one's end-of-launch tail); the fields
    // below name the slot of the LATEST launch, which is what rt_last_stats reports on.
    static constexpr int kSlots = 2;
    unsigned int *q_slots[kSlots] = {nullptr, nullptr};
    unsigned long long *s_slots[kSlots] = {nullptr, nullptr};
    hipEvent_t e0_slots[kSlots] = {nullptr, nullptr}, e1_slots[kSlots] = {nullptr, nullptr};
    bool slot_used[kSlots] = {false, false};
    int cur = 0;
    unsigned int *d_queue = nullptr;
    unsigned long long *d_stats = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t own_stream = nullptr;
    bool launched = false;
    unsigned long long zero_depth_samples = 0;
    rt_stats last{};
    // The staging arena of the host-buffer entry points (rt_host::Stage below): whatever the call in progress laid out in it, nothing
    // between calls.  Device-form entry points never touch it.
    void *d_arena = nullptr; size_t arena_bytes = 0;
    int blocks_per_cu = 0;     // 0 = occupancy query
    // rt_select_pixels_device's scratch (noisy / active flags, the workgroups' counts): a device form's, on the caller's stream, so not
    // in the arena -- rt_render_adaptive calls it while its own frame state lives there
    void *d_sel = nullptr; size_t sel_bytes = 0;
    int last_dense_body = 0;              // rt_last_dense_body (rtiow_hip_diag.h): 1 when the latest rt_render_device launch ran a capped-redraw kernel of rt_dense.hip, else 0
    int ring_min_spp = 0;                 // RTIOW_RING_MIN_SPP (diagnostic): spp per launch from which block sums are kept in LDS (0: the kernel's own minimum)
};

namespace rt_host {

int validate_params(const rt_params *p);
int ensure(void **ptr, size_t *have, size_t need);
void set_scene_params(const rt_context *ctx, rt::KParams &kp);

// the grid of the element-wise kernels: 256 threads a block, at most 8 192 blocks (their grid-stride loops take the rest)
inline unsigned grid_256(long long n)
{
    const long long blocks = (n + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

// Where the blocks of one host-form call lie in the arena: add(bytes) gives the byte offset of a new block.  Every block starts on a
// 256-byte boundary (what hipMalloc gives a buffer of its own; the kernels' 16-byte loads rely on it), in the order declared; a block
// of 0 bytes occupies nothing.  Pure arithmetic, no HIP call (tests/stage_layout_table.cpp tabulates it).
struct StageLayout {
    size_t total = 0;
    size_t add(size_t bytes)
    {
        const size_t offset = total;
        total += (bytes + 255) & ~(size_t)255;
        return offset;
    }
};

// One host-form call's use of the arena.  THE RULE: device-form entry points never touch the arena; a host-form entry point lays its
// blocks out once (add ... commit), before its first copy, and from then on calls only device forms -- so nothing can move or reuse a
// block while the call's work is in flight on own_stream.  commit() grows the arena to this call's total with ensure(): never shrunk,
// contents not preserved.  up / down / sync are hipMemcpyAsync / hipStreamSynchronize on ctx->own_stream.
class Stage {
public:
    explicit Stage(rt_context *ctx) : ctx_(ctx) {}
    size_t add(size_t bytes) { return layout_.add(bytes); }
    int commit() { return ensure(&ctx_->d_arena, &ctx_->arena_bytes, layout_.total); }
    template <class T = void> T *at(size_t block) const { return reinterpret_cast<T *>(static_cast<char *>(ctx_->d_arena) + block); }
    hipError_t up(size_t block, const void *src, size_t bytes) const { return hipMemcpyAsync(at(block), src, bytes, hipMemcpyHostToDevice, ctx_->own_stream); }
    hipError_t down(void *dst, size_t block, size_t bytes) const { return hipMemcpyAsync(dst, at(block), bytes, hipMemcpyDeviceToHost, ctx_->own_stream); }
    hipError_t sync() const { return hipStreamSynchronize(ctx_->own_stream); }
private:
    rt_context *ctx_;
    StageLayout layout_;
};

// Times what body() enqueues on ctx->own_stream with a pair of events of this call's own (the context's belong to its launch slots),
// created here and destroyed on every path: the first is recorded before body -- after the caller's uploads --, the second after it and
// before downloads(), so *kernel_ms (may be NULL) covers the kernels only; then the stream is synchronised.  body returns a device
// form's code, which is passed on as it is with its own message; downloads returns a hipError_t; a HIP failure is "<name>: <error>".
template <class Body, class Downloads>
int timed_section(rt_context *ctx, const char *name, float *kernel_ms, Body body, Downloads downloads)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RT_HIP(hipEventCreate(&e0));
    int rc = RT_OK;
    hipError_t he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, ctx->own_stream);
    if (he == hipSuccess && !(rc = body())) {
        he = hipEventRecord(e1, ctx->own_stream);
        if (he == hipSuccess) he = downloads();
        if (he == hipSuccess) he = hipStreamSynchronize(ctx->own_stream);
        float ms = 0.0f;
        if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
        if (he == hipSuccess && kernel_ms) *kernel_ms = ms;
    }
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (he != hipSuccess) return fail(RT_ERR_HIP, "%s: %s", name, hipGetErrorString(he));
    return RT_OK;
}

// the shipped kernel has a leaner instantiation for scenes whose tile grid (with the tiles every ray scans) has <= 64 cells
inline bool small_grid_scene(const rt_context *ctx) { return ctx->scene.grid_dim > 0 && ctx->scene.n_global + ctx->scene.grid_dim * ctx->scene.grid_dim <= 64; }

// udiv_small (rt_kernels.hpp): numerators are < d + kItemBlockLarge (spp, width) or < 65536 (rows / tile_rows), so for
// d < 2^15 the product x * d stays below 2^32 and floor(x * M / 2^32) is the exact quotient
inline uint32_t magic_for(long long d)
{
    return (d <= 1 || d >= 32768) ? 0u : (uint32_t)(0x100000000ULL / (unsigned long long)d + 1ULL);
}

// How a launch is cut into work blocks.  Block sums in LDS (use_ring): a block's consecutive samples must touch no more pixels than
// its sums have slots -- ceil((items - 1) / spp) + 1 <= 8, or 16 on the shipped kernels (scan mode 5 without the diagnostic counters)
// --: blocks of 256 from 37 (17) samples per pixel on, and below that the largest multiple of 64 (a block is started 64 samples at a
// time) that fits: 192, 128 or 64 pixel-samples, down to 9 (5) samples per pixel.  Fewer, or fewer than ring_min_spp
// (RTIOW_RING_MIN_SPP, tests): every sample is added to the frame buffer with three 64-bit atomics of its own -- a quarter of the frame
// time at 20-32 samples per pixel (1200x675x32: 5.46 ms that way, 4.04 ms with block sums) -- in blocks of 256.
// Blocks of kItemBlockLarge (large_blocks) for launches that are long enough for their last blocks not to matter (rt_kernels.hpp): the
// shipped kernel, block sums in LDS, >= 147 samples per pixel (69 for scenes on the small-grid kernel), >= large_min_items
// pixel-samples; never on pixel lists and frame batches (large_allowed).  The large-grid kernel's instantiation for blocks of 1 024
// keeps a ring of 4 x 8: a launch that will take it is sized for 8 slots.
struct LaunchPlan {
    bool use_ring;
    unsigned block_items;      // KParams::block_items: kItemBlockLarge with large_blocks, else the ring's block, else kItemBlock
    bool large_blocks;
};
inline LaunchPlan plan_launch(int spp, int ring_min_spp, bool shipped_kernel, bool small_grid, bool large_allowed,
                              unsigned long long total_items, unsigned long long large_min_items)
{
    const bool large_fits = shipped_kernel && large_allowed && spp >= ring_min_spp && total_items >= large_min_items &&
                            spp >= (small_grid ? rt::kLargeMinSppSmallGrid : rt::kLargeMinSpp);
    const unsigned slots = (shipped_kernel && (small_grid || !large_fits) ? 2u : 1u) * (unsigned)rt::kRingSlots;
    unsigned ring_block = 0;
    for (unsigned items = rt::kItemBlock; items >= 64u && spp >= 1; items -= 64u)
        if ((items - 1u + (unsigned)spp - 1u) / (unsigned)spp + 1u <= slots) { ring_block = items; break; }
    LaunchPlan plan;
    plan.use_ring = ring_block != 0u && spp >= ring_min_spp;
    plan.large_blocks = large_fits && plan.use_ring && ring_block == (unsigned)rt::kItemBlock;
    plan.block_items = plan.large_blocks ? rt::kItemBlockLarge : plan.use_ring ? ring_block : (unsigned)rt::kItemBlock;
    return plan;
}

// The KParams fields every launch path fills the same way (the rest is zero): image size, samples, depth, key, the plan, the item and
// block counts, the scene's tables and the sums.  The sharding fields say "one shard" (rt_render_device overwrites them); rows,
// magic_width, magic_tile, the camera(s), pix_list and the frame fields are the caller's.
void fill_common_params(const rt_context *ctx, const rt_params *p, const LaunchPlan &plan, unsigned long long npix,
                        unsigned long long total_items, unsigned long long n_blocks, void *d_fix, rt::KParams &kp);
// What every launch does before its kernel: takes the other slot of per-launch state (if the launch that used it last is still running
// on another stream, `stream` waits for it -- the host does not; a call is validated BEFORE it takes a slot), clears clear_bytes of
// d_fix (0: RT_FLAG_ACCUMULATE) and the slot's counters, resets what rt_last_stats reports.  *trace: there is something
// to trace; else (max_depth 0 or no items: ray_color(depth <= 0) is black without tracing, main.rs:40-42) both events are
// recorded, the launch counts as made and reports untraced_scan_mode.
int begin_launch(rt_context *ctx, hipStream_t stream, rt::KParams &kp, int max_depth, size_t clear_bytes, int untraced_scan_mode, bool *trace);

// One launch from slot to tail; launch(&grid) picks and starts the kernel (launch_render) and sets ctx->last.scan_mode / kernel_variant.
template <class Launch>
int run_launch(rt_context *ctx, hipStream_t stream, rt::KParams &kp, int max_depth, size_t clear_bytes, int untraced_scan_mode, Launch launch)
{
    bool trace = false;
    int grid = 0;
    int rc = begin_launch(ctx, stream, kp, max_depth, clear_bytes, untraced_scan_mode, &trace);
    if (rc || !trace) return rc;
    rc = launch(&grid);
    if (rc) return rc;
    ctx->launched = true;
    ctx->last.grid_blocks = grid;
    return RT_OK;
}

template <int MODE, bool DIAG, bool SMALLGRID = false, bool U53 = false, int ITEMS = rt::kItemBlock>
int launch_render(rt_context *ctx, const rt::KParams &kp, hipStream_t stream, int *grid_out)
{
    int per_cu = ctx->blocks_per_cu;
    if (per_cu <= 0) {
        int occ = 0;
        RT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, rt::render_kernel<MODE, DIAG, SMALLGRID, U53, ITEMS>, rt::kBlock, 0));
        per_cu = occ < 1 ? 1 : (occ > 8 ? 8 : occ);
    }
    // persistent grid, but never more lanes than there are work items
    long long grid = (long long)ctx->cu_count * per_cu;
    const long long need = (long long)((kp.total_items + rt::kBlock - 1) / rt::kBlock);
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    *grid_out = (int)grid;
    RT_HIP(hipEventRecord(ctx->ev0, stream));
    hipLaunchKernelGGL((rt::render_kernel<MODE, DIAG, SMALLGRID, U53, ITEMS>), dim3((unsigned)grid), dim3(rt::kBlock), 0, stream, kp);
    RT_HIP(hipGetLastError());
    RT_HIP(hipEventRecord(ctx->ev1, stream));
    return RT_OK;
}

// rt_dense.hip: the dense launch's instantiations with the capped unit-sphere redraw (ITEMS = kItemBlockDense / kItemBlockDenseLarge).
// kDenseCappedDefault[small grid][blocks of 1 024]: the launches that take them when RTIOW_DENSE_BODY is not set.  Measured, interleaved with the
// classic body in both orders (profiles/capped_redraw_ab.txt): small grid on blocks of 1 024 (1200x675x500) -1.1 .. -1.3 %: the default; small grid on
// blocks of 256 -0.8 .. -0.9 % at 1200x675x100 but +0.4 .. +1.5 % on the 0.65 ms launch 400x225x10, large grid +0.3 % (blocks of 1 024) and +0.6 %
// (blocks of 256): those three stay on the classic body and keep the capped one behind RTIOW_DENSE_BODY=capped.
constexpr bool kDenseCappedDefault[2][2] = {{false, false}, {false, true}};
bool dense_body_is_capped(bool small_grid, bool large_blocks);
int launch_dense_capped(rt_context *ctx, const rt::KParams &kp, hipStream_t stream, bool small_grid, bool large_blocks, int *grid_out);

} // namespace rt_host
