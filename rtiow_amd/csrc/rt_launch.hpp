// rt_launch.hpp -- the ONE launch path of the render kernel, which the dense, the pixel-list and the frame-batch entry points all take:
// plan_launch (work-block size, ring, blocks of 1 024: a pure function of a few integers), magic_for, fill_common_params, run_launch (slot,
// clears, the "nothing to trace" exit, the kernel, the tail) and launch_render (one instantiation).  An entry point keeps its own
// validation, its own few KParams fields and its kernel choice.
// Only the translation units that instantiate render_kernel include this file -- rt_api.hip, rt_frames.hip, rt_dense.hip -- and
// tests/launch_plan_table.cpp, which tabulates plan_launch and magic_for; everything else takes rt_host.hpp and never sees the kernel.
// rt_api.hip defines fill_common_params and begin_launch, rt_dense.hip dense_body_is_capped and launch_dense_capped.
#pragma once
#include "rt_host.hpp"
#include "rt_kernels.hpp"

namespace rt_host {

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
// Blocks of kItemBlockLarge (large_blocks) for launches that are long enough for their last blocks not to matter (rt_params.hpp): the
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

// Lane-striped block sums (render_kernel, kStriped: the capped dense kernels whose ring has 16 pixel slots).  A block of block_items consecutive
// samples touches at most ceil((block_items - 1) / spp) + 1 pixels; S, the smallest power of two that holds them (at least 4), is how many of the 16
// slots the launch can use at all, and the slots above them hold further copies, R = 16 / S replicas in all: 4 replicas on blocks of 1 024 from 341 samples per
// pixel, 2 from 147; on blocks of 256 from 85 and from 37.  mask = 15 & ~(S - 1), the replica's bits of a slot number, goes into KParams (stripe_mask).
// Without block sums, on any other kernel, or where a block may touch more than 8 pixels: one replica, mask = 0, every address as it was.
struct StripePlan {
    unsigned slots, replicas;  // S, R
    unsigned mask;             // KParams::stripe_mask
};
inline StripePlan plan_stripes(bool use_ring, unsigned block_items, int spp, bool striped_kernel)
{
    StripePlan sp = {2u * (unsigned)rt::kRingSlots, 1u, 0u};
    if (!use_ring || !striped_kernel || spp < 1 || block_items < 1u) return sp;
    const unsigned touched = (block_items - 1u + (unsigned)spp - 1u) / (unsigned)spp + 1u;
    unsigned s = 4u;
    while (s < touched && s < sp.slots) s <<= 1;
    if (s >= sp.slots) return sp;
    sp.replicas = sp.slots / s; sp.slots = s; sp.mask = 15u & ~(s - 1u);
    return sp;
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
