// rt_params.hpp -- the kernel-argument block (KCamera, KParams) and the launch constants: what every translation unit of librtiow_hip.so
// needs of the render kernel without seeing it.  No kernel and no __device__ function lives here; the kernel is rt_kernels.hpp, the host
// code that fills the block rt_launch.hpp and rt_api.hip.
// A change to KParams or to a constant below bumps kParamsVersion AND the static_assert on it in rt_kernels.hpp: that file is one of
// bench.py's hashed kernel sources and this header is not, so the edit there is what moves kernel_source_sha (as kTablesVersion does for
// rt_scene_core.hpp through rt_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef RTIOW_CROSSCHECK_MODES
#include "xcheck/rt_xcheck_params.hpp"
#endif

namespace rt {

constexpr int kParamsVersion = 2;

struct KCamera {
    double origin[3], llc[3], horizontal[3], vertical[3], u[3], v[3];
    double lens_radius;
};

struct KParams {
    KCamera cam;
    double t_min;
    int32_t width, height;
    int32_t spp, sample_begin, max_depth;
    uint32_t k0, k1;
    int32_t tile_rows, shard_index, shard_count;
    int32_t rows;              // compact rows of this shard
    int32_t n_spheres;
    int32_t use_ring;          // 1: per-wave LDS block sums (whenever a block's pixels fit the ring's pixel slots: plan_launch, rt_launch.hpp, picks block_items for that); 0: every sample goes to the frame buffer directly
    uint32_t npix;             // rows * width
    uint32_t n_blocks;         // work blocks of block_items consecutive pixel-samples, pixel-major: item w = pixel * spp + sample
    unsigned long long total_items;   // npix * spp
    double inv_spp;            // 1.0 / spp (block -> first pixel)
    double inv_width;          // 1.0 / width (first pixel -> row, column)
    // per-lane divisions of small numerators by launch constants, as multiply-high (udiv_small, rt_kernels.hpp):
    // floor(2^32 / d) + 1 for d = spp, width, tile_rows (unused where d == 1 or d >= 2^16)
    uint32_t magic_spp, magic_width, magic_tile;
    uint32_t block_items;      // pixel-samples per work block: ITEMS, or -- launches of few samples per pixel -- the multiple of 64 below it whose pixels
                               // still fit the ring's pixel slots (plan_launch, rt_launch.hpp)
    const float *filt;         // [n][4]  f32 filter record (cx, cy, cz, K')
#ifdef RTIOW_CROSSCHECK_MODES
    KXcheckTables x;           // the B operands of scan modes 2-4 (xcheck/rt_xcheck_params.hpp)
#endif
    const uint4 *btube;        // [tiles/2 + 1][64] MODE 5 B operands: 32 spheres x 16 K-slots, each column scaled by 2 / its bound (rt_device.hpp)
    float tube_rho;            // MODE 5 radius floor
    float scene_scale;         // MODE 5: sum over axes of the largest |coordinate| a scanned sphere reaches (error margins of grid_cells)
    // MODE 5: the table's columns are ordered by position (rt_scene_core.hpp): tiles [0, n_global) hold the spheres every
    // ray scans, tile n_global + iz * grid_dim + ix those whose centre lies in cell (ix, iz) of a square xz grid.
    const double *geo_slot;    // [columns][4] exact (cx, cy, cz, r*r) in column order
    const uint32_t *slot_orig; // [columns] place in the caller's list of the sphere in each column
    float grid[8];             // x0, z0, 1/cell, x1, z1, y lo, y hi, largest radius of a sphere that lives in a cell
    int32_t grid_dim;          // cells per side; 0: no grid (every tile is scanned, columns in list order)
    unsigned long long grid_rows;      // bit k * grid_dim for every k with (k + 1) * grid_dim <= 64 (grids of <= 64 cells)
    int32_t n_global;
    int32_t n_tiles;
    int32_t n_always;          // spheres that skip the filter and are always tested exactly
    int32_t always_idx[8];
    const double *geo;         // [n][4]  exact (cx, cy, cz, r*r)
    const double *mat;         // [n][10] exact (1/r, param, albedo rgb, kind, 1/param, r0(1/ir), r0(ir), -)
    unsigned long long *fix;   // [rows][width][3] exact sums
    unsigned int *queue;       // work counter
    unsigned long long *stats; // [0] rays [1] samples [2] candidates [3] exact roots [4] samples sent to the frame buffer one by one [8..15] diagnostic builds [16..79] rays per bounce index (DIAG)
    const uint32_t *pix_list;  // pixel-list launches (ITEMS = kItemBlockList): [npix] global pixel numbers g = j * width + i; `fix` is then [npix][3], entry k for pix_list[k] (last member: the
                               // offsets of everything render_kernel reads stay where they were)
    // frame-batch launches (ITEMS = kItemBlockFrames; after pix_list for the same reason).  n_blocks = n_frames * frame_blocks and
    // total_items = n_frames * frame_items; `fix` is [n_frames][height][width][3]
    const KCamera *cams;       // [n_frames] cameras, DEVICE memory
    unsigned long long frame_items;    // width * height * spp: pixel-samples of one frame
    double inv_frame_blocks;   // 1.0 / frame_blocks (block -> frame)
    uint32_t frame_blocks;     // work blocks per frame = ceil(frame_items / block_items): no block straddles two frames
    uint32_t frame_pix;        // width * height: virtual pixel f * frame_pix + g is pixel g of frame f
    int32_t sample_stride;     // frame f renders the samples [sample_begin + f * sample_stride, ... + spp)
    // the capped dense kernels (ITEMS = kItemBlockDense / kItemBlockDenseLarge): the ten round-key pairs of (k0, k1), filled by the host (rt_round_keys.hpp)
    // and read where they lie, in the kernel-argument block, with scalar loads (rt_device.hpp, philox4x32_10_table).  The last member, like pix_list and
    // cams before it: the offsets of everything else stay where they were.  No other kernel reads it.
    uint32_t round_keys[20];
    // the capped dense kernels with 16 pixel slots: lane-striped block sums (plan_stripes, rt_launch.hpp).  A launch whose
    // blocks touch at most S <= 8 pixels keeps R = 16 / S replicas of every slot's sums: a sample adds to slot dq | replica * S, and
    // stripe_mask = 15 & ~(S - 1) are the replica's bits of a slot number.  0 (every other kernel and launch): one replica, slot = dq.  The last member.
    uint32_t stripe_mask;
};

constexpr int RT_KIND_LAMBERTIAN = 0, RT_KIND_METAL = 1, RT_KIND_DIALECTRIC = 2;
constexpr int kBlock = 256;
constexpr int kCandCap = 24;        // MODE 1: per-lane candidate slots
constexpr int kScanUnroll = 8;      // MODE 1: spheres per scalar-load batch / overflow check
constexpr int kItemBlock = 256;     // pixel-samples a wave reserves per atomic on the work counter
// ... and 1 024 for launches of at least 2 x 10^8 pixel-samples at >= 147 samples per pixel (ceil(1023 / 147) + 1 = 8 pixels: still kRingSlots; the
// small-grid kernel: >= 69 samples per pixel, ceil(1023 / 69) + 1 = 16 pixels, its large blocks' ring has 2 x 16 pixel slots, render_kernel in rt_kernels.hpp):
// reserving a block is a returning atomic the whole wave waits for, and a block's sums are one frame-buffer request per pixel and channel:
// a quarter of both (1200x675x500: 52.7 -> 51.3 ms; 10k spheres 1920x1080x256: 93.7 -> 91.5 ms).  Smaller launches keep 256: their last
// blocks are the end-of-launch tail (1200x675x147 is 5 % slower with 1 024).
constexpr int kItemBlockLarge = 1024;
constexpr int kItemBlockList = -kItemBlock;   // as the ITEMS of render_kernel: work blocks of kItemBlock pixel-samples over a pixel list (rt_kernels.hpp)
constexpr int kItemBlockFrames = -2 * kItemBlock;   // ... and over a BATCH OF FRAMES, one camera each (rt_render_frames_device; instantiated from rt_frames.hip only)
// ... and the dense launch once more, with the CAPPED unit-sphere redraw (render_kernel, PHASE 4): blocks of kItemBlock /
// of kItemBlockLarge pixel-samples, decoded, queued and summed exactly as ITEMS = kItemBlock / kItemBlockLarge (instantiated from rt_dense.hip only)
constexpr int kItemBlockDense = -3 * kItemBlock;
constexpr int kItemBlockDenseLarge = -4 * kItemBlock;
static_assert(kItemBlockLarge + 32768 < 65536, "udiv_small: numerators x < d + kItemBlockLarge with d < 2^15 keep x * d < 2^32");
constexpr int kLargeMinSpp = 147;
constexpr int kLargeMinSppSmallGrid = 69;
constexpr unsigned long long kLargeMinItems = 200000000ull;   // (1200x675: blocks of 1 024 against 256 at 150 / 200 / 250 / 300 / 350 spp: +3.5 / -0.5 / -1.9 / -2.2 / -2.5 %)
constexpr int kRingSlots = 8;       // pixels a block may touch when its sums are kept in LDS: ceil((block_items - 1) / spp) + 1 <= 8 -- blocks of 256 from
                                    //   37 spp per launch on, of 192 / 128 / 64 down to 9 spp (plan_launch, rt_launch.hpp); below that samples go to the frame buffer one by one
constexpr int kRingDepth = 4;       // blocks of one wave that may be unfinished at the same time (older ones: see `orphan`)
                                    //   (the shipped scan mode's kernels: 2 blocks x 16 pixels, render_kernel: blocks of 256 from 17 spp on, sums down to 5 spp)
constexpr int kMatStride = 10;      // doubles per material record
constexpr int kListCap = 126;       // MODE 5: longest list of tiles a wave scans by list; beyond, it scans the whole table
constexpr int kSegTilesTube = 28;   // MODE 5: 14 bitmap words of 32 columns per segment (a wave's list is 5-13 tiles long)
constexpr int kSegTiles = 36;       // matrix filter: tiles (of 16 spheres) per candidate-bitmap segment

} // namespace rt
