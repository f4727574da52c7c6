// rt_kernels.hpp -- the render megakernel (gfx950).
//
// One launch renders a shard of the image: main.rs:122-139 without to_rgba.
//
// Execution shape:
//   * persistent grid: as many 256-thread workgroups as stay resident; every
//     LANE owns one path at a time and never waits for its neighbours -- when
//     its path ends it immediately starts its next pixel-sample ("path
//     regeneration"), so the sphere scan always runs with full waves;
//   * work = single pixel-samples in PIXEL-MAJOR order (item w = pixel * spp + sample); a wave
//     reserves a block of kItemBlock consecutive items with ONE returning atomic on a device-wide
//     counter, STARTS them 64 at a time (item -> pixel, Philox, lens sample: every lane busy) into a
//     per-wave LDS queue and deals the started samples to the lanes whose paths end (__ballot +
//     popcount + v_mbcnt rank); a block is at most 8 neighbouring pixels, so its 64-lane wave traces
//     coherent camera rays and the launch ends on single samples;
//   * the sphere scan (HittableList::hit, mod.rs:54-70) decides nothing: it is a
//     conservative FILTER (rt_device.hpp) -- it may send a sphere to the exact
//     test needlessly, never drop one the reference would hit.  The shipped form
//     (MODE 5, the tube filter) evaluates it on the bf16 matrix pipe, 16 rays x 2
//     directions x 32 spheres per instruction, and only over the tiles of spheres the wave's
//     rays can reach (the table is tiled by position: a grid over x and z, rt_device.hpp
//     grid_cells); MODE 1 (VALU + scalar loads) and MODE 0 (no filter at all) are the
//     validation modes of the product build, MODEs 2-4 (earlier matrix-pipe forms) exist
//     only in the cross-check build (-DRTIOW_CROSSCHECK_MODES);
//   * spheres the filter keeps are marked in per-ray LDS bitmaps, pooled over the
//     wave and put through the reference's exact f64 test (sphere.rs:16-34), so every
//     hit decision and every shading value is the reference's own f64 arithmetic;
//   * radiance is exact u64 fixed point (contract C5): a finished sample is added to its block's
//     per-pixel sums in the wave's LDS, and a block goes to the frame buffer ONCE, when its last
//     sample has finished (one 64-bit atomic per pixel and channel per block: the frame buffer sees
//     ~3 x 64-byte memory-side requests per 256 samples).
//
// This file holds the kernel and nothing after it.  Its argument block and the launch constants are rt_params.hpp, the host code that
// launches it is rt_launch.hpp; the translation units that instantiate it are rt_api.hip (the dense and the pixel-list launches),
// rt_frames.hip and rt_dense.hip.  Every other kernel of the library lives beside its entry points, in the .hip file that launches it.
#pragma once
#include "rt_params.hpp"
#include "rt_device.hpp"
#include "rt_diag.hpp"
#include <type_traits>
#include <cstddef>

#ifndef RT_GROUP_SKIP
#define RT_GROUP_SKIP 1     // MODE 5: a 16-ray group skips the tiles none of its rays can reach (0: every group scans the wave's whole list)
#endif

namespace rt {

// What rt_params.hpp states of the argument block, pinned here: this file is a hashed kernel source (bench.py, kernel_source_sha)
// and rt_params.hpp is not.
static_assert(kParamsVersion == 2, "KParams or a launch constant changed: bump kParamsVersion in rt_params.hpp AND this assert, so that "
              "this file -- a hashed kernel source -- changes with them");

// x / d for a launch constant d >= 1 and a numerator with x < d + 65536 and x < 2^31, without a division (a `/`
// would have the compiler keep one reciprocal per divisor in a VGPR for the whole bounce loop):
//   d == 1: x;  d >= 2^15: the quotient is 0 or 1;  else floor(x * M / 2^32), M = floor(2^32/d) + 1,
//   exact because x * (M d - 2^32) <= x d < 2^32: the numerators here are < d + kItemBlockLarge (spp, width) or < 2^16
//   (rows / tile_rows), so x < 2^15 + 2^10 and x d < 2^32 for every d < 2^15.
__device__ __forceinline__ uint32_t udiv_small(uint32_t x, uint32_t d, uint32_t magic)
{
    const uint32_t big = x >= d ? 1u : 0u;
    const uint32_t q = __umulhi(x, magic);
    return d == 1u ? x : (d >= 32768u ? big : q);
}



// MODE 0: every sphere goes through the exact test (validation mode, RT_FLAG_NO_FILTER):
//         same results by construction of the filter.
// MODE 1: f32 filter on the VALU with scalar-loaded sphere records + deferred exact tests.
// MODEs 2-4 are earlier matrix-pipe forms of the filter, kept as cross-checks and compiled only with
// -DRTIOW_CROSSCHECK_MODES (the product library carries modes 0, 1 and 5):
// MODE 2: the same filter on the f32 MATRIX pipe: the filter is two K = 4 products,
//         HB = R1 x S and Q = R2 x S, of per-ray rows R1 = (-g, o.g), R2 = (-2o, |o|^2(1-kappa))
//         with per-sphere columns S = (c, 1); v_mfma_f32_16x16x4_f32 evaluates them for
//         16 rays x 16 spheres at a time as the very fma chains of filter_keeps().
// MODE 3: the same two products on the bf16 matrix pipe (16x the f32 rate): every f32 operand
//         is the exact sum of three bf16 pieces, and one v_mfma_f32_16x16x32_bf16 adds up the
//         8 significant piece products of each of the 4 components (K = 32).
// MODE 4: the filter as ONE contraction of 11 per-ray terms with 11 per-sphere terms (rt_device.hpp,
//         "lifted" form) on the bf16 matrix pipe, two chained K = 32 MFMAs per 16 rays x 16 spheres:
//         the VALU no longer squares and subtracts, it only looks at the sign of the result.
// MODE 5: the tube filter: |u_k.(c-o)| <= r for two directions u_1, u_2 perpendicular to the ray, linear
//         in c, so two bf16 pieces per factor suffice: ONE v_mfma_f32_32x32x16_bf16 tests 16 rays
//         (both directions) against 32 spheres -- a third of the matrix-pipe time of modes 3/4.
constexpr int kRowPad = 80;         // floats per row of the ray-operand transpose buffer

typedef float f32x4 __attribute__((ext_vector_type(4)));

// DIAG: also count filter candidates, exact roots and rays per bounce index (rt_stats.candidates /
// exact_roots / live_per_bounce).  Off in the shipped path: the counters cost spilled registers and
// ~15 % of the frame time.
// SMALLGRID (MODE 5 only): the scene's tile grid has at most 64 cells (with the global tiles: a list of <= 64 tiles) --
// the host picks this instantiation then; it carries neither the large-grid list code nor the scan-every-tile fallback.
// U53 (RT_FLAG_UNIFORM53): every uniform takes two consecutive Philox words (53 random bits, as rand's gen::<f64>()) instead
// of one word's 32 bits: same draw order, same runs; the rejection tests run in f64 as the reference writes them (the
// integer form needs the 2^-31 lattice of single words).  An optional mode: ~2x the Philox work of the retry loops.
// ITEMS: pixel-samples per work block (kItemBlock, or kItemBlockLarge for launches with enough samples: see plan_launch, rt_launch.hpp).
// ... or kItemBlockList = -kItemBlock: blocks of kItemBlock pixel-samples over a PIXEL LIST (rt_render_pixels_device).  The launch is then a "virtual
// image" of P.npix pixels in the order of P.pix_list; local pixel k is pixel g = P.pix_list[k] of the frame.  Only the start of a sample
// differs (local pixel -> g -> (i, j)); the work blocks, the queue, the block sums and their write-out address pixels by their local number, so
// the output is compact: entry k belongs to pix_list[k].  The variant is an instantiation of its own -- a __global__ with its own symbol,
// rt::render_kernel<5, false, SMALLGRID, false, -256> -- of this one body, and the text of the body stays where it was: wrapping it into
// a __forceinline__ function shared by two __global__ entries moves opcodes in EVERY existing instantiation (tried: all 14 ops-sha of
// tools/isa_fingerprint.py change), a sixth template parameter would rename the kernels bench.py and the profiles spell.  As built, the existing
// instantiations' machine code is unchanged (profiles/isa_fingerprint_{before,after}_pixel_lists.txt).
// ... or kItemBlockFrames = -2 * kItemBlock: blocks of (at most) kItemBlock pixel-samples over a BATCH OF FRAMES (rt_render_frames_device).  The launch is a
// virtual image of n_frames * height rows: frame f owns the virtual pixels [f * P.frame_pix, (f + 1) * P.frame_pix) and the work blocks
// [f * P.frame_blocks, (f + 1) * P.frame_blocks) -- a block never straddles two frames, so its frame f, hence its camera P.cams[f] and its
// first sample index P.sample_begin + f * P.sample_stride, are wave-uniform.  The work blocks, the queue, the block sums and their
// write-out address pixels by their virtual number (the output is [n_frames][height][width][3]); the Philox counter takes the pixel's
// number g in its OWN frame.  Only the block decode, the start of a sample and the camera differ; the bounce loop is the dense kernel's.
// Same method as the pixel lists (`if constexpr` where the body stands), and the instantiations live in a translation unit of their own
// (rt_frames.hip): rt_api.hip's kernels are the same set with the same machine code (profiles/isa_fingerprint_{before,after}_frame_batches.txt).
// ... or kItemBlockDense / kItemBlockDenseLarge: the DENSE launch on blocks of kItemBlock / kItemBlockLarge with the capped redraw.  A scatter draws at most
// four unit-sphere tries -- the three blocks ev, ev + 1, ev + 2 of the stream contract's period, in straight-line code -- and a lane that accepted none
// of them PARKS: it advances ev by 3 and keeps its ray, depth and throughput, so the next pass traces the same ray to the same hit and its shared first
// block is block ev + 3, "try 0 of the next three blocks".  The accepted words and the final ev are the unbounded loop's; only the pass moves, and the
// per-pixel sums are integer sums.  The wave no longer draws until its unluckiest lane accepts.  Only PHASE 4 differs from the dense kernel; same method
// as the two variants above, instantiations in rt_dense.hip.
template <int MODE, bool DIAG, bool SMALLGRID = false, bool U53 = false, int ITEMS = 256>
// second launch bound = waves per SIMD the register allocator must leave room for: the bounce loop
// is latency-bound, and the 4th wave is worth more than the few cold values it spills.  Only the shipped kernel
// (MODE 5 without the diagnostic counters) fits four workgroups' LDS on a CU (40 000 of 40 960 bytes each); the
// diagnostic variant and the cross-check modes 2-4 carry 1-14 KB more and run three.
__global__ __launch_bounds__(kBlock, (MODE == 5 && !DIAG) ? 4 : (MODE >= 2) ? 3 : 5) void render_kernel(const KParams P)
{
    constexpr bool PIXLIST = ITEMS == kItemBlockList;
    constexpr bool FRAMES = ITEMS == kItemBlockFrames;
    constexpr bool CAPPED = ITEMS == kItemBlockDense || ITEMS == kItemBlockDenseLarge;
    static_assert(ITEMS > 0 || PIXLIST || FRAMES || CAPPED, "ITEMS: a block size, kItemBlockList, kItemBlockFrames, kItemBlockDense or kItemBlockDenseLarge");
    static_assert(!(PIXLIST || FRAMES) || (MODE == 5 && !DIAG && !U53), "pixel lists and frame batches: the shipped kernel, 32-bit uniforms, blocks of 256");
    static_assert(!CAPPED || (MODE == 5 && !DIAG && !U53), "the capped redraw: the shipped kernel, 32-bit uniforms (a 53-bit try is six words: another period)");
    // The block sums' ring (s_ring below) has the same 768 bytes per wave in both shapes: 4 blocks x 8 pixels, or -- the shipped scan mode's
    // kernels, all but the large-grid kernel's instantiation for blocks of 1 024 -- 2 blocks x 16 pixels.  Two blocks in flight are enough: a block of 256 lasts ~11 passes, one of
    // 1 024 ~43, and the samples of the block before the previous one that are still open when a block begins (paths of more than
    // ~15 / ~50 bounces: ~1 in 10^3 / none) go the orphans' way; two counters instead of four, a shorter cascade when samples finish.  And 16
    // pixel slots let launches from 17 samples per pixel on keep the sums of blocks of 256 in LDS (ceil(255 / 17) + 1 = 16; smaller blocks: from 5) and
    // launches from kLargeMinSppSmallGrid = 69 on take large blocks (ceil(1023 / 69) + 1 = 16).  Measured, interleaved: 1200x675x500 48.87 ->
    // 48.74 ms, 1200x675x100 10.53 -> 10.49 ms, 10k spheres 1920x1080 x20 7.78 -> 7.50 ms, x100 34.98 -> 34.88 ms; the large-grid kernel ON LARGE
    // BLOCKS is 0.7 % slower with the same ring (10k spheres 1920x1080x256: 85.99 -> 86.58 ms, fewer instructions, another schedule) and
    // keeps 4 x 8 and kLargeMinSpp = 147.  The cross-check scan modes and the diagnostic-counter kernels keep 4 x 8 too.
    constexpr bool kWideRing = SMALLGRID || (MODE == 5 && !DIAG && (ITEMS == kItemBlock || ITEMS == kItemBlockList || ITEMS == kItemBlockFrames || ITEMS == kItemBlockDense));
    constexpr int kRingDepth = kWideRing ? 2 : 4;
    constexpr int kRingSlots = kWideRing ? 16 : 8;
    constexpr bool kMaskVotes = CAPPED && kRingDepth == 2;      // PHASE 5 on wave masks (the capped kernels with the ring of two)
    // PHASE 1 on wave masks: the capped kernels but the large-grid one on blocks of 1 024, which has no scalar headroom for it (63 parked scalars: 67 with it)
    constexpr bool kMaskHandout = CAPPED && (SMALLGRID || ITEMS == kItemBlockDense);
    static_assert(kRingDepth * kRingSlots == rt::kRingDepth * rt::kRingSlots, "same LDS either way");
    // LANE-STRIPED BLOCK SUMS (the capped kernels with 16 pixel slots).  At many samples per pixel a block touches few pixels -- at most
    // S of the 16 slots, S a power of two the host derives (plan_stripes, rt_launch.hpp) -- and the lanes that finish in one pass add to the same three
    // words, which the LDS serialises.  The unused slots hold R = 16 / S replicas: the refill bakes a replica number, taken from the item's place in the
    // block, into the slot it writes into the queue's meta word (slot = dq | replica bits; P.stripe_mask = 15 & ~(S - 1) are the replica's bits), the per-pass
    // phases address the ring with that slot as they always did, and flush_ring sends every replica to its pixel's address.  A lane's pix_local carries the
    // replica bits too; the one reader, a sample that goes to the frame buffer directly, takes them off.  P.stripe_mask == 0: one replica, nothing moves.
    constexpr bool kStriped = CAPPED && kRingSlots == 16;
    __shared__ uint16_t cand[MODE == 1 ? kCandCap : 1][MODE == 1 ? kBlock : 1];     // MODE 1: per-lane candidate lists
    constexpr bool MATRIX = (MODE >= 2);
    constexpr bool LIFTED = (MODE == 4);
    constexpr bool TUBE = (MODE == 5);
    constexpr bool RAYOP = (MODE == 2 || MODE == 3);
    __shared__ float s_rayop[RAYOP ? kBlock / 64 : 1][RAYOP ? 8 : 1][RAYOP ? kRowPad : 1];
    // per ray, one bit per sphere of the current segment (kSeg tiles of 16 columns): set by whichever lane
    // holds the passing result (ds_or, nothing returned, nothing waited for), read by the owner.  The same LDS
    // first carries the per-ray operand dwords to the MFMA layout (4 KB) and, for large grids, the wave's cell
    // bitmap (512 B).
    constexpr int kSeg = TUBE ? kSegTilesTube : kSegTiles;
    static_assert(TUBE || (kSeg / 2) * 64 * sizeof(unsigned int) >= 32 * kStageStride * sizeof(uint4), "operand staging fits the bitmap");
    // MODE 5: bitmap words (14 x 256 B) and the list of tiles this pass scans (128 x 4 B) share the 4 KB the staging
    // needs before either exists
    static_assert(!TUBE || ((kSeg / 2) * 64 + kListCap + 2) * sizeof(unsigned int) == 64 * 4 * sizeof(uint4), "tube: staging = bitmap + tile list");
    constexpr int kBitWords = TUBE ? (kSeg / 2) * 64 + kListCap + 2 : (kSeg / 2) * 64;
    __shared__ __attribute__((aligned(16))) unsigned int s_bits[MATRIX ? kBlock / 64 : 1][MATRIX ? kBitWords : 1];
    __shared__ unsigned int s_sum[(MATRIX && !TUBE) ? kBlock : 1];     // per ray: which of its bitmap words are non-zero
    // The wave's queue of started samples (below, (a)): the image-plane coordinates u, v (f64) and, as 32-bit columns,
    // the two accepted lens words, pixel, sample and (events drawn << 8 | pixel slot of the block): 36 bytes per entry.
    __shared__ double s_quv[kBlock / 64][2][64];
    __shared__ unsigned int s_qid[kBlock / 64][5][64];
    // pooled exact tests: ring of waiting (column << 6 | ray) pairs per wave (columns < 2^26); per-ray minimum root and its sphere
    __shared__ unsigned int s_pool[MATRIX ? kBlock / 64 : 1][MATRIX ? 128 : 1];
    __shared__ unsigned long long s_best[MATRIX ? kBlock : 1];
    __shared__ unsigned int s_bidx[MATRIX ? kBlock : 1];
    // Per wave, the exact sums (u64 fixed point) of up to kRingDepth unfinished blocks, [pixel slot][channel]; a block is
    // written to the frame buffer once, by whichever pass finishes its last sample (how many samples each block
    // still waits for is wave-uniform state in SGPRs).  s_rpix: first pixel (compact index) of the entry's block.
    __shared__ unsigned long long s_ring[kBlock / 64][kRingDepth][kRingSlots * 3];
    __shared__ unsigned int s_rpix[kBlock / 64][kRingDepth];
    __shared__ unsigned int s_live[DIAG ? kBlock / 64 : 1][DIAG ? 64 : 1];    // DIAG: rays per bounce index, per wave
    // so does the path throughput (contract C3): read and written once per bounce
    __shared__ double s_thr[3][kBlock];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    {   // this wave's block sums and their bookkeeping (own wave only: no barrier needed)
        unsigned long long *z = &s_ring[tid >> 6][0][0];
        for (int k = lane; k < kRingDepth * kRingSlots * 3; k += 64) z[k] = 0ull;
        if (lane < kRingDepth) s_rpix[tid >> 6][lane] = 0u;
    }
    if (DIAG) s_live[tid >> 6][tid & 63] = 0u;                          // this wave's row only
    // number of set bits of a wave mask below this lane (v_mbcnt: no per-lane 64-bit mask to keep)
    auto rank_below = [](unsigned long long m) -> uint32_t {
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    };

    // The filter table is read-only for the whole launch and indexed by a
    // wave-uniform counter: reading it through the constant address space makes
    // the scan's loads scalar (s_load_dwordx4 into SGPRs).
    const float __attribute__((address_space(4))) *filt =
        (const float __attribute__((address_space(4))) *)(uintptr_t)P.filt;
    const double *__restrict__ geo = P.geo;
    const double *__restrict__ mat = P.mat;
    // one Philox block of this launch's key.  The capped dense kernels READ the ten round keys (P.round_keys, scalar loads from the kernel-argument
    // block -- P is the kernel's first argument, at offset 0 of it: rt_device.hpp, philox4x32_10_table); every other instantiation rebuilds them from
    // P.k0, P.k1 as before, and compiles to the code it had.
    auto philox = [&](uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) -> U4 {
        if constexpr (CAPPED) {
            const char __attribute__((address_space(4))) *args = (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
            return philox4x32_10_table(c0, c1, c2, c3, (RoundKeyTable)(args + offsetof(KParams, round_keys)));
        } else return philox4x32_10(c0, c1, c2, c3, P.k0, P.k1);
    };
    const int n = P.n_spheres;
    const double t_min = P.t_min;
    const double wm1 = (double)(P.width - 1);
    const double hm1 = (double)(P.height - 1);

    bool dead = false, alive = false;
    uint32_t pix_local = 0, pix_global = 0;
    int s = 0;
    uint32_t my_frame = 0;                         // FRAMES: frame of the sample this lane has just taken (PHASE 1 -> PHASE 2 only)
    uint32_t my_blk = 0;                           // sequence number (within this wave) of the block of this lane's sample << 4 | its pixel slot
    D3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    int depth = 0;
    uint32_t ev = 0;
    uint32_t n_rays = 0, n_samples = 0, n_direct = 0;   // wave totals (uniform)
    unsigned long long tot_cand = 0, tot_roots = 0;     // wave totals (uniform)
    // this wave's current block of work items (all wave-uniform): items [blk_next, blk_end) of it are still to be dealt;
    // its first item is sample blk_s0 of compact pixel blk_pix0 = row blk_rr0, column blk_i0 of the shard
    uint32_t blk_next = 0, blk_end = 0, blk_seq = 0xFFFFFFFFu, blk_pix0 = 0, blk_s0 = 0, blk_rr0 = 0, blk_i0 = 0;
    uint32_t blk_frame = 0, blk_sbase = (uint32_t)P.sample_begin;   // FRAMES: the current block's frame and the index of that frame's first sample (wave-uniform)
    bool queue_empty = false;
    // the wave's queue of camera rays: entries [q_head, q_head + q_count) of s_qray / s_qid (wave-uniform)
    uint32_t q_head = 0, q_count = 0;
    double *quv_w = &s_quv[tid >> 6][0][0];
    unsigned int *qid_w = &s_qid[tid >> 6][0][0];
    unsigned long long *ring_w = &s_ring[tid >> 6][0][0];
    unsigned int *rpix_w = &s_rpix[tid >> 6][0];
    // samples the wave's four youngest blocks still wait for (wave-uniform; index = age: 0 is the current block
    // blk_seq, k is block blk_seq - k, whose sums are ring entry (blk_seq - k) % kRingDepth); 0 = complete or none
    uint32_t rem0 = 0, rem1 = 0, rem2 = 0, rem3 = 0;           // (rem2, rem3: rings of 4 only)
    static_assert(kRingDepth == 4 || kRingDepth == 2, "the block counters are written out for a ring of 4 or 2");
    // one block's sums -> frame buffer (wave-uniform call; `e` uniform): lane l < 24 holds (pixel slot l/3, channel l%3),
    // which are 24 consecutive u64 of the frame buffer; zero sums (unused slots, black pixels) are not sent
    // (striped sums: ring word `lane` is slot lane / 3, whose replica bits come off the pixel while the channel stays.  Stated ONCE, as this lane's base
    //  pointer into the frame buffer: the other arm's P.fix + lane is hoisted out of the bounce loop into a register pair as well, and this one takes its
    //  place.  Folding at the write-out instead -- per lane, in a loop over the replicas, through a table in LDS -- spills 2 to 15 more scalars in every form tried.)
    unsigned long long *const fix_lane = kStriped ? P.fix + ((uint32_t)lane - ((((uint32_t)lane * 43u) >> 7) & P.stripe_mask) * 3u) : P.fix;
    auto flush_ring = [&](uint32_t e) {
        if (lane < kRingSlots * 3) {
            const unsigned long long v = ring_w[e * (kRingSlots * 3) + lane];
            if (v != 0ull) {
                if constexpr (kStriped) atomicAdd(fix_lane + (size_t)rpix_w[e] * 3u, v);
                else
                atomicAdd(P.fix + (size_t)rpix_w[e] * 3u + (size_t)lane, v);
                ring_w[e * (kRingSlots * 3) + lane] = 0ull;
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    RT_DIAG_DECLARE();              // (rt_diag.hpp: nothing in the shipped library)
    // One pass of the bounce loop = five phases, marked "==== PHASE n" below; the helpers they call are the lambdas defined next to their
    // data (flush_ring, exact_test_g, pool_round, enumerate, finish_pool, look_tube, do_tile, build_list).  The phases themselves stay
    // INLINE: wrapped into named lambdas (round 5 tried it: take_samples / start_camera_rays / shade / accumulate_finished) the same code
    // compiles to a different register allocation at this kernel's zero-headroom budget (128 VGPRs) -- one wrapper alone puts 20 scratch
    // instructions into the small-grid kernel, all four cost +0.3 % frame time (profiles/r05_experiments.txt 8) -- so the structure is in
    // the comments and tools/isa_fingerprint.py guards refactorings (the machine code of this file's kernels before = after).
    for (;;) {
        // Wave priorities through a pass (s_setprio): 1 from here -- taking samples, refill, camera rays, then the filter rows, the ground
        // test and the tile list --, 3 in the tile loop (the matrix pipe is fed sooner and the other waves' vector work fills the time
        // the MFMAs take), 2 while the candidates are enumerated, 1 in the pooled exact rounds, 0 while the hit is shaded (the redraw
        // loop runs at a quarter of the lanes), 1 again for the finished samples' sums.  Measured against round 2's choice (1 in the
        // tile loop, 0 elsewhere): 1200x675x500 50.30 -> 49.73 ms (-1.15 %), configs[1] 10.79 -> 10.69, 10k spheres -1.0 %; no
        // priorities at all +1.1 %; a dozen other assignments within 0.3 % of this one or slower (profiles/r04_experiments.txt 30).
        __builtin_amdgcn_s_setprio(1);
        RT_COUNT(0);
        // ==== PHASE 1: take_samples ============================================================================================
        // ---- (a) lanes without a path take the next camera rays of the wave's queue -------------------------
        // Starting a sample (item -> pixel, Philox, lens rejection, the f64 camera arithmetic: ~340 vector
        // instructions) used to run in every pass with only the ~38 % of lanes whose path had just ended.  Now the
        // wave starts its next 64 items at once, with every lane busy -- everything up to the image-plane coordinates
        // and the accepted lens sample -- parks them in LDS (36 bytes each) and hands them out over the next ~2.7
        // passes: a lane that needs work takes entry head + its rank among the takers and builds its ray (camera.rs:47-54).  The queue is refilled only when it is empty, so its entries always belong to the
        // wave's current block (blk_seq, blk_pix0).
        bool fresh = false;                                         // this lane starts a sample in this pass
        double cam_u = 0.0, cam_v = 0.0;
        uint32_t lens_wx = 0u, lens_wy = 0u;
        // The capped dense kernels (kMaskHandout) hand out on WAVE MASKS.  `fresh` and `dead` as lane booleans carried round the loop below cost a scalar
        // merge of three instructions per boolean at the loop's head and again at its latch, and a select and a compare to vote on each.  There the
        // takers are ONE mask on the scalar unit, want_m: the lanes without a path at the top of the pass, less those that have taken an entry.  The
        // first trip is straight-line -- what the queue holds --, and takers that remain find the queue empty, so every further trip is refill, then
        // take: the loop's own order, trip for trip (rank among the takers, q_head, q_count, blk_next), and so the same entry for every lane.
        // No lane is marked dead: once the device-wide counter has said that no block is left, the queue is empty and the wave's block is used up
        // for good, so a lane without a path asks again in every pass, gets the same answer from queue_empty without an atomic, and takes nothing.
        // The lanes that start a camera ray are the takers that are takers no more.
        unsigned long long want_m = 0ull;
        if constexpr (kMaskHandout) {
            // (read by the lanes that take an entry only: no zeros to write for the others)
            cam_u = unread_f64(); cam_v = unread_f64(); lens_wx = unread_u32(); lens_wy = unread_u32();
            want_m = ~__ballot(alive);
            if (q_count != 0u) {
                const uint32_t r = rank_below(want_m);
                const unsigned long long take_m = want_m & __ballot(r < q_count);
                const bool take = __builtin_amdgcn_inverse_ballot_w64(take_m);     // (the lanes' branch runs on the mask as it is)
                RT_LDS_QUEUE_READS(take, q_head + r);
                if (take) {
                    const uint32_t e = q_head + r;
                    cam_u = quv_w[0 * 64 + e]; cam_v = quv_w[1 * 64 + e];
                    lens_wx = qid_w[0 * 64 + e]; lens_wy = qid_w[1 * 64 + e];
                    pix_global = qid_w[2 * 64 + e];
                    s = (int)qid_w[3 * 64 + e];
                    const uint32_t meta = qid_w[4 * 64 + e];
                    ev = meta >> 8;
                    pix_local = blk_pix0 + (meta & 255u);
                    my_blk = (blk_seq << 4) | (meta & 15u);
                }
                want_m &= ~take_m;
                const uint32_t took = (uint32_t)__popcll(take_m);               // = min(takers, q_count)
                q_head += took; q_count -= took;
            }
        }
        for (;;) {
            const bool want = kMaskHandout ? false : !alive && !dead && !fresh;
            const unsigned long long m = kMaskHandout ? want_m : __ballot(want);
            if (m == 0ull) break;
            if (q_count == 0u) {
                RT_STAMP(0);
                // ---- (b) refill: main.rs:131-134 + camera.rs:47-54 for the next (up to) 64 items of the block ----
                // A wave reserves kItemBlock consecutive items with ONE returning atomic on the device-wide counter:
                // one word sustains only ~88 dequeues/us chip-wide (MI355X_MICROARCH.md, row "dequeue").
                if (blk_next == blk_end) {                          // (wave-uniform) the block is used up: reserve the next one
                    uint32_t nb = 0xFFFFFFFFu;
                    if (!queue_empty) {
                        const int leader = (int)__builtin_ctzll(m);
                        if (lane == leader) nb = atomicAdd(P.queue, 1u);
                        nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(nb, leader));
                    }
                    if (nb >= P.n_blocks) {                         // no work left anywhere: these lanes are done
                        queue_empty = true;
                        if constexpr (kMaskHandout) break;
                        if (want) dead = true;
                        break;
                    }
                    // first item of the block -> (pixel, sample): W0 / spp in f64 (W0 < 2^39: exact), one correction step
                    uint32_t nb_f = nb;                             // FRAMES: the block's number within its frame
                    if constexpr (FRAMES) {
                        // block -> (frame, block of the frame): nb / frame_blocks in f64 (nb < 2^31: exact product, one rounding), one correction step
                        uint32_t fr = (uint32_t)((double)nb * P.inv_frame_blocks);
                        long long br = (long long)nb - (long long)fr * (long long)P.frame_blocks;
                        if (br < 0) { fr -= 1u; br += (long long)P.frame_blocks; }
                        else if (br >= (long long)P.frame_blocks) { fr += 1u; br -= (long long)P.frame_blocks; }
                        blk_frame = (uint32_t)__builtin_amdgcn_readfirstlane((int)fr);
                        nb_f = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)br);
                        blk_sbase = (uint32_t)P.sample_begin + blk_frame * (uint32_t)P.sample_stride;
                    }
                    const unsigned long long W0 = (unsigned long long)nb_f * (unsigned long long)P.block_items;     // (block_items <= ITEMS; FRAMES: first item WITHIN the frame)
                    const unsigned long long left = (FRAMES ? P.frame_items : P.total_items) - W0;
                    const uint32_t n_items = left < (unsigned long long)P.block_items ? (uint32_t)left : P.block_items;
                    uint32_t p0 = (uint32_t)((double)W0 * P.inv_spp);
                    long long rem = (long long)(W0 - (unsigned long long)p0 * (unsigned long long)(uint32_t)P.spp);
                    if (rem < 0) { p0 -= 1u; rem += (long long)P.spp; }
                    else if (rem >= (long long)P.spp) { p0 += 1u; rem -= (long long)P.spp; }
                    blk_pix0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p0);
                    blk_s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rem);
                    if constexpr (!PIXLIST) {
                    uint32_t rr0 = (uint32_t)((double)blk_pix0 * P.inv_width);     // pixel / width the same way
                    int i0 = (int)(blk_pix0 - rr0 * (uint32_t)P.width);
                    if (i0 < 0) { rr0 -= 1u; i0 += P.width; } else if (i0 >= P.width) { rr0 += 1u; i0 -= P.width; }
                    blk_rr0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rr0);                  // (keeps them in SGPRs)
                    blk_i0 = (uint32_t)__builtin_amdgcn_readfirstlane(i0);
                    }
                    if constexpr (FRAMES) blk_pix0 += blk_frame * P.frame_pix;     // (row and column above are the frame's own; from here on the VIRTUAL pixel)
                    blk_next = 0u; blk_end = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_items);
                    blk_seq += 1u;
                    if (P.use_ring) {
                        // The oldest of the four blocks leaves the ring.  If a path of > ~30 bounces still holds it open,
                        // what it has collected goes out now and its remaining samples will go to the frame buffer
                        // directly when they finish ("orphans": their age is then >= kRingDepth).
                        if constexpr (kRingDepth == 4) {
                            if (rem3 != 0u) flush_ring(blk_seq & (uint32_t)(kRingDepth - 1));
                            rem3 = rem2; rem2 = rem1; rem1 = rem0; rem0 = blk_end;
                        } else {
                            if (rem1 != 0u) flush_ring(blk_seq & (uint32_t)(kRingDepth - 1));
                            rem1 = rem0; rem0 = blk_end;
                        }
                        if (lane == 0) rpix_w[blk_seq & (uint32_t)(kRingDepth - 1)] = blk_pix0;
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                const uint32_t n_gen = min(64u, blk_end - blk_next);
                RT_COUNT_MAIN(1);
                if ((uint32_t)lane < n_gen) {
                    // item blk_next + lane of the block: sample blk_s0 + that of pixel blk_pix0, carried over into the next pixels
                    const uint32_t s_rel = blk_s0 + blk_next + (uint32_t)lane;
                    const uint32_t dq = udiv_small(s_rel, (uint32_t)P.spp, P.magic_spp);   // pixel slot within the block (< kRingSlots when use_ring)
                    uint32_t i, j, g_pix;
                    if constexpr (PIXLIST) {
                        // local pixel blk_pix0 + dq of the list (< P.npix: the item exists) -> its pixel of the frame -> (i, j).  g < 2^31 is no
                        // udiv_small numerator: g / width in f64 (exact product, one rounding) and one correction step, as the block decode above
                        g_pix = P.pix_list[blk_pix0 + dq];
                        uint32_t jq = (uint32_t)((double)g_pix * P.inv_width);
                        int ir = (int)(g_pix - jq * (uint32_t)P.width);
                        if (ir < 0) { jq -= 1u; ir += P.width; } else if (ir >= P.width) { jq += 1u; ir -= P.width; }
                        i = (uint32_t)ir; j = jq;
                    } else if constexpr (FRAMES) {
                        // (a frame is never sharded: row blk_rr0 + rq of the frame IS image row j)
                        const uint32_t col = blk_i0 + dq;
                        const uint32_t rq = udiv_small(col, (uint32_t)P.width, P.magic_width);
                        i = col - rq * (uint32_t)P.width;
                        j = blk_rr0 + rq;
                        g_pix = j * (uint32_t)P.width + i;              // the Philox counter's pixel: of the sample's OWN frame
                    } else {
                    const uint32_t col = blk_i0 + dq;
                    const uint32_t rq = udiv_small(col, (uint32_t)P.width, P.magic_width);
                    i = col - rq * (uint32_t)P.width;
                    const uint32_t rr = blk_rr0 + rq;
                    const uint32_t lt = udiv_small(rr, (uint32_t)P.tile_rows, P.magic_tile);   // local tile
                    j = (lt * (uint32_t)P.shard_count + (uint32_t)P.shard_index) * (uint32_t)P.tile_rows
                                       + (rr - lt * (uint32_t)P.tile_rows);
                    g_pix = j * (uint32_t)P.width + i;
                    }
                    const uint32_t g_s = (FRAMES ? blk_sbase : (uint32_t)P.sample_begin) + (s_rel - dq * (uint32_t)P.spp);
                    U4 w = philox(g_pix, g_s, 0u, 0u);
                    uint32_t g_ev = 1u;
                    const double u = ((double)i + (U53 ? u01_53(w.x, w.y) : u01(w.x))) / wm1;     // main.rs:131
                    const double v = ((double)j + (U53 ? u01_53(w.z, w.w) : u01(w.y))) / hm1;     // main.rs:132
                    // vec3.rs:59-68: redraw until x*x + y*y < 1.  x = u11(w) = m * 2^-31 with the integer m = w - 2^31: the loop runs
                    // on the integers (rt_device.hpp, unit_disk_accepts: the reference's f64 comparison, bit for bit), the accepted
                    // pair is converted once.
                    // Block 0 = (u jitter, v jitter, lens x, lens y); every further block holds TWO tries.
                    uint32_t wx = w.z, wy = w.w;
                    if constexpr (U53) {
                        // B_0 = (u jitter, v jitter), then ONE block per unit-disk try (two 53-bit draws); vec3.rs:59-68 in f64 as
                        // written.  The queue keeps no lens words: the lane that takes the sample recomputes block g_ev - 1.
                        double lx, ly;
                        do {
                            w = philox(g_pix, g_s, g_ev, 0u);
                            g_ev++;
                            lx = u11_53(w.x, w.y); ly = u11_53(w.z, w.w);
                        } while (!(lx * lx + ly * ly < 1.0));
                    } else
                    while (!unit_disk_accepts(wx, wy)) {
                        w = philox(g_pix, g_s, g_ev, 0u);
                        g_ev++;
                        wx = w.x; wy = w.y;
                        if (!unit_disk_accepts(wx, wy)) { wx = w.z; wy = w.w; }
                    }
                    quv_w[0 * 64 + lane] = u;
                    quv_w[1 * 64 + lane] = v;
                    qid_w[0 * 64 + lane] = wx;
                    qid_w[1 * 64 + lane] = wy;
                    qid_w[2 * 64 + lane] = g_pix;
                    qid_w[3 * 64 + lane] = g_s;
                    if constexpr (kStriped) {
                        // (consecutive items, which finish together, take the replicas in turn: bits 0-1 of the item's number become bits 2-3 of the slot, cut to
                        //  the replica's bits.  The mask is loaded HERE, from the kernel-argument block: read as P.stripe_mask it is one more scalar parked across
                        //  the whole pass, and the small-grid pair spills 4 more)
                        uint32_t sm;
                        asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(sm) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "n"(offsetof(KParams, stripe_mask)));
                        qid_w[4 * 64 + lane] = (g_ev << 8) | dq | ((s_rel << 2) & sm);
                    }
                    else
                    qid_w[4 * 64 + lane] = (g_ev << 8) | dq;        // (the event counter has 24 bits here: 8 million lens retries)
                }
                blk_next += n_gen;
                q_head = 0u; q_count = n_gen;
                __builtin_amdgcn_wave_barrier();
                RT_STAMP(8);
            }
            if constexpr (kMaskHandout) {                           // (the first trip's take, once more)
                const uint32_t r = rank_below(want_m);
                const unsigned long long take_m = want_m & __ballot(r < q_count);
                const bool take = __builtin_amdgcn_inverse_ballot_w64(take_m);     // (the lanes' branch runs on the mask as it is)
                RT_LDS_QUEUE_READS(take, q_head + r);
                if (take) {
                    const uint32_t e = q_head + r;
                    cam_u = quv_w[0 * 64 + e]; cam_v = quv_w[1 * 64 + e];
                    lens_wx = qid_w[0 * 64 + e]; lens_wy = qid_w[1 * 64 + e];
                    pix_global = qid_w[2 * 64 + e];
                    s = (int)qid_w[3 * 64 + e];
                    const uint32_t meta = qid_w[4 * 64 + e];
                    ev = meta >> 8;
                    pix_local = blk_pix0 + (meta & 255u);
                    my_blk = (blk_seq << 4) | (meta & 15u);
                }
                want_m &= ~take_m;
                const uint32_t took = (uint32_t)__popcll(take_m);               // = min(takers, q_count)
                q_head += took; q_count -= took;
                continue;
            }
            const uint32_t r = rank_below(m);
            RT_LDS_QUEUE_READS(want && r < q_count, q_head + r);
            if (want && r < q_count) {
                const uint32_t e = q_head + r;
                cam_u = quv_w[0 * 64 + e]; cam_v = quv_w[1 * 64 + e];
                lens_wx = qid_w[0 * 64 + e]; lens_wy = qid_w[1 * 64 + e];
                pix_global = qid_w[2 * 64 + e];
                s = (int)qid_w[3 * 64 + e];
                const uint32_t meta = qid_w[4 * 64 + e];
                ev = meta >> 8;
                pix_local = blk_pix0 + (meta & 255u);
                my_blk = (blk_seq << 4) | (meta & 15u);
                if constexpr (FRAMES) my_frame = blk_frame;
                fresh = true;
            }
            const uint32_t cnt = (uint32_t)__popcll(m);
            const uint32_t took = cnt < q_count ? cnt : q_count;
            q_head += took; q_count -= took;
        }
        if constexpr (kMaskHandout) fresh = __builtin_amdgcn_inverse_ballot_w64(__ballot(!alive) & ~want_m);
        RT_STAMP(0);
        // ==== PHASE 2: start_camera_rays =======================================================================================
        if (fresh) {                                                // camera.rs:47-54
            double lx = u11(lens_wx), ly = u11(lens_wy);
            if constexpr (U53) {                                    // the accepted unit-disk try is the last block the start drew
                const U4 lb = philox(pix_global, (uint32_t)s, ev - 1u, 0u);
                lx = u11_53(lb.x, lb.y); ly = u11_53(lb.z, lb.w);
            }
            if constexpr (!FRAMES) {
            const D3 cam_origin = ld3(P.cam.origin);
            const D3 rd = mk(lx, ly, 0.0) * P.cam.lens_radius;
            const D3 offset = ld3(P.cam.u) * rd.x + ld3(P.cam.v) * rd.y;
            o = cam_origin + offset;
            d = (((ld3(P.cam.llc) + ld3(P.cam.horizontal) * cam_u) + ld3(P.cam.vertical) * cam_v) - cam_origin) - offset;
            }
            s_thr[0][tid] = 1.0; s_thr[1][tid] = 1.0; s_thr[2][tid] = 1.0;
            depth = P.max_depth;
            alive = true;
        }
        if constexpr (FRAMES) {
            // The camera of a frame batch.  The lanes that took a sample in this pass took it from the wave's current block -- or, when the
            // queue ran empty and was refilled in the middle of PHASE 1, some from the block before it, which may be the last of the previous
            // frame.  So the wave goes through the frames its fresh lanes belong to (one, rarely two): the frame number is wave-uniform in each
            // turn, and the 19 doubles of P.cams[f] come through the constant address space as SCALAR loads -- no per-lane copy of a camera.
            // The arithmetic is camera.rs:47-54 as above, operation for operation.
            for (unsigned long long todo = __ballot(fresh); todo != 0ull;) {
                const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)my_frame, (int)__builtin_ctzll(todo));
                const bool mine = fresh && my_frame == f;
                // (the address through v_readfirstlane, half by half: the compiler then KNOWS it is wave-uniform and selects scalar loads)
                const unsigned long long ca = (unsigned long long)(uintptr_t)P.cams + (unsigned long long)f * sizeof(KCamera);
                const double __attribute__((address_space(4))) *c = (const double __attribute__((address_space(4))) *)(uintptr_t)(
                    (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ca) |
                    ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ca >> 32)) << 32));
                // (loaded by the WAVE, outside the lanes' branch: wave-uniform address, scalar loads)
                double cc[sizeof(KCamera) / sizeof(double)];
                for (int k = 0; k < (int)(sizeof(KCamera) / sizeof(double)); ++k) cc[k] = c[k];
                if (mine) {
                    const D3 cam_origin = mk(cc[0], cc[1], cc[2]);
                    const D3 rd = mk(u11(lens_wx), u11(lens_wy), 0.0) * cc[18];
                    const D3 offset = mk(cc[12], cc[13], cc[14]) * rd.x + mk(cc[15], cc[16], cc[17]) * rd.y;
                    o = cam_origin + offset;
                    d = (((mk(cc[3], cc[4], cc[5]) + mk(cc[6], cc[7], cc[8]) * cam_u) + mk(cc[9], cc[10], cc[11]) * cam_v) - cam_origin) - offset;
                }
                todo &= ~__ballot(mine);
            }
        }

        RT_STAMP(9);
        // ---- (c) every lane of the wave is out of work: done ------------------
        const unsigned long long alive_mask = __ballot(alive);
        if (alive_mask == 0ull) break;
        n_rays += (uint32_t)__popcll(alive_mask);
        // DIAG: rays traced per bounce index (0 = camera ray), per wave in LDS, flushed at exit
        if (DIAG && alive) atomicAdd(&s_live[tid >> 6][min(P.max_depth - depth, 63)], 1u);

        // ==== PHASE 3: scan (filter rows, tile list, tile loop, enumeration, pooled exact tests) ===============================
        // ---- (d) HittableList::hit, mod.rs:54-70 -------------------------------
        double closest = __builtin_inf();
        int hit = -1;
        uint32_t n_cand = 0, n_roots = 0;                           // this bounce, this lane
        const double a = length_squared(d);                         // sphere.rs:20
        // sphere.rs:16-34 for sphere idx, exactly as the reference computes it.
        // ORDERED (std::true_type): the caller visits the spheres in LIST order and this is HittableList::hit's loop body
        // as written (mod.rs:61-67 with sphere.rs:29-33's `root < t_min || t_max < root`), degenerate values included:
        // a NaN root fails neither comparison and is ACCEPTED, after which closest_so_far is NaN and every later sphere
        // with a root >= t_min is accepted too -- what the reference does with a zero-length, NaN or infinite direction.
        // Used wherever the visit IS in list order: the no-filter and VALU-filter modes, and the rays outside the
        // filter's analysed range (which is where every such direction ends up).
        auto exact_test_g = [&](int idx, const double4 g, auto ordered) {
            const D3 oc = o - mk(g.x, g.y, g.z);
            const double half_b = dot(oc, d);
            const double c = length_squared(oc) - g.w;              // g.w = radius*radius
            const double disc = half_b * half_b - a * c;
            if (disc < 0.0) return;                                 // sphere.rs:25
            if constexpr (decltype(ordered)::value) {
                if (DIAG && !(half_b > 0.0 && c > 0.0)) n_roots++;  // (counted like the other form: where that one takes a root)
                const double sq = __builtin_sqrt(disc);
                double r = (-half_b - sq) / a;                      // sphere.rs:28-34
                if (r < t_min || closest < r) {
                    r = (-half_b + sq) / a;
                    if (r < t_min || closest < r) return;
                }
                closest = r;                                        // mod.rs:63-64
                hit = idx;
                return;
            }
            // Both roots are <= 0 < t_min when the origin is outside (c > 0) and the
            // sphere lies behind the ray (half_b > 0): sqrt(disc) <= half_b, so the
            // reference's two range tests (sphere.rs:29-33) both fail.  Skip the sqrt.
            // (Not for a == 0: there the far root is 0/0, which the reference accepts -- such rays take the ORDERED form.)
            if (half_b > 0.0 && c > 0.0) return;
            if (DIAG) n_roots++;
            const double sqrtd = __builtin_sqrt(disc);
            // sphere.rs:28-34 + mod.rs:61-67, written so that the ORDER in which a ray's
            // candidates are visited does not matter: the reference keeps sphere idx iff
            // its root r* (the near root if >= t_min, else the far root) satisfies
            // t_min <= r* <= closest-so-far, so the scan ends with the smallest r*, and among
            // equal r* with the LAST sphere of the list.
            double root = (-half_b - sqrtd) / a;
            if (root < t_min) {
                root = (-half_b + sqrtd) / a;
                if (root < t_min) return;
            }
            if (root < closest || (root == closest && idx > hit)) {
                closest = root;                                     // mod.rs:63-64
                hit = idx;
            }
        };
        auto exact_test = [&](int idx, auto ordered) {
            exact_test_g(idx, *reinterpret_cast<const double4 *>(geo + 4 * (size_t)idx), ordered);
        };
        // exact tests over a per-lane list of `cnt` sphere indices in cand[][tid]
        auto test_list = [&](int cnt) {
            // trip count = longest list among the active lanes (exec-masked vote)
            for (int k = 0; __any(k < cnt); ++k) {
                if (k < cnt) { if (DIAG) n_cand++; exact_test((int)cand[k][tid], std::true_type{}); }
            }
        };

        if (MATRIX) {
            // ---- the filter on the matrix pipe: the whole wave takes part ------------
            const int wave = tid >> 6;
            const int col = lane & 15, quad = lane >> 4;
            const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            unsigned int *bits_w = &s_bits[wave][0];                // [word][ray]
            unsigned int *sum_w = &s_sum[TUBE ? 0 : wave * 64];         // (MODE 5 has no summary words)
#ifdef RTIOW_CROSSCHECK_MODES
#include "xcheck/rt_xcheck_looks.inc"      // check_half, check_sign_half: the looks of modes 2-4
#endif
            // ---- candidates -> exact tests, pooled over the wave -------------------------
            // A ray has 1.1 candidates on average but the longest list in a wave has 5-6, and the
            // exact test is ~80 f64 instructions: testing list entry k of every lane together would
            // run the test 5-6 times per bounce at ~20 % lane use.  Instead the owners only ENUMERATE
            // their bitmaps into a per-wave ring of (ray, sphere) pairs, and whenever 64 pairs are
            // waiting each lane takes ONE pair: it fetches that ray's (o, d) from the owner lane
            // (ds_bpermute), computes the root with the reference's own f64 operations, and the
            // per-ray minimum is taken in LDS on an order-preserving u64 image of the f64 root
            // (ds_min_u64); equal roots resolve to the larger sphere index (ds_max_u32), the same
            // rule as exact_test().  The ring persists across bitmap segments.
            // The u64 image of a root for ds_min_u64.  Every value that enters is >= t_min > 0, +inf, or a NaN (a root below t_min is not a
            // root, sphere.rs:29-33; rt_render_device refuses t_min <= 0): for those the f64's own bit pattern IS order-preserving, and a NaN
            // (0x7FF8..., or 0xFFF8... with the sign set) sorts above +inf, i.e. never wins -- the identity replaces round 1-4's general
            // total-order transform (a compare, two selects and three bit operations per pooled round and again when the minimum is taken).
            auto f64_key = [](double x) -> unsigned long long { return (unsigned long long)__double_as_longlong(x); };
            auto key_f64 = [](unsigned long long k) -> double { return __longlong_as_double((long long)k); };
            auto from_lane_f64 = [](int byte_addr, double x) -> double {
                const long long b = __double_as_longlong(x);
                const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, (int)(b & 0xFFFFFFFFll));
                const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, (int)(b >> 32));
                return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);
            };
            unsigned int *pool_w = &s_pool[wave][0];
            unsigned long long *best_w = &s_best[wave * 64];
            unsigned int *bidx_w = &s_bidx[wave * 64];
            // The large-grid kernel seeds each ray's minimum with what the always-exact list (or the in-order scan of a ray
            // outside the filter's range) has found, below: `closest` and `hit` then need no registers across the tile loop
            // (1 spilled VGPR instead of 7, their reloads sat in the candidate-recording path; 10k-sphere scene -0.8 %.  The
            // small-grid kernel has no spilled VGPR and measured 0.7 % SLOWER with the seed.)
            constexpr bool SEED = TUBE && !SMALLGRID;
            if constexpr (!SEED) {
                best_w[lane] = 0x7FF0000000000000ull;                   // f64_key(+inf): closest = infinity
                bidx_w[lane] = 0u;                                      // sphere index + 1; 0 = none
            }
            uint32_t pool_n = 0, pool_done = 0;                         // wave-uniform
            auto pool_round = [&]() {
                RT_STAMP(10);
                RT_COUNT(5);
                const uint32_t e_i = pool_done + (uint32_t)lane;
                const bool act = e_i < pool_n;
                const uint32_t e = act ? pool_w[e_i & 127u] : (uint32_t)lane;
                const int r = (int)(e & 63u), slot = (int)(e >> 6);         // (26 bits of column: 64 M columns)
                // MODE 5 numbers candidates by their column in the table (spheres are tiled by position); everything
                // the reference decides by a sphere's place in the list uses idx, the place in the caller's list
                const int idx = TUBE ? (int)P.slot_orig[slot] : slot;
                const double *__restrict__ pgeo = TUBE ? P.geo_slot : geo;
                const int src = r << 2;
                const D3 ro = mk(from_lane_f64(src, o.x), from_lane_f64(src, o.y), from_lane_f64(src, o.z));
                const D3 rd = mk(from_lane_f64(src, d.x), from_lane_f64(src, d.y), from_lane_f64(src, d.z));
                bool has_root = false;
                unsigned long long key = 0ull;
                // (the capped dense kernels: key and, below, old are read only where has_root holds, and there both are defined -- `has_root && old > key`
                //  may be evaluated for every lane, and its value is used under has_root alone: no constant for the lanes without a root)
                if constexpr (CAPPED) key = (unsigned long long)__double_as_longlong(unread_f64());
                if (act) {
                    if (DIAG) n_cand++;
                    // sphere.rs:16-34, exactly as exact_test() computes it
                    const double4 g = *reinterpret_cast<const double4 *>(pgeo + 4 * (size_t)slot);
                    const double ra = length_squared(rd);
                    const D3 oc = ro - mk(g.x, g.y, g.z);
                    const double half_b = dot(oc, rd);
                    const double c = length_squared(oc) - g.w;
                    const double disc = half_b * half_b - ra * c;
                    if (!(disc < 0.0) && !(half_b > 0.0 && c > 0.0)) {
                        if (DIAG) n_roots++;
                        const double sqrtd = __builtin_sqrt(disc);
                        double root = (-half_b - sqrtd) / ra;
                        if (root < t_min) root = (-half_b + sqrtd) / ra;
                        if (!(root < t_min)) {
                            // (a NaN root maps above +inf and never wins, as in exact_test(); root >= t_min > 0 otherwise)
                            key = f64_key(root);
                            has_root = true;
                        }
                    }
                }
                // Three phases, each by all lanes before the next begins (LDS operations of one wave execute in program
                // order; the wave barriers keep the compiler from moving one phase's LDS operations into another's):
                // (1) every root lowers its ray's minimum; (2) a lane that lowered it forgets the sphere recorded for the
                // old minimum; (3) the roots EQUAL to the final minimum record the largest sphere index among them --
                // the order-independent form of mod.rs:61-67 (smallest root, ties -> the later sphere of the list).
                unsigned long long old = 0ull;
                if constexpr (CAPPED) old = (unsigned long long)__double_as_longlong(unread_f64());
                RT_LDS_N(4, 12, 4, false, false, src, true);                            // the twelve ds_bpermute of (o, d)
                RT_LDS(2, 8, true, false, &best_w[r], has_root);
                if (has_root) old = atomicMin(&best_w[r], key);
                __builtin_amdgcn_wave_barrier();
                RT_LDS(3, 4, false, false, &bidx_w[r], has_root && old > key);
                if (has_root && old > key) bidx_w[r] = 0u;
                __builtin_amdgcn_wave_barrier();
                RT_LDS(7, 8, false, true, &best_w[r], has_root);
                RT_LDS_POOL_TIE(has_root, r, key);
                if (has_root && best_w[r] == key) atomicMax(&bidx_w[r], (unsigned)idx + 1u);
                __builtin_amdgcn_wave_barrier();
                pool_done = min(pool_done + 64u, pool_n);
                RT_STAMP(2);
            };
            // owners push the candidates of segment seg0 (ascending sphere order); rounds run as the ring fills
            // MODE 5: the tiles this pass scans -- every tile of the table in turn, or the list behind the bitmap words
            bool list_all = true;
#if defined(RT_LDS_CONFLICTS) || defined(RT_COUNT_ENUM)
            constexpr bool kAsmWalk = false;                    // (the conflict model and the trip counters read each trip's masks and addresses)
#else
            constexpr bool kAsmWalk = CAPPED && TUBE && SMALLGRID;
#endif
            auto enumerate = [&](int seg0, int nwords_tube = 0) {
                unsigned summary = 0u, word = 0u;
                if constexpr (TUBE) {
                    // which of the segment's words hold a candidate of this ray (the recording side sets bits only)
                    // (min(word, 1) << w | summary: a v_min_u32 and a v_lshl_or_b32 per word where `word != 0 ? 1 << w : 0` is a compare, a select and an or)
                    if constexpr (CAPPED) {
                        // (the capped dense kernels: the constant is opaque, or min(word, 1) is canonicalised into a compare and a select.  Small grid: two
                        //  rows per trip and no remainder loop -- every row of the segment is zeroed, so the row behind an odd count reads as no candidate;
                        //  the large-grid pair spills four more scalars with any paired or fixed-trip form, 67 against 63, and keeps one row per trip)
                        uint32_t one = 1u;
                        asm volatile("" : "+v"(one));
                        if constexpr (SMALLGRID) {
                            for (int w = 0; w < nwords_tube; w += 2) {
                                summary |= min(bits_w[w * 64 + lane], one) << w;
                                summary |= min(bits_w[(w + 1) * 64 + lane], one) << (w + 1);
                            }
                        } else
                        for (int w = 0; w < nwords_tube; ++w) summary |= min(bits_w[w * 64 + lane], one) << w;
                    } else
                    for (int w = 0; w < nwords_tube; ++w) summary |= min(bits_w[w * 64 + lane], 1u) << w;
                    if (!alive) summary = 0u;
                } else {
                    summary = alive ? s_sum[tid] : 0u;
                }
                // (kAsmWalk, once per call: the walk's LDS addresses and the full lane mask its trips restore)
                uint32_t row_at = 0u, tl_at = 0u, pool_at = 0u;
                unsigned long long full_exec = 0ull;
                if constexpr (kAsmWalk) {
                    typedef __attribute__((address_space(3))) unsigned int *LdsWord;
                    row_at = (uint32_t)(uintptr_t)(LdsWord)(bits_w + lane);                     // word w of this lane: + 256 w
                    tl_at = (uint32_t)(uintptr_t)(LdsWord)(bits_w + seg0);                      // the tile of word w: + 4 (kSeg / 2) 64 + 4 w
                    pool_at = (uint32_t)(uintptr_t)(LdsWord)pool_w;
                    asm volatile("s_mov_b64 %[fx], exec" : [fx] "=s"(full_exec));
                }
                int wbase = 0;
                if constexpr (kAsmWalk) {
                    // The capped small-grid kernels: the trips of the loop below as ONE asm block that loops until the walk is over or 64 pairs wait
                    // for a pooled round (pool_round stays C++ and runs between two entries) -- lane for lane the same refills and the same pushes
                    // in the same trips, so the ring holds the same pairs in the same order.  v_cmpx narrows exec to the lanes that have a candidate
                    // and leaves their mask in vcc: the rank (v_mbcnt) and the count (s_bcnt1) read it, and the empty-exec branch behind it is the
                    // walk's exit.  A lane never gains a candidate during a call, so exec only narrows from trip to trip and the full mask, saved once
                    // per call, comes back when the block is left, not after every trip.  The refill runs under a second v_cmpx (word == 0) and
                    // exec comes back from vcc; a trip in which no lane refills branches round it: measured without that branch, the two LDS reads
                    // of an empty refill and the wait for them cost more than the branch (profiles/scalar_trim3_ab.txt).  8 scalar instructions and
                    // 3 exec writes per trip where the compiler's form has 15 and 4 (two s_and_saveexec regions with a branch each, two s_or restores,
                    // three copies of pool_n / pool_done, beside two dead v_readfirstlane).  The block touches vector registers, scalar registers and
                    // LDS -- nothing on the scalar unit writes memory -- and waits for its own two LDS reads.
                    for (;;) {
                        uint32_t cnt, av, t0, t1, t2;
                        unsigned long long refill_m;
                        asm volatile("0:\n\t"
                                     "v_or_b32_e32 %[t0], %[sum], %[word]\n\t"
                                     "v_cmpx_ne_u32_e32 vcc, 0, %[t0]\n\t"                     // exec = vcc = has (a lane never gains a candidate: exec only narrows from trip to trip)
                                     "s_cbranch_execz 1f\n\t"
                                     "s_bcnt1_i32_b64 %[cnt], vcc\n\t"
                                     "v_mbcnt_lo_u32_b32 %[t2], vcc_lo, 0\n\t"
                                     "v_mbcnt_hi_u32_b32 %[t2], vcc_hi, %[t2]\n\t"
                                     "v_cmpx_eq_u32_e64 %[rm], 0, %[word]\n\t"                 // exec = has && word == 0: the refill
                                     "s_cbranch_execz 2f\n\t"
                                     "v_ffbl_b32_e32 %[t0], %[sum]\n\t"
                                     "v_lshl_add_u32 %[t1], %[t0], 8, %[row]\n\t"
                                     "v_lshl_add_u32 %[t0], %[t0], 2, %[tl]\n\t"
                                     "ds_read_b32 %[t0], %[t0] offset:%[tlo]\n\t"
                                     "ds_read_b32 %[word], %[t1]\n\t"
                                     "v_add_u32_e32 %[t1], -1, %[sum]\n\t"
                                     "v_and_b32_e32 %[sum], %[t1], %[sum]\n\t"
                                     "s_waitcnt lgkmcnt(1)\n\t"
                                     "v_lshlrev_b32_e32 %[wb], 5, %[t0]\n\t"                   // (32 * (entry & 0x0FFFFFFF): the shift drops the group bits)
                                     "s_waitcnt lgkmcnt(0)\n"
                                     "2:\n\t"
                                     "s_mov_b64 exec, vcc\n\t"                                 // exec = has: the push
                                     "v_ffbl_b32_e32 %[t0], %[word]\n\t"
                                     "v_add_u32_e32 %[t1], -1, %[word]\n\t"
                                     "v_and_b32_e32 %[word], %[t1], %[word]\n\t"
                                     "v_add_u32_e32 %[t2], %[pn], %[t2]\n\t"
                                     "v_add_u32_e32 %[t0], %[t0], %[wb]\n\t"
                                     "v_and_b32_e32 %[t2], 0x7f, %[t2]\n\t"
                                     "v_lshl_or_b32 %[t0], %[t0], 6, %[ln]\n\t"
                                     "v_lshl_add_u32 %[t2], %[t2], 2, %[pool]\n\t"
                                     "ds_write_b32 %[t2], %[t0]\n\t"
                                     "s_add_i32 %[pn], %[pn], %[cnt]\n\t"
                                     "s_sub_i32 %[av], %[pn], %[pd]\n\t"
                                     "s_cmp_lt_u32 %[av], 64\n\t"
                                     "s_cbranch_scc1 0b\n"                                     // (64 pairs wait: out, for a pooled round)
                                     "1:\n\t"
                                     "s_mov_b64 exec, %[fx]"
                                     : [sum] "+v"(summary), [word] "+v"(word), [wb] "+v"(wbase), [pn] "+s"(pool_n), [cnt] "=&s"(cnt), [av] "=&s"(av), [rm] "=&s"(refill_m),
                                       [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2)
                                     : [row] "v"(row_at), [tl] "v"(tl_at), [pool] "v"(pool_at), [ln] "v"(lane), [fx] "s"(full_exec), [pd] "s"(pool_done),
                                       [tlo] "i"(4 * (kSeg / 2) * 64)
                                     : "vcc", "scc", "memory");
                        if (pool_n - pool_done < 64u) break;
                        pool_round();
                    }
                } else
                for (;;) {
                    const bool has = (summary | word) != 0u;
                    const unsigned long long m = __ballot(has);
                    if (m == 0ull) break;
                    RT_COUNT_ENUM_TRIP(m);
                    RT_LDS_ENUM_READS(has, word, summary, seg0);
                    if (has) {
                        if (word == 0u) {
                            const int w = __builtin_ctz(summary);
                            summary &= summary - 1u;
                            word = bits_w[w * 64 + lane];
                            if constexpr (TUBE)         // seg0: position in the tile list of the segment's first tile
                                wbase = 32 * (!SMALLGRID && list_all ? seg0 + w : (int)(bits_w[(kSeg / 2) * 64 + seg0 + w] & 0x0FFFFFFFu));
                            else
                                wbase = 16 * seg0 + 32 * w;
                        }
                        const int bpos = __builtin_ctz(word);
                        word &= word - 1u;
                        const uint32_t pos = pool_n + rank_below(m);
                        pool_w[pos & 127u] = ((uint32_t)(wbase + bpos) << 6) | (uint32_t)lane;
                    }
                    pool_n += (uint32_t)__popcll(m);
                    if (pool_n - pool_done >= 64u) pool_round();
                }
            };
            // after the last segment: drain the ring, then every owner takes its minimum
            auto finish_pool = [&]() {
                RT_STAMP(10);
                while (pool_done < pool_n) pool_round();
                const unsigned int hb = bidx_w[lane];
                if constexpr (SEED) {
                    // (the seeded minimum IS the closest hit: equal roots took the maximum of the list indices, seed included --
                    //  mod.rs:61-67's later-sphere-wins; a ray outside the filter's range has no candidates, its seed, NaN roots
                    //  included, comes back bit for bit)
                    if (alive) { hit = (int)hb - 1; closest = key_f64(best_w[lane]); }
                } else if constexpr (CAPPED) {
                    // (the capped dense kernels: the same decision without a lane-level region -- every lane reads its own minimum, the four
                    //  compares are combined as masks on the scalar unit and three selects take the hit: two nested exec regions with a branch
                    //  and two restores less.  A lane without a ray or without a pooled root takes nothing, as below; a NaN root passes no compare.)
                    const double root = key_f64(best_w[lane]);
                    const int idx = (int)hb - 1;
                    const bool take = alive & (hb != 0u) & ((root < closest) | ((root == closest) & (idx > hit)));
                    closest = take ? root : closest;
                    hit = take ? idx : hit;
                } else
                if (alive && hb != 0u) {
                    const double root = key_f64(best_w[lane]);
                    const int idx = (int)hb - 1;
                    if (root < closest || (root == closest && idx > hit)) { closest = root; hit = idx; }
                }
            };
            const int nt = P.n_tiles;                   // even; the tables hold nt + 2 tiles

            if constexpr (TUBE) {
                // The record of the first always-exact sphere (the ground) is asked for HERE and used after the filter rows have been
                // built: ~130 vector instructions that need nothing from memory run under its latency (-0.5 % frame time).
                const double4 g_first = *reinterpret_cast<const double4 *>(geo + 4 * (size_t)(P.n_always > 0 ? P.always_idx[0] : 0));
                const bool scan = alive;
                const unsigned long long scan_mask = __ballot(scan);
                if (scan_mask != 0ull) {
                float ray_of[3], ray_df[3], ray_o1;                 // (the ray in f32, shared by the filter rows and the footprint)
                ray_f32(o, d, ray_of, ray_df, ray_o1);
                // (rows of every lane as if it had a ray inside the analysed range; the lanes without one -- none in the steady state: a lane
                //  whose path ends starts its next sample at once -- and the rays outside it get rows that keep nothing behind ONE wave-level
                //  branch: 16 selects per pass less)
                TubeRay T = make_tube<false>(ray_of, ray_df, ray_o1, P.tube_rho);
                if (!scan) T.sane = true;
                if (__builtin_expect(__ballot(!scan || !T.sane) != 0ull, 0)) {
                    if (!scan || !T.sane) tube_rows_keep_nothing(T);
                }
                bf16x8 A[4];
                {
                    uint32_t w[2][8];
                    tube_a_words(T, w);
                    tube_stage_operands(reinterpret_cast<uint4 *>(bits_w), lane, w, A);
                }
                // the spheres that skip the filter (the ground): tested exactly by every ray
                if (alive)
                    for (int e = 0; e < P.n_always; ++e) {
                        if (DIAG) n_cand++;
                        if (e == 0) exact_test_g(P.always_idx[0], g_first, std::false_type{});
                        else exact_test(P.always_idx[e], std::false_type{});
                    }
                // outside the analysed range (zero, NaN and infinite directions are): HittableList::hit as written, over
                // the whole list in list order (what the always-exact list and the pool find for this ray is a subset of it)
                if (scan && !T.sane) {
                    closest = __builtin_inf(); hit = -1;
                    for (int i = 0; i < n; ++i) { if (DIAG) n_cand++; exact_test(i, std::true_type{}); }
                }
                if constexpr (SEED) {
                    best_w[lane] = f64_key(closest);                    // (+inf without a hit: 0x7FF0000000000000)
                    bidx_w[lane] = (unsigned)(hit + 1);                 // sphere index + 1; 0 = none
                }
                typedef float f32x16 __attribute__((ext_vector_type(16)));
                const int ntt = nt >> 1;                    // tiles of 32 spheres; the tables hold ntt + 1
                const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<uint4 *>(P.btube), 0, (ntt + 1) * 1024, 0x00020000);
                const int voff = lane * 16;
                auto load_b = [&](int t32) -> bf16x8 {
                    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(brs, voff, t32 * 1024, 0));
                };
                const int col32 = lane & 31, hh = lane >> 5;
                const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                // results of one MFMA: acc[8bb + j] / acc[8bb + 4 + j] are H_1 / H_2 of ray 16G + 8bb + 4hh + j against
                // sphere 32 t + col32, in units of half the sphere's bound (the host scales every column): the pair is
                // kept iff |H_1| < 2 and |H_2| < 2, i.e. iff bit 30 of BOTH f32 patterns is clear (biased exponent
                // < 128; infinities and NaNs have it set).  So the look is bit logic: X_bb = AND over the lane's four rays
                // 8 bb + j of (H_1 | H_2) -- one v_or_b32 and three v_bitop3_b32 (a & (b | c)) per half -- has bit 30
                // clear iff one of them keeps this sphere, and one compare per half, |X_bb| < 2.0, reads that bit: the OR of the two
                // wave masks feeds the wave-level branch, each mask its half of the recording path.  10 vector instructions of
                // 2.7-4.9 SIMD cycles where max/min-trees took 14 of 4.3-5.4 (tools/valu_cost_table.hip: v_max/v_min*
                // cost 4.3-5.4 cycles at four waves per SIMD, v_or/v_bitop3 2.7-3.1).
                auto keeps = [](uint32_t x) -> bool { return __builtin_fabsf(__uint_as_float(x)) < kTubeKeepBelow; };
                static_assert(kTubeKeepBelow == 2.0f, "the recording path's asm spells the bound as the inline constant 2.0");
#if defined(RT_LDS_CONFLICTS)
                constexpr bool kAsmRecord = false;              // (the conflict model reads each step's address and mask)
#else
                constexpr bool kAsmRecord = CAPPED;
#endif
                auto look_tube = [&](int G, const f32x16 &acc, int wrel) {
                    // X_bb: the AND over the four rays 8 bb + j of this lane; the wave-level branch tests X_0 & X_1
                    uint32_t X[2];
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) {
                        X[bb] = __float_as_uint(acc[8 * bb]) | __float_as_uint(acc[8 * bb + 4]);
#pragma unroll
                        for (int j = 1; j < 4; ++j)
                            X[bb] = __builtin_amdgcn_bitop3_b32(X[bb], __float_as_uint(acc[8 * bb + j]), __float_as_uint(acc[8 * bb + 4 + j]), 0xE0);
                    }
                    // one wave-level test per HALF, made once: the branch below is taken when either half keeps something, and the halves'
                    // masks are what the recording path branches on (round 4 tested X_0 & X_1 here -- one compare -- and each half again behind
                    // the branch, which two thirds of the looks take: -0.3 % on the book scene, -2 % on the 10k-sphere scene)
                    const unsigned long long kh[2] = {__ballot(keeps(X[0])), __ballot(keeps(X[1]))};
                    if (__builtin_expect((kh[0] | kh[1]) != 0ull, 0)) {
                        RT_COUNT(3);
                        unsigned bit;
                        if constexpr (CAPPED) {
                            // (the capped dense kernels: 1 << (lane & 31) as ONE instruction on the register that holds the lane id -- the shift reads
                            //  the low five bits of its count -- where the pinned copy of col32 cost a v_mov beside the shift per look with a candidate;
                            //  the asm is what keeps the address arithmetic on this side of the branch, as the pin did)
                            asm volatile("v_lshlrev_b32_e64 %0, %1, 1" : "=v"(bit) : "v"(lane));
                        } else {
                        int colv = col32;
                        asm volatile("" : "+v"(colv));              // keep the address arithmetic on this side of the branch
                        bit = 1u << colv;
                        }
                        int rbase = wrel * 64 + 4 * hh;             // (4 hh folded into the row's base, not into each word's index: -0.3 %)
                        unsigned int *row = bits_w + rbase;
#pragma unroll
                        for (int bb = 0; bb < 2; ++bb) {
                            if (kh[bb] != 0ull) {
                                RT_COUNT(4);
                                if constexpr (kAsmRecord) {
                                    // The capped dense kernels: ONE scalar instruction per ray step, not two.  v_cmpx narrows exec to the lanes that keep
                                    // (it replaces the v_cmp; s_and_saveexec is gone), the ds_or runs under it, and exec comes back from the half's saved
                                    // mask with one s_mov -- which is also what lets the next compare see the half's full mask.  5 scalar instructions
                                    // per half where the compiler's form has 8; written as one asm block so that no step gets an exec-empty branch.
                                    // (LDS operations of a wave complete in order: the walk's later reads of these words see them.)
                                    typedef __attribute__((address_space(3))) unsigned int *LdsWord;
                                    const uint32_t at = (uint32_t)(uintptr_t)(LdsWord)row;             // (the steps' words: immediate offsets, as the compiler's form has them)
                                    uint32_t xs[4];
#pragma unroll
                                    for (int j = 0; j < 4; ++j) xs[j] = __float_as_uint(acc[8 * bb + j]) | __float_as_uint(acc[8 * bb + 4 + j]);
                                    unsigned long long half_exec;
                                    asm volatile("s_mov_b64 %[sv], exec\n\t"
                                                 "v_cmpx_lt_f32_e64 vcc, |%[x0]|, 2.0\n\t"
                                                 "ds_or_b32 %[at], %[bit] offset:%[o0]\n\t"
                                                 "s_mov_b64 exec, %[sv]\n\t"
                                                 "v_cmpx_lt_f32_e64 vcc, |%[x1]|, 2.0\n\t"
                                                 "ds_or_b32 %[at], %[bit] offset:%[o1]\n\t"
                                                 "s_mov_b64 exec, %[sv]\n\t"
                                                 "v_cmpx_lt_f32_e64 vcc, |%[x2]|, 2.0\n\t"
                                                 "ds_or_b32 %[at], %[bit] offset:%[o2]\n\t"
                                                 "s_mov_b64 exec, %[sv]\n\t"
                                                 "v_cmpx_lt_f32_e64 vcc, |%[x3]|, 2.0\n\t"
                                                 "ds_or_b32 %[at], %[bit] offset:%[o3]\n\t"
                                                 "s_mov_b64 exec, %[sv]"
                                                 : [sv] "=&s"(half_exec)
                                                 : [x0] "v"(xs[0]), [x1] "v"(xs[1]), [x2] "v"(xs[2]), [x3] "v"(xs[3]), [at] "v"(at), [bit] "v"(bit),
                                                   [o0] "i"(4 * (16 * G + 8 * bb)), [o1] "i"(4 * (16 * G + 8 * bb + 1)), [o2] "i"(4 * (16 * G + 8 * bb + 2)),
                                                   [o3] "i"(4 * (16 * G + 8 * bb + 3))
                                                 : "vcc", "memory");
                                } else
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    RT_LDS(0, 4, true, false, &row[16 * G + 8 * bb + j],
                                           keeps(__float_as_uint(acc[8 * bb + j]) | __float_as_uint(acc[8 * bb + 4 + j])));
                                    if (keeps(__float_as_uint(acc[8 * bb + j]) | __float_as_uint(acc[8 * bb + 4 + j])))
                                        atomicOr(&row[16 * G + 8 * bb + j], bit);
                                }
                            }
                        }
                    }
                };
                // ---- which tiles: the global ones and the grid cells some ray of the wave can reach ---------------
                // Every ray finds the cells of its footprint (rt_device.hpp, grid_cells: columns ix0.., rows iz0..); the
                // union over the wave becomes a list of tiles in LDS (tl[]: the global tiles, then the cells' tiles in
                // ascending order, then two spare entries for the loop's look-ahead).  If a footprint cannot be
                // computed, or the list is longer than kListCap, the wave scans every tile of the table instead.
                int n_list = ntt;
                unsigned int *tl = bits_w + (kSeg / 2) * 64;                // (behind the bitmap words)
                auto wave_or = [](int v) -> int {               // the OR over the wave (DPP; lane 63 collects it)
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);    // row_shr:1
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);    // row_shr:2
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);    // row_shr:4
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);    // row_shr:8
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast15 -> rows 1, 3
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast31 -> rows 2, 3
                    return __builtin_amdgcn_readlane(v, 63);
                };
                auto rows_or = [](int v) -> int {               // the OR over each row of 16 lanes (lane 16 g + 15 collects group g's)
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);    // row_shr:1
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);    // row_shr:2
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);    // row_shr:4
                    v |= __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);    // row_shr:8
                    return v;
                };
                auto wave_scan_add = [](int v) -> int {         // inclusive prefix sum over the lanes (DPP)
                    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
                    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
                    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
                    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
                    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
                    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
                    return v;
                };
                if (SMALLGRID || P.grid_dim > 0) {
                    int ix0 = 0, nx = 0, iz0 = 0, nz = 0, cnt = 0;
                    GridSeg seg;
                    RT_STAMP(5);
                    if (scan && T.sane) cnt = grid_cells(ray_of, ray_df, ray_o1, P.grid, P.grid_dim, P.scene_scale, ix0, nx, iz0, nz, SMALLGRID ? nullptr : &seg);
                    RT_STAMP(7);
                    const int gcells = P.grid_dim * P.grid_dim;
                    if (SMALLGRID || P.n_global + gcells <= 64) {
                        // a small grid: the cells fit ONE 64-bit mask per ray (bit iz * grid_dim + ix); the wave's set
                        // of cells is the OR over its lanes, taken in registers, and lane c finds the place of cell c's
                        // tile in the list by counting the set cells below it
                        unsigned long long m = cnt < 0 ? ~0ull : 0ull;          // (cannot tell: every cell)
                        if (cnt > 0) {
                            // the footprint's columns, repeated in each of its rows: the rows sit grid_dim bits apart and
                            // the run is narrower than that, so the product has no carries
                            const unsigned long long run = (unsigned long long)(((1u << nx) - 1u) << ix0);
                            const unsigned long long rows = P.grid_rows & (~0ull >> (64 - nz * P.grid_dim));
                            m = (run * rows) << (iz0 * P.grid_dim);
                        }
#if RT_GROUP_SKIP
                        // ... and per 16-ray GROUP: a DPP row is 16 lanes, so after the four row steps lane 16 g + 15 holds group g's
                        // cells; the wave's set is the OR of the four.  Each list entry carries, in its top four bits, which groups
                        // can reach the tile: the tile loop skips the matrix instruction and the look of the others.
                        // (skipping the high dword for grids of at most 32 cells -- the book scene's 4 x 4 -- measured SLOWER: 11.18 vs 11.10 ms)
                        const int vlo = rows_or((int)(unsigned)m), vhi = rows_or((int)(unsigned)(m >> 32));
                        unsigned mlo = 0u, mhi = 0u, gm = 0u;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const unsigned lo = (unsigned)__builtin_amdgcn_readlane(vlo, 16 * g + 15), hi = (unsigned)__builtin_amdgcn_readlane(vhi, 16 * g + 15);
                            mlo |= lo; mhi |= hi;
                            if (__builtin_amdgcn_inverse_ballot_w64(((unsigned long long)hi << 32) | lo)) gm |= 1u << g;    // (lane c: is cell c in group g's set)
                        }
                        const unsigned kAll = 0xF0000000u;
#else
                        const unsigned mlo = (unsigned)wave_or((int)(unsigned)m), mhi = (unsigned)wave_or((int)(unsigned)(m >> 32));
                        const unsigned gm = 0u, kAll = 0u;
#endif
                        const unsigned long long cells = (((unsigned long long)mhi << 32) | mlo) & (~0ull >> (64 - gcells));
                        const int rank = (int)__builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
                        tl[lane] = (unsigned)(lane < P.n_global ? lane : ntt) | kAll;      // (past the list: the spare tile)
                        if (lane < 2) tl[64 + lane] = (unsigned)ntt | kAll;
                        __builtin_amdgcn_wave_barrier();
                        if ((cells >> lane) & 1ull) tl[P.n_global + rank] = (unsigned)(P.n_global + lane) | (gm << 28);
                        __builtin_amdgcn_wave_barrier();
                        list_all = false;
                        n_list = P.n_global + __builtin_popcountll(cells);
                    } else if (!SMALLGRID && __ballot(cnt < 0) == 0ull) {
                        // a large grid: one word per grid ROW in LDS (32 bits for grids of at most 32 cells per side -- the 10k-sphere
                        // scene's 19 x 19 --, else 64: shifts, counts and bit scans of a 64-bit word are two or three instructions each),
                        // ORed by the rays; lane l then owns row l, a prefix sum over the rows' cell counts gives each row its place in
                        // the list.  One set of row words per 16-ray group (at most 2 KB of the bitmap area, free until the tile loop):
                        // each list entry carries in its top four bits which groups can reach the tile.
                        if (cnt == 0) nz = 0;
                        auto build_list = [&](auto zero) {
                            typedef decltype(zero) W;
                            constexpr int kGroups = RT_GROUP_SKIP ? 4 : 1;
                            W *tm = reinterpret_cast<W *>(bits_w);                          // [kGroups][64]
#pragma unroll
                            for (int g = 0; g < kGroups; ++g) tm[g * 64 + lane] = (W)0;
                            int lg_ = lane;
                            asm volatile("" : "+v"(lg_));           // (computed here, per pass: hoisted out of the bounce loop this address was spilled to scratch memory -- a vector-memory
                                                                    //  round trip and an s_waitcnt vmcnt(0) per pass; 10k-sphere scene -0.65 %)
                            W *tm_g = tm + (RT_GROUP_SKIP ? (lg_ >> 4) * 64 : 0);
                            __builtin_amdgcn_wave_barrier();
                            // row by row: the columns of the part of the clipped piece that lies in the row's band (grid_row_run)
                            for (int k = 0; __any(k < nz); ++k) {
                                RT_COUNT_ROWS_TRIP(1);
                                if (k < nz) {
                                    int rx0, rnx;                                           // 1 <= rnx, rnx + rx0 <= grid_dim <= 32 or 63
                                    grid_row_run(seg, ix0, ix0 + nx - 1, (float)(iz0 + k), rx0, rnx);
                                    atomicOr(&tm_g[iz0 + k], (W)((W)(~(W)0 >> (8 * (int)sizeof(W) - rnx)) << rx0));
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                            W wg[kGroups];
                            W mw = (W)0;
#pragma unroll
                            for (int g = 0; g < kGroups; ++g) { wg[g] = tm[g * 64 + lane]; mw |= wg[g]; }
                            const int mine = sizeof(W) == 8 ? __builtin_popcountll(mw) : __builtin_popcount((unsigned)mw);
                            const int upto = wave_scan_add(mine);
                            const int tn = P.n_global + __builtin_amdgcn_readlane(upto, 63);
                            if (tn <= kListCap) {
                                const unsigned kAll = RT_GROUP_SKIP ? 0xF0000000u : 0u;
                                if (lane < P.n_global) tl[lane] = (unsigned)lane | kAll;
                                int pos = P.n_global + upto - mine;
                                const int row0 = P.n_global + lane * P.grid_dim;
                                while (__any(mw != (W)0)) {
                                    RT_COUNT_ROWS_TRIP(6);
                                    if (mw != (W)0) {
                                        const int bpos = sizeof(W) == 8 ? __builtin_ctzll(mw) : __builtin_ctz((unsigned)mw);
                                        unsigned gm = 0u;
#pragma unroll
                                        for (int g = 0; g < (RT_GROUP_SKIP ? 4 : 0); ++g) gm |= (unsigned)((wg[g] >> bpos) & (W)1) << g;
                                        tl[pos++] = (unsigned)(row0 + bpos) | (gm << 28);
                                        mw &= mw - (W)1;
                                    }
                                }
                                int ntt_ = ntt;
                                asm volatile("" : "+s"(ntt_));      // (likewise: the broadcast of this scalar sat in a spilled register; -0.6 %)
                                if (lane < 2) tl[tn + lane] = (unsigned)ntt_ | kAll;
                                __builtin_amdgcn_wave_barrier();
                                list_all = false;
                                n_list = tn;
                            }
                        };
                        if (P.grid_dim <= 32) build_list(0u); else build_list(0ull);
                    }
                }
                RT_STAMP(3);
                RT_STAMP(5);
                for (int t0 = 0; t0 < n_list; t0 += kSeg / 2) {
                    __builtin_amdgcn_s_setprio(3);
                    const int nwords = min(kSeg / 2, n_list - t0);          // one bitmap word per 32-sphere tile
                    if constexpr (CAPPED) {
                        // (the capped dense kernels: every row of the bitmap, seven paired stores and no loop around them -- the rows are exactly the area in
                        //  front of the tile list, and a row the segment does not use stays zero for the summary above)
                        static_assert(TUBE, "the rows in front of the tile list");
#pragma unroll
                        for (int w = 0; w < kSeg / 2; ++w) bits_w[w * 64 + lane] = 0u;
                    } else
                    for (int w = 0; w < nwords; ++w) bits_w[w * 64 + lane] = 0u;
                    // the segment's tiles (and two more for the look-ahead), one per lane
                    const int listv = !SMALLGRID && list_all ? (min(t0 + lane, ntt) | (RT_GROUP_SKIP ? (int)0xF0000000u : 0))
                                                             : (int)tl[min(t0 + lane, kListCap + 1)];
                    // j < 20, wave-uniform: the tile, and (top four bits) the 16-ray groups that can reach it
                    auto tile_at = [&](int j) -> int { return __builtin_amdgcn_readlane(listv, j) & 0x0FFFFFFF; };
                    auto groups_at = [&](int j) -> unsigned { return (unsigned)__builtin_amdgcn_readlane(listv, j) >> 28; };
                    __builtin_amdgcn_wave_barrier();
                    // one 32-sphere tile: four independent MFMAs (one per 16-ray group); two results in
                    // flight so the matrix pipe works on the next group while the VALU looks at this one
                    auto do_tile = [&](int w, const bf16x8 &b, unsigned groups) {
                        RT_COUNT(7);
                        RT_COUNT_N(2, __builtin_popcount(groups));      // (counter 2: matrix instructions + looks executed)
                        RT_COUNT_TILE_GROUPS(groups);
#if RT_GROUP_SKIP
                        if (groups != 0xFu) {
                            // some groups cannot reach this tile (none of their rays' footprints holds its cell): only the others
                            // go through the matrix pipe and the look
#pragma unroll
                            for (int G = 0; G < 4; ++G)
                                if ((groups >> G) & 1u) {
                                    f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[G], b, zero16, 0, 0, 0);
                                    look_tube(G, acc, w);
                                }
                            return;
                        }
#endif
                        // (the empty asm pins the issue order: the scheduler would otherwise sink each MFMA
                        //  below the previous look to share registers, and the wave would sit out the full
                        //  matrix-pipe latency four times per tile)
                        f32x16 acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], b, zero16, 0, 0, 0);
                        f32x16 acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], b, zero16, 0, 0, 0);
                        asm volatile("" : "+v"(acc1));
                        look_tube(0, acc0, w);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2], b, zero16, 0, 0, 0);
                        asm volatile("" : "+v"(acc0));
                        look_tube(1, acc1, w);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[3], b, zero16, 0, 0, 0);
                        asm volatile("" : "+v"(acc1));
                        look_tube(2, acc0, w);
                        look_tube(3, acc1, w);
                    };
                    {
                        // B operands ping-pong between two register sets, each fetched a tile ahead.
                        bf16x8 bp, bq;
                        int w = 0;
                        if constexpr (CAPPED) {
                            // (the capped dense kernels: a list entry is read ONCE -- its tile when the B operand is asked for, its groups a tile later from
                            //  the same scalar -- not once for each: one v_readlane and its index less per tile)
                            auto entry_at = [&](int j) -> unsigned { return (unsigned)__builtin_amdgcn_readlane(listv, j); };
                            unsigned ep = entry_at(0), eq;
                            bp = load_b((int)(ep & 0x0FFFFFFFu));
                            for (; w + 1 < nwords; w += 2) {
                                eq = entry_at(w + 1);
                                bq = load_b((int)(eq & 0x0FFFFFFFu));
                                do_tile(w, bp, ep >> 28);
                                ep = entry_at(w + 2);
                                bp = load_b((int)(ep & 0x0FFFFFFFu));
                                do_tile(w + 1, bq, eq >> 28);
                            }
                            if (w < nwords) do_tile(w, bp, ep >> 28);
                        } else {
                        bp = load_b(tile_at(0));
                        for (; w + 1 < nwords; w += 2) {
                            bq = load_b(tile_at(w + 1));
                            do_tile(w, bp, groups_at(w));
                            bp = load_b(tile_at(w + 2));
                            do_tile(w + 1, bq, groups_at(w + 1));
                        }
                        if (w < nwords) do_tile(w, bp, groups_at(w));
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    RT_STAMP(6);
                    __builtin_amdgcn_s_setprio(2);
                    enumerate(t0, nwords);
                }
                __builtin_amdgcn_s_setprio(1);
                finish_pool();
                __builtin_amdgcn_s_setprio(0);              // (the shading below)
                }   // scan_mask != 0
            }
#ifdef RTIOW_CROSSCHECK_MODES
#include "xcheck/rt_xcheck_scan.inc"       // else if constexpr (LIFTED) { mode 4 } else { modes 2, 3 }
#endif
        }
        RT_STAMP(2);
        if (alive && !MATRIX) {
            if (MODE == 0) {
                for (int i = 0; i < n; ++i) { if (DIAG) n_cand++; exact_test(i, std::true_type{}); }
            } else {
                const RayFilter f = make_filter(o, d);
                int cnt = 0;
                auto drain = [&]() { test_list(cnt); cnt = 0; };
                // One filter test.  Candidates are rare per sphere (about one wave-test in ten
                // has any), so the push sits behind a wave-level branch that is normally not taken.
                auto test = [&](float cx, float cy, float cz, float kp, int i) {
                    const bool keep = filter_keeps(f, cx, cy, cz, kp);
                    if (__builtin_expect(__ballot(keep) != 0ull, 0)) {
                        if (keep) {
                            cand[cnt][tid] = (uint16_t)i;
                            cnt++;
                        }
                    }
                };
                // The filter records stream through SGPRs in batches of kScanUnroll spheres
                // (32 dwords, two s_load_dwordx16): one scalar-memory wait per ~100 VALU ops,
                // hidden by the other waves of the SIMD.
                constexpr int BW = 4 * kScanUnroll;
                const int nb = n / kScanUnroll;
                for (int bidx = 0; bidx < nb; ++bidx) {
                    const float __attribute__((address_space(4))) *q = filt + (size_t)BW * (size_t)bidx;
                    float rec[BW];
#pragma unroll
                    for (int k = 0; k < BW; ++k) rec[k] = q[k];
#pragma unroll
                    for (int k = 0; k < kScanUnroll; ++k)
                        test(rec[4 * k + 0], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3], bidx * kScanUnroll + k);
                    // drain before any lane could overflow its list
                    if (__any(cnt > kCandCap - kScanUnroll)) drain();
                }
                for (int i = nb * kScanUnroll; i < n; ++i) {
                    const float __attribute__((address_space(4))) *q = filt + 4 * (size_t)i;
                    test(q[0], q[1], q[2], q[3], i);
                }
                drain();
            }
        }

        if (DIAG) {   // fold this bounce's counts into the wave totals (all lanes are here)
            unsigned long long pk = (unsigned long long)n_cand | ((unsigned long long)n_roots << 32);
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) pk += __shfl_xor(pk, sh);      // both halves < 2^32: no carry across
            tot_cand += pk & 0xFFFFFFFFull; tot_roots += pk >> 32;
        }
        RT_STAMP(3);
        // ==== PHASE 4: shade ===================================================================================================
        // ---- (e) shade: main.rs:44-56 + materials.rs ----------------------------
        bool finished = false;                                          // this lane's sample ended in this pass
        bool parked = false;                                            // CAPPED: this lane's scatter accepted none of its four tries in this pass
        D3 radiance = mk(0.0, 0.0, 0.0);
        if (alive) {
            bool done = false;
            // (the capped dense kernels: L IS radiance -- zero from the top of the pass, the sky's colour written in place -- where a second triple
            //  cost three v_mov for its zeros and three for `radiance = L`; a lane that does not finish leaves with zeros nobody reads)
            D3 L_ = mk(0.0, 0.0, 0.0);
            D3 &L = CAPPED ? radiance : L_;
            const bool is_hit = hit >= 0;
            int kind = -1;
            bool front = false;
            D3 p = o, nrm = mk(0.0, 0.0, 0.0), sp = mk(0.0, 0.0, 0.0), albedo = mk(1.0, 1.0, 1.0);
            double param = 0.0, inv_param = 0.0, r0_front = 0.0, r0_back = 0.0;
            uint32_t w_first = 0u, w_second = 0u;
            if constexpr (CAPPED) {
                // The capped dense kernels: a lane without a hit (sky) takes none of these from a constant -- sixteen v_mov for every alive lane of every
                // pass.  What reads them below, and why a lane without a hit (kind == -1) never uses what it read:
                //   p          nobody: these kernels compute the hit point in o's registers (below)
                //   nrm        reflect(d, nrm) for V: computed, then discarded unless kind == METAL; every other read is inside `else` of `!is_hit`
                //   sp         `V = sp`: selected only where kind == LAMBERTIAN; `uV + sp * param`: kind == METAL
                //   albedo     the throughput's product: inside `else` of `!is_hit`, kind != DIALECTRIC and not parked (a hit lane has the record's)
                //   param, inv_param, r0_front, r0_back, w_first (w_second: the 53-bit stream only)   the Dialectric branch, the Metal branch: kind >= 0
                // kind (-1) and front keep their definitions: they decide the paths.  A hit lane defines every one of them from the sphere's records,
                // but for sp (Lambertian, Metal: the draw) which a Dialectric lane never reads.
                p = unread_d3(); nrm = unread_d3(); sp = unread_d3(); albedo = unread_d3();
                param = unread_f64(); inv_param = unread_f64(); r0_front = unread_f64(); r0_back = unread_f64();
                w_first = unread_u32();
            }
            if (is_hit) {
                const double *mrec = mat + kMatStride * (size_t)hit;
                const double4 g = *reinterpret_cast<const double4 *>(geo + 4 * (size_t)hit);
                const double2 mA = *reinterpret_cast<const double2 *>(mrec);          // 1/r, param
                const double2 mB = *reinterpret_cast<const double2 *>(mrec + 2);      // albedo r, g
                const double2 mC = *reinterpret_cast<const double2 *>(mrec + 4);      // albedo b, kind
                // (the Dialectric's constants with the rest of the record -- one round trip, not two when the sphere turns out to be glass: -0.25 %)
                const double2 mD_ = *reinterpret_cast<const double2 *>(mrec + 6);     // 1/ir, r0(1/ir)
                const double2 mE_ = *reinterpret_cast<const double2 *>(mrec + 8);     // r0(ir), -
                // One Philox block for every lane with a hit: the first unit-sphere try of a Lambertian/Metal lane, and -- computed
                // ahead, consumed (ev++) only if the draw is really made -- the Dialectric's reflectance draw.  One wave-level call,
                // not two; and it runs HERE, between asking for the sphere's records and using them: it needs nothing from memory,
                // so its ~160 issue cycles pass under the loads' latency (-0.45 % frame time; the empty asm pins the order).
                U4 w = philox(pix_global, (uint32_t)s, ev, 0u);
                asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(w.z), "+v"(w.w));
                kind = (int)mC.y;
                param = mA.y;
                albedo = mk(mB.x, mB.y, mC.x);
                // sphere.rs:36-37 + mod.rs:20-30
                // (the capped dense kernels: the hit point is computed AFTER the tries, under the mask of the lanes that scatter, into o's own registers --
                //  it is the next ray's origin, and `o = p` at the end of the pass cost three v_mov_b64.  A parked lane keeps o and computes a hit record
                //  from it that nobody reads: it is neither shaded nor moved in this pass.)
                if constexpr (!CAPPED) {
                p = o + d * closest;                                             // ray.rs:15-17
                const D3 outward = (p - mk(g.x, g.y, g.z)) * mA.x;               // / radius = * (1/radius)
                front = dot(d, outward) < 0.0;
                nrm = front ? outward : (mk(0.0, 0.0, 0.0) - outward);
                }
                w_first = w.x;
                if constexpr (U53) w_second = w.y;
                RT_STAMP(11);
                if constexpr (U53) {
                  if (kind != RT_KIND_DIALECTRIC) {
                    // vec3.rs:37-45 with 53-bit draws: a try is SIX consecutive words -- two tries per three blocks -- and the
                    // test is the reference's own f64 expression x*x + y*y + z*z < 1.0 (vec3.rs:87-89)
                    U4 b1 = philox(pix_global, (uint32_t)s, ev + 1u, 0u);
                    uint32_t nblk = 2u, c0 = b1.z, c1 = b1.w;
                    double sx = u11_53(w.x, w.y), sy = u11_53(w.z, w.w), sz = u11_53(b1.x, b1.y);
                    bool ok = sx * sx + sy * sy + sz * sz < 1.0;
                    while (!ok) {
                        RT_COUNT_MAIN(6);
                        U4 b = philox(pix_global, (uint32_t)s, ev + nblk, 0u);
                        nblk++;
                        sx = u11_53(c0, c1); sy = u11_53(b.x, b.y); sz = u11_53(b.z, b.w);       // try 2m+1: ends its block
                        ok = sx * sx + sy * sy + sz * sz < 1.0;
                        if (!ok) {
                            b = philox(pix_global, (uint32_t)s, ev + nblk, 0u);
                            b1 = philox(pix_global, (uint32_t)s, ev + nblk + 1u, 0u);
                            nblk += 2u;
                            sx = u11_53(b.x, b.y); sy = u11_53(b.z, b.w); sz = u11_53(b1.x, b1.y); // try 2m+2 = try 0 of the next three blocks
                            c0 = b1.z; c1 = b1.w;
                            ok = sx * sx + sy * sy + sz * sz < 1.0;
                        }
                    }
                    ev += nblk;
                    sp = mk(sx, sy, sz);
                  } else {
                    inv_param = mD_.x; r0_front = mD_.y; r0_back = mE_.x;
                  }
                } else if constexpr (CAPPED) {
                  // (the Dialectric's constants are read by Dialectric lanes only, and every hit lane has loaded them: taken as loaded, not selected by kind --
                  //  six v_cndmask at the join below)
                  inv_param = mD_.x; r0_front = mD_.y; r0_back = mE_.x;
                  if (kind != RT_KIND_DIALECTRIC) {
                    // vec3.rs:37-45 with a budget of one period of the stream contract per pass: tries 0-3 use every word of the blocks
                    // ev, ev + 1, ev + 2 and leave none over.  No loop, no carried word; the two wave-level branches stay (nearly always taken).
                    uint32_t tx = w.x, ty = w.y, tz = w.z, nblk = 1u;
                    bool ok = unit_sphere_accepts(tx, ty, tz);
                    RT_COUNT_REDRAW_LANES(ok);
                    if (!ok) {
                        RT_COUNT_MAIN(6);
                        U4 b = philox(pix_global, (uint32_t)s, ev + 1u, 0u);
                        nblk = 2u;
                        tx = w.w; ty = b.x; tz = b.y;                            // try 1
                        ok = unit_sphere_accepts(tx, ty, tz);
                        if (!ok) {
                            RT_COUNT_MAIN(6);
                            const uint32_t c1 = b.z, c2 = b.w;
                            b = philox(pix_global, (uint32_t)s, ev + 2u, 0u);
                            nblk = 3u;
                            tx = c1; ty = c2; tz = b.x;                          // try 2
                            ok = unit_sphere_accepts(tx, ty, tz);
                            if (!ok) {
                                tx = b.y; ty = b.z; tz = b.w;                    // try 3: no new block
                                ok = unit_sphere_accepts(tx, ty, tz);
                            }
                        }
                    }
                    parked = !ok;                                                // (then nblk == 3: the next pass starts at "try 0 of the next three blocks")
                    ev += nblk;
                    sp = mk(u11(tx), u11(ty), u11(tz));
                  }
                  if (!parked) o = o + d * closest;                              // ray.rs:15-17: p, in place
                  // (a lambda on purpose: the same three statements written in line compile to 50 spilled scalar registers on the small-grid pair, through the
                  //  lambda to 37 -- the parent has 39; tools/kernel_resources.py is the gate for any edit here, profiles/vector_trim_ab.txt)
                  auto hit_record = [&]() {
                      const D3 outward = (o - mk(g.x, g.y, g.z)) * mA.x;         // / radius = * (1/radius)
                      front = dot(d, outward) < 0.0;
                      nrm = front ? outward : (mk(0.0, 0.0, 0.0) - outward);
                  };
                  hit_record();
                } else
                if (kind != RT_KIND_DIALECTRIC) {
                    // vec3.rs:37-45: redraw until |p|^2 < 1 -- on the integers behind the three uniforms, where the
                    // reference's f64 comparison is exact (see unit_sphere_accepts); converted once, after the loop.
                    // The tries of one scatter take consecutive words of consecutive blocks:
                    // four tries per three blocks.
                    uint32_t tx = w.x, ty = w.y, tz = w.z, nblk = 1u;
                    bool ok = unit_sphere_accepts(tx, ty, tz);
                    RT_COUNT_REDRAW_LANES(ok);                                   // (diagnostic builds: lanes that draw a unit-sphere sample / that fail try 0)
                    if (!ok) {
                        uint32_t c0 = w.w;                                       // the word left over from the block before
                        do {
                            RT_COUNT_MAIN(6);
                            U4 b = philox(pix_global, (uint32_t)s, ev + nblk, 0u);
                            nblk++;
                            tx = c0; ty = b.x; tz = b.y;                         // try 4m+1
                            ok = unit_sphere_accepts(tx, ty, tz);
                            if (!ok) {
                                const uint32_t c1 = b.z, c2 = b.w;
                                b = philox(pix_global, (uint32_t)s, ev + nblk, 0u);
                                nblk++;
                                tx = c1; ty = c2; tz = b.x;                      // try 4m+2
                                ok = unit_sphere_accepts(tx, ty, tz);
                                if (!ok) {
                                    tx = b.y; ty = b.z; tz = b.w;                // try 4m+3: no new block
                                    ok = unit_sphere_accepts(tx, ty, tz);
                                    if (!ok) {
                                        b = philox(pix_global, (uint32_t)s, ev + nblk, 0u);
                                        nblk++;
                                        tx = b.x; ty = b.y; tz = b.z; c0 = b.w;  // try 4m+4 = try 0 of the next three blocks
                                        ok = unit_sphere_accepts(tx, ty, tz);
                                    }
                                }
                            }
                        } while (!ok);
                    }
                    ev += nblk;
                    sp = mk(u11(tx), u11(ty), u11(tz));
                } else {
                    inv_param = mD_.x; r0_front = mD_.y; r0_back = mE_.x;
                }
            }
            // Every branch normalises exactly one vector (vec3.rs:107-109: v * (1/sqrt(v.v))): the
            // sky and Dialectric take unit(d), Lambertian unit(sample), Metal unit(reflect(d,n)).
            // One shared f64 sqrt + divide for the whole wave instead of one per branch.
            RT_STAMP(12);
            D3 V = d;
            if (kind == RT_KIND_LAMBERTIAN) V = sp;
            if (kind == RT_KIND_METAL) V = reflect(d, nrm);
            const D3 uV = unit_vector(V);
            if (!is_hit) {
                const double t = 0.5 * (uV.y + 1.0);                             // main.rs:54-55
                const D3 sky = mk(1.0, 1.0, 1.0) * (1.0 - t) + mk(0.5, 0.7, 1.0) * t;
                L = mk(s_thr[0][tid], s_thr[1][tid], s_thr[2][tid]) * sky;       // contract C3
                done = true;
            } else {
                // (the capped dense kernels: the materials run for the lanes that scatter only, and write the new direction into d's own registers --
                //  none of them reads d, they read uV -- where `d = ndir` cost three v_mov_b64.  A parked lane keeps d.)
                constexpr bool kDirInPlace = CAPPED;
                D3 ndir_;
                D3 &ndir = kDirInPlace ? d : ndir_;
                if (kDirInPlace && parked) {
                } else
                if (kind == RT_KIND_LAMBERTIAN) {                                // materials.rs:21-31
                    ndir = nrm + uV;
                    const double eps = 1e-8;
                    // (vec3.rs:111-114 is_near_zero: three compares, and the six selects only behind a wave-level branch that is all but never taken)
                    const bool near_zero = __builtin_fabs(ndir.x) < eps && __builtin_fabs(ndir.y) < eps && __builtin_fabs(ndir.z) < eps;
                    if (__builtin_expect(__ballot(near_zero) != 0ull, 0)) {
                        if (near_zero) ndir = nrm;
                    }
                } else if (kind == RT_KIND_METAL) {                              // materials.rs:48-62
                    ndir = uV + sp * param;
                    if (dot(ndir, nrm) <= 0.0) done = true;                      // absorbed: L = 0
                } else {                                                         // materials.rs:76-105
                    // 1.0/ir and ((1-ri)/(1+ri))^2 for both ratios are per-sphere constants: the same
                    // f64 operations, done once on the host (rt_api.hip)
                    const double ratio = front ? inv_param : param;
                    const double cos_theta = min_1(-dot(uV, nrm));
                    const double sin_theta = __builtin_sqrt(1.0 - cos_theta * cos_theta);
                    bool do_refract = false;
                    if (ratio * sin_theta <= 1.0) {                              // && short-circuit
                        const double r0 = front ? r0_front : r0_back;            // materials.rs:79
                        const double x = 1.0 - cos_theta;
                        const double x2 = x * x;
                        const double refl = r0 + (1.0 - r0) * ((x2 * x2) * x);   // materials.rs:80
                        ev++;                                                    // the block drawn above
                        do_refract = refl <= (U53 ? u01_53(w_first, w_second) : u01(w_first));
                    }
                    ndir = do_refract ? refract(uV, nrm, ratio) : reflect(uV, nrm);
                }
                if constexpr (CAPPED) {
                    // a parked lane (Lambertian or Metal) has not scattered: ray, depth and throughput stay, and it is neither done nor finished
                    if (parked) done = false;
                    else {
                        if (kind != RT_KIND_DIALECTRIC) {
                            s_thr[0][tid] = s_thr[0][tid] * albedo.x;
                            s_thr[1][tid] = s_thr[1][tid] * albedo.y;
                            s_thr[2][tid] = s_thr[2][tid] * albedo.z;
                        }
                        // (o and d hold the next ray already: the hit point and the materials above)
                        depth -= 1;
                        if (depth <= 0) done = true;
                    }
                } else {
                if (kind != RT_KIND_DIALECTRIC) {                                // Dialectric: (1,1,1), x * 1.0 == x
                    s_thr[0][tid] = s_thr[0][tid] * albedo.x;
                    s_thr[1][tid] = s_thr[1][tid] * albedo.y;
                    s_thr[2][tid] = s_thr[2][tid] * albedo.z;
                }
                o = p;
                d = ndir;
                depth -= 1;
                if (depth <= 0) done = true;                                    // main.rs:40-42: L = 0
                }
            }
            if (done) {
                alive = false;
                finished = true;
                radiance = L;
            }
        }
        if constexpr (CAPPED) {
            // the parked lanes' rays were counted at the top of this pass and will be counted again in the next one: scalar work only
            const uint32_t n_parked = (uint32_t)__popcll(__ballot(parked));
            RT_COUNT_CAPPED_PARKS(n_parked);
            n_rays -= n_parked;
        }
        RT_STAMP(13);
        __builtin_amdgcn_s_setprio(1);
        // ==== PHASE 5: accumulate_finished =====================================================================================
        // ---- (f) finished samples -> their block's sums (LDS) or, without a ring entry, the frame buffer ----
        {
            // age of this lane's block among the wave's blocks (0 = the current one); blocks of age >= kRingDepth have
            // lost their ring entry (sequence numbers compare modulo 2^28: the ring is 4 deep)
            const uint32_t age = (blk_seq - (my_blk >> 4)) & 0x0FFFFFFFu;
            const bool direct = finished && !(P.use_ring && age < (uint32_t)kRingDepth);
            const bool ringed = finished && !direct;
            // (the capped dense kernels: `finished` comes out of the shading's joins as a bool, and every vote on it or on a bool made from it costs a
            //  select and a compare to rebuild the lane mask.  One vote on it; the others are votes on compares, combined as wave masks.)
            const unsigned long long fin_m = kMaskVotes ? __ballot(finished) : 0ull;
            const unsigned long long ring_m = kMaskVotes && P.use_ring ? __ballot(age < (uint32_t)kRingDepth) : 0ull;
            RT_LDS_RING_ADDS(ringed, my_blk);
            if (finished) {
                const unsigned long long q0 = quantize(radiance.x), q1 = quantize(radiance.y), q2 = quantize(radiance.z);
                if (ringed) {
                    unsigned long long *acc = ring_w + ((my_blk >> 4) & (uint32_t)(kRingDepth - 1)) * (kRingSlots * 3) + (my_blk & 15u) * 3u;
                    atomicAdd(acc + 0, q0); atomicAdd(acc + 1, q1); atomicAdd(acc + 2, q2);
                } else {                                            // too few samples per pixel for block sums, or an orphan of a long-gone block
                    unsigned long long *px = P.fix + (size_t)(kStriped ? pix_local - (my_blk & P.stripe_mask) : pix_local) * 3u;
                    atomicAdd(px + 0, q0); atomicAdd(px + 1, q1); atomicAdd(px + 2, q2);
                }
            }
            n_direct += (uint32_t)__popcll(kMaskVotes ? fin_m & ~ring_m : __ballot(direct));
            unsigned long long fm = kMaskVotes ? fin_m & ring_m : __ballot(ringed);
            if constexpr (kMaskVotes) n_samples += (uint32_t)__popcll(fin_m);
            if constexpr (kMaskVotes) {
                if (fm != 0ull) {
                    // (as below for a ring of two; a block's count changes only where its mask is not empty, so each test is one scalar compare and branch)
                    __builtin_amdgcn_wave_barrier();
                    const unsigned long long m0 = fm & __ballot(age == 0u);
                    if (m0 != 0ull) {
                        rem0 -= (uint32_t)__popcll(m0);
                        if (rem0 == 0u) flush_ring(blk_seq & 1u);
                    }
                    fm &= ~m0;
                    if (fm != 0ull) {
                        rem1 -= (uint32_t)__popcll(fm);
                        if (rem1 == 0u) flush_ring((blk_seq - 1u) & 1u);
                    }
                }
            } else
            if (fm != 0ull) {
                // count the finished samples per block (nearly always the current and the previous one), and write
                // out the blocks that have just received their last sample (LDS operations of a wave execute in
                // program order: the adds above are in the sums flush_ring reads)
                __builtin_amdgcn_wave_barrier();
                const unsigned long long m0 = __ballot(ringed && age == 0u);
                rem0 -= (uint32_t)__popcll(m0);
                if (m0 != 0ull && rem0 == 0u) flush_ring(blk_seq & (uint32_t)(kRingDepth - 1));
                fm &= ~m0;
                if constexpr (kRingDepth == 2) {
                    if (fm != 0ull) {                               // (the rest finished in the block before)
                        rem1 -= (uint32_t)__popcll(fm);
                        if (rem1 == 0u) flush_ring((blk_seq - 1u) & 1u);
                    }
                } else
                if (fm != 0ull) {
                    const unsigned long long m1 = __ballot(ringed && age == 1u);
                    rem1 -= (uint32_t)__popcll(m1);
                    if (m1 != 0ull && rem1 == 0u) flush_ring((blk_seq - 1u) & 3u);
                    fm &= ~m1;
                    if (fm != 0ull) {
                        const unsigned long long m2 = __ballot(ringed && age == 2u);
                        rem2 -= (uint32_t)__popcll(m2);
                        if (m2 != 0ull && rem2 == 0u) flush_ring((blk_seq - 2u) & 3u);
                        fm &= ~m2;
                        if (fm != 0ull) {
                            rem3 -= (uint32_t)__popcll(fm);
                            if (rem3 == 0u) flush_ring((blk_seq - 3u) & 3u);
                        }
                    }
                }
            }
        }
        if constexpr (!kMaskVotes) n_samples += (uint32_t)__popcll(__ballot(finished));
        RT_STAMP(4);
    }
    // every block of this wave has finished its last sample and has been written out; a ring entry that
    // still holds something here would be a bookkeeping error -- its sums go out rather than get lost
    if (rem0 != 0u) flush_ring(blk_seq & (uint32_t)(kRingDepth - 1));
    if (rem1 != 0u) flush_ring((blk_seq - 1u) & (uint32_t)(kRingDepth - 1));
    if constexpr (kRingDepth == 4) {
        if (rem2 != 0u) flush_ring((blk_seq - 2u) & 3u);
        if (rem3 != 0u) flush_ring((blk_seq - 3u) & 3u);
    }

        // (end of the bounce loop body is stamped at the top of the next iteration as phase 4)
    // wave totals -> device counters
    RT_DIAG_FLUSH();
    {
        const unsigned long long nc = tot_cand, nr = tot_roots;
        if (DIAG) {
            const unsigned int nl = s_live[tid >> 6][lane];
            if (nl) atomicAdd(P.stats + 16 + lane, (unsigned long long)nl);
        }
        if (lane == 0) {
            atomicAdd(P.stats + 0, (unsigned long long)n_rays);
            atomicAdd(P.stats + 1, (unsigned long long)n_samples);
            if (n_direct) atomicAdd(P.stats + 4, (unsigned long long)n_direct);
            atomicAdd(P.stats + 2, nc);
            atomicAdd(P.stats + 3, nr);
        }
    }
}

} // namespace rt
