/*
 * rtiow_hip.h -- C ABI of librtiow_hip.so, the MI355X (gfx950) replacement for
 * the per-pixel Monte-Carlo loop of Druthyn/rtiow.
 *
 * What it replaces.  The reference has no FFI or plugin seam: the path is the
 * inlined iterator expression at src/main.rs:122-139 and everything it calls
 * (ray_color main.rs:38-57, HittableList::hit shapes/mod.rs:54-70, Sphere::hit
 * shapes/sphere.rs:15-41, {Lambertian,Metal,Dialectric}::scatter
 * materials.rs:21-31,48-62,76-105, Camera::get_ray camera.rs:47-54 and
 * Color::to_rgba vec3.rs:403-421).  Each entry point below names the reference
 * lines it stands in for; INTEGRATION.md shows the Rust `extern "C"` block and
 * the edit to main.rs that binds them.
 *
 * Rules of the boundary
 *   - plain C types, plain pointers and sizes; no C++/torch types;
 *   - every function returns 0 on success or a negative rt_status; it never
 *     aborts or throws across the ABI (the reference unwrap()s, main.rs:147,177);
 *     rt_last_error() gives the thread-local message of the last failure;
 *   - the caller owns every buffer it passes; the library owns the device
 *     memory tied to an rt_context;
 *   - a context is used from one host thread at a time; it may have TWO
 *     renders in flight (rt_render_device on two different streams: the work
 *     counter, statistics words and events exist twice and are used in turn --
 *     see rt_render_device); distinct contexts (one per GPU) may be used
 *     concurrently;
 *   - there is NO CPU fallback: without a usable gfx950 device rt_create fails.
 *
 * Arithmetic.  Results are those of the reference's own f64 arithmetic: every
 * value that decides or shades a path is computed in IEEE binary64 in the
 * reference's operation order (no fused multiply-add), so a render equals the
 * literal CPU restatement (oracle/oracle_f64.c, Oracle B) bit for bit.  f32
 * is used only as a CONSERVATIVE FILTER in the sphere scan (it may send a
 * sphere to the exact f64 test needlessly, never the reverse; DESIGN.md
 * section 5.2).  A pixel's sum over samples is exact: every sample's radiance
 * is truncated to a 2^-32 grid and summed in an unsigned 64-bit integer, so
 * the result does not depend on how samples are sharded over lanes, launches,
 * passes or GPUs.
 */
#ifndef RTIOW_HIP_H
#define RTIOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTIOW_HIP_ABI_VERSION 5

typedef struct rt_context rt_context;

typedef enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1,
    RT_ERR_NO_DEVICE = -2,       /* no HIP device / not gfx950 */
    RT_ERR_HIP = -3,             /* a HIP runtime call failed  */
    RT_ERR_NO_SCENE = -4,        /* render before rt_upload_scene */
    RT_ERR_OUT_OF_MEMORY = -5
} rt_status;

/* Material kinds: the three `impl Scatter` of materials.rs. */
enum { RT_LAMBERTIAN = 0, RT_METAL = 1, RT_DIALECTRIC = 2 };

/* One sphere, flattened, in the reference's own f64.  The reference keeps
 * Sphere{center,radius,mat} (shapes/sphere.rs:9-13) and the material structs
 * (materials.rs:9-11,34-37,64-66) private behind Box<dyn Hit>/Arc<dyn Scatter>,
 * so the host flattens each object where it is pushed (main.rs:64,87,93-99).
 * LIST ORDER IS PART OF THE INPUT: on equal t the later sphere wins
 * (mod.rs:61-67, sphere.rs:29). */
typedef struct {
    double center[3];
    double radius;
    double albedo[3];    /* Lambertian, Metal                        */
    double param;        /* Metal: fuzz; Dialectric: ir              */
    int32_t kind;        /* RT_LAMBERTIAN / RT_METAL / RT_DIALECTRIC */
    int32_t reserved;    /* 0                                        */
} rt_sphere;             /* 72 bytes */

/* Camera (camera.rs:4-13) minus `w`, which get_ray never reads; f64 as in the
 * reference.  The host computes it with its Camera::new (camera.rs:17-45). */
typedef struct {
    double origin[3];
    double lower_left_corner[3];
    double horizontal[3];
    double vertical[3];
    double u[3];
    double v[3];
    double lens_radius;
} rt_camera;             /* 152 bytes */

/* What main.rs:24-28,44 fixes at compile time, plus sharding.
 *
 * Rows: j = 0 is the BOTTOM image row, as in main.rs:122-132.  The image is
 * cut into row tiles of `tile_rows` rows; a call renders the tiles t with
 * t % shard_count == shard_index, and its output holds those rows only,
 * ascending j ("compact rows"; rt_shard_rows() gives how many).
 * shard_count = 1 renders the whole image. */
typedef struct {
    int32_t width, height;       /* main.rs:25-26 (>= 2: u,v divide by W-1,H-1)   */
    int32_t spp;                 /* samples per pixel rendered by this call :27    */
    int32_t sample_begin;        /* index of the first sample (additive passes)    */
    int32_t max_depth;           /* :28, 50                                        */
    double  t_min;               /* :44, 1e-4; must be > 0                         */
    uint64_t seed;               /* Philox key                                     */
    int32_t tile_rows;           /* >= 1                                           */
    int32_t shard_index;         /* 0 <= shard_index < shard_count                 */
    int32_t shard_count;         /* >= 1                                           */
    uint32_t flags;              /* RT_FLAG_*                                      */
} rt_params;

#define RT_FLAG_ACCUMULATE 0x1u  /* rt_render_device: add to d_fix instead of overwriting it */
#define RT_FLAG_NO_FILTER  0x2u  /* validation: send EVERY sphere to the exact f64 test     */
#define RT_FLAG_DIAG_STATS 0x4u  /* also fill rt_stats.candidates / exact_roots / live_per_bounce (~15 % slower) */
#define RT_FLAG_UNIFORM53  0x8u  /* every uniform from TWO Philox words, u = ((w0 << 32 | w1) >> 11) * 2^-53: the 53 random bits of
                                    rand's gen::<f64>() (main.rs:131-132, vec3.rs:31-33,63, materials.rs:96) instead of one word's 32
                                    (the default: u = w * 2^-32, symmetric ranges (int32_t)w * 2^-31; ABI <= 4: 24 bits); same draw
                                    order; another (equally valid) random stream, so frames differ from the default's; scan mode 5 or
                                    RT_FLAG_NO_FILTER, not with RT_FLAG_DIAG_STATS */
#define RT_FLAG_OVERLAPPED 0x10u /* rt_render_device: this launch is one of a sequence of passes that OVERLAP on two streams (below): the next
                                    pass fills its end-of-launch tail, so it takes the work blocks of 1 024 pixel-samples whatever its size
                                    (alone, a launch of < 2 x 10^8 pixel-samples is up to 6 % slower on them: its last blocks are its tail).
                                    The same frame either way; 2 x 250 spp at 1200x675: 1.045 -> 1.012 x one 500-spp launch */
#define RT_FLAG_KNOWN      0x1fu /* every other bit of rt_params.flags is an error (RT_ERR_INVALID_ARGUMENT), not ignored */

typedef struct {
    uint64_t samples;            /* pixel-samples finished                          */
    uint64_t rays_traced;        /* HittableList::hit calls (mod.rs:56)             */
    uint64_t sphere_tests;       /* rays_traced * n_spheres (sphere.rs:16 calls)    */
    uint64_t candidates;         /* tests the filter passed on to the f64 test (RT_FLAG_DIAG_STATS, else 0) */
    uint64_t exact_roots;        /* f64 tests that reached the sqrt, sphere.rs:26   (RT_FLAG_DIAG_STATS, else 0) */
    float    kernel_ms;          /* render kernel, HIP events on its stream         */
    int32_t  n_spheres;
    int32_t  grid_blocks, block_threads;
    int32_t  scan_mode;          /* sphere-scan filter that ran: 0 none (RT_FLAG_NO_FILTER), 5 tube filter (shipped),
                                    1 VALU cross-check (RTIOW_SCAN_MODE=1); 2-4 only in RTIOW_CROSSCHECK_MODES builds */
    int32_t  kernel_variant;     /* which instantiation of the kernel ran, as bits: 1 the scan_mode-5 kernel for scenes whose
                                    tile grid has <= 64 cells (else the general one, and every other scan mode); 2 the
                                    RT_FLAG_UNIFORM53 instantiation; 4 work blocks of 1 024 pixel-samples instead of 256 (launches of
                                    >= 2 x 10^8 pixel-samples at >= 147 samples per pixel; >= 69 on the small-grid kernel); 8 the
                                    pixel-list variant (rt_render_pixels_device); 16 the frame-batch variant
                                    (rt_render_frames_device) */
    uint64_t live_per_bounce[64]; /* rays traced at bounce index k (0 = camera ray; indices >= 63 share the
                                    last slot); sums to rays_traced (RT_FLAG_DIAG_STATS, else 0) */
    uint64_t direct_samples;     /* samples added to the frame buffer one by one instead of through their block's
                                    sums: all of them in a launch of < 5 spp (< 9 with RT_FLAG_NO_FILTER / RT_FLAG_DIAG_STATS), else only the last samples of blocks
                                    that a long path held open for too long (more than ~30 bounces at >= 37 spp, ~15 on the small-grid
                                    kernel; a few bounces on the 64-sample work blocks of launches with < 13 spp) */
} rt_stats;

/* ---- diagnostic knobs (environment; none changes a result) -------------------
 * Read by the library, for tests and measurements only -- every one of them selects another way of computing the
 * SAME frame (the parity tests run the knobs against the oracle):
 *   RTIOW_SCAN_MODE=1|5            rt_create: the sphere-scan filter (5 tube filter on the matrix pipe, shipped; 1 VALU cross-check)
 *   RTIOW_NO_GRID=1, RTIOW_GRID_DIM=G   rt_upload_scene: no tile grid / G x G cells instead of the cost model's choice
 *   RTIOW_BLOCKS_PER_CU=k          rt_create: workgroups per CU of the persistent grid (default: the occupancy query)
 *   RTIOW_RING_MIN_SPP=n           rt_create: no per-block pixel sums in LDS below n samples per pixel (default: wherever a block's pixels fit the sums' slots,
 *                                  i.e. from 5 samples per pixel on; 9 with RT_FLAG_NO_FILTER / RT_FLAG_DIAG_STATS)
 *   RTIOW_LARGE_BLOCK_MIN_ITEMS=n  per launch: work blocks of 1 024 pixel-samples instead of 256 from n pixel-samples per launch on
 *                                  (default 2 x 10^8; also needs >= 147 samples per pixel, 69 on the small-grid kernel; rt_stats.kernel_variant bit 2 says which ran)
 *   RTIOW_DENSE_BODY=classic|capped   per launch: rt_render_device's shipped kernel (scan mode 5 without RT_FLAG_DIAG_STATS / RT_FLAG_UNIFORM53) with the unbounded
 *                                  unit-sphere redraw loop (classic) or with at most four tries per scatter and pass, a lane without an accepted try keeping its
 *                                  ray for the next pass (capped); default: per kernel, whichever measured faster.  kernel_variant is the same either way;
 *                                  rt_last_dense_body (rtiow_hip_diag.h) says which ran */

/* ---- lifetime -------------------------------------------------------------- */

/* Opens HIP device `device_id`.  Fails with RT_ERR_NO_DEVICE when there is no
 * HIP device or it is not gfx950 -- there is no fallback path. */
int rt_create(int32_t device_id, rt_context **out);
int rt_destroy(rt_context *ctx);

/* ---- scene: stands in for `&world` captured at main.rs:135 ----------------- */
/* The reference's list is a Vec<Box<dyn Hit>> of any length (shapes/mod.rs:52).  Here n <= RT_MAX_SPHERES: the
 * kernel numbers the columns of its filter table in 26 bits.  (Rounds 1-3 stopped at 65 535: 16-bit candidate numbers.)
 * A performance cliff sits far below the limit: the tile grid has at most 63 x 63 cells of 32 columns (+ 48 tiles every ray
 * scans), i.e. ~128 K columns; a scene that needs more -- upwards of ~130 000 filtered spheres -- gets NO grid, every wave
 * then scans all n/32 tiles per bounce (O(n) per ray, still exact: tests/test_limits.py renders 70 227 spheres both ways).
 * Coordinates and radii must be finite and below 1e15 in magnitude, radii non-zero, kinds RT_LAMBERTIAN / RT_METAL /
 * RT_DIALECTRIC. */
#define RT_MAX_SPHERES (1 << 24)
int rt_upload_scene(rt_context *ctx, const rt_sphere *spheres, int32_t n);

/* Rows owned by (shard_index, shard_count, tile_rows) of an image `height`
 * rows tall; and the image row j of compact row r. */
int rt_shard_rows(const rt_params *p, int32_t *out_rows);
int rt_shard_row_index(const rt_params *p, int32_t compact_row, int32_t *out_j);

/* ---- the hot path: main.rs:122-139 up to (not including) to_rgba ----------- */

/* The exact sums and their range (contract C5).  The reference adds every sample's colour into an f64 per pixel
 * (main.rs:127,135), unbounded.  Here one channel of one sample enters the pixel's sum as
 *     q = floor(min(x, RT_SAMPLE_CLAMP) * 2^32)   (0 for a NaN or a negative x)
 * and the sums are u64: exact, associative, identical however the samples are spread over lanes, launches or GPUs.
 * With q <= 2^48 a sum CANNOT wrap while a pixel has received FEWER THAN 65 536 samples (at most 65 535: all launches
 * that accumulate into the same buffer together; 65 536 saturated samples would sum to exactly 2^64), whatever the scene;
 * and within that limit the clamp cannot change a byte of
 * Color::to_rgba: a clamped sample alone puts the pixel's mean at >= 1, i.e. at byte 255, where the reference's
 * unbounded sum puts it too.  From 65 536 samples per pixel on the sums stay exact while the pixel's mean radiance is
 * below 2^32 / samples; a scene whose albedos are <= 1 (every scene of the reference) has x <= 1 and no limit below
 * 2^32 samples.  (Rounds 1-3 clamped at 2^30: four saturated samples wrapped a sum.) */
#define RT_SAMPLE_CLAMP 65536.0

/* Host-buffer form.  out_sum: [rows][width][3] f32 radiance SUMS over the spp
 * samples (divide by spp for the mean), rows = rt_shard_rows().  out_fix
 * (optional, may be NULL): the exact sums, u64 with quantum 2^-32.
 * Synchronous. */
int rt_render(rt_context *ctx, const rt_camera *cam, const rt_params *p,
              float *out_sum, uint64_t *out_fix, rt_stats *stats);

/* Device-buffer form, asynchronous on `stream` (a hipStream_t, or NULL for the
 * default stream).  d_fix: device pointer to [rows][width][3] u64.
 * Progressive passes (main.rs:130-137 split over launches with sample_begin and RT_FLAG_ACCUMULATE): the sums are exact
 * integers added with atomics, so passes may OVERLAP -- issue pass k + 1 on another stream than pass k (and say so: RT_FLAG_OVERLAPPED) and it fills the tail
 * of pass k (the last paths of a launch leave most of the chip idle: 5 % of a 100-spp launch at 1200x675).  A context holds
 * the per-launch state of two launches; a third launch makes ITS stream wait for the one before the previous (no host wait).
 * The caller orders what must be ordered: the buffer is zeroed (by a launch without RT_FLAG_ACCUMULATE, or by the caller)
 * before any other stream adds to it, and it is read after every stream that adds to it has been waited for.
 * rt_last_stats reports on the latest launch only. */
int rt_render_device(rt_context *ctx, const rt_camera *cam, const rt_params *p,
                     void *d_fix, void *stream);

/* Exact sums -> f32 sums, on the device (count = rows*width*3 values). */
int rt_fix_to_f32_device(rt_context *ctx, const void *d_fix, int64_t count,
                         void *d_out_f32, void *stream);

/* Waits for the context's last launch and returns its counters and time. */
int rt_last_stats(rt_context *ctx, rt_stats *stats);

/* ---- Color::to_rgba (vec3.rs:403-421) + the row flip (main.rs:141-145) ----- */

/* d_fix: device [rows][width][3] exact sums; d_rgba: device [rows][width][4]
 * u8.  spp = total samples in the sums.  Each channel is (f64)q * 2^-32 put
 * through vec3.rs:403-421 in f64.  flip != 0 writes row r at rows-1-r, which
 * for a whole image is the top-to-bottom order main.rs:141-145 produces. */
int rt_resolve_rgba8_device(rt_context *ctx, const void *d_fix, int32_t width, int32_t rows,
                            int64_t spp, int32_t flip, void *d_rgba, void *stream);
/* Host-buffer form (copies in, resolves on the device, copies out). */
int rt_resolve_rgba8(rt_context *ctx, const uint64_t *fix, int32_t width, int32_t rows,
                     int64_t spp, int32_t flip, uint8_t *out_rgba);

/* ---- the whole of main.rs:122-145 in ONE call ------------------------------- */

/* Renders (main.rs:122-136), keeps the exact sums ON THE DEVICE, puts them through Color::to_rgba with
 * p->spp samples (main.rs:137, vec3.rs:403-421) and the row flip (main.rs:141-145, flip != 0), and copies the
 * bytes out: out_rgba is [rows][width][4] u8, rows = rt_shard_rows() -- exactly the Vec<u8> that
 * ImageBuffer::from_vec takes at main.rs:147.  4 bytes per pixel cross PCIe, once (rt_render + rt_resolve_rgba8
 * move the 24-byte sums out and back in first).  Same bytes as that pair of calls.  Starts from zero
 * (RT_FLAG_ACCUMULATE is ignored, as in rt_render); synchronous.  stats may be NULL. */
int rt_render_rgba8(rt_context *ctx, const rt_camera *cam, const rt_params *p, int32_t flip,
                    uint8_t *out_rgba, rt_stats *stats);

/* ---- pixel lists: main.rs:122-139 for SOME pixels of the frame ------------- */

/* Renders p->spp samples of the n_pixels listed pixels of the p->width x p->height frame (crop windows, masks, re-rendering a
 * region, picking; the passes of rt_render_adaptive).  d_pixels: device [n_pixels] u32 global pixel numbers g = j * width + i
 * (j = 0 the BOTTOM row, as everywhere), each < width * height, in any order, duplicates allowed.  d_fix: device
 * [n_pixels][3] u64 exact sums, COMPACT: entry k belongs to d_pixels[k].
 * Sample s of listed pixel g is exactly the sample a dense render gives that pixel -- the body of main.rs:130-136 with
 * Philox key (g, sample_begin + s) and u, v (main.rs:131-132) from the pixel's own (i, j) over the FULL frame's width - 1,
 * height - 1 --, so entry k equals the dense render's sums at (j, i): a list is still ONE Oracle-B render of those samples.
 * Honours spp, sample_begin, max_depth, t_min, seed and RT_FLAG_ACCUMULATE (which adds to d_fix -- not with duplicates in flight
 * on two streams unless d_fix was zeroed first, as for rt_render_device); RT_FLAG_OVERLAPPED is accepted and ignored.
 * Runs the shipped kernel's pixel-list variant only: RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS, RT_FLAG_NO_FILTER, a context created
 * under RTIOW_SCAN_MODE=1 and shard_count != 1 are RT_ERR_INVALID_ARGUMENT, found before anything is touched (tile_rows and
 * shard_index are unused).  n_pixels == 0 succeeds and does nothing.  Asynchronous on `stream`; shares the context's two
 * per-launch slots with rt_render_device, and rt_last_stats reports on it (samples = n_pixels * spp).  Lists in ascending
 * order keep a wave's 64 camera rays on neighbouring pixels, which the tile grid relies on for speed (not for correctness). */
int rt_render_pixels_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const uint32_t *d_pixels,
                            int64_t n_pixels, void *d_fix, void *stream);
/* Host-buffer form, synchronous, starts from zero (RT_FLAG_ACCUMULATE is ignored); a listed number >= width * height is
 * RT_ERR_INVALID_ARGUMENT.  stats may be NULL. */
int rt_render_pixels(rt_context *ctx, const rt_camera *cam, const rt_params *p, const uint32_t *pixels, int64_t n_pixels,
                     uint64_t *out_fix, rt_stats *stats);

/* ---- adaptive sampling: main.rs:130-137 with a per-pixel number of samples -- */

/* The reference gives every pixel samples_per_pixel samples (main.rs:27,130).  Here a pixel stops when its error estimate
 * is small.  State per frame: fix [H][W][3] u64 (all samples), half [H][W][3] u64 (the samples of the EVEN-numbered passes
 * only), count [H][W] u32 (samples in fix).  Pass k renders samples [k step, (k + 1) step) of the pixels active in its
 * round; a round is two passes, so half always holds exactly count / 2 samples.  After a round that brought the active
 * pixels to n samples, for every pixel with count == n (a "candidate"):
 *     d_c  = | 2 half_c - fix_c |                       exact integers, c = r, g, b
 *     D    = ((double)d_r + (double)d_g) + (double)d_b
 *     S    = ((double)fix_r + (double)fix_g) + (double)fix_b
 *     sc   = 1.0 / ((double)n * 4294967296.0)
 *     err  = (D * sc) / sqrt(max(S * sc, dark_floor))
 *     noisy = candidate && !(err <= threshold)
 *     active_next = candidate && (a pixel of the 3x3 neighbourhood, clipped at the frame's edges, is noisy)
 * in IEEE binary64, this operation order, no fused multiply-add.  D sc is the mean absolute difference of the two half
 * means (an estimate of the standard error of the pixel's mean); the denominator makes it relative for bright pixels.
 * A pixel that leaves the active set never returns. */
typedef struct {
    int32_t step;                /* samples per pass, >= 1                           */
    int32_t reserved;            /* 0                                                */
    double  threshold;           /* >= 0; 0: every pixel goes on to the cap          */
    double  dark_floor;          /* > 0: the least mean radiance (r + g + b) the error is taken relative to */
} rt_adaptive;                   /* 24 bytes */

/* The selection on device buffers, asynchronous on `stream`.  d_fix, d_half: [height][width][3] u64; d_count:
 * [height][width] u32; n: even, 2 <= n <= 32766.  d_list_out: capacity width * height u32, receives the active pixels'
 * numbers g in ASCENDING order (the same list on every run: an ordered compaction, no atomics); d_n_out: one u32, their number. */
int rt_select_pixels_device(rt_context *ctx, const void *d_fix, const void *d_half, const void *d_count, int32_t width,
                            int32_t height, int32_t n, const rt_adaptive *a, void *d_list_out, void *d_n_out, void *stream);
/* The same selection on host buffers, no device needed: the library's own CPU statement of the rule. */
int rt_select_pixels_host(const uint64_t *fix, const uint64_t *half, const uint32_t *count, int32_t width, int32_t height,
                          int32_t n, const rt_adaptive *a, uint32_t *list_out, int64_t *n_out);

/* The loop.  p->spp = the MOST samples a pixel may get: a multiple of 2 * step and <= 32766 (so that n * 2^48 < 2^63 and the
 * differences above fit a signed 64-bit integer whatever the scene); p->sample_begin == 0; shard_count == 1; the flags
 * rt_render_pixels_device rejects are rejected.  Round 1 renders every pixel (2 passes of `step`); then select, render the
 * list, add back, until the list is empty or count == p->spp.  Everything stays on the device between passes; per round the
 * host reads back one word (the list's length).  out_fix, out_half: [height][width][3] u64 (out_half may be NULL);
 * out_count: [height][width] u32.  stats (may be NULL): samples and rays_traced summed over the passes (samples ==
 * the sum of out_count), kernel_ms the sum of the render kernels, the launch shape of the last pass.  Synchronous. */
int rt_render_adaptive(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_adaptive *a,
                       uint64_t *out_fix, uint64_t *out_half, uint32_t *out_count, rt_stats *stats);

/* Color::to_rgba with each pixel's OWN sample count (vec3.rs:403-421 with samples_per_pixel = count[p]) + the row flip
 * (main.rs:141-145): the resolve of an adaptive frame.  d_count: device [rows][width] u32, every entry >= 1. */
int rt_resolve_rgba8_counts_device(rt_context *ctx, const void *d_fix, const void *d_count, int32_t width, int32_t rows,
                                   int32_t flip, void *d_rgba, void *stream);
/* Host-buffer form (copies in, resolves on the device, copies out). */
int rt_resolve_rgba8_counts(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int32_t width, int32_t rows,
                            int32_t flip, uint8_t *out_rgba);

/* ---- frame batches: main.rs:108-145 once per camera, in ONE launch ---------- */

/* A batch is n_frames cameras over the uploaded scene -- a turntable, a fly-through, a stereo pair, a contact sheet of
 * viewpoints -- with the same rt_params (width, height, spp, max_depth, t_min, seed) and a sample_stride >= 0:
 *     frame f equals, bit for bit, the dense render of cams[f] with sample_begin' = p->sample_begin + f * sample_stride
 * -- the exact sums rt_render gives for that camera and those parameters.  The Philox key stays p->seed and the counter stays
 * (pixel g = j * width + i of the frame's OWN image, sample index, event, 0): the frame number enters nothing but the sample
 * index.  sample_stride = 0 gives every frame the same random numbers (common random numbers: stereo pairs, differences
 * between viewpoints); sample_stride >= the samples a pixel gets in all gives every frame a stream of its own (no
 * fixed-pattern noise across an animation).  Why one launch: a launch ends when the longest path among its last samples does
 * (~650 us for a 50-bounce path whatever the frame size), so a sequence of small frames rendered one launch each is mostly
 * tails; the persistent grid does not care which frame a work block belongs to, and a batch has ONE tail.
 *
 * Device form (stands in for main.rs:108-139, once per camera).  d_cams: DEVICE [n_frames] rt_camera, alive until the launch
 * has finished (as d_pixels of rt_render_pixels_device).  d_fix: device [n_frames][height][width][3] u64, frame after frame,
 * rows as rt_render_device's with shard_count 1.  Honours spp, sample_begin, max_depth, t_min, seed and RT_FLAG_ACCUMULATE;
 * RT_FLAG_OVERLAPPED is accepted and ignored; tile_rows and shard_index are unused.  Runs the shipped kernel's frame-batch
 * variant only.  RT_ERR_INVALID_ARGUMENT, found before anything is touched (no buffer zeroed, no launch slot taken,
 * rt_last_stats unchanged): RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS, RT_FLAG_NO_FILTER, unknown flag bits, a context created
 * under RTIOW_SCAN_MODE=1, shard_count != 1, n_frames < 0, sample_stride < 0, n_frames * width * height > 2^31,
 * sample_begin + (n_frames - 1) * sample_stride + spp > 2^31 - 1, more than 2^31 - 1 work blocks (a frame has
 * ceil(width * height * spp / 256) of them; blocks of 192 / 128 / 64 pixel-samples below 17 / 13 / 9 samples per pixel), NULL
 * pointers with n_frames > 0; RT_ERR_NO_SCENE before an upload.  n_frames == 0 succeeds and does nothing; max_depth == 0 gives
 * black frames without a launch, as rt_render_device does.  Asynchronous on `stream`; shares the context's two per-launch slots
 * with rt_render_device and rt_render_pixels_device, and rt_last_stats reports on it: samples = n_frames * width * height * spp,
 * rays_traced = the sum over the frames, scan_mode 5, kernel_variant bit 16. */
int rt_render_frames_device(rt_context *ctx, const rt_camera *d_cams, int32_t n_frames, int32_t sample_stride,
                            const rt_params *p, void *d_fix, void *stream);
/* Host-buffer form: host cameras, host sums out_fix [n_frames][height][width][3]; synchronous; starts from zero
 * (RT_FLAG_ACCUMULATE is ignored); stats may be NULL. */
int rt_render_frames(rt_context *ctx, const rt_camera *cams, int32_t n_frames, int32_t sample_stride,
                     const rt_params *p, uint64_t *out_fix, rt_stats *stats);
/* ... + Color::to_rgba with p->spp samples (main.rs:137, vec3.rs:403-421) and the row flip (main.rs:141-145, flip != 0) PER
 * FRAME: out_rgba is [n_frames][height][width][4] u8, frame f holds exactly the bytes rt_render_rgba8 gives for cams[f] and
 * sample_begin + f * sample_stride; the sums never leave the device.  Needs spp >= 1.  Synchronous; stats may be NULL. */
int rt_render_frames_rgba8(rt_context *ctx, const rt_camera *cams, int32_t n_frames, int32_t sample_stride,
                           const rt_params *p, int32_t flip, uint8_t *out_rgba, rt_stats *stats);

/* ---- feature buffers: what the FIRST hit of every camera ray shows ----------- */

/* Denoiser guides (first-hit albedo, normal, depth), alpha / coverage and an object id, from a kernel of its own that traces
 * bounce 0 of ray_color only (main.rs:131-134 + HittableList::hit, mod.rs:54-70) and keeps the hit record.  DESIGN.md section 14.
 *
 * The camera ray of pixel g = j * width + i (j = 0 the BOTTOM row) and sample index s in [sample_begin, sample_begin + spp) is the
 * one the dense render traces for (g, s): Philox key `seed`, counter (g, s, block, 0); words 0, 1 of block 0 are the u01 draws of
 * u = (i + e0) / (width - 1), v = (j + e1) / (height - 1); words 2, 3 the first random_in_unit_disk try (symmetric draws); every retry
 * takes the next two consecutive words, on into blocks 1, 2, ...; accepted when length_squared < 1.0 in f64; then Camera::get_ray
 * (camera.rs:47-54) in f64, reference operation order, no fused multiply-add.  The FIRST HIT is HittableList::hit(ray, t_min, +inf)
 * over the whole list: Sphere::hit as written, the later sphere winning on equal t -- exactly bounce 0 of ray_color; rays with
 * zero / NaN / infinite directions take the list in list order as written, NaN roots included, as the render kernel does.
 *
 * A pixel has RT_FEATURE_WORDS = 8 exact sums, u64 with quantum 2^-32, wrap-free within the 65 535-sample bound above.  A sample
 * that hits sphere k adds (a miss adds nothing):
 *   words 0-2  albedo   quantize(a_c): a = the sphere's albedo for RT_LAMBERTIAN / RT_METAL, (1, 1, 1) for RT_DIALECTRIC (its
 *                       attenuation, materials.rs:103) -- BY KIND: the albedo field of a Dialectric is not read
 *   words 3-5  normal   qs(n_c): n = HitRecord::new's normal (mod.rs:20-30: outward = (p - c) * (1/r), flipped against the ray; a
 *                       negative radius flips it as the reference does); qs(x) = 0 for a NaN, else
 *                       (int64) floor(clamp(x, -65536, 65536) * 2^32), added modulo 2^64 (two's complement)
 *   word  6    depth    quantize(t), the C5 rule above (clamp RT_SAMPLE_CLAMP)
 *   word  7    hits     1
 * The lens offset is perpendicular to the view axis and the image plane lies at focus_dist: t * focus_dist is the z-depth along
 * the view axis, t = 1 the focus plane.  hits / spp is alpha: the share of the pixel's camera rays that hit anything, for
 * compositing over another background than the reference's sky.
 * The id buffer (optional, i32 per pixel): the list index of the first hit of sample index p->sample_begin (the call's first
 * sample), -1 for a miss; written, never accumulated. */
#define RT_FEATURE_WORDS 8
/* Device form, asynchronous on `stream`.  d_feat: device [height][width][8] u64; d_ids: device [height][width] i32 or NULL.
 * Honours width, height, spp (>= 1 here), sample_begin, t_min, seed and RT_FLAG_ACCUMULATE; max_depth, tile_rows, shard_index and
 * RT_FLAG_OVERLAPPED are unused or ignored.  RT_FLAG_ACCUMULATE adds to d_feat: a pixel is owned by ONE lane and added with a plain
 * load / add / store (no atomics), so two feature launches must NOT add to the same buffer concurrently -- order them on one
 * stream or with events (unlike rt_render_device's passes, which may overlap).
 * RT_ERR_INVALID_ARGUMENT, found before anything is touched (nothing written, rt_last_stats unchanged; the checks that need no
 * context come first): RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS, RT_FLAG_NO_FILTER, unknown flag bits, a context created under
 * RTIOW_SCAN_MODE=1, shard_count != 1, spp < 1, NULL cam or d_feat; RT_ERR_NO_SCENE before an upload.
 * A feature launch takes NONE of the context's two launch slots and rt_last_stats does not report on it. */
int rt_render_features_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, void *d_feat, void *d_ids, void *stream);
/* Host form: synchronous, starts from zero (RT_FLAG_ACCUMULATE is ignored); out_feat [height][width][8], out_ids [height][width]
 * or NULL; kernel_ms (may be NULL): the kernel's time, from a pair of events the call creates and destroys itself. */
int rt_render_features(rt_context *ctx, const rt_camera *cam, const rt_params *p, uint64_t *out_feat, int32_t *out_ids, float *kernel_ms);
/* Exact sums -> what a denoiser takes: d_out device [rows][width][8] f32.  With v = the sum's value in f64 (hi/lo form:
 * ((f64)(q >> 32) * 2^32 + (f64)(u32)q) * 2^-32) and IEEE f64 throughout: albedo = (f32)(v / spp); normal = (f32)(+-v(|q|) / spp), q read
 * as a two's-complement integer; depth = hits ? (f32)(v / hits) : 0, the mean over the HITTING samples; word 7 = (f32)(hits / spp).
 * spp = the samples in the sums, >= 1. */
int rt_features_to_f32_device(rt_context *ctx, const void *d_feat, int32_t width, int32_t rows, int64_t spp, void *d_out, void *stream);
/* Host-buffer form (copies in, converts on the device, copies out). */
int rt_features_to_f32(rt_context *ctx, const uint64_t *feat, int32_t width, int32_t rows, int64_t spp, float *out);

/* ---- denoiser: an edge-avoiding a-trous filter driven by the first-hit guides ---- */

/* Turns the radiance sums of a low-spp (or adaptively stopped) frame and the feature sums of the same camera into a filtered
 * ONE-SAMPLE frame of exact sums: rt_resolve_rgba8(..., spp = 1, ...) makes the picture of it, rt_fix_to_f32_device its f32 form.
 * DESIGN.md section 15.  Buffers, all full frames, j = 0 the BOTTOM row:
 *   fix    [H][W][3] u64   the radiance sums any render entry point gives
 *   count  [H][W] u32 or NULL: each pixel's own number of samples, every entry >= 1 (the adaptive frame); NULL: every pixel has
 *          `spp` samples (>= 1); when given, spp is ignored
 *   feat   [H][W][8] u64   the sums of rt_render_features over feat_spp >= 1 samples
 *   out    [H][W][3] u64   the denoised mean radiance on the 2^-32 grid (one sample)
 *
 * The contract: IEEE binary64 throughout, in this operation order, no fused multiply-add.  v(q) = the sum's value, hi/lo form
 * (above).  Pixel p = (i, j).
 *   Prepare.  c_ch = v(fix_ch) / (double)count_p;  alb_ch = v(feat_ch) / (double)feat_spp;  n_ch = +-v(|q|) / (double)feat_spp for
 *     words 3-5 read as two's complement (the rule of rt_features_to_f32 without the cast);  hits = word 7;
 *     z = hits ? v(word 6) / (double)hits : 0.0;  alpha = (double)hits / (double)feat_spp.  With RT_DENOISE_DEMODULATE
 *     m_ch = alb_ch + (1.0 - alpha) (the part of a pixel that sees the sky counts as albedo 1), then
 *     m_ch = m_ch < RT_DENOISE_ALBEDO_FLOOR ? RT_DENOISE_ALBEDO_FLOOR : m_ch; without it m_ch = 1.0.  The filter runs on c / m.
 *   Level l = 0 .. levels - 1, hole step s = 2^l:  scl = sigma_color * 0.5^l, ic = 1.0 / (scl * scl),
 *     in = 1.0 / (sigma_normal * sigma_normal), sz2 = sigma_depth * sigma_depth.
 *     1. g_p = the 3x3 box mean of the level's input c: the in-frame neighbours summed dy = -1..1 outer, dx = -1..1 inner, from 0.0,
 *        divided by their number as a double.  The colour edge-stop compares these means, not the noisy values.
 *     2. izp = 1.0 / (sz2 * (z_p * z_p) + 1e-12).  For dy = -2..2 outer, dx = -2..2 inner, q = p + s (dx, dy), taps outside the
 *        frame skipped:  k = h[dy + 2] * h[dx + 2], h = (1/16, 1/4, 3/8, 1/4, 1/16);  xc = ((dr dr + dg dg) + db db) * ic with
 *        d = g_p - g_q;  xn likewise on n_p - n_q, times in;  xz = ((z_p - z_q) * (z_p - z_q)) * izp;
 *        t(x) = x < 1.0 ? 1.0 - x : 0.0 (a NaN gives 0);  w = ((k * (tc * tc)) * (tn * tn)) * (tz * tz);
 *        acc_ch = acc_ch + w * c_q,ch and ws = ws + w, both from 0.0;  c'_p,ch = acc_ch / ws (the centre tap gives ws >= 9/64).
 *   Finish.  out_ch = quantize(c_ch * m_ch), the C5 rule above.
 * The result is a pure function of the inputs: the same bits from the device forms, from rt_denoise_host, and from either form of
 * the level kernel (RTIOW_DENOISE_LEVEL_KERNEL=gather|tile, a diagnostic knob read per call).
 *
 * The struct shares its name with the host-buffer entry point, as stat does: write `struct rt_denoise`. */
struct rt_denoise {
    int32_t  levels;        /* 1 .. RT_DENOISE_MAX_LEVELS (8): level l uses hole step 2^l */
    uint32_t flags;         /* RT_DENOISE_DEMODULATE; every other bit is an error       */
    double   sigma_color;   /* > 0, finite; halves with every level                     */
    double   sigma_normal;  /* > 0, finite                                              */
    double   sigma_depth;   /* > 0, finite; relative to the centre pixel's depth        */
};                          /* 32 bytes */
#define RT_DENOISE_DEMODULATE   0x1u
#define RT_DENOISE_MAX_LEVELS   8
#define RT_DENOISE_ALBEDO_FLOOR 0.015625

/* RT_ERR_INVALID_ARGUMENT from every form, found before anything is touched, the checks that need no context first: NULL dn, fix,
 * feat, out or workspace; levels out of range; unknown flag bits; a sigma <= 0 or not finite; width or height < 1;
 * width * height > 2^31; spp < 1 with a NULL count; feat_spp < 1. */

/* The bytes of workspace the device form needs for a width x height frame (16 doubles per pixel). */
int rt_denoise_workspace_bytes(int32_t width, int32_t height, int64_t *out_bytes);
/* Device form, asynchronous on `stream`.  Every pointer is a device pointer, 8-byte aligned; the buffers must not overlap.  d_work:
 * rt_denoise_workspace_bytes() bytes, the caller's (contents undefined afterwards).  Takes NONE of the context's launch slots,
 * rt_last_stats does not report on it, and it needs no uploaded scene. */
int rt_denoise_device(rt_context *ctx, const void *d_fix, const void *d_count, int64_t spp, const void *d_feat, int64_t feat_spp,
                      int32_t width, int32_t height, const struct rt_denoise *dn, void *d_work, void *d_out_fix, void *stream);
/* Host-buffer form (copies in, filters on the device, copies out); synchronous.  kernel_ms (may be NULL): the kernels' time, from a
 * pair of events the call creates and destroys itself. */
int rt_denoise(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp,
               int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix, float *kernel_ms);
/* The same filter on host buffers, no device needed: the library's own CPU statement of the contract (it compiles the very
 * functions the kernels do, rt_denoise_core.hpp). */
int rt_denoise_host(const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp, int32_t width,
                    int32_t height, const struct rt_denoise *dn, uint64_t *out_fix);

/* ---- variance-guided denoiser: the a-trous filter with its colour stop in units of the local standard deviation ---- */

/* The denoiser above with ONE change of principle (the spatial filter of SVGF, Schied et al., HPG 2017): a per-pixel variance, estimated
 * from the sums of HALF of each pixel's samples, travels through the levels; colour differences are measured in units of the local
 * standard deviation, not against an absolute width; the variance is propagated with the squared weights.  DESIGN.md section 25.
 * Buffers as above, and
 *   half   [H][W][3] u64   the sums of half of each pixel's samples: what rt_render_adaptive and rt_render_wavefront_adaptive return as
 *          `half`, or the first of two equal accumulated passes.  Any split into two halves of equal size is valid (the samples are
 *          independent).  count (or spp) is meant to be even and >= 2; odd values are not rejected and have the arithmetic below.
 * `struct rt_denoise` is the one above, unchanged; flags: RT_DENOISE_DEMODULATE only; sigma_color is in STANDARD DEVIATIONS and does not
 * halve with the level (the variance shrinks by itself).  The output is a one-sample frame of exact sums, like rt_denoise's.
 *
 * The contract: IEEE binary64 throughout, in this operation order, no fused multiply-add.  samples = (double)count_p (or spp).
 *   Prepare.  c0 = c / m, m, n, z: exactly rt_denoise's.  Per channel  d_ch = 2 * half_ch - fix_ch  in wrapping uint64 arithmetic, read
 *     as two's complement, absolute value taken (the selection rule's d_c);  e_ch = (v(d_ch) / samples) / m_ch;
 *     var_p = (e_r * e_r + e_g * e_g) + e_b * e_b: the squared half-difference of the two half means, an estimate of the variance of
 *     the pixel's demodulated mean summed over the channels -- commensurate with the squared RGB distance the colour stop uses.
 *   Level l = 0 .. levels - 1, hole step s = 2^l:  sc2 = sigma_color * sigma_color;  in, sz2: rt_denoise's.
 *     1. g_p = the 3x3 box mean of the level's input colour, as above.
 *     2. gv_p = the 3x3 Gaussian of the level's input variance: the in-frame neighbours q, dy = -1..1 outer, dx = -1..1 inner,
 *        kk = (1, 2, 1; 2, 4, 2; 1, 2, 1) / 16;  sv = sv + kk * var_q and sk = sk + kk, both from 0.0;  gv_p = sv / sk.
 *     3. izp as above;  icv = 1.0 / (sc2 * gv_p + 1e-12).  The 25 taps in rt_denoise's order with its skip rule, k, xn, xz and t(x):
 *        xc = ((dr dr + dg dg) + db db) * icv with d = g_p - g_q;  w = ((k * (tc * tc)) * (tn * tn)) * (tz * tz);
 *        acc_ch = acc_ch + w * c_q,ch,  ws = ws + w  and  va = va + (w * w) * var_q, all from 0.0;
 *        c'_p,ch = acc_ch / ws  and  var'_p = va / (ws * ws).
 *   Finish.  rt_denoise's.
 * The same bits from the device forms, from rt_denoise_var_host and from either form of the level kernel
 * (RTIOW_DENOISE_LEVEL_KERNEL=gather|tile, the knob of rt_denoise, read per call).
 *
 * RT_ERR_INVALID_ARGUMENT from every form, found before anything is touched, in this order, the checks that need no context first: NULL
 * dn; NULL fix; NULL half; NULL feat or out; levels out of range; unknown flag bits; a sigma <= 0 or not finite; width or height < 1;
 * width * height > 2^31; spp < 1 with a NULL count; feat_spp < 1; then a NULL workspace (device form), then a NULL context. */

/* The bytes of workspace the device form needs for a width x height frame: 19 doubles per pixel (rt_denoise's 16, two variance planes
 * and the variance's Gaussian).  This call is the only source of the number. */
int rt_denoise_var_workspace_bytes(int32_t width, int32_t height, int64_t *out_bytes);
/* Device form, asynchronous on `stream`.  Every pointer is a device pointer, 8-byte aligned; the buffers must not overlap.  d_work:
 * rt_denoise_var_workspace_bytes() bytes, the caller's (contents undefined afterwards).  Takes NONE of the context's launch slots,
 * rt_last_stats does not report on it, and it needs no uploaded scene. */
int rt_denoise_var_device(rt_context *ctx, const void *d_fix, const void *d_half, const void *d_count, int64_t spp, const void *d_feat,
                          int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, void *d_work, void *d_out_fix,
                          void *stream);
/* Host-buffer form (copies in, filters on the device, copies out); synchronous.  kernel_ms (may be NULL): the kernels' time. */
int rt_denoise_var(rt_context *ctx, const uint64_t *fix, const uint64_t *half, const uint32_t *count, int64_t spp, const uint64_t *feat,
                   int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix, float *kernel_ms);
/* The same filter on host buffers, no device needed: the library's own CPU statement of the contract (rt_denoise_var_core.hpp). */
int rt_denoise_var_host(const uint64_t *fix, const uint64_t *half, const uint32_t *count, int64_t spp, const uint64_t *feat,
                        int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix);

/* ---- temporal accumulation: last frame's result, reprojected through the first hit ---- */

/* Blends the radiance sums of the current frame of an animation over a STATIC scene with the result of the previous call, fetched where
 * the surface each pixel shows lay in the previous camera's image.  The scene does not move, so no motion vectors are needed: the first-hit
 * depth of a pixel gives a world point, and that point projects into the previous image.  Tests on depth and normal reject disocclusions.
 * The result is a ONE-SAMPLE frame of exact sums, like the denoiser's: rt_denoise(..., spp = 1, the current frame's feat, ...),
 * rt_resolve_rgba8(..., spp = 1) and rt_fix_to_f32_device take it as it is.  DESIGN.md section 16.  Buffers, all full frames, j = 0 the
 * BOTTOM row:
 *   current frame   fix [H][W][3] u64; count [H][W] u32 or NULL (every entry >= 1; NULL: every pixel has `spp` samples, >= 1; when
 *                   given, spp is ignored); feat [H][W][8] u64 over feat_spp >= 1 samples; cam: the frame's rt_camera, a HOST pointer
 *                   in every form, read during the call
 *   history         all four or none (none = the first frame): prev_fix [H][W][3] u64 and prev_len [H][W] u32, the previous call's
 *                   out_fix and out_len (length 0: no history at that pixel); prev_feat [H][W][8] u64 over prev_feat_spp >= 1 samples,
 *                   the previous frame's feature sums; prev_cam, the previous frame's rt_camera (host pointer)
 *   outputs         out_fix [H][W][3] u64, the accumulated mean radiance on the 2^-32 grid (one sample); out_len [H][W] u32, the
 *                   number of frames behind each pixel, 1 .. RT_TEMPORAL_MAX_LEN.  They must NOT overlap the history (a pixel reads
 *                   its neighbours' history): callers ping-pong two pairs of buffers.
 *
 * The contract: IEEE binary64 throughout, in this operation order, no fused multiply-add.  v(q) = the sum's value, hi/lo form (above);
 * quantize = the C5 rule; dot(a, b) = (a0 b0 + a1 b1) + a2 b2; cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 *   Constants, once per call, with Hh = prev.horizontal, Vv = prev.vertical:  L_k = prev.lower_left_corner_k - prev.origin_k;
 *     nrm = cross(Hh, Vv);  iLn = 1.0 / dot(L, nrm);  LH = dot(L, Hh);  LV = dot(L, Vv);  iHH = 1.0 / dot(Hh, Hh);  iVV = 1.0 / dot(Vv, Vv);
 *     wm1 = (double)(W - 1);  hm1 = (double)(H - 1);  sz2 = sigma_depth * sigma_depth;  in = 1.0 / (sigma_normal * sigma_normal).
 *     The formulas assume horizontal and vertical are perpendicular, as Camera::new (camera.rs:17-45) makes them; they are the contract
 *     whatever camera is passed.
 *   Pixel p = (i, j):
 *   1. Prepare (the denoiser's rules, no demodulation).  c_ch = v(fix_ch) / (double)count_p (or spp);  hits = word 7;
 *      z = hits ? v(word 6) / (double)hits : 0.0;  n_ch = +-v(|q|) / (double)feat_spp for words 3-5 read as two's complement.
 *   2. No history: out_ch = quantize(c_ch), len = 1 -- when there is no history argument, when hits == 0 (a pure sky pixel has nothing
 *      to reproject and no noise to remove), and at every "no history" exit below.
 *   3. The world point of the pixel centre through the lens centre.  u = ((double)i + 0.5) / wm1;  v = ((double)j + 0.5) / hm1;
 *      d_k = ((cur.lower_left_corner_k + u * cur.horizontal_k) + v * cur.vertical_k) - cur.origin_k;  P_k = cur.origin_k + z * d_k.
 *      (z is the ray parameter whose value 1 is the focus plane; lens offsets average out of it.)
 *   4. Into the previous image.  e_k = P_k - prev.origin_k;  s = dot(e, nrm) * iLn (the point's ray parameter in the previous camera, the
 *      unit of that frame's z);  no history unless s > 0.0;  is = 1.0 / s;  up = (dot(e, Hh) * is - LH) * iHH;
 *      vp = (dot(e, Vv) * is - LV) * iVV;  fx = up * wm1 - 0.5;  fy = vp * hm1 - 0.5;  no history unless
 *      fx >= -1.0 && fx < (double)W && fy >= -1.0 && fy < (double)H (a NaN fails);  i0 = floor(fx), a = fx - (double)i0;  j0, b likewise.
 *   5. Four taps q, in the order (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1), with the weights kw = (1.0 - a) * (1.0 - b),
 *      a * (1.0 - b), (1.0 - a) * b, a * b.  A tap is skipped when it lies outside the frame, when kw is not > 0.0, when prev_len_q == 0,
 *      when the previous frame's hits_q == 0, and unless both
 *          ((z_q - s) * (z_q - s)) < sz2 * (s * s) + 1e-12      and      ((dn0 dn0 + dn1 dn1) + dn2 dn2) * in < 1.0,  dn = n_p - n_q,
 *      with z_q, n_q the previous frame's guides at q prepared as in step 1 over prev_feat_spp.  A kept tap adds
 *      acc_ch = acc_ch + kw * v(prev_fix_q,ch) and ws = ws + kw, both from 0.0, and N = min(N, prev_len_q).  No history unless ws > 0.0;
 *      h_ch = acc_ch / ws.
 *   6. With RT_TEMPORAL_CLAMP (it limits ghosting on mirrors and glass, which first-hit reprojection does not describe): lo_ch = hi_ch =
 *      c_p,ch, then for the other in-frame pixels q of the 3 x 3 neighbourhood of p in the CURRENT frame, dy = -1..1 outer, dx = -1..1
 *      inner: lo = c_q < lo ? c_q : lo, hi = c_q > hi ? c_q : hi.  mid = (lo + hi) * 0.5;  ext = ((hi - lo) * 0.5) * clamp_scale;
 *      h = h < mid - ext ? mid - ext : h;  then h = h > mid + ext ? mid + ext : h.
 *   7. Blend.  at = 1.0 / (double)(N + 1);  at = at < alpha_min ? alpha_min : at;  out_ch = quantize(h_ch + at * (c_ch - h_ch));
 *      len = min(N + 1, RT_TEMPORAL_MAX_LEN).
 * The result is a pure function of the inputs: the same bits from the device forms and from rt_temporal_host.
 *
 * The struct shares its name with the host-buffer entry point, as rt_denoise does: write `struct rt_temporal`. */
struct rt_temporal {
    uint32_t flags;         /* RT_TEMPORAL_CLAMP; every other bit is an error                                   */
    uint32_t reserved;      /* 0                                                                                */
    double   alpha_min;     /* in (0, 1]: the least weight of the current frame (the history's memory is 1 / alpha_min frames) */
    double   sigma_normal;  /* > 0, finite                                                                      */
    double   sigma_depth;   /* > 0, finite; relative to the reprojected depth                                   */
    double   clamp_scale;   /* >= 0, finite: 1 the neighbourhood's box, 0 its centre (no history survives), read with RT_TEMPORAL_CLAMP */
};                          /* 40 bytes */
#define RT_TEMPORAL_CLAMP   0x1u
#define RT_TEMPORAL_MAX_LEN 65535

/* RT_ERR_INVALID_ARGUMENT from every form, found before anything is touched, the checks that need no context first: NULL options, fix,
 * feat, cam, out_fix or out_len; a partial history (some but not all of prev_fix, prev_len, prev_feat, prev_cam); unknown flag bits; an
 * option out of range or not finite; width or height < 2 (u, v divide by W - 1, H - 1); width * height > 2^31; spp < 1 with a NULL
 * count; feat_spp < 1; prev_feat_spp < 1 with a history. */

/* Device form, asynchronous on `stream`.  Every buffer is a device pointer, 8-byte aligned (4 for the u32 ones); the two cameras and the
 * options are host pointers read during the call.  Takes NONE of the context's launch slots, rt_last_stats does not report on it, and it
 * needs no uploaded scene. */
int rt_temporal_device(rt_context *ctx, const void *d_fix, const void *d_count, int64_t spp, const void *d_feat, int64_t feat_spp,
                       const rt_camera *cam, const void *d_prev_fix, const void *d_prev_len, const void *d_prev_feat, int64_t prev_feat_spp,
                       const rt_camera *prev_cam, int32_t width, int32_t height, const struct rt_temporal *tp, void *d_out_fix,
                       void *d_out_len, void *stream);
/* Host-buffer form (copies in, accumulates on the device, copies out); synchronous.  kernel_ms (may be NULL): the kernel's time, from a
 * pair of events the call creates and destroys itself. */
int rt_temporal(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp,
                const rt_camera *cam, const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp,
                const rt_camera *prev_cam, int32_t width, int32_t height, const struct rt_temporal *tp, uint64_t *out_fix, uint32_t *out_len,
                float *kernel_ms);
/* The same accumulation on host buffers, no device needed: the library's own CPU statement of the contract (it compiles the very
 * functions the kernel does, rt_temporal_core.hpp). */
int rt_temporal_host(const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp, const rt_camera *cam,
                     const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp,
                     const rt_camera *prev_cam, int32_t width, int32_t height, const struct rt_temporal *tp, uint64_t *out_fix,
                     uint32_t *out_len);

/* ---- temporal accumulation with second moments; the variance-guided denoiser fed by a given variance ---- */

/* rt_temporal with the second moment of the frame means carried beside the colour, and a per-channel variance of the accumulated value as
 * an output: the temporal half of SVGF (Schied et al., HPG 2017).  DESIGN.md section 26.  Arguments, `struct rt_temporal` and
 * RT_TEMPORAL_CLAMP are rt_temporal's, and
 *   history   prev_m2 [H][W][3] double, the previous call's out_m2.  The history is now all FIVE buffers or none.
 *   outputs   out_m2 [H][W][3] double, the accumulated mean of the squared frame means; out_var [H][W][3] double, per channel the variance
 *             of the accumulated value out_fix holds, in radiance units squared -- what rt_denoise_var_given takes as `var`.  Like out_fix
 *             and out_len they must NOT overlap the history.
 * Doubles, not exact sums: a squared radiance passes the 2^16 sample clamp at c = 256, and a light seen directly is brighter than that.
 *
 * The contract: IEEE binary64 throughout, in this operation order, no fused multiply-add.
 *   Steps 1-7 of rt_temporal are unchanged: out_fix and out_len are rt_temporal's bits for the same inputs.  Below, o_ch is the double of
 *   step 7 before quantize (c_ch at a "no history" exit) and len is step 7's result.
 *   s2_ch = c_ch * c_ch.
 *   No history (step 2 and every "no history" exit): m2_ch = s2_ch, at = 1.0, len = 1.
 *   Step 5.  Every kept tap also adds acc2_ch = acc2_ch + kw * prev_m2_q,ch, from 0.0;  h2_ch = acc2_ch / ws.
 *   Step 6, only with the clamp.  hb_ch = h_ch before the two limits; after them h2_ch = (h2_ch - hb_ch * hb_ch) + h_ch * h_ch: the clamp
 *     moves the history's mean and keeps its central variance.
 *   Step 7.  m2_ch = h2_ch + at * (s2_ch - h2_ch);  vt_ch = m2_ch - o_ch * o_ch;  vt_ch = vt_ch > 0.0 ? vt_ch : 0.0 (a NaN gives 0).
 *   Spatial estimate (SVGF's rule for young pixels; always computed).  Over the in-frame pixels q of the 3 x 3 neighbourhood of p in the
 *     CURRENT frame, the centre included in its place, dy = -1..1 outer, dx = -1..1 inner:  a1_ch = a1_ch + c_q,ch,
 *     a2_ch = a2_ch + c_q,ch * c_q,ch  and  cnt = cnt + 1.0, all from 0.0.  mu = a1_ch / cnt;  vs_ch = a2_ch / cnt - mu * mu, clipped at 0
 *     the same way as vt_ch.
 *   Result.  vf_ch = len < RT_TEMPORAL_VAR_MIN_LEN ? vs_ch : vt_ch;  out_var_ch = vf_ch * at;  out_m2_ch = m2_ch.
 * vf estimates the variance of ONE frame's mean; multiplying by at makes it the variance of the accumulated value.  That is exact for
 * the running mean (at = 1 / len); once alpha_min holds at up, the exponential average's variance is at / (2 - at) of one frame's, so
 * vf * at is conservative by at most 2x.
 * The result is a pure function of the inputs: the same bits from the device forms and from rt_temporal_var_host.
 *
 * RT_ERR_INVALID_ARGUMENT from every form, found before anything is touched and leaving all four outputs untouched: rt_temporal's
 * checks in its order, with out_m2 and out_var in the NULL check and prev_m2 in the history count (some but not all five is a partial
 * history); the context check comes last. */
#define RT_TEMPORAL_VAR_MIN_LEN 4

/* Device form, asynchronous on `stream`: as rt_temporal_device.  Takes NONE of the context's launch slots, rt_last_stats does not report
 * on it, and it needs no uploaded scene. */
int rt_temporal_var_device(rt_context *ctx, const void *d_fix, const void *d_count, int64_t spp, const void *d_feat, int64_t feat_spp,
                           const rt_camera *cam, const void *d_prev_fix, const void *d_prev_len, const void *d_prev_feat, int64_t prev_feat_spp,
                           const rt_camera *prev_cam, const void *d_prev_m2, int32_t width, int32_t height, const struct rt_temporal *tp,
                           void *d_out_fix, void *d_out_len, void *d_out_m2, void *d_out_var, void *stream);
/* Host-buffer form (copies in, accumulates on the device, copies out); synchronous.  kernel_ms (may be NULL): the kernel's time. */
int rt_temporal_var(rt_context *ctx, const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp,
                    const rt_camera *cam, const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp,
                    const rt_camera *prev_cam, const double *prev_m2, int32_t width, int32_t height, const struct rt_temporal *tp,
                    uint64_t *out_fix, uint32_t *out_len, double *out_m2, double *out_var, float *kernel_ms);
/* The same accumulation on host buffers, no device needed: the library's own CPU statement of the contract (rt_temporal_var_core.hpp). */
int rt_temporal_var_host(const uint64_t *fix, const uint32_t *count, int64_t spp, const uint64_t *feat, int64_t feat_spp, const rt_camera *cam,
                         const uint64_t *prev_fix, const uint32_t *prev_len, const uint64_t *prev_feat, int64_t prev_feat_spp,
                         const rt_camera *prev_cam, const double *prev_m2, int32_t width, int32_t height, const struct rt_temporal *tp,
                         uint64_t *out_fix, uint32_t *out_len, double *out_m2, double *out_var);

/* rt_denoise_var with `half` replaced by
 *   var   [H][W][3] double   per channel, the variance of the pixel's mean c_ch in radiance units squared: rt_temporal_var's out_var (then
 *         fix is its out_fix and spp = 1).
 * Everything else is rt_denoise_var's: `struct rt_denoise`, the levels, the statistics, the taps, finish, both forms of the level kernel
 * and their knob, and the workspace of rt_denoise_var_workspace_bytes.  The one new rule is in Prepare:
 *   x_ch = (var_ch / m_ch) / m_ch;  x_ch = x_ch > 0.0 ? x_ch : 0.0 (a NaN and a negative give 0);  var_p = (x_r + x_g) + x_b.
 * The checks are rt_denoise_var's in its order, with var in half's place. */
int rt_denoise_var_given_device(rt_context *ctx, const void *d_fix, const void *d_var, const void *d_count, int64_t spp, const void *d_feat,
                                int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, void *d_work, void *d_out_fix,
                                void *stream);
int rt_denoise_var_given(rt_context *ctx, const uint64_t *fix, const double *var, const uint32_t *count, int64_t spp, const uint64_t *feat,
                         int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix, float *kernel_ms);
int rt_denoise_var_given_host(const uint64_t *fix, const double *var, const uint32_t *count, int64_t spp, const uint64_t *feat,
                              int64_t feat_spp, int32_t width, int32_t height, const struct rt_denoise *dn, uint64_t *out_fix);

/* ---- ray queries: closest hit and occlusion for rays the caller supplies ---- */

/* HittableList::hit (mod.rs:54-70) for rays that do not come from an rt_camera: picking, visibility between two points, ambient
 * occlusion, collision probes, a wavefront integrator of the caller's own over the uploaded scene.  What other libraries call
 * intersect / occluded.  DESIGN.md section 17.  Structure-of-arrays, so that a tensor passes as it is.
 *
 * The contract.  The closest hit of ray k is HittableList::hit(Ray { origin[k], dir[k] }, t_min, t_max[k]) over the uploaded list:
 * closest_so_far starts at t_max[k] (mod.rs:56); Sphere::hit (sphere.rs:15-41) as written, in IEEE binary64, in the reference's operation
 * order, no fused multiply-add; a root EQUAL to closest_so_far is accepted (sphere.rs:29, 31 reject only t_max < root), so the later
 * sphere wins on equal t and a root equal to t_max is a hit.  The direction is not normalised (ray.rs: Ray as it stands): t is in units
 * of |dir|.
 *   Rays inside the filter's analysed range are answered in the order-independent form the render and feature kernels use, which
 *   gives the same answer: a sphere's root is the near one if it is >= t_min, else the far one; the smallest root <= t_max wins, on
 *   ties the later index.
 *   Rays outside it take the list in list order exactly as written, NaN roots included (a NaN fails neither comparison of
 *   sphere.rs:29, 31 and is accepted): a zero, NaN or infinite direction (precisely: |dir|^2, rounded to f32, not inside
 *   (1e-20, 1e20)), |origin|_1 >= 1e15, a NaN t_max.
 *   t_min is per call, > 0 and finite, as rt_params.t_min.  t_max is per ray and any double is legal: negative, zero and below t_min
 *   simply miss.
 *   A hit writes index (the place in the uploaded list), t, point = origin + dir * t (Ray::at, ray.rs:15-17), normal (HitRecord::new,
 *   mod.rs:20-30: outward = (point - center) * (1/radius), flipped against the ray; a negative radius flips it as the reference does)
 *   and front_face.  A miss writes index = -1, t = +inf, point = normal = 0, front_face = 0.  A NaN in t, point or normal is written as
 *   the quiet NaN 0x7FF8000000000000 (IEEE 754 leaves the sign and payload of a generated NaN open, and processors differ).
 *   occluded[k] = 1 iff the closest-hit query of ray k would return an index >= 0, else 0 (the kernel stops a ray at its first
 *   accepted root; the answer does not depend on which root that is).
 * The result is a pure function of scene, rays and t_min: the same bits from the device and the host forms, under RTIOW_NO_GRID /
 * RTIOW_GRID_DIM, from either candidate scheme (RTIOW_TRACE_CANDIDATES=wave|ray, a diagnostic knob read per call), whatever the
 * launch's size (RTIOW_TRACE_GRID_BLOCKS=k, likewise: at most k workgroups) and whichever position in the batch a ray has. */
typedef struct {
    const double *origin;   /* [n][3]                                              */
    const double *dir;      /* [n][3], not normalised: Ray as ray.rs has it        */
    const double *t_max;    /* [n], or NULL: +inf for every ray                    */
    int64_t n;
} rt_rays;
typedef struct {
    int32_t *index;         /* [n]  required: list index of the winner, -1 a miss  */
    double  *t;             /* [n]     or NULL */
    double  *point;         /* [n][3]  or NULL: Ray::at(t), ray.rs:15-17           */
    double  *normal;        /* [n][3]  or NULL: HitRecord::new, mod.rs:20-30       */
    uint8_t *front_face;    /* [n]     or NULL */
} rt_hits;
/* RT_ERR_INVALID_ARGUMENT from every form, found before anything is touched, the checks that need no context first: NULL rays or
 * hits; n < 0 or n > 2^31; t_min not > 0 or not finite; with n > 0 a NULL origin, dir, index or occluded; then a NULL context or one
 * created under RTIOW_SCAN_MODE=1.  RT_ERR_NO_SCENE before an upload.  n == 0 then succeeds and touches nothing.  Outputs must not
 * overlap inputs or each other. */

/* Device forms, asynchronous on `stream`.  The two structs are HOST pointers read during the call; the arrays they name are device
 * pointers, 8-byte aligned (4 for index).  A query takes NONE of the context's launch slots and rt_last_stats does not report on it. */
int rt_trace_rays_device(rt_context *ctx, const rt_rays *rays, double t_min, const rt_hits *hits, void *stream);
/* Host-buffer form (copies in, traces on the device, copies out); synchronous.  kernel_ms (may be NULL): the kernel's time, from a pair
 * of events the call creates and destroys itself. */
int rt_trace_rays(rt_context *ctx, const rt_rays *rays, double t_min, const rt_hits *hits, float *kernel_ms);
/* Occlusion: d_occluded / occluded is [n] u8. */
int rt_occluded_device(rt_context *ctx, const rt_rays *rays, double t_min, void *d_occluded, void *stream);
int rt_occluded(rt_context *ctx, const rt_rays *rays, double t_min, uint8_t *occluded, float *kernel_ms);

/* ---- wavefront path steps: camera rays, material scatter, accumulate ---------- */

/* The three things a path needs besides its closest hit, as calls of their own, so that a wavefront integrator driven from outside --
 * camera rays -> loop { rt_trace_rays; accumulate the misses; scatter; throughput *= attenuation } -- reproduces the exact sums of
 * rt_render bit for bit, and whatever the megakernel does not do (AOVs per bounce, a direct-only pass, the caller's own termination
 * rule, extra radiance terms) is a few lines of caller code on top.  DESIGN.md section 18.  Structure-of-arrays like the ray queries:
 * the arrays of one step are named by one struct, inputs and outputs alike.
 *
 * The random stream of a path: Philox key `seed`, counter (pixel, sample, event, 0) with pixel the global number
 * g = j * width + i (j = 0 the BOTTOM row) and event the index of the NEXT UNUSED block of that (pixel, sample).  event is the only
 * random state a path carries between steps: the camera step gives it, every scatter advances it.  Draws are the default stream's:
 * u01(w) = w * 2^-32, u11(w) = (int32_t)w * 2^-31.  flags: 0; RT_FLAG_UNIFORM53 (not built for these steps) and every other bit is
 * RT_ERR_INVALID_ARGUMENT.
 * IEEE binary64, the reference's operation order, no fused multiply-add; a NaN in a double output is written as the quiet NaN
 * 0x7FF8000000000000, as the ray queries write it.  A result is a pure function of its inputs: the same bits from the device and the
 * host forms, whatever the launch's size (RTIOW_SHADE_GRID_BLOCKS=k, a diagnostic knob read per call: at most k workgroups) and
 * wherever in the batch a path stands. */

/* sample_ray: main.rs:131-134 + Camera::get_ray, camera.rs:47-54.  Block 0 of (pixel[k], sample[k]) = (u jitter, v jitter, lens x,
 * lens y); every further random_in_unit_disk try (vec3.rs:59-68) takes the next two words, on into blocks 1, 2, ...; i = pixel % width,
 * j = pixel / width, u = (i + e0) / (width - 1), v = (j + e1) / (height - 1).  event[k] = 1 + ceil((tries - 1) / 2).  Exactly the camera
 * ray rt_render traces for that pixel and sample index.  Needs no uploaded scene. */
typedef struct {
    const uint32_t *pixel;   /* [n]    in                                            */
    const uint32_t *sample;  /* [n]    in                                            */
    double   *origin;        /* [n][3] out                                           */
    double   *dir;           /* [n][3] out, not normalised                           */
    uint32_t *event;         /* [n]    out: the next unused block                    */
    int64_t n;
} rt_camera_batch;

/* Scatter::scatter of materials.rs (:21-31 Lambertian, :48-62 Metal, :76-105 Dialectric) in the order Oracle B states it, for the hit
 * (index, point, normal, front_face) exactly as rt_trace_rays writes it and the incoming direction dir.  The material is the uploaded
 * sphere index[k].  Lambertian and Metal take one run of unit-sphere tries (vec3.rs:37-45) of three consecutive words each, starting at
 * block event[k], to acceptance: event += ceil(3 tries / 4); Metal draws whatever its fuzz, as the reference does.  The Dialectric draws
 * one word of one block, only when it can refract: event += 1 then, unchanged otherwise (total internal reflection).  A Lambertian
 * whose normal + unit vector is near zero (vec3.rs:111-114) scatters along the normal. */
enum { RT_SCATTER_ABSORBED = 0,    /* Metal with dot(scattered, normal) <= 0: attenuation written as zeros, out_origin / out_dir NOT written, event advanced */
       RT_SCATTER_SCATTERED = 1,   /* out_origin = point, out_dir, attenuation and event written                                                          */
       RT_SCATTER_MISS = 2,        /* index == -1: nothing but the status written, event unchanged                                                        */
       RT_SCATTER_BAD_INDEX = 3 }; /* index < -1 or >= the sphere count: nothing read from the scene, nothing but the status written                      */
typedef struct {
    const double  *dir;         /* [n][3] in: the direction of the ray that hit                  */
    const int32_t *index;       /* [n]    in: rt_hits.index                                      */
    const double  *point;       /* [n][3] in: rt_hits.point                                      */
    const double  *normal;      /* [n][3] in: rt_hits.normal                                     */
    const uint8_t *front_face;  /* [n]    in: rt_hits.front_face                                 */
    const uint32_t *pixel;      /* [n]    in                                                     */
    const uint32_t *sample;     /* [n]    in                                                     */
    uint32_t *event;            /* [n]    in and out                                             */
    double   *out_origin;       /* [n][3] out: may be the very array the next trace reads        */
    double   *out_dir;          /* [n][3] out: may be `dir` itself (a path reads its own elements before it writes them); no other overlap */
    double   *attenuation;      /* [n][3] out                                                    */
    uint8_t  *status;           /* [n]    out: RT_SCATTER_*                                      */
    int64_t n;
} rt_scatter_batch;

/* Contract C5 for samples the caller finishes: per channel, quantize(weight * sky(sky_dir)) is added to d_fix[pixel[k]] -- the very
 * buffer rt_render_device fills and rt_resolve_rgba8 reads -- with one 64-bit atomic add.  sky: main.rs:54-56 (unit_direction = unit_vector(dir),
 * t = 0.5 * (unit_direction.y + 1.0), (1, 1, 1) * (1.0 - t) + (0.5, 0.7, 1.0) * t), multiplied as Oracle B's mulv(throughput, sky).  With
 * sky_dir NULL the value is weight itself.  Paths with select[k] == 0 (select given) or pixel[k] >= npix add nothing and touch no memory:
 * documented, not an error.  Integer sums: the result does not depend on order, on how a batch is split, or on the streams the calls run
 * on (the caller orders zeroing before and reading after, as for rt_render_device's passes).  Needs no uploaded scene. */
typedef struct {
    const uint32_t *pixel;      /* [n]    in: entry of d_fix                                     */
    const double   *weight;     /* [n][3] in                                                     */
    const double   *sky_dir;    /* [n][3] in, or NULL                                            */
    const uint8_t  *select;     /* [n]    in, or NULL: every path                                */
    int64_t n;
} rt_accumulate_batch;

/* RT_ERR_INVALID_ARGUMENT from every form, found before anything is touched, the checks that need no context first: a NULL camera or
 * batch struct, a NULL fix buffer; n < 0 or n > 2^31; with n > 0 a NULL array other than sky_dir and select; width or height < 2;
 * npix <= 0 or > 2^32; flags != 0; then a NULL context.  RT_ERR_NO_SCENE from the scatter step before an upload.  n == 0 then succeeds and
 * touches nothing.
 * Device forms: asynchronous on `stream`; the structs (and the camera) are HOST pointers read during the call, the arrays they name device
 * pointers, 8-byte aligned (4 for the 32-bit ones).  A step takes NONE of the context's launch slots and rt_last_stats does not report on it.
 * Host-buffer forms: copy in, run on the device, copy out; synchronous; what a step does not write keeps the caller's bytes; kernel_ms
 * (may be NULL): the kernel's time, from a pair of events the call creates and destroys itself. */
int rt_camera_rays_device(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags,
                          const rt_camera_batch *batch, void *stream);
int rt_camera_rays(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags,
                   const rt_camera_batch *batch, float *kernel_ms);
int rt_scatter_device(rt_context *ctx, uint64_t seed, uint32_t flags, const rt_scatter_batch *batch, void *stream);
int rt_scatter(rt_context *ctx, uint64_t seed, uint32_t flags, const rt_scatter_batch *batch, float *kernel_ms);
/* d_fix / fix: [npix][3] u64 exact sums, added to. */
int rt_accumulate_device(rt_context *ctx, const rt_accumulate_batch *batch, void *d_fix, int64_t npix, void *stream);
int rt_accumulate(rt_context *ctx, const rt_accumulate_batch *batch, uint64_t *fix, int64_t npix, float *kernel_ms);

/* ---- path queue: a fused bounce step on device-resident paths, and the frame rendered from it ---------- */

/* The wavefront integrator of the steps above with the paths, and their NUMBER, kept on the device: one call per bounce, no host wait
 * between bounces.  DESIGN.md section 19.  A queue is structure-of-arrays and caller-owned (torch tensors pass as they are): the live
 * paths are slots [0, *count), in order; `count` is ONE word of device memory that the kernels read and the host never does.  The
 * random stream, the arithmetic and the NaN rule are those of the wavefront path steps; flags: 0 only.  RTIOW_PATHS_GRID_BLOCKS=k (a
 * diagnostic knob read per call): at most k workgroups per launch; a result does not depend on it. */
typedef struct rt_path_queue {
    int64_t   capacity;        /* 1 .. 2^24 slots                                                                    */
    uint32_t *count;           /* device, ONE word: the live paths; a value above capacity is read as capacity       */
    uint32_t *pixel;           /* [capacity]                                                                         */
    uint32_t *sample;          /* [capacity]                                                                         */
    uint32_t *event;           /* [capacity]    the next unused Philox block, as in the wavefront steps              */
    double   *origin;          /* [capacity][3]                                                                      */
    double   *dir;             /* [capacity][3] not normalised                                                       */
    double   *throughput;      /* [capacity][3]                                                                      */
    uint32_t *scratch;         /* [rt_path_scratch_words(capacity)]: the compaction's counts, offsets and alive marks */
} rt_path_queue;
/* 3 words per 64 slots: 3 * ceil(capacity / 64); 0 for a capacity outside [1, 2^24] */
int64_t rt_path_scratch_words(int64_t capacity);

/* Slot k in [0, n) becomes item first_item + k of a frame of width x height pixels with spp samples each, pixel-major:
 * pixel = item / spp, sample = sample_begin + item % spp; origin, dir and event are rt_camera_rays' for that pair; throughput (1, 1, 1);
 * *q->count = n.  Slots at or past n keep their bytes.  Needs 0 <= n <= capacity, spp >= 1, sample_begin >= 0, first_item >= 0 and
 * first_item + n <= width * height * spp.  Needs no uploaded scene. */
int rt_paths_begin_device(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags, int32_t spp,
                          int32_t sample_begin, int64_t first_item, int64_t n, const rt_path_queue *q, void *stream);

/* One bounce of every live path of `in`.  Closest hit: HittableList::hit(ray, t_min, +inf), as rt_trace_rays answers it.  A miss adds
 * quantize(throughput * sky(dir)) to d_fix[pixel] exactly as rt_accumulate does with sky_dir (pixel >= npix adds nothing) and the path
 * ends.  A hit scatters exactly as rt_scatter: RT_SCATTER_ABSORBED ends the path; RT_SCATTER_SCATTERED survives with origin = the hit
 * point, dir = the scattered direction, throughput = throughput * attenuation (one f64 multiply per channel) and the advanced event.
 * The survivors are written to `out` IN THE ORDER THEY HAD IN `in`, into slots [0, m), and *out->count = m; slots of `out` at or past m
 * keep the caller's bytes.  `in` and `out` are distinct queues that share no array, out->capacity >= in->capacity.  After the call the
 * arrays of `in` (its scratch included) hold intermediate values and *in->count is unchanged.  d_rays (may be NULL): one device u64 that
 * gains the number of live paths of `in` (a plain add: calls that share it are ordered by their streams).  A count of 0 does nothing but
 * *out->count = 0.  d_fix: [npix][3] u64 exact sums, added to. */
int rt_paths_step_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                         void *d_fix, int64_t npix, void *d_rays, void *stream);

/* The whole frame from the two calls above: rt_render_device's exact sums bit for bit, and in *d_rays / *rays_traced (may be NULL) the
 * rt_stats.rays_traced of that render.  Honours width, height, spp, sample_begin, max_depth, t_min and seed of `p`; flags must be 0 and
 * shard_count 1.  d_fix ([height][width][3] u64) and d_rays are zeroed first.  The frame's width * height * spp items go in batches of
 * RTIOW_WAVEFRONT_BATCH (read per call; default 2^20, at most 2^24): per batch one begin, then max_depth steps between two queues the
 * context owns (allocated on first use, regrown when a batch is larger, freed by rt_destroy); a path still alive after max_depth steps
 * adds nothing.  No host wait inside the call: the device form is asynchronous on `stream` (calls on one context must be ordered by the
 * caller: they share its queues).  The host-buffer form copies out and synchronises; kernel_ms (may be NULL): the kernels' time.
 *
 * RT_ERR_INVALID_ARGUMENT from every form of this block, found before anything is touched, the checks that need no context first: a
 * NULL camera, params or queue struct, a NULL array of a queue, a NULL d_fix / fix; capacity outside [1, 2^24]; n outside [0, capacity];
 * `in` == `out` or a shared array; out->capacity < in->capacity; width or height < 2 (and spp, sample_begin, first_item as above); npix
 * outside [1, 2^32]; flags != 0 (RT_FLAG_UNIFORM53 named); t_min not finite or not > 0; then a NULL context; then a context created under
 * another scan mode than the shipped one (RTIOW_SCAN_MODE); then RT_ERR_NO_SCENE (not for rt_paths_begin_device).  These calls take NONE
 * of the context's launch slots and rt_last_stats does not report on them. */
int rt_render_wavefront_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, void *d_fix, void *d_rays, void *stream);
int rt_render_wavefront(rt_context *ctx, const rt_camera *cam, const rt_params *p, uint64_t *fix, uint64_t *rays_traced, float *kernel_ms);

/* ---- lighting: a settable sky and emissive spheres for the path queue ---------------------------------- */

/* What lights a frame of the path queue.  rt_render* and the unlit forms above know nothing of it: their sky is
 * the reference's gradient and no sphere emits.  The struct is a HOST pointer read during the call.  `emission` is a DEVICE pointer in
 * the two _device forms and a HOST pointer in rt_render_wavefront_lit, which stages it like every host-buffer form. */
typedef struct {
    double sky_bottom[3];    /* sky colour where unit_vector(dir).y = -1;  the reference: (1, 1, 1)        */
    double sky_top[3];       /* ... where it is +1;                        the reference: (0.5, 0.7, 1.0)  */
    const double *emission;  /* [n_emission][3] radiance per uploaded sphere, list order; NULL: no lights  */
    int32_t n_emission;      /* the uploaded sphere count when emission != NULL, else 0                    */
    uint32_t flags;          /* 0                                                                          */
} rt_lighting;               /* 64 bytes */

/* One lit bounce.  Everything rt_paths_step_device promises holds (stable order, *out->count, d_rays, the count clamp, what `in` holds
 * afterwards, no launch slot, the NaN rule).  Two things differ:
 *  - a MISS adds quantize(throughput * sky) with ud = unit_vector(dir), t = 0.5 * (ud.y + 1.0), sky = sky_bottom * (1.0 - t) + sky_top * t:
 *    the operations and their order are those of the unlit step with the two constants replaced, so with the reference's two colours
 *    the result is that step's bit for bit;
 *  - a HIT on sphere s (its list index) reads e = emission[s] when emission is given.  s is a light iff e.x > 0 || e.y > 0 || e.z > 0 (a
 *    NaN or a non-positive channel compares false: every bit pattern has a meaning, the device forms validate no table).  On a light the
 *    path adds quantize(throughput * e) per channel to d_fix[pixel] (nothing when pixel >= npix; a negative or NaN channel of the product
 *    adds 0, one above RT_SAMPLE_CLAMP adds the clamp) and ENDS: it draws nothing from its stream, its material is not read, both faces
 *    emit.  A sphere that is not a light scatters exactly as in the unlit step.  Tie rule, t_min and NaN roots are the closest-hit
 *    scan's: a light is an ordinary sphere until the hit is known.
 * The frame forms are rt_render_wavefront*'s loop with the lit step: the same batches, the same context-owned queues, the same
 * RTIOW_WAVEFRONT_BATCH, no host wait; a path alive after max_depth steps adds nothing, one that reaches a light at step max_depth or
 * earlier adds.  With the reference's sky and no light the frame is rt_render_device's sums and ray count bit for bit.
 *
 * RT_ERR_INVALID_ARGUMENT, found before anything is touched: first every context-free check of the unlit form, in its order; then a NULL
 * light; light->flags != 0; a sky component that is not finite or is negative; emission == NULL with n_emission != 0; n_emission < 0;
 * in rt_render_wavefront_lit, which can see them, an emission entry that is NaN, infinite or negative; then the context checks of the
 * unlit form (NULL, scan mode, RT_ERR_NO_SCENE); then emission != NULL with n_emission different from the uploaded sphere count. */
int rt_paths_step_lit_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                             void *d_fix, int64_t npix, void *d_rays, const rt_lighting *light, void *stream);
int rt_render_wavefront_lit_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, void *d_fix, void *d_rays,
                                   void *stream);
int rt_render_wavefront_lit(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, uint64_t *fix,
                            uint64_t *rays_traced, float *kernel_ms);

/* ---- direct lighting: next-event estimation in the lit path queue -------------------------------------- */

/* Shadow rays towards the lights at Lambertian hits.  The light is sampled BY AREA: a uniform point of the
 * sphere from the rejection-sampled unit vector, so that pi cancels (Lambertian BRDF albedo / pi, area pdf 1 / (4 pi r^2)) and the
 * whole estimator is + - * / and one sqrt in binary64, without contraction: bit-exact like everything else here.
 *
 * RT_PATH_EVENT_DIRECT, bit 31 of a path's `event` word: the path's last scatter sampled the lights directly.  rt_paths_begin_device never
 * sets it; the NEE step reads it, masks it off before any Philox use, and writes it.  The unlit and lit steps know nothing of it: handed
 * a queue with the bit set they take it for part of the event and draw another Philox block. */
#define RT_PATH_EVENT_DIRECT 0x80000000u
/* the only legal step flag: the step neither samples lights nor sets the bit */
#define RT_STEP_NO_DIRECT 1u

typedef struct {
    const int32_t *lights;   /* [n_lights] sphere indices (list order of the upload); a DEVICE pointer in the _device forms */
    int32_t n_lights;
    uint32_t flags;          /* 0, RT_DIRECT_CONE, or RT_DIRECT_WEIGHTED | RT_DIRECT_CONE                                 */
} rt_direct;                 /* 16 bytes */
/* the bits of rt_direct.flags.  CONE: the light is sampled BY SOLID ANGLE, a uniform direction of the cone it subtends.  WEIGHTED, legal
 * only together with CONE: the light is CHOSEN by what it can contribute at the hit point, not uniformly (both below).  The legal values
 * are 0, 2 and 10. */
#define RT_DIRECT_CONE 2u
#define RT_DIRECT_WEIGHTED 8u

/* Pure host function: the indices s in [0, n_emission) with e.x > 0 || e.y > 0 || e.z > 0 for e = emission[s] (what the lit step takes
 * for a light), ascending, to lights_out (room for n_emission entries; may be NULL when n_emission is 0), their number to *n_lights_out.
 * RT_ERR_INVALID_ARGUMENT: n_emission < 0, a NULL output, emission or lights_out NULL with n_emission > 0. */
int rt_light_list(const double *emission, int32_t n_emission, int32_t *lights_out, int32_t *n_lights_out);

/* One NEE bounce: rt_paths_step_lit_device -- the same order, compaction, *out->count, d_rays and NaN rules -- except at two places.
 *  - a HIT on a light s: front = dot(dir, p - centre_s) < 0.0 with p = origin + dir * t.  A path that carries RT_PATH_EVENT_DIRECT and meets
 *    the front face ends and adds nothing (the previous hit's shadow ray counted that face); every other hit on a light adds
 *    quantize(throughput * e) as in the lit step.  A light's inner face is never sampled directly, so it always adds.
 *  - a HIT on a Lambertian sphere that is not a light, with n_lights > 0 and without RT_STEP_NO_DIRECT: the scatter runs first and
 *    unchanged (the same blocks, event, direction and albedo).  Then, with ev_in the path's event on entry (bit 31 masked off):
 *      b0 = philox(pixel, sample, ev_in, 1);  j = ((uint64)b0.x * n_lights) >> 32;  li = lights[j]
 *      (li outside [0, n_spheres) or outside the emission table: no contribution)
 *      unit-sphere tries (b0.y, b0.z, b0.w), then (x, y, z) of philox(pixel, sample, ev_in, 1 + m), m = 1, 2, ... until accepted
 *      u = unit_vector(u11 of the accepted try);  q = centre_li + u * sqrt(r2_li);  dv = q - p
 *      ns = dot(n, dv) (n: the record's normal);  nl = 0.0 - dot(u, dv);  dd = dot(dv, dv);  nothing unless ns > 0.0 && nl > 0.0
 *      w = ((4.0 * r2_li) * (double)n_lights) * ((ns * nl) / (dd * dd));  c = ((throughput * albedo) * e_li) * w
 *      the shadow ray (p, dv) with t_min and t_max = +inf: the light is visible iff its CLOSEST hit is sphere li (no epsilon);
 *      if visible and pixel < npix, d_fix[pixel] gains quantize(c).
 *    The path continues with event | RT_PATH_EVENT_DIRECT.  Every other scatter clears the bit.
 * With n_lights == 0 or RT_STEP_NO_DIRECT, on a queue without the bit, the step is rt_paths_step_lit_device byte for byte; with lights every
 * queue array and d_rays equal that step's except bit 31 of `event`, and the sums: NEE changes what is added, never where paths go.
 * d_shadow_rays (may be NULL): one device u64 that gains the number of shadow rays traced (atomic adds); d_rays counts path rays only.
 *
 * The frame forms run rt_render_wavefront_lit*'s loop with this step; step max_depth, the LAST of each batch, runs with
 * RT_STEP_NO_DIRECT (its shadow ray would stand for the lit frame's step max_depth + 1, which does not exist), so the NEE frame and the
 * lit frame have the same expectation at every max_depth.  *d_rays equals the lit frame's.  d_shadow_rays / shadow_rays (may be NULL) is
 * zeroed first.  rt_render_wavefront_nee builds the list itself with rt_light_list from the emission table it is given.
 *
 * RT_ERR_INVALID_ARGUMENT, found before anything is touched: first every context-free check of the lit form, in its order; then a NULL
 * direct; direct->flags other than 0, RT_DIRECT_CONE and RT_DIRECT_WEIGHTED | RT_DIRECT_CONE; n_lights < 0; lights == NULL with n_lights != 0; step_flags other than 0 or RT_STEP_NO_DIRECT; then the context
 * checks and the table's length as in the lit form; then n_lights > the uploaded sphere count. */
int rt_paths_step_nee_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                             void *d_fix, int64_t npix, void *d_rays, const rt_lighting *light, const rt_direct *direct, uint32_t step_flags,
                             void *d_shadow_rays, void *stream);
int rt_render_wavefront_nee_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_direct *direct,
                                   void *d_fix, void *d_rays, void *d_shadow_rays, void *stream);
int rt_render_wavefront_nee(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, uint64_t *fix,
                            uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms);

/* ---- direct lighting by solid angle --------------------------------------------- */

/* direct->flags == RT_DIRECT_CONE: the NEE step above in every respect -- the state bit, front-face suppression, when the bit is set
 * (decided before sampling; also when the sample yields nothing), RT_STEP_NO_DIRECT, the order and the compaction, d_rays, "visible iff
 * the closest hit is sphere li" -- except the light sample.  Area sampling weighs a sample with 4 r^2 n (ns nl) / dd^2, which is unbounded
 * as the hit point approaches the light, and throws away every sample of the far hemisphere; a uniform direction inside the cone the
 * sphere subtends has the weight 2 (1 - cos theta_max) n_lights ns <= 2 n_lights whatever the geometry.  It needs no sin or cos: one u01
 * for the polar angle and one rejection-sampled point of the unit disk, normalised, for (cos phi, sin phi); pi cancels (BRDF albedo / pi,
 * cone pdf 1 / (2 pi (1 - cos theta_max))).  With p, n and throughput * albedo as above, blocks philox(pixel, sample, ev_in, 1 + m),
 * everything binary64 without contraction in exactly this order:
 *    1. b0 = block 0;  j = ((uint64)b0.x * n_lights) >> 32;  li = lights[j]   (li outside the tables: no contribution)
 *    2. (c, r2) = geo[li];  wv = c - p;  d2 = (wv.x*wv.x + wv.y*wv.y) + wv.z*wv.z;  nothing unless d2 > r2 (p inside or on the light; NaN)
 *    3. q = r2 / d2;  cm = sqrt(1.0 - q);  k = q / (1.0 + cm)            (1 - cos theta_max without the cancellation)
 *    4. s = u01(b0.y) * k;  ct = 1.0 - s;  st = sqrt(s * (1.0 + ct))
 *    5. unit-disk tries (b0.z, b0.w), then (x, y) of block m = 1, 2, ... until accepted;  hx = u11(tx);  hy = u11(ty);
 *       il = 1.0 / sqrt(hx*hx + hy*hy);  cphi = hx * il;  sphi = hy * il   (the all-zero try gives NaNs, which step 9 drops)
 *    6. w = wv * (1.0 / sqrt(d2))
 *    7. a = fabs(w.x) > 0.9 ? (0, 1, 0) : (1, 0, 0);  t0 = cross(a, w) = (a.y*w.z - a.z*w.y, a.z*w.x - a.x*w.z, a.x*w.y - a.y*w.x);
 *       t = t0 * (1.0 / sqrt(dot(t0, t0)));  b = cross(w, t), the same form
 *    8. dir = (t * (st * cphi) + b * (st * sphi)) + w * ct
 *    9. ns = dot(n, dir);  nothing unless ns > 0.0
 *   10. wgt = ((2.0 * k) * (double)n_lights) * ns;  cadd = ((throughput * albedo) * e_li) * wgt
 *   11. the shadow ray (p, dir) with t_min and t_max = +inf: visible iff its closest hit is sphere li, either face; if visible and
 *       pixel < npix, d_fix[pixel] gains quantize(cadd).
 * d_shadow_rays counts these rays.  Every queue array and d_rays equal the area step's; only the sums and the shadow count differ.
 * rt_paths_step_nee_device and rt_render_wavefront_nee_device honour the bit through the rt_direct they take; direct->flags other than 0,
 * RT_DIRECT_CONE and RT_DIRECT_WEIGHTED | RT_DIRECT_CONE (below) is rejected where direct->flags != 0 was.  The host form takes no rt_direct, so it has a sibling:
 * rt_render_wavefront_nee_sampled is rt_render_wavefront_nee with direct_flags for the list it builds (0: that function bit for bit).
 * direct_flags other than those: RT_ERR_INVALID_ARGUMENT after the lit form's context-free checks and before the context. */
int rt_render_wavefront_nee_sampled(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, uint32_t direct_flags,
                                    uint64_t *fix, uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms);

/* ---- direct lighting with a weighted choice of the light ------------------------ */

/* direct->flags == (RT_DIRECT_WEIGHTED | RT_DIRECT_CONE), or that value as direct_flags of rt_render_wavefront_nee_sampled: the cone step
 * above in every respect -- the state bit, set before sampling and also when nothing is sampled; front-face suppression;
 * RT_STEP_NO_DIRECT; the order and the compaction; d_rays; "visible iff the closest hit is sphere li"; the blocks
 * philox(pixel, sample, ev_in, 1 + m); word y of block 0 as the polar draw and (z, w) as the first disk try; steps 2 to 9 and 11 for the
 * chosen light -- except steps 1 and 10.  The uniform choice is the dominant noise with many lights: most are far from a given hit point,
 * and the rare near one arrives with the weight 2 k n_lights ns.  Here light i is chosen with a probability proportional to
 * (r^2 / d^2) max(e), the solid angle it subtends at p (up to the factor the cone sample's k brings) times its largest channel: one
 * division per light, no sqrt, no table.  Binary64 without contraction, in exactly this order; p is the hit point:
 *   1a. for i = 0 .. n_lights - 1 in list order: s = lights[i]; s outside [0, n_spheres) or outside the emission table: imp_i = 0.
 *       Otherwise (c, r2) = geo[s];  wv = c - p;  d2 = (wv.x*wv.x + wv.y*wv.y) + wv.z*wv.z;  e = emission[s];
 *       em = max2(max2(e.x, e.y), e.z) with max2(a, b) = a > b ? a : b (a NaN on the left is dropped, one on the right is taken);
 *       v = (r2 / d2) * em;  imp_i = (d2 > r2 && v > 0.0) ? v : 0.0   (a NaN fails either test)
 *   1b. tot = ((0.0 + imp_0) + imp_1) + ..., adding only the imp_i > 0.0, in order.  !(tot > 0.0): no shadow ray, no contribution; the
 *       state bit is still set.
 *   1c. x = u01(b0.x) * tot.  The list is walked again, imp_i recomputed with the same expressions and summed into the same running sum
 *       acc;  j = the first i with imp_i > 0.0 && x < acc;  if none qualifies (x rounded up to tot), the last i with imp_i > 0.0;
 *       li = lights[j].
 *   10'. wgt = ((2.0 * k) * ns) * (tot / imp_j);  cadd = ((throughput * albedo) * e_li) * wgt
 * Consequences.  k <= r2 / d2 and e / em <= 1 per channel, so one light sample adds at most 2 * sum_i max(e_i) per unit of throughput,
 * whatever the geometry.  With a list of one valid light tot / imp_j is exactly 1.0, and the step and the frame are the cone step and
 * frame bit for bit: sums, queues, d_rays, the shadow count.  Every queue array and d_rays after a weighted step equal the cone step's;
 * only the sums and the shadow count differ.  A list entry that names no sphere, a sphere that does not emit, or a light that contains
 * p is never chosen, where the cone step chooses it and gets nothing.  The cost is two walks over the list per Lambertian hit.
 * RT_DIRECT_WEIGHTED alone (8), and every value other than 0, 2 and 10, is rejected where and how an unknown flag was. */

/* ---- wavefront frames over pixel lists, accumulated and adaptively sampled ------- */

/* rt_paths_begin_device over a LIST: slot k in [0, n) becomes item first_item + k of n_pixels listed pixels with spp samples each,
 * list-major: idx = item / spp, pixel = d_pixels[idx], sample = sample_begin + item % spp; origin, dir and event are rt_camera_rays' for
 * that (pixel, sample) over the FULL frame's width - 1, height - 1; throughput (1, 1, 1); *q->count = n.  Slots at or past n keep their
 * bytes.  d_pixels: device [n_pixels] u32 global pixel numbers g = j * width + i, any order, duplicates allowed.  A device list cannot be
 * validated on the host: a listed g >= width * height yields a path with that pixel word and the camera ray of (g % width, g / width), for
 * which the steps add nothing (their pixel >= npix rule); every bit pattern means something and nothing is read or written outside a
 * buffer.  Needs first_item + n <= n_pixels * spp.  RT_ERR_INVALID_ARGUMENT: rt_paths_begin_device's checks in their order, the items
 * measured against n_pixels * spp; then, still before the context, a NULL list with n_pixels != 0; then n_pixels outside [0, 2^31 - 1].
 * Needs no uploaded scene. */
int rt_paths_begin_pixels_device(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags, int32_t spp,
                                 int32_t sample_begin, int64_t first_item, int64_t n, const uint32_t *d_pixels, int64_t n_pixels,
                                 const rt_path_queue *q, void *stream);

/* The frame of rt_render_wavefront*_device for the listed pixels only, optionally ADDED to what the buffers hold: ONE driver for the
 * unlit, the lit and the NEE frame.  light == NULL: the unlit step (the reference's sky, no lights); direct == NULL: no direct lighting;
 * direct without light is rejected (light is NULL); direct->flags chooses the light sample as in rt_render_wavefront_nee_device.
 * d_pixels as above; d_pixels == NULL is the identity list 0, 1, ..., width * height - 1, and n_pixels must then be width * height: a
 * dense frame that can accumulate.  The n_pixels * spp items go in batches of RTIOW_WAVEFRONT_BATCH, per batch one begin over the list
 * and max_depth steps, the last with RT_STEP_NO_DIRECT, between the context's two queues; sample_begin is honoured; no host wait.
 *
 * d_fix is FRAME-ADDRESSED: [height][width][3] u64, and listed pixel g adds into entry g -- unlike rt_render_pixels_device, whose output
 * is COMPACT (entry k belongs to d_pixels[k]).  An entry of an unlisted pixel is zeroed or kept like the rest and gains nothing.  A
 * pixel listed m times receives its samples' sums m times.  A listed g >= width * height adds nothing and costs its rays, which
 * d_rays and d_shadow_rays count.  Sample s of listed pixel g is the sample the dense frame gives that pixel, and the sums are exact
 * integers: a list frame, a resumed frame and a dense frame of the same samples hold the same bits.
 *
 * p->flags: 0 or RT_FLAG_ACCUMULATE.  Without the flag d_fix (the whole frame), *d_rays and *d_shadow_rays are zeroed first; with it
 * nothing is zeroed and all three are added to.  n_pixels == 0 (with a list) succeeds and does nothing but that zeroing.
 *
 * RT_ERR_INVALID_ARGUMENT, found before anything is touched: the context-free checks of rt_render_wavefront_device in their order
 * (RT_FLAG_ACCUMULATE passes; every other flag and shard_count != 1 are rejected as there); with a light or a direct, the lighting checks
 * of the lit form; with a direct, the direct checks of the NEE form; then d_pixels == NULL with n_pixels != width * height; n_pixels
 * outside [0, 2^31 - 1]; in the host form a listed number >= width * height; then the context checks, the table's length and the list's
 * length as in the NEE form.
 *
 * The host form: light as in rt_render_wavefront_lit (emission a HOST pointer), or NULL; direct != 0 samples the lights of that table
 * (rt_light_list) with direct_flags as in rt_render_wavefront_nee_sampled (direct == 0: direct_flags must be 0, checked first); pixels: host
 * [n_pixels] u32 or NULL.  With RT_FLAG_ACCUMULATE fix, *rays_traced and *shadow_rays are copied in first and come back added to.
 * rays_traced, shadow_rays and kernel_ms may be NULL.  Synchronous. */
int rt_render_wavefront_pixels_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_direct *direct,
                                      const uint32_t *d_pixels, int64_t n_pixels, void *d_fix, void *d_rays, void *d_shadow_rays, void *stream);
int rt_render_wavefront_pixels(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, int32_t direct,
                               uint32_t direct_flags, const uint32_t *pixels, int64_t n_pixels, uint64_t *fix, uint64_t *rays_traced,
                               uint64_t *shadow_rays, float *kernel_ms);

/* rt_render_adaptive's loop and rule, unchanged, over the wavefront frame: the same rt_adaptive, the same rt_select_pixels_device, the
 * same out_fix / out_half / out_count (out_half holds the EVEN-numbered passes and may be NULL; a pixel that leaves the active set never
 * returns), one word of host read-back per round.  Round 1 renders every pixel; pass k of a later round renders samples
 * [n + k step, n + (k + 1) step) of the active list through the driver above.  light, direct and direct_flags as in
 * rt_render_wavefront_pixels.  rays_traced, shadow_rays (both summed over the passes) and kernel_ms (the rounds' device time, the
 * selections included) may be NULL.  The samples rendered are the sum of out_count.  Synchronous.
 *
 * RT_ERR_INVALID_ARGUMENT, before anything is touched: NULL cam, params, out_fix or out_count; the parameter and rt_adaptive validation
 * of rt_render_adaptive; sample_begin != 0; spp not a multiple of 2 * step, or > 32766; direct_flags != 0 with direct == 0; then flags != 0, shard_count != 1 and t_min as
 * in rt_render_wavefront; then the lighting and the direct checks as above; then the one rejection of its own: with direct lighting a
 * sample adds up to max_depth clamped terms of at most 2^48 each (max_depth - 1 light samples and one terminal term), so the selection's
 * signed differences need spp * max_depth * 2^48 < 2^63, and (int64)spp * max_depth > 32767 is rejected when direct != 0; then the
 * context checks. */
int rt_render_wavefront_adaptive(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_adaptive *a, const rt_lighting *light,
                                 int32_t direct, uint32_t direct_flags, uint64_t *out_fix, uint64_t *out_half, uint32_t *out_count,
                                 uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms);

/* ---- environment: a cube map the lit path queue looks up and importance-samples ---- */

/* Image-based lighting for the path queue: a fourth light source beside the sky and the emissive spheres.  A cube map, because a
 * latitude-longitude map needs atan2 and asin, for which the bit-exact contract has no statement: here the face is chosen by
 * comparisons and the texel by one division per coordinate, and a direction uniform over a texel's square has the solid-angle density
 * r^3 / A with r^2 = 1 + a^2 + b^2, so the lookup and the estimator are + - * / in binary64 with ONE stated constant for pi,
 * PI = 0x400921FB54442D18, and no sqrt per path.  rt_render*, the megakernel, and the unlit, lit and NEE forms know nothing of it.
 *
 * Faces: f = 2 * axis + (negative ? 1 : 0), axis 0 = x, 1 = y, 2 = z; the in-face coordinates (a, b) are the other two components in
 * axis order, divided by the magnitude of the face's own; texel (f, i, j) has the index k = (f * size + i) * size + j, i from a, j from b. */
#define RT_ENV_MAX_SIZE 1024
typedef struct {
    const double *texels;    /* [6][size][size][3] radiance; DEVICE pointer in the _device forms, HOST pointer in the host form        */
    const double *cdf;       /* [6*size*size] running sums from rt_environment_cdf, same residency; NULL: looked up, never sampled     */
    int32_t size;            /* texels per face edge: a power of two, 1 .. RT_ENV_MAX_SIZE                                             */
    uint32_t flags;          /* 0                                                                                                      */
} rt_environment;            /* 24 bytes */

/* LOOKUP env_lookup(d), for any d, not normalised:
 *   ax = 0, m = |d.x|;  if (|d.y| > m) ax = 1, m = |d.y|;  if (|d.z| > m) ax = 2, m = |d.z|      (strict: x wins ties over y, y over z; a
 *                                                                                                  NaN never wins)
 *   f = 2 * ax + (d[ax] < 0.0 ? 1 : 0);  (a, b) = the other two components in axis order, each divided by m
 *   x = ((a + 1.0) * 0.5) * (double)size;  i = x >= size ? size - 1 : (x >= 0.0 ? (int)x : 0);  j from b the same way   (a NaN gives 0)
 *   k = (f * size + i) * size + j
 * Every bit pattern of d -- zero, infinite and NaN directions included -- names a texel inside the table: no content sends a read
 * outside it, as with the emission table.
 *
 * TABLE: a pure host function.  s = 2.0 / (double)size; for texel k = (f, i, j): ac = ((double)i + 0.5) * s - 1.0, bc likewise from j,
 * r2 = (1.0 + ac * ac) + bc * bc; mx = the largest channel that compares > 0.0, else 0 (NaN and negative channels count as 0);
 * W = mx / (r2 * sqrt(r2)); cdf_out[k] = (k ? cdf_out[k - 1] : 0.0) + W, in index order.  A texel whose weight vanishes against the
 * running sum (below 2^-53 of it) repeats the entry before it and is never chosen.
 * RT_ERR_INVALID_ARGUMENT: a NULL pointer, a size that is not a power of two in [1, RT_ENV_MAX_SIZE]. */
int rt_environment_cdf(const double *texels, int32_t size, double *cdf_out);

/* One environment bounce.  Everything rt_paths_step_lit_device promises holds, with these differences.
 *  - a MISS adds quantize(throughput * texels[env_lookup(dir)]) per channel; the sky colours of `light` are validated and otherwise
 *    unused.  A path that carries RT_PATH_EVENT_DIRECT adds nothing on a miss: the previous hit's shadow ray already counted the
 *    environment.  The bit is read, masked off before any Philox use, and written, as in rt_paths_step_nee_device.
 *  - a HIT on a light always adds, as in the lit step: sphere lights are not sampled in this mode, so no face is suppressed.
 *  - a HIT on a Lambertian sphere that is not a light is SAMPLED when env->cdf != NULL, step_flags lacks RT_STEP_NO_DIRECT and
 *    tot = cdf[n - 1], n = 6 * size * size, satisfies tot > 0.0 && tot < inf.  The scatter runs first and unchanged; the path continues
 *    with event | RT_PATH_EVENT_DIRECT (decided before sampling: also when the sample yields nothing).  Then, with ev_in the masked
 *    event on entry:
 *      b = philox(pixel, sample, ev_in, 1)                                      (ONE block, no loop)
 *      x = u01(b.x) * tot
 *      lo = 0, hi = n - 1;  while (lo < hi) { mid = (lo + hi) >> 1;  if (cdf[mid] > x) hi = mid; else lo = mid + 1; }   k = lo
 *                                                        (the first entry above x; NaNs send the search right; it never leaves the table)
 *      P = (cdf[k] - (k ? cdf[k - 1] : 0.0)) / tot;  nothing follows unless P > 0.0
 *      (f, i, j) from k;  s = 2.0 / (double)size;  a = ((double)i + u01(b.y)) * s - 1.0;  b' = ((double)j + u01(b.z)) * s - 1.0
 *      dv: +-1.0 on the face's axis, (a, b') on the other two axes in axis order
 *      ns = dot(n, dv) (n: the record's normal);  dd = dot(dv, dv);  nothing follows unless ns > 0.0
 *      w = (ns * (s * s)) / ((PI * P) * (dd * dd));  c = ((throughput * albedo) * texels[k]) * w
 *      the shadow ray (p, dv) with t_min and t_max = +inf: visible iff the closest-hit scan finds NO sphere;
 *      if visible and pixel < npix, d_fix[pixel] gains quantize(c).
 *    For power-of-two sizes every step of a and b' is exact, so env_lookup(dv) == k -- except on the cube's edge: offset word 0 in row 0
 *    gives the coordinate -1.0, which ties with the face's own +-1.0, and the lookup's strict comparisons give a tie to the lower axis (one
 *    word in 2^32 per coordinate; the sample takes texels[k] and looks nothing up, so the estimator does not see it).
 *  - every other scatter clears the bit.
 * With cdf == NULL or RT_STEP_NO_DIRECT nothing is sampled and no bit is set; with sampling on, every queue array and d_rays after a step
 * equal the unsampled step's except bit 31 of `event`, and the sums.  d_shadow_rays (may be NULL) gains the shadow rays traced.
 *
 * The frame forms run rt_render_wavefront_lit*'s loop with this step, the LAST step of each batch with RT_STEP_NO_DIRECT; sample_begin
 * and RTIOW_WAVEFRONT_BATCH are honoured; d_shadow_rays / shadow_rays (may be NULL) is zeroed first.  The host form stages the texels
 * like every host buffer, ignores env->cdf, and with sample != 0 builds the table itself with rt_environment_cdf.
 *
 * RT_ERR_INVALID_ARGUMENT, found before anything is touched: first every context-free check of the lit form, in its order; then a NULL
 * env; env->flags != 0; a size that is not a power of two in [1, RT_ENV_MAX_SIZE]; NULL texels; a step flag other than 0 or
 * RT_STEP_NO_DIRECT; in the host form, which can see them, a texel that is NaN, infinite or negative; then the context checks and the
 * emission table's length as in the lit form. */
int rt_paths_step_env_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                             void *d_fix, int64_t npix, void *d_rays, const rt_lighting *light, const rt_environment *env, uint32_t step_flags,
                             void *d_shadow_rays, void *stream);
int rt_render_wavefront_env_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_environment *env,
                                   void *d_fix, void *d_rays, void *d_shadow_rays, void *stream);
int rt_render_wavefront_env(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_environment *env,
                            int32_t sample, uint64_t *fix, uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms);

/* ---- misc ------------------------------------------------------------------ */
const char *rt_last_error(void);
const char *rt_backend_name(void);     /* "hip-gfx950" */
int32_t rt_abi_version(void);
/* sha256 (first 16 hex digits) over the product kernel sources (csrc/rt_*.hpp, rt_api.hip) this library was BUILT from, as the build recorded it
 * ("unknown" for a build that did not pass it): bench.py labels its line with it, so that a stale .so shows */
const char *rt_build_source_sha(void);
/* Known-answer test hooks, computed ON THE DEVICE:
 * one Philox4x32-10 block; and elementwise a[i]/b[i] and sqrt(a[i]) in f64 (the
 * two operations whose correct rounding the bit-exact contract leans on). */
int rt_f64_div_sqrt_device(rt_context *ctx, const double *a, const double *b, int32_t n,
                           double *out_div, double *out_sqrt);
/* ... and the kernel's quantisation of one radiance channel to the exact 2^-32 grid (contract C5, DESIGN.md
 * section 4): out[i] = floor(min(x[i], RT_SAMPLE_CLAMP) * 2^32) for x[i] >= 0, and 0 for negatives and NaN. */
int rt_quantize_device(rt_context *ctx, const double *x, int32_t n, uint64_t *out);
/* ... and the kernel's rejection tests and word -> draw rules on n triples (wx, wy, wz) of Philox words: u01(w) = w * 2^-32 (draws
 * from [0,1)), u11(w) = (int32_t)w * 2^-31 (draws from (-1..1) and (-1..=1): the word as a two's-complement integer).  out_accept[k]
 * bit 0 = random_in_unit_sphere's `length_squared() < 1.0` (vec3.rs:37-45) for (u11(wx), u11(wy), u11(wz)), bit 1 =
 * random_in_unit_disk's (vec3.rs:59-68) for (u11(wx), u11(wy)), as the retry loops decide them (on the integers behind the draws,
 * with the f64 expression where its roundings could decide: DESIGN.md section 3); out_uniforms[k] = (u01(wx), u11(wx), u11(wy), u11(wz)). */
int rt_unit_accept_device(rt_context *ctx, const uint32_t *words, int32_t n, uint32_t *out_accept, double *out_uniforms);
/* Known-answer hooks of the EARLIER matrix-pipe forms of the filter (scan modes 2-4), and of the
 * shipped mode's tile-grid footprint (kept out of the product ABI).  They exist only in a library built with -DRTIOW_CROSSCHECK_MODES (tools/librtiow_hip_xcheck.so, a test
 * artefact); the product library carries scan modes 0, 1 and 5 and does not export them. */
#ifdef RTIOW_CROSSCHECK_MODES
/* The two K = 4 products of the scan filter exactly as the render
 * kernel's matrix-pipe tiles evaluate them: r1, r2: [64][4] ray rows, s: [16][4] sphere
 * columns, out_hb, out_q: [64][16].  bf16x3 != 0 selects the three-piece bf16 form. */
int rt_filter_products_device(rt_context *ctx, const float *r1, const float *r2, const float *s,
                               int32_t bf16x3, float *out_hb, float *out_q);
/* One tile of the single-contraction ("lifted") form of the same filter (scan mode 4):
 * o, d: [64][3] f64 rays; spheres16: 16 spheres (one tile of columns, built exactly as
 * rt_upload_scene builds them); out_D: [64][16] the sums whose sign the kernel tests;
 * out_R: [64][11] the per-ray terms (the last entry: 1 if the ray is inside the analysed range);
 * out_C: [16][11] the per-sphere terms. */
int rt_filter_lifted_device(rt_context *ctx, const double *o, const double *d, const rt_sphere *spheres16,
                            float *out_D, float *out_R, float *out_C);
/* The tile grid's footprint of the shipped scan mode (rt_device.hpp, grid_cells / grid_row_run) for n rays o + t d
 * (f64, [n][3]; rounded to f32 as the render kernel rounds them) on the grid `grid` (x0, z0, 1/cell, x1, z1, y lo,
 * y hi, pad: rt_tile_layout_host's out_grid) of grid_dim (1..63) cells per side, with error margins for `scale`.
 * out_rect: [n][5] = (verdict, ix0, nx, iz0, nz), verdict -1 cannot tell / 0 no cell / else nx * nz;
 * out_runs (or NULL): [n][63][2] = (rx0, rnx), the columns of row iz0 + k for k < nz, zeros beyond.
 * Fails when grid_cells with and without the row-by-row segment disagree on some ray. */
int rt_grid_cells_device(rt_context *ctx, const double *o, const double *d, int32_t n, const float grid[8], int32_t grid_dim,
                         float scale, int32_t *out_rect, int32_t *out_runs);
#endif /* RTIOW_CROSSCHECK_MODES */
/* One tile of the tube filter, the shipped scan mode: o, d: [64][3] f64 rays; spheres32: 32 spheres
 * (one tile of columns, built exactly as rt_upload_scene builds them, radius floor included);
 * out_h: [64][32][2] the two per-direction values H_k as the matrix pipe returns them, in units of HALF the
 * sphere's bound: the kernel keeps a (ray, sphere) pair iff |H_1| < 2 and |H_2| < 2 (it tests one bit of each);
 * out_bound[32]: the bound max(R, rho) each column was scaled with (sigma = 2 (1 - 2^-6) / bound, rounded down
 * to a bf16, is the value in K-slots 12..14 of the column); out_rows: [64][9] = (lambda u_1, lambda u_2, t_1, t_2,
 * 1 if the ray is inside the analysed range); out_rho: the radius floor chosen for these 32 spheres. */
int rt_filter_tube_device(rt_context *ctx, const double *o, const double *d, const rt_sphere *spheres32,
                          float *out_h, float *out_rows, float *out_bound, float *out_rho);
/* The host half of the same tile, no device needed: the 32 columns exactly as rt_upload_scene lays them
 * out.  out_words: [64][4] u32 = the B operand of lane l (column l&31, K-slots 8(l>>5)..+7, two bf16 per
 * word, low half first): slots 0..11 two bf16 pieces of sigma * centre per coordinate as (y1, y2, y1, y2),
 * slots 12..14 sigma, slot 15 zero (4.0 in a column no ray may keep); out_bound: [32]; out_rho: the radius floor. */
int rt_tube_tile_host(const rt_sphere *spheres32, uint32_t *out_words, float *out_bound, float *out_rho);
/* Where rt_upload_scene puts each sphere in the filter's table of columns, no device needed.  The table is made
 * of tiles of 32 columns: tiles [0, n_global) are scanned for every ray (spheres too large for a grid cell, and what
 * did not fit its cell's tile); tile n_global + iz * grid_dim + ix holds spheres whose centre lies in cell (ix, iz)
 * of a square grid over x and z.  out_dims = (grid_dim, n_global), grid_dim 0: no grid, columns in list order;
 * out_grid = (x0, z0, 1 / cell size, x1, z1, y lo, y hi, largest radius in a cell): every sphere of a cell tile has
 * its centre in that cell, its radius <= out_grid[7] and its extent in y within [out_grid[5], out_grid[6]];
 * out_slot_of[column] = the sphere's place in the list, -1 for padding.  Spheres on the always-exact list are in no
 * column.  Returns the number of columns (a multiple of 32, <= cap) or a negative RT_ERR_*. */
int rt_tile_layout_host(const rt_sphere *spheres, int32_t n, int32_t out_dims[2], float out_grid[8], int32_t *out_slot_of, int32_t cap);
int rt_philox_device(rt_context *ctx, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
