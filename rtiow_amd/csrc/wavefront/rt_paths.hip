// rt_paths.hip -- the device path queue: a fused bounce step on device-resident paths and the frame rendered from it (rtiow_hip.h, "path
// queue").
//
// The eleventh translation unit of librtiow_hip.so.  Eleven kernels of its own:
//   path_begin_kernel     one lane per path, grid-stride: item -> (pixel, sample), the camera ray (sample_ray), throughput 1; *count = n.
//   path_begin_pixels_kernel  the same body (path_begin<LISTED>, stated once) over a list of pixels: item -> (list index, sample), the pixel
//                         read from the list (rtiow_hip.h, "wavefront frames over pixel lists").
//   pass_add_listed_kernel  rt_render_wavefront_adaptive's: an even pass's frame-addressed sums into fix and half at the listed pixels.
//   bounce_kernel         one wave per 64 consecutive slots, grid-stride over the live slots: closest hit (first_hit_wave<false> whole, the
//                         record in registers), then the sky add of a miss or Scatter::scatter -- both from rt_shade_core.hpp --; the new
//                         state is written IN PLACE, and per wave the number of survivors and their ballot go to the queue's scratch.
//   bounce_lit_kernel     the same trip (bounce_trip<MODE>, stated once) with the sky's two colours from its argument and emissive spheres: a hit
//                         on a sphere whose entry of the emission table has a channel > 0 adds throughput * e and ends the path (rtiow_hip.h,
//                         "lighting").
//   bounce_nee_kernel     the lit trip with next-event estimation: a Lambertian hit also samples one light by area and traces a shadow ray
//                         to it -- first_hit_wave<false> a second time in the trip, wave-wide -- (rtiow_hip.h, "direct lighting"; DESIGN.md
//                         section 21).
//   bounce_cone_kernel    the NEE trip with the light sampled by solid angle instead of by area (rtiow_hip.h, "direct lighting by solid
//                         angle").
//   bounce_weighted_kernel  the cone trip with the light chosen by its contribution at the hit point instead of uniformly (rtiow_hip.h,
//                         "direct lighting with a weighted choice").
//   bounce_env_kernel     the NEE trip with an environment cube map in the place of the sky and of the light list: a miss looks it up, a
//                         Lambertian hit samples it by its running sums and traces a shadow ray that must meet nothing (rtiow_hip.h,
//                         "environment").
//   queue_scan_kernel     ONE workgroup: the exclusive scan of the waves' counts, in place; *out->count; d_rays.
//   queue_compact_kernel  one wave per 64 slots: the survivors move to `out` at offset + rank, so their order is kept.
// The live count is a word of device memory every kernel reads for itself; the host sizes the grids from the capacity and never waits.
// NO kernel waits for another workgroup (no look-back chain, no flag, no grid-wide barrier): a wave that waits for a workgroup that has not
// been scheduled would hang, so the scan is a launch of its own, ordered by the stream.  No atomics except the three 64-bit adds of a miss or of a light hit.
// It composes rt_first_hit.hpp and rt_shade_core.hpp and restates none of their arithmetic; rt_kernels.hpp and rt_launch.hpp are not read.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_host.hpp"
#include "rt_adaptive_check.hpp"
#include "rt_env_core.hpp"
#include "rt_first_hit.hpp"
#include "rt_shade_core.hpp"

using namespace rt_host;

namespace rt {

constexpr int kPathBlock = 256;                     // four waves, each on 64 consecutive slots
constexpr int kPathWaves = kPathBlock / 64;
constexpr int kScanBlock = 1024;                    // the one workgroup of the scan
constexpr int kScratchPerWave = 3;                  // scratch words per 64 slots: [0] survivors, then their exclusive offset; [1], [2] the alive ballot

struct QueueArrays {
    uint32_t *count, *pixel, *sample, *event;
    double *origin, *dir, *thr;
    uint32_t *scratch;
    uint32_t capacity;
};

struct BeginArgs {
    long long n, first_item;
    uint32_t spp, sample_begin;
    int32_t width, height;
    uint32_t k0, k1;
};

// the live count as every kernel of a step reads it: the word in device memory, clamped to the capacity
__device__ __forceinline__ uint32_t live_count(const QueueArrays &Q)
{
    const uint32_t n = *Q.count;
    return n < Q.capacity ? n : Q.capacity;
}

// The body of the two begin kernels.  LISTED (rt_paths_begin_pixels_device): item -> (list index, sample), the pixel
// read from the list; else item -> (pixel, sample) and `pixels` is not looked at.  The host has checked first_item + n <= n_pixels * spp,
// so every read of `pixels` lies inside the list; the pixel word itself is not looked at: one at or past width * height gets the camera
// ray of (g % width, g / width) and adds nothing in the steps.
template <bool LISTED>
__device__ __forceinline__ void path_begin(const KCamera &cam, const QueueArrays &Q, const BeginArgs &A, const uint32_t *pixels)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *Q.count = (uint32_t)A.n;
    const double wm1 = (double)(A.width - 1), hm1 = (double)(A.height - 1);
    const long long stride = (long long)gridDim.x * kPathBlock;
    for (long long k = (long long)blockIdx.x * kPathBlock + threadIdx.x; k < A.n; k += stride) {
        const unsigned long long item = (unsigned long long)(A.first_item + k);
        const unsigned long long idx = item / A.spp;                    // pixel-major (list-major): item = pixel (index) * spp + sample
        uint32_t g_pix = (uint32_t)idx;
        if constexpr (LISTED) g_pix = pixels[idx];
        const uint32_t g_s = A.sample_begin + (uint32_t)(item - idx * A.spp);
        D3 origin, dir;
        const uint32_t ev = sample_ray(cam, (uint32_t)A.width, wm1, hm1, g_pix, g_s, A.k0, A.k1, origin, dir);
        Q.pixel[k] = g_pix; Q.sample[k] = g_s; Q.event[k] = ev;
        store3(Q.origin, k, origin);
        store3(Q.dir, k, dir);
        Q.thr[3 * k] = 1.0; Q.thr[3 * k + 1] = 1.0; Q.thr[3 * k + 2] = 1.0;
    }
}

__global__ __launch_bounds__(kPathBlock) void path_begin_kernel(const KCamera cam, const QueueArrays Q, const BeginArgs A)
{
    path_begin<false>(cam, Q, A, nullptr);
}

__global__ __launch_bounds__(kPathBlock) void path_begin_pixels_kernel(const KCamera cam, const QueueArrays Q, const BeginArgs A,
                                                                       const uint32_t *__restrict__ pixels)
{
    path_begin<true>(cam, Q, A, pixels);
}

// An even-numbered pass of rt_render_wavefront_adaptive, rendered into a frame-addressed pass buffer, back into the frame's state at the
// listed pixels (a selection's list: ascending, no duplicates, every entry inside the frame): fix += pass, half += pass, the entries read
// are zeroed for the next round, count += count_add (the round's two passes: the odd one goes straight into fix).
__global__ __launch_bounds__(256) void pass_add_listed_kernel(const uint32_t *__restrict__ list, uint32_t n_list, unsigned long long *__restrict__ pass,
                                                              unsigned long long *__restrict__ fix, unsigned long long *__restrict__ half,
                                                              uint32_t *__restrict__ count, uint32_t count_add, uint32_t npix)
{
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n_list; k += stride) {
        const size_t g = list[k];
        if (g >= (size_t)npix) continue;                                // (cannot happen; a store never leaves the frame whatever the list holds)
        for (int c = 0; c < 3; ++c) {
            const unsigned long long v = pass[g * 3u + c];
            pass[g * 3u + c] = 0ull;
            fix[g * 3u + c] += v;
            half[g * 3u + c] += v;
        }
        count[g] += count_add;
    }
}

// What a lit step knows beyond P (rtiow_hip.h, "lighting"): the two ends of the sky gradient and the per-sphere radiance
// table.  By value: the colours are wave-uniform and stay in scalar registers.  emission: [n_emission][3] device doubles or NULL.
struct LitArgs {
    double sky_bottom[3], sky_top[3];
    const double *emission;
    int32_t n_emission;
};

// What an NEE step knows beyond L (rtiow_hip.h, "direct lighting").  lights: [n_lights] device sphere indices;
// no_direct: RT_STEP_NO_DIRECT; shadow_rays: the device u64 that gains the shadow rays traced, or NULL.
struct NeeArgs {
    const int32_t *lights;
    unsigned long long *shadow_rays;
    int32_t n_lights;
    uint32_t no_direct;
};

// What an environment step knows beyond L and N (rtiow_hip.h, "environment"): the cube map's texels, [6][size][size][3]
// device doubles, and its sampling table, [6 size^2] running sums or NULL (looked up, never sampled).  Of N it reads no_direct and
// shadow_rays; there is no light list.
struct EnvArgs {
    const double *texels, *cdf;
    int32_t size;
};

// the three 64-bit adds of a path that ends with radiance v (contract C5); g_pix: inside the frame
__device__ __forceinline__ void add_sample(const KParams &P, uint32_t g_pix, const D3 &v)
{
    unsigned long long *px = P.fix + (size_t)g_pix * 3u;
    atomicAdd(px + 0, quantize(v.x)); atomicAdd(px + 1, quantize(v.y)); atomicAdd(px + 2, quantize(v.z));
}

// One trip of a wave over the 64 slots from 64 wv on: the body of the three bounce kernels.  MODE >= kLit: the sky's two colours come from
// L, and a hit on a sphere whose entry of L.emission has a channel > 0 adds throughput * e and ends the path before its material is read.
// MODE == kNee: the path's event carries RT_PATH_EVENT_DIRECT in bit 31 (masked off before any Philox use); a path that carries it adds
// nothing on a light's front face; a Lambertian hit samples one light of N.lights (nee_sample) and, after the new state has been stored,
// the wave traces the shadow rays together: only the contribution, the pixel and the light's index are live across that scan.
// MODE == kNeeCone: the same trip with the light sampled by solid angle (nee_sample_cone).
// MODE == kNeeWeighted: ... and chosen by its contribution at the hit point (nee_sample_weighted).
// MODE == kEnv: the NEE trip's shape with the environment E in the place of the sky and of the light list: a miss
// looks the map up unless the path carries the bit; a light always adds; a Lambertian hit samples the map (env_sample) when env_tot, the
// table's last entry as the wave read it, says there is something to sample; the shadow ray is visible iff it meets no sphere.
// The modes are rt_shade_core.hpp's, and so is the choice of the sampler among them (nee_sample_for<MODE>).
template <int MODE>
__device__ __forceinline__ void bounce_trip(const KParams &P, const QueueArrays &Q, const unsigned long long npix, const LitArgs &L, const NeeArgs &N,
                                            uint4 *stage, const int lane, const long long wv, const long long n, const EnvArgs &E = {},
                                            const double env_tot = 0.0)
{
    constexpr bool LIT = MODE >= kLit, NEE = MODE >= kNee, ENV = MODE == kEnv;
    const long long k = wv * 64 + lane;
    // lanes past the live count stay in the wave: rows that keep nothing, nothing written
    const bool valid = k < n;
    D3 o = mk(0.0, 0.0, 0.0), d = mk(0.0, 0.0, 0.0), thr = mk(0.0, 0.0, 0.0);
    uint32_t g_pix = 0u, g_s = 0u, ev = 0u;
    if (valid) {
        o = ld3(Q.origin + 3 * k); d = ld3(Q.dir + 3 * k); thr = ld3(Q.thr + 3 * k);
        g_pix = Q.pixel[k]; g_s = Q.sample[k]; ev = Q.event[k];
    }
    bool was_direct = false;
    if constexpr (NEE) { was_direct = (ev & RT_PATH_EVENT_DIRECT) != 0u; ev &= ~RT_PATH_EVENT_DIRECT; }
    FirstHit fh = {__builtin_inf(), -1};                // mod.rs:56: closest_so_far = t_max = +inf
    ScanCounts cnt = {true};
    first_hit_wave<false>(P, stage, lane, o, d, valid, fh, cnt);

    bool alive = false, shadow = false;
    D3 so = mk(0.0, 0.0, 0.0), sd = mk(0.0, 0.0, 0.0), sc = mk(0.0, 0.0, 0.0);
    int li = -1;
    if (valid) {
        if (fh.hit < 0) {
            // contract C5, as rt_accumulate with sky_dir: the path ends in the sky
            if ((unsigned long long)g_pix < npix) {
                if constexpr (ENV) {
                    // (a path that carries the bit: the previous hit's shadow ray already counted the environment)
                    if (!was_direct) add_sample(P, g_pix, thr * ld3(E.texels + 3 * (size_t)env_lookup(d, E.size)));
                } else if constexpr (LIT) add_sample(P, g_pix, sky_blend(thr, d, ld3(L.sky_bottom), ld3(L.sky_top)));
                else add_sample(P, g_pix, sky_sample(thr, d));
            }
        } else {
            bool light = false;
            if constexpr (LIT) {
                // (fh.hit < n_emission: no table content or count makes this read leave the table)
                if (L.emission && fh.hit < L.n_emission) {
                    const D3 e = ld3(L.emission + 3 * (size_t)fh.hit);
                    light = e.x > 0.0 || e.y > 0.0 || e.z > 0.0;    // a NaN or a non-positive channel compares false
                    bool adds = light && (unsigned long long)g_pix < npix;
                    // (NEE: the previous hit's shadow ray already counted a light's front face)
                    // (ENV: sphere lights are not sampled, so a light always adds)
                    if constexpr (NEE && !ENV) adds = adds && !(was_direct && light_front(P, o, d, fh.hit, fh.closest));
                    // both faces emit; no draw; the path ends; a pixel outside the frame adds nothing
                    if (adds) add_sample(P, g_pix, thr * e);
                }
            }
            if (!light) {
                const HitRecord rec = hit_record(P, o, d, fh);      // (in registers: never written to memory)
                D3 ndir, albedo;
                [[maybe_unused]] const uint32_t ev_in = ev;
                alive = !scatter_path(rec.mrec, d, rec.normal, rec.front, g_pix, g_s, ev, P.k0, P.k1, ndir, albedo);
                if (alive) {
                    bool direct = false;
                    if constexpr (ENV) direct = env_tot > 0.0 && (int)rec.mrec[5] == RT_KIND_LAMBERTIAN;
                    else if constexpr (NEE) direct = N.n_lights > 0 && !N.no_direct && (int)rec.mrec[5] == RT_KIND_LAMBERTIAN;
                    if (direct) ev |= RT_PATH_EVENT_DIRECT;
                    store3(Q.origin, k, rec.p);
                    store3(Q.dir, k, ndir);
                    store3(Q.thr, k, thr * albedo);
                    Q.event[k] = ev;
                    if constexpr (ENV) {
                        if (direct) {
                            shadow = env_sample(P, E.texels, E.cdf, E.size, env_tot, rec.normal, thr * albedo, g_pix, g_s, ev_in, sd, sc);
                            so = rec.p;
                        }
                    } else if constexpr (NEE) {
                        if (direct) {
                            shadow = nee_sample_for<MODE>(P, L.emission, L.n_emission, N.lights, N.n_lights, rec.p, rec.normal, thr * albedo, g_pix, g_s, ev_in, sd, sc, li);
                            so = rec.p;
                        }
                    }
                }
            }
        }
    }
    const unsigned long long live = __ballot(alive);
    if (lane == 0) {
        uint32_t *s = Q.scratch + kScratchPerWave * wv;
        s[0] = (uint32_t)__popcll(live); s[1] = (uint32_t)live; s[2] = (uint32_t)(live >> 32);
    }
    if constexpr (NEE) {
        // the shadow rays of the wave, traced together: idle lanes are rows that keep nothing; no lane branches around the scan
        const unsigned long long rays = __ballot(shadow);
        if (rays == 0ull) return;
        if (lane == 0 && N.shadow_rays) atomicAdd(N.shadow_rays, (unsigned long long)__popcll(rays));
        FirstHit sh = {__builtin_inf(), -1};
        ScanCounts scnt = {true};
        first_hit_wave<false>(P, stage, lane, so, sd, shadow, sh, scnt);
        // visible iff the CLOSEST hit is the sampled light itself: no epsilon (ENV: iff the scan finds no sphere)
        if (shadow && sh.hit == (ENV ? -1 : li) && (unsigned long long)g_pix < npix) add_sample(P, g_pix, sc);
    }
}

// the waves' grid-stride loop over the live slots, one trip per 64 of them: the same text in the three kernels, with the LDS stage a kernel's own
#define RT_BOUNCE_LOOP(MODE, L, N, ...) \
    __shared__ uint4 s_stage[kPathWaves][64 * 4]; \
    const int lane = (int)threadIdx.x & 63; \
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6); \
    uint4 *stage = s_stage[wave]; \
    const long long n = (long long)live_count(Q); \
    const long long n_trips = (n + 63) >> 6; \
    const long long n_waves = (long long)gridDim.x * kPathWaves; \
    for (long long wv = (long long)blockIdx.x * kPathWaves + wave; wv < n_trips; wv += n_waves) bounce_trip<MODE>(P, Q, npix, L, N, stage, lane, wv, n, ##__VA_ARGS__)

// One bounce of the live paths.  P: the scene's tables, t_min, the key (k0, k1) and the sums (fix); npix: entries of P.fix.
__global__ __launch_bounds__(kPathBlock) void bounce_kernel(const KParams P, const QueueArrays Q, const unsigned long long npix)
{
    const LitArgs none = {};
    const NeeArgs no_direct = {};
    RT_BOUNCE_LOOP(kUnlit, none, no_direct);
}

// ... with a settable sky and emissive spheres (rt_paths_step_lit_device)
__global__ __launch_bounds__(kPathBlock) void bounce_lit_kernel(const KParams P, const QueueArrays Q, const unsigned long long npix, const LitArgs L)
{
    const NeeArgs no_direct = {};
    RT_BOUNCE_LOOP(kLit, L, no_direct);
}

// ... and with next-event estimation at Lambertian hits (rt_paths_step_nee_device).  amdgpu_waves_per_eu(4): left to itself the compiler
// takes 129 vector registers, one more than occupancy 4 allows; told to fit it takes 111 and spills none.
__global__ __launch_bounds__(kPathBlock) __attribute__((amdgpu_waves_per_eu(4)))
void bounce_nee_kernel(const KParams P, const QueueArrays Q, const unsigned long long npix, const LitArgs L, const NeeArgs N)
{
    RT_BOUNCE_LOOP(kNee, L, N);
}

// ... with the light sampled by solid angle instead of by area (rt_direct.flags & RT_DIRECT_CONE): bounce_nee_kernel's
// shape, the sampler swapped.  (Defined here, not last: tools/isa_fingerprint.py counts the padding behind a translation unit's last kernel.)
__global__ __launch_bounds__(kPathBlock) __attribute__((amdgpu_waves_per_eu(4)))
void bounce_cone_kernel(const KParams P, const QueueArrays Q, const unsigned long long npix, const LitArgs L, const NeeArgs N)
{
    RT_BOUNCE_LOOP(kNeeCone, L, N);
}

// ... and with the light chosen by its contribution at the hit point (rt_direct.flags == RT_DIRECT_WEIGHTED | RT_DIRECT_CONE; DESIGN.md
// section 23): bounce_cone_kernel's shape, the sampler swapped.  (Defined here, not last, for bounce_cone_kernel's reason.)
__global__ __launch_bounds__(kPathBlock) __attribute__((amdgpu_waves_per_eu(4)))
void bounce_weighted_kernel(const KParams P, const QueueArrays Q, const unsigned long long npix, const LitArgs L, const NeeArgs N)
{
    RT_BOUNCE_LOOP(kNeeWeighted, L, N);
}

// ... with an environment cube map in the place of the sky, looked up on a miss and importance-sampled at Lambertian hits
// (rt_paths_step_env_device): bounce_nee_kernel's shape.  The table's last entry is read once per wave; a table
// that is absent, switched off by RT_STEP_NO_DIRECT, or whose total is not positive and finite samples nothing and sets no bit.
// (Defined here, not last, for bounce_cone_kernel's reason.)
__global__ __launch_bounds__(kPathBlock) __attribute__((amdgpu_waves_per_eu(4)))
void bounce_env_kernel(const KParams P, const QueueArrays Q, const unsigned long long npix, const LitArgs L, const NeeArgs N, const EnvArgs E)
{
    double tot = 0.0;
    if (E.cdf && !N.no_direct) tot = E.cdf[6 * E.size * E.size - 1];
    if (!(tot > 0.0 && tot < __builtin_inf())) tot = 0.0;
    RT_BOUNCE_LOOP(kEnv, L, N, E, tot);
}
#undef RT_BOUNCE_LOOP

// ONE workgroup: thread t owns a run of consecutive waves' counts; the threads' sums are scanned in LDS; the run is rewritten as offsets.
__global__ __launch_bounds__(kScanBlock) void queue_scan_kernel(const QueueArrays Q, uint32_t *out_count, unsigned long long *rays)
{
    __shared__ uint32_t s_sum[kScanBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t n = live_count(Q);
    const uint32_t n_trips = (n + 63u) >> 6;
    const uint32_t per = (n_trips + kScanBlock - 1u) / kScanBlock;
    const uint32_t lo = min(t * per, n_trips), hi = min(lo + per, n_trips);
    uint32_t sum = 0u;
    for (uint32_t w = lo; w < hi; ++w) sum += Q.scratch[kScratchPerWave * (size_t)w];
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t off = 1u; off < (uint32_t)kScanBlock; off <<= 1) {
        const uint32_t below = t >= off ? s_sum[t - off] : 0u;
        __syncthreads();
        s_sum[t] += below;
        __syncthreads();
    }
    uint32_t run = s_sum[t] - sum;
    for (uint32_t w = lo; w < hi; ++w) {
        const uint32_t c = Q.scratch[kScratchPerWave * (size_t)w];
        Q.scratch[kScratchPerWave * (size_t)w] = run;
        run += c;
    }
    if (t == 0u) {
        *out_count = s_sum[kScanBlock - 1];
        if (rays) *rays += (unsigned long long)n;
    }
}

// The survivors of `in` to `out` at offset + rank: stable.  offset + rank < the survivors' total <= the live count <= in.capacity <=
// out.capacity (checked on the host), so every store lies inside `out`.
__global__ __launch_bounds__(kPathBlock) void queue_compact_kernel(const QueueArrays In, const QueueArrays Out)
{
    const int lane = (int)threadIdx.x & 63;
    const long long wave = (long long)((int)threadIdx.x >> 6);
    const long long n_trips = ((long long)live_count(In) + 63) >> 6;
    const long long n_waves = (long long)gridDim.x * kPathWaves;
    for (long long wv = (long long)blockIdx.x * kPathWaves + wave; wv < n_trips; wv += n_waves) {
        const uint32_t *s = In.scratch + kScratchPerWave * wv;
        const unsigned long long live = ((unsigned long long)s[2] << 32) | (unsigned long long)s[1];
        if (((live >> lane) & 1ull) == 0ull) continue;
        const long long k = wv * 64 + lane;
        const long long to = (long long)s[0] + __popcll(live & ((1ull << lane) - 1ull));
        if (to >= (long long)Out.capacity) continue;    // (cannot happen; a store never leaves `out` whatever the scratch holds)
        Out.pixel[to] = In.pixel[k]; Out.sample[to] = In.sample[k]; Out.event[to] = In.event[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Out.origin[3 * to + c] = In.origin[3 * k + c]; Out.dir[3 * to + c] = In.dir[3 * k + c]; Out.thr[3 * to + c] = In.thr[3 * k + c];
        }
    }
}

} // namespace rt

namespace {

constexpr int64_t kMaxCapacity = (int64_t)1 << 24;
constexpr long long kDefaultBatch = 1ll << 20;

// RTIOW_PATHS_GRID_BLOCKS: the diagnostic cap on the kernels' grids; at least one workgroup
unsigned paths_grid(long long grid)
{
    grid = capped_grid("RTIOW_PATHS_GRID_BLOCKS", grid);
    return (unsigned)(grid < 1 ? 1 : grid);
}

// RTIOW_PATHS_STEP_PARTS=mask (diagnostic, read per call; tools/paths_bench.py times the kernels of a step one by one with it): which of
// a step's launches are issued -- 1 the bounce, 2 the scan, 4 the compaction; not set: all three
int step_parts()
{
    const char *e = getenv("RTIOW_PATHS_STEP_PARTS");
    const int v = e && *e ? atoi(e) : 0;
    return v > 0 ? v & 7 : 7;
}

const char *const kNoun = "the path queue";

int check_queue(const char *what, const char *name, const rt_path_queue *q)
{
    if (!q) return fail(RT_ERR_INVALID_ARGUMENT, "%s: %s is NULL", what, name);
    const void *arrays[8] = {q->count, q->pixel, q->sample, q->event, q->origin, q->dir, q->throughput, q->scratch};
    static const char *const field[8] = {"count", "pixel", "sample", "event", "origin", "dir", "throughput", "scratch"};
    for (int k = 0; k < 8; ++k)
        if (!arrays[k]) return fail(RT_ERR_INVALID_ARGUMENT, "%s: %s->%s is NULL", what, name, field[k]);
    if (q->capacity < 1 || q->capacity > kMaxCapacity)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: %s->capacity must be in [1, 2^24] (is %lld)", what, name, (long long)q->capacity);
    return RT_OK;
}

// the context-free part of the lighting checks, after the entry point's own; host_table: the emission is a host pointer the call may read
int check_light(const char *what, const rt_lighting *light, bool host_table)
{
    RT_NEED(light, what, "light");
    if (light->flags) return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown light->flags 0x%x (only 0 is legal)", what, light->flags);
    for (int c = 0; c < 3; ++c) {
        if (!(light->sky_bottom[c] >= 0.0) || !std::isfinite(light->sky_bottom[c]))
            return fail(RT_ERR_INVALID_ARGUMENT, "%s: light->sky_bottom[%d] must be finite and >= 0 (is %g)", what, c, light->sky_bottom[c]);
        if (!(light->sky_top[c] >= 0.0) || !std::isfinite(light->sky_top[c]))
            return fail(RT_ERR_INVALID_ARGUMENT, "%s: light->sky_top[%d] must be finite and >= 0 (is %g)", what, c, light->sky_top[c]);
    }
    if (!light->emission && light->n_emission != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: light->n_emission must be 0 when light->emission is NULL (is %d)", what, light->n_emission);
    if (light->n_emission < 0) return fail(RT_ERR_INVALID_ARGUMENT, "%s: light->n_emission must be >= 0 (is %d)", what, light->n_emission);
    if (host_table && light->emission)
        for (long long k = 0; k < 3ll * light->n_emission; ++k)
            if (!(light->emission[k] >= 0.0) || !std::isfinite(light->emission[k]))
                return fail(RT_ERR_INVALID_ARGUMENT, "%s: light->emission[%lld][%d] must be finite and >= 0 (is %g)", what, k / 3, (int)(k % 3),
                            light->emission[k]);
    return RT_OK;
}

// ... and the part that needs the uploaded scene: a table has one entry per sphere
int check_light_count(const rt_context *ctx, const char *what, const rt_lighting *light)
{
    if (light->emission && light->n_emission != ctx->n_spheres)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: light->n_emission (%d) must be the uploaded sphere count (%d)", what, light->n_emission, ctx->n_spheres);
    return RT_OK;
}

// What an NEE call has beyond a lit one; a NULL NeeCall: the call is none.  direct->lights: a device pointer.
struct NeeCall {
    const rt_direct *direct;
    uint32_t step_flags;
    void *d_shadow_rays;
};

// the context-free part of the direct-lighting checks, after the lighting's
int check_direct(const char *what, const NeeCall *nee)
{
    const rt_direct *direct = nee->direct;
    RT_NEED(direct, what, "direct");
    if (direct->flags != 0u && direct->flags != RT_DIRECT_CONE && direct->flags != (RT_DIRECT_WEIGHTED | RT_DIRECT_CONE))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown direct->flags 0x%x (only 0, RT_DIRECT_CONE and RT_DIRECT_WEIGHTED | RT_DIRECT_CONE are legal)", what,
                    direct->flags);
    if (direct->n_lights < 0) return fail(RT_ERR_INVALID_ARGUMENT, "%s: direct->n_lights must be >= 0 (is %d)", what, direct->n_lights);
    if (!direct->lights && direct->n_lights != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: direct->n_lights must be 0 when direct->lights is NULL (is %d)", what, direct->n_lights);
    if (nee->step_flags & ~RT_STEP_NO_DIRECT)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown step_flags 0x%x (only 0 and RT_STEP_NO_DIRECT are legal)", what, nee->step_flags);
    return RT_OK;
}

// ... and the part that needs the uploaded scene: a list names each sphere at most once
int check_direct_count(const rt_context *ctx, const char *what, const NeeCall *nee)
{
    if (nee->direct->n_lights > ctx->n_spheres)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: direct->n_lights (%d) must be <= the uploaded sphere count (%d)", what, nee->direct->n_lights,
                    ctx->n_spheres);
    return RT_OK;
}

// What an environment call has beyond a lit one; a NULL EnvCall: the call is none.  env->texels and env->cdf: device pointers.
struct EnvCall {
    const rt_environment *env;
    uint32_t step_flags;
    void *d_shadow_rays;
};

static_assert(RT_ENV_MAX_SIZE == rt_env::kMaxSize, "the pure header's limit is the ABI's");

// the context-free part of the environment checks, after the lighting's; host_texels: the texels are a host pointer the call may read
int check_env(const char *what, const EnvCall *call, bool host_texels)
{
    const rt_environment *env = call->env;
    RT_NEED(env, what, "env");
    if (env->flags) return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown env->flags 0x%x (only 0 is legal)", what, env->flags);
    if (!rt_env::valid_size(env->size))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: env->size must be a power of two in [1, %d] (is %d)", what, RT_ENV_MAX_SIZE, env->size);
    if (!env->texels) return fail(RT_ERR_INVALID_ARGUMENT, "%s: env->texels is NULL", what);
    if (call->step_flags & ~RT_STEP_NO_DIRECT)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown step_flags 0x%x (only 0 and RT_STEP_NO_DIRECT are legal)", what, call->step_flags);
    if (host_texels)
        for (size_t k = 0; k < 3 * rt_env::texel_count(env->size); ++k)
            if (!(env->texels[k] >= 0.0) || !std::isfinite(env->texels[k]))
                return fail(RT_ERR_INVALID_ARGUMENT, "%s: env->texels[%lld][%d] must be finite and >= 0 (is %g)", what, (long long)(k / 3), (int)(k % 3),
                            env->texels[k]);
    return RT_OK;
}

// A list of global pixel numbers as an entry point was handed it.  identity_ok: a NULL list stands for 0, 1, ...,
// width * height - 1 and n_pixels must be that many (the frame forms); else a NULL list must be empty (the begin).  host: the call may
// read the entries.
constexpr int64_t kMaxListed = 0x7fffffffLL;

struct PixelList {
    const uint32_t *pixels;
    int64_t n_pixels;
    bool identity_ok, host;
};

int check_list(const char *what, const PixelList &list, long long npix)
{
    if (!list.pixels && list.identity_ok && list.n_pixels != npix)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: n_pixels must be width * height = %lld when the list is NULL (is %lld)", what, npix, (long long)list.n_pixels);
    if (!list.pixels && !list.identity_ok && list.n_pixels != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: n_pixels must be 0 when the list is NULL (is %lld)", what, (long long)list.n_pixels);
    if (list.n_pixels < 0 || list.n_pixels > kMaxListed)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: n_pixels must be in [0, 2^31 - 1] (is %lld)", what, (long long)list.n_pixels);
    if (list.host && list.pixels)
        for (int64_t k = 0; k < list.n_pixels; ++k)
            if ((long long)list.pixels[k] >= npix)
                return fail(RT_ERR_INVALID_ARGUMENT, "%s: pixels[%lld] = %u lies outside the frame of %lld pixels", what, (long long)k, list.pixels[k], npix);
    return RT_OK;
}

// list: NULL for rt_paths_begin_device, whose items are the frame's; else the items are the list's
int check_begin(const rt_context *ctx, const char *what, const rt_camera *cam, int32_t width, int32_t height, uint32_t flags, int32_t spp,
                int32_t sample_begin, int64_t first_item, int64_t n, const rt_path_queue *q, const PixelList *list = nullptr)
{
    RT_NEED(cam, what, "cam");
    if (int rc = check_queue(what, "queue", q)) return rc;
    if (n < 0 || n > q->capacity)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: n must be in [0, capacity = %lld] (is %lld)", what, (long long)q->capacity, (long long)n);
    if (int rc = check_frame_dims(what, width, height)) return rc;
    if ((long long)width * height > 0x7fffffffLL)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: width * height does not fit the 32-bit Philox pixel counter", what);
    if (spp < 1 || sample_begin < 0 || (long long)spp + sample_begin > 0x7fffffffLL)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: spp must be >= 1, sample_begin >= 0 and spp + sample_begin <= 2^31 - 1 (are %d, %d)", what, spp, sample_begin);
    if (!list && (first_item < 0 || first_item + n > (long long)width * height * spp))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: the items [first_item, first_item + n) must lie in [0, width * height * spp) (first_item %lld, n %lld)",
                    what, (long long)first_item, (long long)n);
    // (a count outside [0, 2^31 - 1] has its own message below; inside it n_pixels * spp < 2^62)
    if (list && (first_item < 0 || (list->n_pixels >= 0 && list->n_pixels <= kMaxListed && first_item + n > list->n_pixels * spp)))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: the items [first_item, first_item + n) must lie in [0, n_pixels * spp) (first_item %lld, n %lld, n_pixels %lld)",
                    what, (long long)first_item, (long long)n, (long long)list->n_pixels);
    if (int rc = check_no_flags(what, flags, kNoun)) return rc;
    if (list)
        if (int rc = check_list(what, *list, (long long)width * height)) return rc;
    return check_context(ctx, what, true, false);
}

// light: NULL for the unlit step (lit: whether the call is a lit one); nee: NULL unless it is an NEE one; env: NULL unless it is an
// environment one
int check_step(const rt_context *ctx, const char *what, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out, const void *d_fix,
               int64_t npix, bool lit, const rt_lighting *light, const NeeCall *nee = nullptr, const EnvCall *env = nullptr)
{
    if (int rc = check_queue(what, "in", in)) return rc;
    if (int rc = check_queue(what, "out", out)) return rc;
    RT_NEED(d_fix, what, "d_fix");
    if (in == out) return fail(RT_ERR_INVALID_ARGUMENT, "%s: in and out must be distinct queues", what);
    const void *a[8] = {in->count, in->pixel, in->sample, in->event, in->origin, in->dir, in->throughput, in->scratch};
    const void *b[8] = {out->count, out->pixel, out->sample, out->event, out->origin, out->dir, out->throughput, out->scratch};
    for (const void *x : a)
        for (const void *y : b)
            if (x == y) return fail(RT_ERR_INVALID_ARGUMENT, "%s: in and out share an array", what);
    if (out->capacity < in->capacity)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: out->capacity (%lld) must be >= in->capacity (%lld)", what, (long long)out->capacity, (long long)in->capacity);
    if (int rc = check_npix(what, npix)) return rc;
    if (int rc = check_no_flags(what, flags, kNoun)) return rc;
    if (int rc = check_t_min(what, t_min)) return rc;
    if (lit)
        if (int rc = check_light(what, light, false)) return rc;
    if (nee)
        if (int rc = check_direct(what, nee)) return rc;
    if (env)
        if (int rc = check_env(what, env, false)) return rc;
    if (int rc = check_context(ctx, what, true, true)) return rc;
    if (lit)
        if (int rc = check_light_count(ctx, what, light)) return rc;
    return nee ? check_direct_count(ctx, what, nee) : RT_OK;
}

rt::QueueArrays arrays_of(const rt_path_queue *q)
{
    rt::QueueArrays a;
    a.count = q->count; a.pixel = q->pixel; a.sample = q->sample; a.event = q->event;
    a.origin = q->origin; a.dir = q->dir; a.thr = q->throughput; a.scratch = q->scratch; a.capacity = (uint32_t)q->capacity;
    return a;
}

// (validated arguments from here on)  d_pixels: NULL launches path_begin_kernel (the items are the frame's), else path_begin_pixels_kernel
int launch_begin(const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, int32_t spp, int32_t sample_begin, int64_t first_item, int64_t n,
                 const rt_path_queue *q, hipStream_t stream, const uint32_t *d_pixels = nullptr)
{
    rt::BeginArgs a;
    memset(&a, 0, sizeof(a));
    a.n = (long long)n; a.first_item = (long long)first_item; a.spp = (uint32_t)spp; a.sample_begin = (uint32_t)sample_begin;
    a.width = width; a.height = height; a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    // (at least one workgroup: an empty batch still writes the count)
    if (!d_pixels) hipLaunchKernelGGL(rt::path_begin_kernel, dim3(paths_grid(grid_256(a.n))), dim3(rt::kPathBlock), 0, stream, to_kcamera(cam), arrays_of(q), a);
    else hipLaunchKernelGGL(rt::path_begin_pixels_kernel, dim3(paths_grid(grid_256(a.n))), dim3(rt::kPathBlock), 0, stream, to_kcamera(cam), arrays_of(q), a, d_pixels);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// light: NULL launches bounce_kernel, else bounce_lit_kernel with the struct's values (light->emission: a device pointer), or with nee
// bounce_nee_kernel (or its cone or weighted sibling), or with env bounce_env_kernel
int launch_step(const rt_context *ctx, uint64_t seed, double t_min, const rt_path_queue *in, const rt_path_queue *out, void *d_fix, int64_t npix,
                void *d_rays, const rt_lighting *light, const NeeCall *nee, hipStream_t stream, const EnvCall *env = nullptr)
{
    rt::KParams kp;
    memset(&kp, 0, sizeof(kp));
    kp.t_min = t_min;
    kp.n_spheres = ctx->n_spheres;
    kp.k0 = (uint32_t)seed; kp.k1 = (uint32_t)(seed >> 32);
    kp.fix = (unsigned long long *)d_fix;
    set_scene_params(ctx, kp);
    const rt::QueueArrays qi = arrays_of(in), qo = arrays_of(out);
    // the grids come from the CAPACITY: the live count is the device's to know.  One wave per 64 slots; waves past the count leave at once.
    const dim3 grid(paths_grid(rt::wave_grid(((long long)in->capacity + 63) / 64, rt::kPathWaves))), block(rt::kPathBlock);
    const int parts = step_parts();
    if ((parts & 1) && !light) hipLaunchKernelGGL(rt::bounce_kernel, grid, block, 0, stream, kp, qi, (unsigned long long)npix);
    if ((parts & 1) && light) {
        rt::LitArgs la;
        memset(&la, 0, sizeof(la));
        memcpy(la.sky_bottom, light->sky_bottom, sizeof(la.sky_bottom));
        memcpy(la.sky_top, light->sky_top, sizeof(la.sky_top));
        la.emission = light->emission; la.n_emission = light->emission ? light->n_emission : 0;
        if (env) {
            rt::NeeArgs na;
            memset(&na, 0, sizeof(na));
            na.shadow_rays = (unsigned long long *)env->d_shadow_rays; na.no_direct = env->step_flags & RT_STEP_NO_DIRECT;
            rt::EnvArgs ea;
            memset(&ea, 0, sizeof(ea));
            ea.texels = env->env->texels; ea.cdf = env->env->cdf; ea.size = env->env->size;
            hipLaunchKernelGGL(rt::bounce_env_kernel, grid, block, 0, stream, kp, qi, (unsigned long long)npix, la, na, ea);
        } else if (nee) {
            rt::NeeArgs na;
            memset(&na, 0, sizeof(na));
            na.lights = nee->direct->lights; na.n_lights = nee->direct->lights ? nee->direct->n_lights : 0;
            na.shadow_rays = (unsigned long long *)nee->d_shadow_rays; na.no_direct = nee->step_flags & RT_STEP_NO_DIRECT;
            const uint32_t how = nee->direct->flags;    // (the three NEE kernels have one signature)
            const auto kernel = how & RT_DIRECT_WEIGHTED ? rt::bounce_weighted_kernel : how & RT_DIRECT_CONE ? rt::bounce_cone_kernel : rt::bounce_nee_kernel;
            hipLaunchKernelGGL(kernel, grid, block, 0, stream, kp, qi, (unsigned long long)npix, la, na);
        } else {
            hipLaunchKernelGGL(rt::bounce_lit_kernel, grid, block, 0, stream, kp, qi, (unsigned long long)npix, la);
        }
    }
    if (parts & 2) hipLaunchKernelGGL(rt::queue_scan_kernel, dim3(1), dim3(rt::kScanBlock), 0, stream, qi, out->count, (unsigned long long *)d_rays);
    if (parts & 4) hipLaunchKernelGGL(rt::queue_compact_kernel, grid, block, 0, stream, qi, qo);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// one context-owned queue of `capacity` slots laid out from `base` on (256-byte blocks, as the staging arena lays its own out)
struct OwnedQueues {
    StageLayout layout;
    size_t at[2][8];
    explicit OwnedQueues(int64_t capacity)
    {
        const size_t cap = (size_t)capacity, w32 = cap * sizeof(uint32_t), v3 = cap * 3 * sizeof(double);
        for (int k = 0; k < 2; ++k) {
            size_t *o = at[k];
            o[0] = layout.add(sizeof(uint32_t)); o[1] = layout.add(w32); o[2] = layout.add(w32); o[3] = layout.add(w32);
            o[4] = layout.add(v3); o[5] = layout.add(v3); o[6] = layout.add(v3);
            o[7] = layout.add((size_t)rt_path_scratch_words(capacity) * sizeof(uint32_t));
        }
    }
    rt_path_queue queue(void *base, int k, int64_t capacity) const
    {
        char *b = static_cast<char *>(base);
        const size_t *o = at[k];
        rt_path_queue q;
        q.capacity = capacity;
        q.count = (uint32_t *)(b + o[0]); q.pixel = (uint32_t *)(b + o[1]); q.sample = (uint32_t *)(b + o[2]); q.event = (uint32_t *)(b + o[3]);
        q.origin = (double *)(b + o[4]); q.dir = (double *)(b + o[5]); q.throughput = (double *)(b + o[6]); q.scratch = (uint32_t *)(b + o[7]);
        return q;
    }
};

// RTIOW_WAVEFRONT_BATCH (read per call): items per batch, default 2^20, in [1, 2^24]
long long batch_items()
{
    const char *e = getenv("RTIOW_WAVEFRONT_BATCH");
    long long v = e && *e ? atoll(e) : 0;
    if (v < 1) v = kDefaultBatch;
    return v > kMaxCapacity ? (long long)kMaxCapacity : v;
}

// the part of a frame's checks that every frame form has first; accumulate_ok: RT_FLAG_ACCUMULATE passes (the list forms)
int check_frame_params(const char *what, const rt_params *p, bool accumulate_ok)
{
    if (accumulate_ok && !(p->flags & RT_FLAG_UNIFORM53)) {
        if (p->flags & ~RT_FLAG_ACCUMULATE)
            return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x (only 0 and RT_FLAG_ACCUMULATE are legal)", what, p->flags);
    } else if (int rc = check_no_flags(what, p->flags, kNoun)) return rc;
    if (p->shard_count != 1) return fail(RT_ERR_INVALID_ARGUMENT, "%s: shard_count must be 1 (is %d)", what, p->shard_count);
    if (!std::isfinite(p->t_min)) return fail(RT_ERR_INVALID_ARGUMENT, "%s: t_min must be > 0 and finite (is %g)", what, p->t_min);
    return RT_OK;
}

// lit / light / host_table / nee as in check_step and check_light; list: the list forms' (RT_FLAG_ACCUMULATE passes), NULL for the others;
// extra: a check of the caller's own between the context-free ones and the context's (rt_render_wavefront_adaptive), or NULL;
// env / host_texels: as in check_step and check_env
int check_render(const rt_context *ctx, const char *what, const rt_camera *cam, const rt_params *p, const void *fix, bool lit = false,
                 const rt_lighting *light = nullptr, bool host_table = false, const NeeCall *nee = nullptr, const PixelList *list = nullptr,
                 int (*extra)(const char *, const rt_params *, bool) = nullptr, const EnvCall *env = nullptr, bool host_texels = false)
{
    RT_NEED(cam, what, "cam");
    RT_NEED(p, what, "params");
    RT_NEED(fix, what, "fix");
    if (int rc = validate_params(p)) return rc;
    if (int rc = check_frame_params(what, p, list != nullptr)) return rc;
    if (lit)
        if (int rc = check_light(what, light, host_table)) return rc;
    if (nee)
        if (int rc = check_direct(what, nee)) return rc;
    if (env)
        if (int rc = check_env(what, env, host_texels)) return rc;
    if (list)
        if (int rc = check_list(what, *list, (long long)p->width * p->height)) return rc;
    if (extra)
        if (int rc = extra(what, p, nee != nullptr)) return rc;
    if (int rc = check_context(ctx, what, true, true)) return rc;
    if (lit)
        if (int rc = check_light_count(ctx, what, light)) return rc;
    return nee ? check_direct_count(ctx, what, nee) : RT_OK;
}

// The frame of every device form (validated arguments): per batch one begin, then max_depth steps from one queue to the other; nothing
// here waits for the device.  (A step on an empty queue leaves at once; what the empty steps of a batch cost is in profiles/paths.txt.)
// nee: the frame's direct lighting (step_flags 0); the LAST step of a batch runs with RT_STEP_NO_DIRECT.
// d_pixels / n_pixels: the pixels whose samples are rendered -- NULL: all width * height of them, in order --;
// d_fix is frame-addressed either way.  p->flags & RT_FLAG_ACCUMULATE: nothing is zeroed, the sums and both counters are added to.
// env: the frame's environment (step_flags 0) in the place of nee, with the same rule for the last step.
int render_frame(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const NeeCall *nee, const uint32_t *d_pixels,
                 long long n_pixels, void *d_fix, void *d_rays, hipStream_t stream, const EnvCall *env = nullptr)
{
    const long long npix = (long long)p->width * p->height, total = n_pixels * p->spp;
    if (!(p->flags & RT_FLAG_ACCUMULATE)) {
        RT_HIP(hipMemsetAsync(d_fix, 0, (size_t)npix * 3 * sizeof(uint64_t), stream));
        if (d_rays) RT_HIP(hipMemsetAsync(d_rays, 0, sizeof(uint64_t), stream));
        if (nee && nee->d_shadow_rays) RT_HIP(hipMemsetAsync(nee->d_shadow_rays, 0, sizeof(uint64_t), stream));
        if (env && env->d_shadow_rays) RT_HIP(hipMemsetAsync(env->d_shadow_rays, 0, sizeof(uint64_t), stream));
    }
    if (total == 0) return RT_OK;
    const long long batch = batch_items() < total ? batch_items() : total;
    const OwnedQueues own(batch);
    if (int rc = ensure(ctx->paths, own.layout.total)) return rc;
    const rt_path_queue q[2] = {own.queue(ctx->paths.ptr, 0, batch), own.queue(ctx->paths.ptr, 1, batch)};
    NeeCall last = {};
    if (nee) { last = *nee; last.step_flags = RT_STEP_NO_DIRECT; }
    EnvCall last_env = {};
    if (env) { last_env = *env; last_env.step_flags = RT_STEP_NO_DIRECT; }
    for (long long first = 0; first < total; first += batch) {
        const long long n = total - first < batch ? total - first : batch;
        if (int rc = launch_begin(cam, p->width, p->height, p->seed, p->spp, p->sample_begin, first, n, &q[0], stream, d_pixels)) return rc;
        for (int depth = 0; depth < p->max_depth; ++depth) {
            const NeeCall *step_nee = nee && depth + 1 == p->max_depth ? &last : nee;
            const EnvCall *step_env = env && depth + 1 == p->max_depth ? &last_env : env;
            if (int rc = launch_step(ctx, p->seed, p->t_min, &q[depth & 1], &q[(depth + 1) & 1], d_fix, npix, d_rays, light, step_nee, stream, step_env)) return rc;
        }
    }
    return RT_OK;
}

// A host form's lighting on its way to the device (render_frame_host, rt_render_wavefront_adaptive): the caller's `light`, its table in host
// memory; direct: the frame samples its lights, their list (flags direct_flags) rebuilt from the table the call can see.  checked(): what
// check_render takes where a device form checks direct->flags.  declare(): on the caller's Stage before commit(), where the table and the
// list stand among its buffers.  resolve(): after upload(); then frame_light() and frame_nee() are what a device form takes, NULL for none.
struct HostLighting {
    const rt_lighting *const light;
    const bool lit, direct;
    const rt_direct no_list;
    const NeeCall flags_only;
    std::vector<int32_t> list;
    Staged<const double> emission;
    Staged<const int32_t> lights;
    rt_lighting dev = {};
    rt_direct on_device = {};
    NeeCall nee = {};

    HostLighting(const rt_lighting *light, bool lit, bool direct, uint32_t direct_flags)
        : light(light), lit(lit), direct(direct), no_list{nullptr, 0, direct_flags}, flags_only{&no_list, 0u, nullptr} {}
    HostLighting(const HostLighting &) = delete;        // (flags_only and nee point into the struct)

    const NeeCall *checked() const { return direct ? &flags_only : nullptr; }
    int declare(Stage &st)
    {
        const double *table = lit ? light->emission : nullptr;
        const size_t n_table = table ? (size_t)light->n_emission : 0;
        list.resize(direct ? n_table : 0);
        if (int rc = rt_light_list(table, (int32_t)list.size(), list.data(), &on_device.n_lights)) return rc;
        emission = st.in(table, n_table * 3);
        lights = st.in(static_cast<const int32_t *>(list.data()), (size_t)on_device.n_lights);
        return RT_OK;
    }
    // d_shadow_rays: the device u64 that gains the frame's shadow rays
    void resolve(const Stage &st, void *d_shadow_rays)
    {
        dev = lit ? *light : rt_lighting{};             // the same lighting with the table on the device
        dev.emission = st.ptr(emission);
        if (!dev.emission || !dev.n_emission) { dev.emission = nullptr; dev.n_emission = 0; }    // (a table of no entries lights nothing)
        on_device.lights = st.ptr(lights); on_device.flags = no_list.flags;
        if (!on_device.lights) on_device.n_lights = 0;
        nee = {&on_device, 0u, d_shadow_rays};
    }
    const rt_lighting *frame_light() const { return lit ? &dev : nullptr; }
    const NeeCall *frame_nee() const { return direct ? &nee : nullptr; }
};

// The body of the four host frames.  mode: kUnlit (light is not looked at), kLit, or kNee: the frame samples its lights directly, their
// list rebuilt from the table the call can see.  The counters are counted whether or not the caller asks; a frame without direct lighting
// has no shadow counter (shadow_rays NULL: absent).
// pixel_list: the list form's host list (rt_render_wavefront_pixels), NULL for the four dense frames; with it RT_FLAG_ACCUMULATE passes, and
// the sums and the counters the caller gave are then copied in first.
int render_frame_host(rt_context *ctx, const char *what, const rt_camera *cam, const rt_params *p, const rt_lighting *light, int mode, uint64_t *fix,
                      uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms, uint32_t direct_flags = 0u, const PixelList *pixel_list = nullptr)
{
    const bool lit = mode >= rt::kLit, direct = mode == rt::kNee;
    HostLighting lighting(light, lit, direct, direct_flags);
    if (int rc = check_render(ctx, what, cam, p, fix, lit, light, true, lighting.checked(), pixel_list)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    const bool adds = (p->flags & RT_FLAG_ACCUMULATE) != 0u;          // (only a list form gets here with the flag)
    const size_t n_sums = (size_t)p->width * p->height * 3;
    Stage st(ctx);
    const auto sums = adds ? st.inout(fix, n_sums) : st.out(fix, n_sums);
    const auto rays = !rays_traced ? st.scratch<uint64_t>(1) : adds ? st.inout(rays_traced, 1) : st.out(rays_traced, 1);
    const auto shadow = direct && !shadow_rays ? st.scratch<uint64_t>(1) : adds ? st.inout(shadow_rays, 1) : st.out(shadow_rays, 1);
    if (int rc = lighting.declare(st)) return rc;
    const auto pixels = st.in(pixel_list ? pixel_list->pixels : nullptr, pixel_list && pixel_list->pixels ? (size_t)pixel_list->n_pixels : 0);
    const long long n_pixels = pixel_list ? (long long)pixel_list->n_pixels : (long long)p->width * p->height;
    if (int rc = st.commit()) return rc;
    RT_HIP(st.upload());
    lighting.resolve(st, st.ptr(shadow));
    return timed_section(ctx, what, kernel_ms, st, [&] {
        return render_frame(ctx, cam, p, lighting.frame_light(), lighting.frame_nee(), st.ptr(pixels), n_pixels, st.ptr(sums), st.ptr(rays), ctx->own_stream);
    });
}

// rt_render_wavefront_adaptive's own rejection, between the context-free checks of the frame and the context's (check_render's `extra`)
int check_adaptive_terms(const char *what, const rt_params *p, bool direct)
{
    if (direct && (long long)p->spp * p->max_depth > 32767)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: with direct lighting a sample adds up to max_depth terms of at most 2^48, and the selection's signed "
                    "differences need spp * max_depth * 2^48 < 2^63: spp * max_depth must be <= 32767 (is %lld)", what, (long long)p->spp * p->max_depth);
    return RT_OK;
}

// a pair of events around each round of rt_render_wavefront_adaptive, destroyed on every path
struct RoundTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.0f;
    ~RoundTimer()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

} // namespace

extern "C" {

int64_t rt_path_scratch_words(int64_t capacity)
{
    if (capacity < 1 || capacity > kMaxCapacity) return 0;
    return rt::kScratchPerWave * ((capacity + 63) / 64);
}

int rt_paths_begin_device(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags, int32_t spp,
                          int32_t sample_begin, int64_t first_item, int64_t n, const rt_path_queue *q, void *stream_v)
{
    if (int rc = check_begin(ctx, "rt_paths_begin", cam, width, height, flags, spp, sample_begin, first_item, n, q)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_begin(cam, width, height, seed, spp, sample_begin, first_item, n, q, (hipStream_t)stream_v);
}

int rt_paths_step_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                         void *d_fix, int64_t npix, void *d_rays, void *stream_v)
{
    if (int rc = check_step(ctx, "rt_paths_step", flags, t_min, in, out, d_fix, npix, false, nullptr)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_step(ctx, seed, t_min, in, out, d_fix, npix, d_rays, nullptr, nullptr, (hipStream_t)stream_v);
}

int rt_paths_step_lit_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                             void *d_fix, int64_t npix, void *d_rays, const rt_lighting *light, void *stream_v)
{
    if (int rc = check_step(ctx, "rt_paths_step_lit", flags, t_min, in, out, d_fix, npix, true, light)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_step(ctx, seed, t_min, in, out, d_fix, npix, d_rays, light, nullptr, (hipStream_t)stream_v);
}

int rt_paths_step_nee_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                             void *d_fix, int64_t npix, void *d_rays, const rt_lighting *light, const rt_direct *direct, uint32_t step_flags,
                             void *d_shadow_rays, void *stream_v)
{
    const NeeCall nee = {direct, step_flags, d_shadow_rays};
    if (int rc = check_step(ctx, "rt_paths_step_nee", flags, t_min, in, out, d_fix, npix, true, light, &nee)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_step(ctx, seed, t_min, in, out, d_fix, npix, d_rays, light, &nee, (hipStream_t)stream_v);
}

int rt_environment_cdf(const double *texels, int32_t size, double *cdf_out)
{
    const char *what = "rt_environment_cdf";
    RT_NEED(texels, what, "texels");
    RT_NEED(cdf_out, what, "cdf_out");
    if (!rt_env::valid_size(size))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: size must be a power of two in [1, %d] (is %d)", what, RT_ENV_MAX_SIZE, size);
    rt_env::cdf(texels, size, cdf_out);
    return RT_OK;
}

int rt_paths_step_env_device(rt_context *ctx, uint64_t seed, uint32_t flags, double t_min, const rt_path_queue *in, const rt_path_queue *out,
                             void *d_fix, int64_t npix, void *d_rays, const rt_lighting *light, const rt_environment *env, uint32_t step_flags,
                             void *d_shadow_rays, void *stream_v)
{
    const EnvCall call = {env, step_flags, d_shadow_rays};
    if (int rc = check_step(ctx, "rt_paths_step_env", flags, t_min, in, out, d_fix, npix, true, light, nullptr, &call)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_step(ctx, seed, t_min, in, out, d_fix, npix, d_rays, light, nullptr, (hipStream_t)stream_v, &call);
}

int rt_render_wavefront_env_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_environment *env,
                                   void *d_fix, void *d_rays, void *d_shadow_rays, void *stream_v)
{
    const EnvCall call = {env, 0u, d_shadow_rays};
    if (int rc = check_render(ctx, "rt_render_wavefront_env", cam, p, d_fix, true, light, false, nullptr, nullptr, nullptr, &call, false)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return render_frame(ctx, cam, p, light, nullptr, nullptr, (long long)p->width * p->height, d_fix, d_rays, (hipStream_t)stream_v, &call);
}

// The host form: the emission table and the texels staged like every host buffer; sample != 0: the table built here with rt_env::cdf.
// The counters are counted whether or not the caller asks.
int rt_render_wavefront_env(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_environment *env,
                            int32_t sample, uint64_t *fix, uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms)
{
    const char *what = "rt_render_wavefront_env";
    const EnvCall given = {env, 0u, nullptr};
    if (int rc = check_render(ctx, what, cam, p, fix, true, light, true, nullptr, nullptr, nullptr, &given, true)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    HostLighting lighting(light, true, false, 0u);
    const size_t n_texels = rt_env::texel_count(env->size);
    std::vector<double> table(sample ? n_texels : 0);
    if (sample) rt_env::cdf(env->texels, env->size, table.data());
    Stage st(ctx);
    const auto sums = st.out(fix, (size_t)p->width * p->height * 3);
    const auto rays = rays_traced ? st.out(rays_traced, 1) : st.scratch<uint64_t>(1);
    const auto shadow = shadow_rays ? st.out(shadow_rays, 1) : st.scratch<uint64_t>(1);
    if (int rc = lighting.declare(st)) return rc;
    const auto texels = st.in(env->texels, n_texels * 3);
    const auto cdf = st.in(static_cast<const double *>(sample ? table.data() : nullptr), table.size());
    if (int rc = st.commit()) return rc;
    RT_HIP(st.upload());
    lighting.resolve(st, nullptr);
    rt_environment dev = *env;
    dev.texels = st.ptr(texels); dev.cdf = st.ptr(cdf);
    const EnvCall call = {&dev, 0u, st.ptr(shadow)};
    return timed_section(ctx, what, kernel_ms, st, [&] {
        return render_frame(ctx, cam, p, lighting.frame_light(), nullptr, nullptr, (long long)p->width * p->height, st.ptr(sums), st.ptr(rays),
                            ctx->own_stream, &call);
    });
}

int rt_render_wavefront_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, void *d_fix, void *d_rays, void *stream_v)
{
    if (int rc = check_render(ctx, "rt_render_wavefront", cam, p, d_fix)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return render_frame(ctx, cam, p, nullptr, nullptr, nullptr, (long long)p->width * p->height, d_fix, d_rays, (hipStream_t)stream_v);
}

int rt_render_wavefront_lit_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, void *d_fix, void *d_rays,
                                   void *stream_v)
{
    if (int rc = check_render(ctx, "rt_render_wavefront_lit", cam, p, d_fix, true, light, false)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return render_frame(ctx, cam, p, light, nullptr, nullptr, (long long)p->width * p->height, d_fix, d_rays, (hipStream_t)stream_v);
}

int rt_render_wavefront_nee_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_direct *direct,
                                   void *d_fix, void *d_rays, void *d_shadow_rays, void *stream_v)
{
    const NeeCall nee = {direct, 0u, d_shadow_rays};
    if (int rc = check_render(ctx, "rt_render_wavefront_nee", cam, p, d_fix, true, light, false, &nee)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    return render_frame(ctx, cam, p, light, &nee, nullptr, (long long)p->width * p->height, d_fix, d_rays, (hipStream_t)stream_v);
}

int rt_paths_begin_pixels_device(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags, int32_t spp,
                                 int32_t sample_begin, int64_t first_item, int64_t n, const uint32_t *d_pixels, int64_t n_pixels,
                                 const rt_path_queue *q, void *stream_v)
{
    const PixelList list = {d_pixels, n_pixels, false, false};
    if (int rc = check_begin(ctx, "rt_paths_begin_pixels", cam, width, height, flags, spp, sample_begin, first_item, n, q, &list)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    // (an empty list: n is 0, and the frame's kernel writes the count without a list to read)
    return launch_begin(cam, width, height, seed, spp, sample_begin, first_item, n, q, (hipStream_t)stream_v, d_pixels);
}

int rt_render_wavefront_pixels_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, const rt_direct *direct,
                                      const uint32_t *d_pixels, int64_t n_pixels, void *d_fix, void *d_rays, void *d_shadow_rays, void *stream_v)
{
    const char *what = "rt_render_wavefront_pixels";
    const NeeCall nee = {direct, 0u, d_shadow_rays};
    const PixelList list = {d_pixels, n_pixels, true, false};
    if (int rc = check_render(ctx, what, cam, p, d_fix, light || direct, light, false, direct ? &nee : nullptr, &list)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    // (a frame without direct lighting traces no shadow ray: its counter is zeroed like the others and gains nothing)
    if (!direct && d_shadow_rays && !(p->flags & RT_FLAG_ACCUMULATE)) RT_HIP(hipMemsetAsync(d_shadow_rays, 0, sizeof(uint64_t), stream));
    return render_frame(ctx, cam, p, light, direct ? &nee : nullptr, d_pixels, (long long)n_pixels, d_fix, d_rays, stream);
}

int rt_render_wavefront_pixels(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, int32_t direct,
                               uint32_t direct_flags, const uint32_t *pixels, int64_t n_pixels, uint64_t *fix, uint64_t *rays_traced,
                               uint64_t *shadow_rays, float *kernel_ms)
{
    const char *what = "rt_render_wavefront_pixels";
    const PixelList list = {pixels, n_pixels, true, true};
    const int mode = direct ? rt::kNee : light ? rt::kLit : rt::kUnlit;
    if (!direct && direct_flags)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: direct_flags must be 0 without direct lighting (is 0x%x)", what, direct_flags);
    const bool adds = p && (p->flags & RT_FLAG_ACCUMULATE);
    const int rc = render_frame_host(ctx, what, cam, p, light, mode, fix, rays_traced, direct ? shadow_rays : nullptr, kernel_ms, direct_flags, &list);
    if (!rc && !direct && shadow_rays && !adds) *shadow_rays = 0;
    return rc;
}

int rt_render_wavefront_adaptive(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_adaptive *a, const rt_lighting *light,
                                 int32_t direct, uint32_t direct_flags, uint64_t *out_fix, uint64_t *out_half, uint32_t *out_count,
                                 uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms)
{
    const char *what = "rt_render_wavefront_adaptive";
    RT_NEED(cam, what, "cam");
    RT_NEED(p, what, "params");
    RT_NEED(out_fix, what, "out_fix");
    RT_NEED(out_count, what, "out_count");
    if (int rc = validate_params(p)) return rc;
    if (int rc = validate_adaptive(a)) return rc;
    if (int rc = check_adaptive_frame(what, p, a)) return rc;
    if (!direct && direct_flags)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: direct_flags must be 0 without direct lighting (is 0x%x)", what, direct_flags);
    HostLighting lighting(light, light || direct, direct, direct_flags);
    if (int rc = check_render(ctx, what, cam, p, out_fix, lighting.lit, light, true, lighting.checked(), nullptr, check_adaptive_terms)) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->own_stream;
    // the frame's state, all on the device: fix | half | the even pass's frame-addressed sums | count | list | the two counters | the list's length
    const size_t npix = (size_t)p->width * p->height;
    uint64_t counters[2] = {0, 0};
    Stage st(ctx);
    const auto fix = st.out(out_fix, npix * 3);
    const auto half = out_half ? st.out(out_half, npix * 3) : st.scratch<uint64_t>(npix * 3);       // (the selection reads it either way)
    const auto pass = st.scratch<uint64_t>(npix * 3);
    const auto count = st.out(out_count, npix);
    const auto list = st.scratch<uint32_t>(npix);
    const auto totals = st.out(counters, 2);
    const auto length = st.scratch<uint32_t>(1);
    if (int rc = lighting.declare(st)) return rc;
    if (int rc = st.commit()) return rc;
    RT_HIP(st.upload());
    uint64_t *d_fix = st.ptr(fix), *d_half = st.ptr(half), *d_pass = st.ptr(pass), *d_totals = st.ptr(totals);
    uint32_t *d_count = st.ptr(count), *d_list = st.ptr(list), *d_n = st.ptr(length);
    lighting.resolve(st, d_totals + 1);
    const rt_lighting *frame_light = lighting.frame_light();
    const NeeCall *frame_nee = lighting.frame_nee();

    RoundTimer timer;
    RT_HIP(hipEventCreate(&timer.e0));
    RT_HIP(hipEventCreate(&timer.e1));
    const uint32_t step = (uint32_t)a->step;
    rt_params q = *p;
    q.spp = (int32_t)step;
    // round 1: every pixel.  Pass 0 -> fix (which zeroes it and both counters), a copy of it is `half`, pass 1 is added to fix.
    RT_HIP(hipEventRecord(timer.e0, stream));
    RT_HIP(hipMemsetAsync(d_totals, 0, sizeof(counters), stream));
    RT_HIP(hipMemsetAsync(d_pass, 0, npix * 3 * sizeof(uint64_t), stream));
    q.sample_begin = 0; q.flags = 0u;
    if (int rc = render_frame(ctx, cam, &q, frame_light, frame_nee, nullptr, (long long)npix, d_fix, d_totals, stream)) return rc;
    RT_HIP(hipMemcpyAsync(d_half, d_fix, npix * 3 * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    q.sample_begin = (int32_t)step; q.flags = RT_FLAG_ACCUMULATE;
    if (int rc = render_frame(ctx, cam, &q, frame_light, frame_nee, nullptr, (long long)npix, d_fix, d_totals, stream)) return rc;
    RT_HIP(hipMemsetD32Async((hipDeviceptr_t)d_count, (int)(2u * step), npix, stream));
    for (uint32_t n = 2u * step; ; n += 2u * step) {
        uint32_t n_list = 0;
        if (n < (uint32_t)p->spp) {
            if (int rc = rt_select_pixels_device(ctx, d_fix, d_half, d_count, p->width, p->height, (int32_t)n, a, d_list, d_n, stream)) return rc;
        }
        RT_HIP(hipEventRecord(timer.e1, stream));
        if (n < (uint32_t)p->spp) RT_HIP(hipMemcpyAsync(&n_list, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));    // the round's ONE word
        RT_HIP(st.sync());
        float ms = 0.0f;
        RT_HIP(hipEventElapsedTime(&ms, timer.e0, timer.e1));
        timer.ms += ms;
        if (n_list == 0u) break;
        RT_HIP(hipEventRecord(timer.e0, stream));
        // pass n / step (even) -> the pass buffer, then into fix and half at the listed pixels; pass n / step + 1 (odd) straight into fix:
        // `half` never sees it
        q.sample_begin = (int32_t)n;
        if (int rc = render_frame(ctx, cam, &q, frame_light, frame_nee, d_list, (long long)n_list, d_pass, d_totals, stream)) return rc;
        hipLaunchKernelGGL(rt::pass_add_listed_kernel, dim3(grid_256((long long)n_list)), dim3(256), 0, stream, (const uint32_t *)d_list, n_list,
                           (unsigned long long *)d_pass, (unsigned long long *)d_fix, (unsigned long long *)d_half, d_count, 2u * step, (uint32_t)npix);
        RT_HIP(hipGetLastError());
        q.sample_begin = (int32_t)(n + step);
        if (int rc = render_frame(ctx, cam, &q, frame_light, frame_nee, d_list, (long long)n_list, d_fix, d_totals, stream)) return rc;
    }
    RT_HIP(st.finish());                                // the sums, half if asked for, the counts and the two counters
    if (rays_traced) *rays_traced = counters[0];
    if (shadow_rays) *shadow_rays = counters[1];
    if (kernel_ms) *kernel_ms = timer.ms;
    return RT_OK;
}

int rt_light_list(const double *emission, int32_t n_emission, int32_t *lights_out, int32_t *n_lights_out)
{
    const char *what = "rt_light_list";
    if (n_emission < 0) return fail(RT_ERR_INVALID_ARGUMENT, "%s: n_emission must be >= 0 (is %d)", what, n_emission);
    RT_NEED(n_lights_out, what, "n_lights_out");
    if (n_emission > 0) {
        RT_NEED(emission, what, "emission");
        RT_NEED(lights_out, what, "lights_out");
    }
    int32_t n = 0;
    for (int32_t s = 0; s < n_emission; ++s) {
        const double *e = emission + 3 * (size_t)s;
        if (e[0] > 0.0 || e[1] > 0.0 || e[2] > 0.0) lights_out[n++] = s;       // what the lit step takes for a light
    }
    *n_lights_out = n;
    return RT_OK;
}

int rt_render_wavefront(rt_context *ctx, const rt_camera *cam, const rt_params *p, uint64_t *fix, uint64_t *rays_traced, float *kernel_ms)
{
    return render_frame_host(ctx, "rt_render_wavefront", cam, p, nullptr, rt::kUnlit, fix, rays_traced, nullptr, kernel_ms);
}

int rt_render_wavefront_lit(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, uint64_t *fix, uint64_t *rays_traced,
                            float *kernel_ms)
{
    return render_frame_host(ctx, "rt_render_wavefront_lit", cam, p, light, rt::kLit, fix, rays_traced, nullptr, kernel_ms);
}

int rt_render_wavefront_nee(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, uint64_t *fix, uint64_t *rays_traced,
                            uint64_t *shadow_rays, float *kernel_ms)
{
    return render_frame_host(ctx, "rt_render_wavefront_nee", cam, p, light, rt::kNee, fix, rays_traced, shadow_rays, kernel_ms);
}

int rt_render_wavefront_nee_sampled(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_lighting *light, uint32_t direct_flags,
                                    uint64_t *fix, uint64_t *rays_traced, uint64_t *shadow_rays, float *kernel_ms)
{
    return render_frame_host(ctx, "rt_render_wavefront_nee_sampled", cam, p, light, rt::kNee, fix, rays_traced, shadow_rays, kernel_ms, direct_flags);
}

} // extern "C"
