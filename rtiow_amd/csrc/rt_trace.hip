// rt_trace.hip -- ray queries: closest hit and occlusion for rays the CALLER supplies (rtiow_hip.h, "ray queries").
//
// The seventh translation unit of librtiow_hip.so.  It owns ONE kernel template of its own, rt::trace_kernel<RAY, ANY>: HittableList::hit
// (mod.rs:54-70) of every ray of a batch against the uploaded list, with a t_max per ray.  It reads the tables rt_upload_scene built
// (rt_host::set_scene_params); the first-hit scan is rt_first_hit.hpp, which the feature kernel of rt_features.hip shares.  rt_kernels.hpp,
// rt_device.hpp, rt_api.hip and rt_diag.hpp are untouched, so every render kernel keeps its machine code.  What only this kernel needs
// -- the `ray` scheme's cell set and per-ray keep bits -- lives here.
//
// Shape of the kernel: ray k is lane k & 63 of wave k >> 6, the waves stride over the batch; no work queue, no atomics on global memory.
// Per trip a wave loads its 64 rays, scans, and writes their answers.  WHICH tiles of 32 columns the tube filter runs over and WHO tests a
// kept column exactly is the candidate scheme (RAY):
//   wave  first_hit_wave, whole: the global tiles plus the bounding rectangle of the wave's footprints; the keep bits are ORed over
//         the wave and every lane tests every kept column, the sphere's record fetched through scalar loads.  Cheap for coherent batches.
//   ray   for incoherent batches, from the same pieces: the wave's CELL SET -- the union of the lanes' footprints, row by row (GridSeg / grid_row_run): one
//         64-bit mask on grids of at most 64 cells, one 64-bit word per grid row in LDS above --, and per-ray keep bits: a ray tests only its own candidates, in a loop that may diverge.
// The filter is conservative and the exact f64 test decides, so both give the same bytes.  ANY (occlusion): a lane with an accepted root
// goes idle and the wave leaves the tile loop when no lane is left.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "rt_host.hpp"
#ifdef RT_TRACE_COUNT
#define RT_SCAN_COUNT               // rt_first_hit.hpp: the scan's diagnostic counters (tools/trace_bench.py --counts)
#endif
#include "rt_first_hit.hpp"

using namespace rt_host;

namespace rt {

constexpr int kTraceBlock = 256;                    // four waves, each on batches of 64 rays of its own
constexpr int kTraceWaves = kTraceBlock / 64;

struct TraceArgs {
    const double *origin;           // [n][3]
    const double *dir;              // [n][3]
    const double *t_max;            // [n] or NULL (+inf)
    long long n;
    int32_t *index;                 // closest hit: [n]
    double *t, *point, *normal;     // closest hit: [n], [n][3], [n][3] or NULL
    uint8_t *front;                 // closest hit: [n] or NULL
    uint8_t *occluded;              // occlusion: [n]
};

// v_writelane_b32: lane `to` (wave-uniform) of the result is the wave-uniform `value`, every other lane keeps `old`.  Where the compiler
// offers __builtin_amdgcn_writelane it is used.  The one this was written with does not, so there its own intrinsic is declared through
// an assembler label carrying the intrinsic's overload-mangled name: a name that misses is an undefined symbol when the device code is
// linked, i.e. a failed build, never a wrong result, and tests/test_gpu_trace.py compares the `ray` scheme, which alone uses this, with the
// CPU reference bit for bit.  NOT inline assembly: an SGPR a VALU instruction has just written (the ballot) needs wait states before
// v_writelane may read it as data, and only the compiler's hazard recogniser inserts them.
#if defined(__has_builtin) && __has_builtin(__builtin_amdgcn_writelane)
__device__ __forceinline__ uint32_t write_lane(uint32_t value, int to, uint32_t old)
{
    return (uint32_t)__builtin_amdgcn_writelane((int)value, to, (int)old);
}
#else
extern "C" __device__ int rt_llvm_amdgcn_writelane(int, int, int) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ uint32_t write_lane(uint32_t value, int to, uint32_t old)
{
    return (uint32_t)rt_llvm_amdgcn_writelane((int)value, to, (int)old);
}
#endif

// a NaN result leaves as THE quiet NaN 0x7FF8000000000000: IEEE 754 leaves sign and payload of a generated NaN open and processors differ
__device__ __forceinline__ double canonical_nan(double x)
{
    return x != x ? __longlong_as_double(0x7FF8000000000000ll) : x;
}

template <bool RAY, bool ANY>
__global__ __launch_bounds__(kTraceBlock) void trace_kernel(const KParams P, const TraceArgs R)
{
    __shared__ uint4 s_stage[kTraceWaves][64 * 4];
    __shared__ unsigned long long s_rows[RAY ? kTraceWaves : 1][64];     // RAY: the wave's cell set, one word per grid row (grid_dim <= 63)
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    uint4 *stage = s_stage[wave];
    unsigned long long *rows = s_rows[RAY ? wave : 0];
    const int ntt = P.n_tiles >> 1;                     // tiles of 32 columns; the tables hold ntt + 1
    const int G = P.grid_dim;
    const long long n_trips = (R.n + 63) >> 6;
    const long long n_waves = (long long)gridDim.x * kTraceWaves;

    for (long long wv = (long long)blockIdx.x * kTraceWaves + wave; wv < n_trips; wv += n_waves) {
        const long long k = wv * 64 + lane;
        // lanes past the end of the batch stay in the wave: rows that keep nothing, nothing written
        const bool valid = k < R.n;
        D3 o = mk(0.0, 0.0, 0.0), d = mk(0.0, 0.0, 0.0);
        FirstHit fh = {__builtin_inf(), -1};            // mod.rs:56: closest_so_far = t_max
        if (valid) {
            o = mk(R.origin[3 * k], R.origin[3 * k + 1], R.origin[3 * k + 2]);
            d = mk(R.dir[3 * k], R.dir[3 * k + 1], R.dir[3 * k + 2]);
            if (R.t_max) fh.closest = R.t_max[k];
        }
        ScanCounts cnt = {true};

        // ---- HittableList::hit, mod.rs:54-70: the `wave` scheme whole, or the `ray` scheme -- the same pieces around a cell set and per-ray
        // keep bits.  (In the kernel's body, not a function of its own: compiled as one and then inlined, it took 131 vector registers instead
        // of 123, three waves per SIMD instead of four.)
        if constexpr (!RAY) {
            first_hit_wave<ANY>(P, stage, lane, o, d, valid, fh, cnt);
        } else {
            RayF32 rf;
            bf16x8 A[4];
            const bool sane = filter_rows(stage, lane, o, d, P.tube_rho, valid && fh.closest == fh.closest, rf, A);
            const double a = length_squared(d);                 // sphere.rs:20
            exact_prologue<ANY>(P, lane, o, d, a, sane, valid, fh, cnt);

            // one tile of 32 columns: the filter on the matrix pipe, then the exact tests of the kept (ray, column) pairs
            auto scan_tile = [&](int t) {
                f32x16 acc[4];
                if (filter_tile(P, t, lane, A, acc, cnt) == 0ull) return;
                // per-ray keep bits: the ballot of one accumulator pair IS the 32-column mask of two rays (lanes 0-31: ray 16 Gq + 8 bb + jj,
                // lanes 32-63: that ray + 4); v_writelane hands each to its owner.  32 ballots and 64 v_writelane per tile, no branch, no LDS
                // (one ds_or_b32 per kept pair under its own exec mask is 32 compare / saveexec / ds_or / restore groups: more instructions).
                uint32_t mine = 0u;
#pragma unroll
                for (int Gq = 0; Gq < 4; ++Gq)
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            const uint32_t h = __float_as_uint(acc[Gq][8 * bb + jj]) | __float_as_uint(acc[Gq][8 * bb + 4 + jj]);
                            const unsigned long long bal = __ballot((h & 0x40000000u) == 0u);
                            const int ray = 16 * Gq + 8 * bb + jj;
                            mine = write_lane((uint32_t)bal, ray, mine);
                            mine = write_lane((uint32_t)(bal >> 32), ray + 4, mine);
                        }
                // a ray tests only its own candidates (stand-in rows keep nothing: lanes without a ray in range have no bit)
                uint32_t cols = lane_live<ANY>(sane, fh) ? mine : 0u;
                while (cols != 0u) {
                    const int slot = 32 * t + __builtin_ctz(cols);
                    cols &= cols - 1u;
                    const uint32_t idx = P.slot_orig[slot];
                    if (idx == 0xFFFFFFFFu) continue;           // (padding: never kept by construction)
                    const double4 g = *reinterpret_cast<const double4 *>(P.geo_slot + 4 * (size_t)slot);
                    exact_any_order(fh, o, d, a, P.t_min, (int)idx, g.x, g.y, g.z, g.w, cnt);
                    if (ANY && fh.hit >= 0) break;
                }
            };

            // ---- which tiles: the global ones, and the wave's cell set -- the union of the lanes' footprints, row by row.  A grid of at most
            // 64 cells has it in ONE 64-bit mask (bit iz * G + ix), larger grids one word per grid row in LDS
            GridSeg seg;
            const Footprint f = wave_footprint(P, rf, sane, &seg);
            const bool one_mask = G * G <= 64;
            unsigned long long cell_mask = 0ull;
            if (f.all_tiles) {
            } else if (one_mask) {
                // the cell set in registers: a lane's runs (1 <= rnx, rx0 + rnx <= G <= 8) shifted to their rows, ORed over the wave
                unsigned long long own = 0ull;
                if (f.has)
                    for (int r = 0; r < f.nz; ++r) {
                        int rx0, rnx;
                        grid_row_run(seg, f.ix0, f.ix0 + f.nx - 1, (float)(f.iz0 + r), rx0, rnx);
                        own |= ((~0ull >> ((64 - rnx) & 63)) << (rx0 & 63)) << (((f.iz0 + r) * G) & 63);
                    }
                uint32_t lo = (uint32_t)own, hi = (uint32_t)(own >> 32);
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) { lo |= (uint32_t)__shfl_xor((int)lo, m, 64); hi |= (uint32_t)__shfl_xor((int)hi, m, 64); }
                cell_mask = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)hi) << 32) |
                            (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
            } else {
                // the cell set in LDS: every lane ORs the run of each row of its footprint into the row's word (1 <= rnx, rx0 + rnx <= G <= 63)
                rows[lane] = 0ull;
                __builtin_amdgcn_wave_barrier();            // LDS ops of one wave execute in order
                if (f.has)
                    for (int r = 0; r < f.nz; ++r) {
                        int rx0, rnx;
                        grid_row_run(seg, f.ix0, f.ix0 + f.nx - 1, (float)(f.iz0 + r), rx0, rnx);
                        atomicOr(&rows[(f.iz0 + r) & 63], (~0ull >> ((64 - rnx) & 63)) << (rx0 & 63));
                    }
                __builtin_amdgcn_wave_barrier();
            }
            if (f.all_tiles) {
                for (int t = 0; t < ntt && wave_live<ANY>(sane, fh); ++t) scan_tile(t);
            } else {
                for (int t = 0; t < P.n_global && t < ntt && wave_live<ANY>(sane, fh); ++t) scan_tile(t);
                while (cell_mask != 0ull && wave_live<ANY>(sane, fh)) {     // (a grid of at most 64 cells; else empty)
                    const int cell = __builtin_ctzll(cell_mask);
                    cell_mask &= cell_mask - 1ull;
                    const int t = P.n_global + cell;
                    if (cell < G * G && t < ntt) scan_tile(t);
                }
                for (int iz = f.z_lo; iz <= f.z_hi && !one_mask && wave_live<ANY>(sane, fh); ++iz) {
                    const unsigned long long rw = rows[iz & 63];            // (one address for the wave: a broadcast read)
                    unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(rw >> 32)) << 32) |
                                           (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rw);
                    while (m != 0ull && wave_live<ANY>(sane, fh)) {
                        const int ix = __builtin_ctzll(m);
                        m &= m - 1ull;
                        const int t = P.n_global + iz * G + ix;
                        if (ix < G && t < ntt) scan_tile(t);
                    }
                }
                if (!one_mask) __builtin_amdgcn_wave_barrier();             // the next trip's clear comes after this trip's reads
            }
        }

        // ---- the answer: sphere.rs:36-37 + mod.rs:20-30 for the winner
        if (valid) {
            if constexpr (ANY) {
                R.occluded[k] = fh.hit >= 0 ? (uint8_t)1 : (uint8_t)0;
            } else {
                HitRecord rec = {mk(0.0, 0.0, 0.0), mk(0.0, 0.0, 0.0), false, nullptr};
                if (fh.hit >= 0) rec = hit_record(P, o, d, fh);
                R.index[k] = fh.hit;
                if (R.t) R.t[k] = canonical_nan(fh.hit >= 0 ? fh.closest : __builtin_inf());
                if (R.point) {
                    R.point[3 * k] = canonical_nan(rec.p.x); R.point[3 * k + 1] = canonical_nan(rec.p.y); R.point[3 * k + 2] = canonical_nan(rec.p.z);
                }
                if (R.normal) {
                    R.normal[3 * k] = canonical_nan(rec.normal.x); R.normal[3 * k + 1] = canonical_nan(rec.normal.y);
                    R.normal[3 * k + 2] = canonical_nan(rec.normal.z);
                }
                if (R.front) R.front[k] = rec.front ? (uint8_t)1 : (uint8_t)0;
            }
        }
        flush_counts(cnt);
    }
}

} // namespace rt

namespace {

// the candidate scheme of a launch: RTIOW_TRACE_CANDIDATES=wave|ray (diagnostic, read per call); not set: kTraceDefaultRay
constexpr bool kTraceDefaultRay = true;
bool candidates_knob_ray()
{
    const char *e = getenv("RTIOW_TRACE_CANDIDATES");
    if (e && !strcmp(e, "wave")) return false;
    if (e && !strcmp(e, "ray")) return true;
    return kTraceDefaultRay;
}

// The start of every ray query.  What it accepts is checked before anything is touched: the checks that need no context come first (a
// caller without a device still gets the precise message), then the context's own; then the device.  `out`: hits->index or d_occluded.
// *go: there are rays to trace (an empty batch is RT_OK with nothing done).
int begin_trace(const rt_context *ctx, const char *what, const rt_rays *rays, double t_min, bool has_out_struct, const void *out, bool *go)
{
    *go = false;
    if (!rays) return fail(RT_ERR_INVALID_ARGUMENT, "%s: rays is NULL", what);
    if (!has_out_struct) return fail(RT_ERR_INVALID_ARGUMENT, "%s: hits is NULL", what);
    if (int rc = check_count(what, rays->n)) return rc;
    if (int rc = check_t_min(what, t_min)) return rc;
    if (rays->n > 0) {
        if (!rays->origin) return fail(RT_ERR_INVALID_ARGUMENT, "%s: rays->origin is NULL", what);
        if (!rays->dir) return fail(RT_ERR_INVALID_ARGUMENT, "%s: rays->dir is NULL", what);
        if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "%s: the required output (hits->index / occluded) is NULL", what);
    }
    if (int rc = check_context(ctx, what, true, true)) return rc;
    if (rays->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    *go = true;
    return RT_OK;
}

int launch_trace(rt_context *ctx, const rt_rays *rays, double t_min, const rt_hits *hits, void *d_occluded, hipStream_t stream)
{
    rt::KParams kp;
    memset(&kp, 0, sizeof(kp));
    kp.t_min = t_min;
    kp.n_spheres = ctx->n_spheres;
    set_scene_params(ctx, kp);
    // (no launch slot: the kernel has no work counter and no statistics words, and rt_last_stats does not report on it)
    rt::TraceArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.origin = rays->origin; ta.dir = rays->dir; ta.t_max = rays->t_max; ta.n = (long long)rays->n;
    if (hits) { ta.index = hits->index; ta.t = hits->t; ta.point = hits->point; ta.normal = hits->normal; ta.front = hits->front_face; }
    ta.occluded = (uint8_t *)d_occluded;
    // one wave per 64 rays; RTIOW_TRACE_GRID_BLOCKS: the diagnostic cap
    const long long grid = capped_grid("RTIOW_TRACE_GRID_BLOCKS", rt::wave_grid(((long long)rays->n + 63) / 64, rt::kTraceWaves));
    const bool ray = candidates_knob_ray(), any = hits == nullptr;
    const dim3 g((unsigned)grid), b(rt::kTraceBlock);
    if (ray && any) hipLaunchKernelGGL((rt::trace_kernel<true, true>), g, b, 0, stream, kp, ta);
    else if (ray) hipLaunchKernelGGL((rt::trace_kernel<true, false>), g, b, 0, stream, kp, ta);
    else if (any) hipLaunchKernelGGL((rt::trace_kernel<false, true>), g, b, 0, stream, kp, ta);
    else hipLaunchKernelGGL((rt::trace_kernel<false, false>), g, b, 0, stream, kp, ta);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// the host forms' common part: the three ray buffers, declared
struct StagedRays {
    Staged<const double> origin, dir, t_max;
};
StagedRays stage_rays(Stage &st, const rt_rays *rays)
{
    const size_t n = (size_t)rays->n;
    return {st.in(rays->origin, 3 * n), st.in(rays->dir, 3 * n), st.in(rays->t_max, n)};
}

} // namespace

extern "C" {

// HittableList::hit(ray, t_min, t_max[k]), mod.rs:54-70, of every ray of the batch
int rt_trace_rays_device(rt_context *ctx, const rt_rays *rays, double t_min, const rt_hits *hits, void *stream_v)
{
    bool go;
    int rc = begin_trace(ctx, "rt_trace_rays", rays, t_min, hits != nullptr, hits ? hits->index : nullptr, &go);
    if (rc || !go) return rc;
    return launch_trace(ctx, rays, t_min, hits, nullptr, (hipStream_t)stream_v);
}

int rt_trace_rays(rt_context *ctx, const rt_rays *rays, double t_min, const rt_hits *hits, float *kernel_ms)
{
    bool go;
    int rc = begin_trace(ctx, "rt_trace_rays", rays, t_min, hits != nullptr, hits ? hits->index : nullptr, &go);
    if (rc || !go) return rc;
    const size_t n = (size_t)rays->n;
    Stage st(ctx);
    const StagedRays sr = stage_rays(st, rays);
    const auto index = st.out(hits->index, n);
    const auto t = st.out(hits->t, n), point = st.out(hits->point, 3 * n), normal = st.out(hits->normal, 3 * n);
    const auto front = st.out(hits->front_face, n);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    const rt_rays dr = {st.ptr(sr.origin), st.ptr(sr.dir), st.ptr(sr.t_max), rays->n};
    const rt_hits dh = {st.ptr(index), st.ptr(t), st.ptr(point), st.ptr(normal), st.ptr(front)};
    return timed_section(ctx, "rt_trace_rays", kernel_ms, st, [&] { return rt_trace_rays_device(ctx, &dr, t_min, &dh, ctx->own_stream); });
}

int rt_occluded_device(rt_context *ctx, const rt_rays *rays, double t_min, void *d_occluded, void *stream_v)
{
    bool go;
    int rc = begin_trace(ctx, "rt_occluded", rays, t_min, true, d_occluded, &go);
    if (rc || !go) return rc;
    return launch_trace(ctx, rays, t_min, nullptr, d_occluded, (hipStream_t)stream_v);
}

int rt_occluded(rt_context *ctx, const rt_rays *rays, double t_min, uint8_t *occluded, float *kernel_ms)
{
    bool go;
    int rc = begin_trace(ctx, "rt_occluded", rays, t_min, true, occluded, &go);
    if (rc || !go) return rc;
    Stage st(ctx);
    const StagedRays sr = stage_rays(st, rays);
    const auto occ = st.out(occluded, (size_t)rays->n);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    const rt_rays dr = {st.ptr(sr.origin), st.ptr(sr.dir), st.ptr(sr.t_max), rays->n};
    return timed_section(ctx, "rt_occluded", kernel_ms, st, [&] { return rt_occluded_device(ctx, &dr, t_min, st.ptr(occ), ctx->own_stream); });
}

#ifdef RT_TRACE_COUNT
int rt_debug_trace_counts(rt_context *ctx, unsigned long long out[8]) { return rt::read_and_zero_counts(ctx, out); }
#endif

} // extern "C"
