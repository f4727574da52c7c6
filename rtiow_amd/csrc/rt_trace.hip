// rt_trace.hip -- ray queries: closest hit and occlusion for rays the CALLER supplies (rtiow_hip.h, "ray queries").
//
// The seventh translation unit of librtiow_hip.so.  It owns ONE kernel template of its own, rt::trace_kernel<RAY, ANY>: HittableList::hit
// (mod.rs:54-70) of every ray of a batch against the uploaded list, with a t_max per ray.  It reads the tables rt_upload_scene built
// (rt_host::set_scene_params) and uses the building blocks of rt_device.hpp as rt_features.hip does; rt_kernels.hpp, rt_device.hpp,
// rt_api.hip and rt_diag.hpp are untouched, so every existing kernel keeps its machine code.  Helpers only this kernel needs live here.
//
// Shape of the kernel: ray k is lane k & 63 of wave k >> 6, the waves stride over the batch; no work queue, no atomics on global memory.
// Per trip a wave loads its 64 rays, builds their filter rows and runs the tube filter over tiles of 32 columns (four matrix instructions
// each).  WHICH tiles and WHO tests a kept column exactly is the candidate scheme (RAY):
//   wave  the feature kernel's scheme: the global tiles plus the bounding rectangle of the wave's footprints; the keep bits are ORed over
//         the wave and every lane tests every kept column, the sphere's record fetched through scalar loads.  Cheap for coherent batches.
//   ray   for incoherent batches: the wave's CELL SET -- the union of the lanes' footprints, row by row (GridSeg / grid_row_run): one
//         64-bit mask on grids of at most 64 cells, one 64-bit word per grid row in LDS above --, and per-ray keep bits: a ray tests only its own candidates, in a loop that may diverge.
// The filter is conservative and the exact f64 test decides, so both give the same bytes.  ANY (occlusion): a lane with an accepted root
// goes idle and the wave leaves the tile loop when no lane is left.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#define RT_RENDER_KERNEL_ONLY       // rt_kernels.hpp: KParams and the constants; rt_api.hip owns the kernels defined there
#include "rt_host.hpp"

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

// (rt_features.hip has the same helper; a wave-uniform address in the constant address space makes the compiler select scalar loads.
//  Legal because the scene's tables are written before the launch and only read during it.)
template <typename T>
__device__ __forceinline__ const T __attribute__((address_space(4))) *trace_uniform_ptr(const T *p)
{
    return (const T __attribute__((address_space(4))) *)(uintptr_t)p;
}

__device__ __forceinline__ int trace_wave_min(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int trace_wave_max(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

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

// RT_TRACE_COUNT (a diagnostic build, never the product: tools/trace_bench.py --counts).  Per launch: [0] wave trips, [1] tiles scanned,
// [2] exact tests run, as (lane, column) pairs, [3] lanes with a ray inside the analysed range, [4] pairs whose test reached a root >= t_min.
#ifdef RT_TRACE_COUNT
__device__ unsigned long long g_trace_counts[8];
#define RT_TRACE_CNT(k, n) (cnt[k] += (unsigned long long)(n))
#else
#define RT_TRACE_CNT(k, n) ((void)0)
#endif

template <bool RAY, bool ANY>
__global__ __launch_bounds__(kTraceBlock) void trace_kernel(const KParams P, const TraceArgs R)
{
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    __shared__ uint4 s_stage[kTraceWaves][64 * 4];
    __shared__ unsigned long long s_rows[RAY ? kTraceWaves : 1][64];     // RAY: the wave's cell set, one word per grid row (grid_dim <= 63)
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    uint4 *stage = s_stage[wave];
    unsigned long long *rows = s_rows[RAY ? wave : 0];
    const int ntt = P.n_tiles >> 1;                     // tiles of 32 columns; the tables hold ntt + 1
    const int n = P.n_spheres;
    const int G = P.grid_dim;
    const double t_min = P.t_min;
    const double *__restrict__ geo = P.geo;
    const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long n_trips = (R.n + 63) >> 6;
    const long long n_waves = (long long)gridDim.x * kTraceWaves;

    for (long long wv = (long long)blockIdx.x * kTraceWaves + wave; wv < n_trips; wv += n_waves) {
        const long long k = wv * 64 + lane;
        // lanes past the end of the batch stay in the wave: rows that keep nothing, nothing written
        const bool valid = k < R.n;
        D3 o = mk(0.0, 0.0, 0.0), d = mk(0.0, 0.0, 0.0);
        double closest = __builtin_inf();               // mod.rs:56: closest_so_far = t_max
        if (valid) {
            o = mk(R.origin[3 * k], R.origin[3 * k + 1], R.origin[3 * k + 2]);
            d = mk(R.dir[3 * k], R.dir[3 * k + 1], R.dir[3 * k + 2]);
            if (R.t_max) closest = R.t_max[k];
        }
#ifdef RT_TRACE_COUNT
        unsigned long long cnt[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
#endif

        // ---- the filter rows of the wave's 64 rays
        float ray_of[3], ray_df[3], ray_o1;
        ray_f32(o, d, ray_of, ray_df, ray_o1);
        TubeRay T = make_tube<false>(ray_of, ray_df, ray_o1, P.tube_rho);
        // inside the filter's analysed range, and a t_max that compares: the order-independent form below is the loop as written
        const bool sane = valid && T.sane && closest == closest;
        if (!sane) tube_rows_keep_nothing(T);
        bf16x8 A[4];
        {
            uint32_t w[2][8];
            tube_a_words(T, w);
            tube_stage_operands(stage, lane, w, A);
        }

        int hit = -1;
        const double a = length_squared(d);                 // sphere.rs:20
        // sphere.rs:16-34 + mod.rs:61-67 in the order-independent form of the render and feature kernels: a sphere's root r* is the near
        // one if >= t_min, else the far one; the smallest r* <= t_max wins, among equal roots the LATER sphere of the list (hit starts at
        // -1: a root equal to t_max is accepted)
        auto exact_any_order = [&](int idx, double gx, double gy, double gz, double r2) {
            RT_TRACE_CNT(2, 1);
            const D3 oc = o - mk(gx, gy, gz);
            const double half_b = dot(oc, d);
            const double c = length_squared(oc) - r2;
            const double disc = half_b * half_b - a * c;
            if (disc < 0.0) return;                         // sphere.rs:25
            if (half_b > 0.0 && c > 0.0) return;            // origin outside, sphere behind the ray: both roots <= 0 < t_min
            const double sqrtd = __builtin_sqrt(disc);
            double root = (-half_b - sqrtd) / a;
            if (root < t_min) {
                root = (-half_b + sqrtd) / a;
                if (root < t_min) return;
            }
            RT_TRACE_CNT(4, 1);
            if (root < closest || (root == closest && idx > hit)) { closest = root; hit = idx; }
        };
        // ... and as written, for a visit in LIST order (a NaN root or a NaN t_max fails neither comparison and is accepted)
        auto exact_in_order = [&](int idx) {
            const double4 g = *reinterpret_cast<const double4 *>(geo + 4 * (size_t)idx);
            const D3 oc = o - mk(g.x, g.y, g.z);
            const double half_b = dot(oc, d);
            const double c = length_squared(oc) - g.w;
            const double disc = half_b * half_b - a * c;
            if (disc < 0.0) return;
            const double sq = __builtin_sqrt(disc);
            double r = (-half_b - sq) / a;                  // sphere.rs:28-34
            if (r < t_min || closest < r) {
                r = (-half_b + sq) / a;
                if (r < t_min || closest < r) return;
            }
            closest = r;                                    // mod.rs:63-64
            hit = idx;
        };

        if (sane) {
            // the spheres that skip the filter (the ground): tested exactly by every ray
            for (int e = 0; e < P.n_always; ++e) {
                const int idx = P.always_idx[e];
                const double4 g = *reinterpret_cast<const double4 *>(geo + 4 * (size_t)idx);
                exact_any_order(idx, g.x, g.y, g.z, g.w);
            }
        } else if (valid) {
            // outside the analysed range: the whole list in list order, as written (occlusion: up to the first accepted root)
            for (int s = 0; s < n && !(ANY && hit >= 0); ++s) exact_in_order(s);
        }

        // occlusion: a lane with an accepted root is idle; the wave goes on while a lane is left
        auto lane_live = [&]() { return sane && !(ANY && hit >= 0); };
        auto wave_live = [&]() { return !ANY || __ballot(lane_live()) != 0ull; };

        // one tile of 32 columns: the filter on the matrix pipe, then the exact tests of the kept (ray, column) pairs
        auto scan_tile = [&](int t) {
            if (lane == 0) RT_TRACE_CNT(1, 1);
            const bf16x8 b = __builtin_bit_cast(bf16x8, P.btube[(size_t)t * 64 + lane]);
            // acc[8 bb + jj] / acc[8 bb + 4 + jj]: H_1 / H_2 of ray 16 Gq + 8 bb + 4 (lane >> 5) + jj against column lane & 31; the pair is
            // kept iff |H_1| < 2 and |H_2| < 2, i.e. iff bit 30 of both f32 patterns is clear (rt_features.hip, scan_tile)
            f32x16 acc[4];
            uint32_t X = 0xFFFFFFFFu;
#pragma unroll
            for (int Gq = 0; Gq < 4; ++Gq) {
                acc[Gq] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[Gq], b, zero16, 0, 0, 0);
#pragma unroll
                for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) X &= __float_as_uint(acc[Gq][8 * bb + jj]) | __float_as_uint(acc[Gq][8 * bb + 4 + jj]);
            }
            const unsigned long long kept = __ballot((X & 0x40000000u) == 0u);      // two lanes per column
            if (kept == 0ull) return;
            if constexpr (!RAY) {
                // every lane tests every column some ray keeps; the sphere is wave-uniform: its records come through scalar loads
                uint32_t cols = (uint32_t)kept | (uint32_t)(kept >> 32);
                while (cols != 0u) {
                    const int slot = 32 * t + __builtin_ctz(cols);
                    cols &= cols - 1u;
                    const uint32_t idx = trace_uniform_ptr(P.slot_orig)[slot];
                    if (idx == 0xFFFFFFFFu) continue;           // (padding: never kept by construction)
                    const double __attribute__((address_space(4))) *gs = trace_uniform_ptr(P.geo_slot) + 4 * (size_t)slot;
                    const double gx = gs[0], gy = gs[1], gz = gs[2], r2 = gs[3];
                    if (lane_live()) exact_any_order((int)idx, gx, gy, gz, r2);
                }
            } else {
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
                uint32_t cols = lane_live() ? mine : 0u;
                while (cols != 0u) {
                    const int slot = 32 * t + __builtin_ctz(cols);
                    cols &= cols - 1u;
                    const uint32_t idx = P.slot_orig[slot];
                    if (idx == 0xFFFFFFFFu) continue;           // (padding: never kept by construction)
                    const double4 g = *reinterpret_cast<const double4 *>(P.geo_slot + 4 * (size_t)slot);
                    exact_any_order((int)idx, g.x, g.y, g.z, g.w);
                    if (ANY && hit >= 0) break;
                }
            }
        };

        if (lane == 0) RT_TRACE_CNT(0, 1);
        if (sane) RT_TRACE_CNT(3, 1);
        // ---- which tiles: the global ones, and the grid cells the wave's rays can reach
        bool all_tiles = G <= 0;
        int z_lo = 0, z_hi = -1, x_lo = 0, x_hi = -1;
        // RAY: a grid of at most 64 cells has its cell set in ONE 64-bit mask (bit iz * G + ix), larger grids one word per grid row in LDS
        const bool one_mask = RAY && G * G <= 64;
        unsigned long long cell_mask = 0ull;
        if (G > 0) {
            int ix0 = 0, nx = 0, iz0 = 0, nz = 0, verdict = 0;
            GridSeg seg;
            if (sane) verdict = grid_cells(ray_of, ray_df, ray_o1, P.grid, G, P.scene_scale, ix0, nx, iz0, nz, RAY ? &seg : nullptr);
            if (__ballot(verdict < 0) != 0ull) all_tiles = true;        // "cannot tell": every tile
            const bool has = verdict > 0;
            z_lo = __builtin_amdgcn_readfirstlane(trace_wave_min(has ? iz0 : 0x7fffffff));
            z_hi = __builtin_amdgcn_readfirstlane(trace_wave_max(has ? iz0 + nz - 1 : -1));
            if constexpr (!RAY) {
                x_lo = __builtin_amdgcn_readfirstlane(trace_wave_min(has ? ix0 : 0x7fffffff));
                x_hi = __builtin_amdgcn_readfirstlane(trace_wave_max(has ? ix0 + nx - 1 : -1));
            } else if (all_tiles) {
            } else if (one_mask) {
                // the cell set in registers: a lane's runs (1 <= rnx, rx0 + rnx <= G <= 8) shifted to their rows, ORed over the wave
                unsigned long long own = 0ull;
                if (has)
                    for (int r = 0; r < nz; ++r) {
                        int rx0, rnx;
                        grid_row_run(seg, ix0, ix0 + nx - 1, (float)(iz0 + r), rx0, rnx);
                        own |= ((~0ull >> ((64 - rnx) & 63)) << (rx0 & 63)) << (((iz0 + r) * G) & 63);
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
                if (has)
                    for (int r = 0; r < nz; ++r) {
                        int rx0, rnx;
                        grid_row_run(seg, ix0, ix0 + nx - 1, (float)(iz0 + r), rx0, rnx);
                        atomicOr(&rows[(iz0 + r) & 63], (~0ull >> ((64 - rnx) & 63)) << (rx0 & 63));
                    }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (all_tiles) {
            for (int t = 0; t < ntt && wave_live(); ++t) scan_tile(t);
        } else {
            for (int t = 0; t < P.n_global && t < ntt && wave_live(); ++t) scan_tile(t);
            while (cell_mask != 0ull && wave_live()) {                      // (RAY on a grid of at most 64 cells; else empty)
                const int cell = __builtin_ctzll(cell_mask);
                cell_mask &= cell_mask - 1ull;
                const int t = P.n_global + cell;
                if (cell < G * G && t < ntt) scan_tile(t);
            }
            for (int iz = z_lo; iz <= z_hi && !one_mask && wave_live(); ++iz) {
                if constexpr (!RAY) {
                    for (int ix = x_lo; ix <= x_hi && wave_live(); ++ix) {
                        const int t = P.n_global + iz * G + ix;
                        if (t < ntt) scan_tile(t);
                    }
                } else {
                    const unsigned long long rw = rows[iz & 63];            // (one address for the wave: a broadcast read)
                    unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(rw >> 32)) << 32) |
                                           (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rw);
                    while (m != 0ull && wave_live()) {
                        const int ix = __builtin_ctzll(m);
                        m &= m - 1ull;
                        const int t = P.n_global + iz * G + ix;
                        if (ix < G && t < ntt) scan_tile(t);
                    }
                }
            }
            if (RAY && !one_mask) __builtin_amdgcn_wave_barrier();          // the next trip's clear comes after this trip's reads
        }

        // ---- the answer: sphere.rs:36-37 + mod.rs:20-30 for the winner
        if (valid) {
            if constexpr (ANY) {
                R.occluded[k] = hit >= 0 ? (uint8_t)1 : (uint8_t)0;
            } else {
                double t_out = __builtin_inf();
                D3 p = mk(0.0, 0.0, 0.0), nrm = mk(0.0, 0.0, 0.0);
                bool front = false;
                if (hit >= 0) {
                    const double inv_r = P.mat[kMatStride * (size_t)hit];
                    const double4 g = *reinterpret_cast<const double4 *>(geo + 4 * (size_t)hit);
                    t_out = closest;
                    p = o + d * closest;                                            // ray.rs:15-17
                    const D3 outward = (p - mk(g.x, g.y, g.z)) * inv_r;             // / radius = * (1/radius)
                    front = dot(d, outward) < 0.0;
                    nrm = front ? outward : (mk(0.0, 0.0, 0.0) - outward);
                }
                R.index[k] = hit;
                if (R.t) R.t[k] = canonical_nan(t_out);
                if (R.point) {
                    R.point[3 * k] = canonical_nan(p.x); R.point[3 * k + 1] = canonical_nan(p.y); R.point[3 * k + 2] = canonical_nan(p.z);
                }
                if (R.normal) {
                    R.normal[3 * k] = canonical_nan(nrm.x); R.normal[3 * k + 1] = canonical_nan(nrm.y); R.normal[3 * k + 2] = canonical_nan(nrm.z);
                }
                if (R.front) R.front[k] = front ? (uint8_t)1 : (uint8_t)0;
            }
        }
#ifdef RT_TRACE_COUNT
        for (int c = 0; c < 5; ++c) if (cnt[c] != 0ull) atomicAdd(&g_trace_counts[c], cnt[c]);
#endif
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

// RTIOW_TRACE_GRID_BLOCKS=k (diagnostic, read per call): at most k workgroups, so that the kernel's grid-stride trip runs at a test's size
long long grid_blocks_knob()
{
    const char *e = getenv("RTIOW_TRACE_GRID_BLOCKS");
    if (!e || !*e) return 0;
    const long long v = atoll(e);
    return v > 0 ? v : 0;
}

// What a ray query accepts: checked before anything is touched.  The checks that need no context come first (a caller without a device
// still gets the precise message), then the context's own.  `out`: hits->index or d_occluded.
int validate_trace(const rt_context *ctx, const char *what, const rt_rays *rays, double t_min, bool has_out_struct, const void *out)
{
    if (!rays) return fail(RT_ERR_INVALID_ARGUMENT, "%s: rays is NULL", what);
    if (!has_out_struct) return fail(RT_ERR_INVALID_ARGUMENT, "%s: hits is NULL", what);
    if (rays->n < 0 || rays->n > (int64_t)1 << 31)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: n must be in [0, 2^31] (is %lld)", what, (long long)rays->n);
    if (!(t_min > 0.0) || !std::isfinite(t_min)) return fail(RT_ERR_INVALID_ARGUMENT, "%s: t_min must be > 0 and finite (is %g)", what, t_min);
    if (rays->n > 0) {
        if (!rays->origin) return fail(RT_ERR_INVALID_ARGUMENT, "%s: rays->origin is NULL", what);
        if (!rays->dir) return fail(RT_ERR_INVALID_ARGUMENT, "%s: rays->dir is NULL", what);
        if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "%s: the required output (hits->index / occluded) is NULL", what);
    }
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->scan_mode != 5)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s needs the shipped scan mode 5; this context was created under RTIOW_SCAN_MODE=%d", what, ctx->scan_mode);
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
    // one wave per 64 rays, handed out by the hardware as workgroups retire; the kernel's grid-stride loop takes over beyond 2^20 workgroups
    const long long trips = ((long long)rays->n + 63) / 64;
    long long grid = (trips + rt::kTraceWaves - 1) / rt::kTraceWaves;
    if (grid > (1 << 20)) grid = 1 << 20;
    const long long cap = grid_blocks_knob();
    if (cap > 0 && grid > cap) grid = cap;
    if (grid < 1) grid = 1;
    const bool ray = candidates_knob_ray(), any = hits == nullptr;
    const dim3 g((unsigned)grid), b(rt::kTraceBlock);
    if (ray && any) hipLaunchKernelGGL((rt::trace_kernel<true, true>), g, b, 0, stream, kp, ta);
    else if (ray) hipLaunchKernelGGL((rt::trace_kernel<true, false>), g, b, 0, stream, kp, ta);
    else if (any) hipLaunchKernelGGL((rt::trace_kernel<false, true>), g, b, 0, stream, kp, ta);
    else hipLaunchKernelGGL((rt::trace_kernel<false, false>), g, b, 0, stream, kp, ta);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// the host forms' common part: rays up, `device` on own_stream between the events, `downloads` after them
struct StagedRays {
    size_t b_o, b_d, b_tmax;
    rt_rays dev;
};
void stage_rays(Stage &st, const rt_rays *rays, StagedRays &s)
{
    const size_t n = (size_t)rays->n;
    s.b_o = st.add(n * 3 * sizeof(double));
    s.b_d = st.add(n * 3 * sizeof(double));
    s.b_tmax = st.add(rays->t_max ? n * sizeof(double) : 0);
}
hipError_t upload_rays(const Stage &st, const rt_rays *rays, StagedRays &s)
{
    const size_t n = (size_t)rays->n;
    hipError_t he = st.up(s.b_o, rays->origin, n * 3 * sizeof(double));
    if (he == hipSuccess) he = st.up(s.b_d, rays->dir, n * 3 * sizeof(double));
    if (he == hipSuccess && rays->t_max) he = st.up(s.b_tmax, rays->t_max, n * sizeof(double));
    s.dev.origin = st.at<double>(s.b_o);
    s.dev.dir = st.at<double>(s.b_d);
    s.dev.t_max = rays->t_max ? st.at<double>(s.b_tmax) : nullptr;
    s.dev.n = rays->n;
    return he;
}

} // namespace

extern "C" {

// HittableList::hit(ray, t_min, t_max[k]), mod.rs:54-70, of every ray of the batch
int rt_trace_rays_device(rt_context *ctx, const rt_rays *rays, double t_min, const rt_hits *hits, void *stream_v)
{
    int rc = validate_trace(ctx, "rt_trace_rays", rays, t_min, hits != nullptr, hits ? hits->index : nullptr);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (rays->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_trace(ctx, rays, t_min, hits, nullptr, (hipStream_t)stream_v);
}

int rt_trace_rays(rt_context *ctx, const rt_rays *rays, double t_min, const rt_hits *hits, float *kernel_ms)
{
    int rc = validate_trace(ctx, "rt_trace_rays", rays, t_min, hits != nullptr, hits ? hits->index : nullptr);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (rays->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)rays->n;
    Stage st(ctx);
    StagedRays sr;
    stage_rays(st, rays, sr);
    const size_t b_index = st.add(n * sizeof(int32_t)), b_t = st.add(hits->t ? n * sizeof(double) : 0);
    const size_t b_point = st.add(hits->point ? n * 3 * sizeof(double) : 0), b_normal = st.add(hits->normal ? n * 3 * sizeof(double) : 0);
    const size_t b_front = st.add(hits->front_face ? n : 0);
    if ((rc = st.commit())) return rc;
    RT_HIP(upload_rays(st, rays, sr));
    rt_hits dh;
    dh.index = st.at<int32_t>(b_index);
    dh.t = hits->t ? st.at<double>(b_t) : nullptr;
    dh.point = hits->point ? st.at<double>(b_point) : nullptr;
    dh.normal = hits->normal ? st.at<double>(b_normal) : nullptr;
    dh.front_face = hits->front_face ? st.at<uint8_t>(b_front) : nullptr;
    return timed_section(ctx, "rt_trace_rays", kernel_ms,
        [&] { return rt_trace_rays_device(ctx, &sr.dev, t_min, &dh, ctx->own_stream); },
        [&] {
            hipError_t he = st.down(hits->index, b_index, n * sizeof(int32_t));
            if (he == hipSuccess && hits->t) he = st.down(hits->t, b_t, n * sizeof(double));
            if (he == hipSuccess && hits->point) he = st.down(hits->point, b_point, n * 3 * sizeof(double));
            if (he == hipSuccess && hits->normal) he = st.down(hits->normal, b_normal, n * 3 * sizeof(double));
            if (he == hipSuccess && hits->front_face) he = st.down(hits->front_face, b_front, n);
            return he;
        });
}

int rt_occluded_device(rt_context *ctx, const rt_rays *rays, double t_min, void *d_occluded, void *stream_v)
{
    int rc = validate_trace(ctx, "rt_occluded", rays, t_min, true, d_occluded);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (rays->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_trace(ctx, rays, t_min, nullptr, d_occluded, (hipStream_t)stream_v);
}

int rt_occluded(rt_context *ctx, const rt_rays *rays, double t_min, uint8_t *occluded, float *kernel_ms)
{
    int rc = validate_trace(ctx, "rt_occluded", rays, t_min, true, occluded);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (rays->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)rays->n;
    Stage st(ctx);
    StagedRays sr;
    stage_rays(st, rays, sr);
    const size_t b_occ = st.add(n);
    if ((rc = st.commit())) return rc;
    RT_HIP(upload_rays(st, rays, sr));
    return timed_section(ctx, "rt_occluded", kernel_ms,
        [&] { return rt_occluded_device(ctx, &sr.dev, t_min, st.at(b_occ), ctx->own_stream); },
        [&] { return st.down(occluded, b_occ, n); });
}

#ifdef RT_TRACE_COUNT
// diagnostic builds only: reads the counters and zeroes them
int rt_debug_trace_counts(rt_context *ctx, unsigned long long out[8])
{
    if (!ctx || !out) return fail(RT_ERR_INVALID_ARGUMENT, "ctx/out is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rt::g_trace_counts), 8 * sizeof(unsigned long long)));
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_trace_counts), zero, sizeof(zero)));
    return RT_OK;
}
#endif

} // extern "C"
