// rt_first_hit.hpp -- HittableList::hit (mod.rs:54-70) of the 64 rays of one wave against the uploaded list: the scan that
// rt::features_kernel (rt_features.hip, camera rays, t_max = +inf) and rt::trace_kernel (rt_trace.hip, the caller's rays, a t_max per ray)
// share.  Both include it after rt_host.hpp (KParams and the constants: rt_params.hpp); it uses the building blocks of rt_device.hpp and the tables rt_upload_scene built.
//
// Per wave: the rays' filter rows (filter_rows), the spheres that skip the filter or, for a ray outside the filter's analysed range, the
// whole list as written (exact_prologue), which tiles of 32 columns the rays can reach (wave_footprint), the tube filter on a tile (four
// matrix instructions: filter_tile), the exact f64 test of what it keeps, and the winner's record (hit_record).  first_hit_wave puts them
// together in the `wave` scheme: the global tiles plus the bounding rectangle of the wave's footprints, the keep bits ORed over the wave,
// EVERY lane testing every kept column with the sphere's record fetched through scalar loads.  The filter is conservative and the f64 test
// decides, so a superset is still exact; 64 coherent rays keep it small.  (rt_trace.hip's `ray` scheme composes the same pieces with a
// cell set and per-ray keep bits of its own.)  ANY (occlusion): a lane with an accepted root goes idle, the wave leaves when none is left.
//
// The tie rule (among equal roots the LATER sphere of the list), the strict t_min and the NaN behaviour of the two exact tests are stated
// HERE and nowhere else outside the render kernel (rt_kernels.hpp, exact_test).
#pragma once
#include "rt_params.hpp"
#include "rt_device.hpp"

namespace rt {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// A wave-uniform address in the constant address space: the compiler selects scalar loads for it.  Legal because the scene's tables
// are written by rt_upload_scene before the launch and only read during it.  Correctness does not depend on the choice: were the
// loads issued as vector loads, every lane would read the same record.
template <typename T>
__device__ __forceinline__ const T __attribute__((address_space(4))) *uniform_ptr(const T *p)
{
    return (const T __attribute__((address_space(4))) *)(uintptr_t)p;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

// the launch grid of a kernel whose waves each take `units` in turn: one wave per unit, handed out by the hardware as workgroups retire
// (no static split); the kernel's grid-stride loop takes over beyond 2^20 workgroups
inline long long wave_grid(long long units, int waves_per_block)
{
    const long long grid = (units + waves_per_block - 1) / waves_per_block;
    return grid > (1 << 20) ? 1 << 20 : grid < 1 ? 1 : grid;
}

// RT_SCAN_COUNT (the including file sets it in ITS diagnostic build, never in the product: -DRT_FEATURES_COUNT for tools/features_bench.py
// --counts, -DRT_TRACE_COUNT for tools/trace_bench.py --counts): how large the superset is.  [0] wave-samples / wave trips, [1] tiles
// scanned, [2] exact tests run -- `pairs` false: columns some ray of the wave kept = tests EVERY lane ran (the feature kernel's unit),
// true: (lane, column) pairs, the always-exact list included (the ray-query kernel's) --, [3] lanes with a ray inside the analysed range,
// [4] (lane, column) pairs whose exact test reached a root >= t_min (the tests that were needed at most).
struct ScanCounts {
    bool pairs;
#ifdef RT_SCAN_COUNT
    unsigned long long n[5];
#endif
};
#ifdef RT_SCAN_COUNT
static __device__ unsigned long long g_scan_counts[8];
#define RT_SCAN_CNT(k, v) (cnt.n[k] += (unsigned long long)(v))
#else
#define RT_SCAN_CNT(k, v) ((void)0)
#endif
__device__ __forceinline__ void flush_counts(const ScanCounts &cnt)
{
#ifdef RT_SCAN_COUNT
    for (int k = 0; k < 5; ++k) if (cnt.n[k] != 0ull) atomicAdd(&g_scan_counts[k], cnt.n[k]);
#endif
}
#ifdef RT_SCAN_COUNT
// diagnostic builds only: reads the counters and zeroes them
inline int read_and_zero_counts(rt_context *ctx, unsigned long long out[8])
{
    if (!ctx || !out) return rt_host::fail(RT_ERR_INVALID_ARGUMENT, "ctx/out is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_scan_counts), 8 * sizeof(unsigned long long)));
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_scan_counts), zero, sizeof(zero)));
    return RT_OK;
}
#endif

struct FirstHit {
    double closest;     // mod.rs:56: closest_so_far, t_max at the start
    int hit;            // the list index of the sphere that set it, -1: none yet
};

// sphere.rs:16-34 + mod.rs:61-67 in the order-independent form of the render kernel's exact_test: a sphere's root r* is the near one if
// >= t_min, else the far one; the smallest r* <= t_max wins, among equal roots the LATER sphere of the list (hit starts at -1: a root
// equal to t_max is accepted).  a = |d|^2 (sphere.rs:20).
__device__ __forceinline__ void exact_any_order(FirstHit &fh, const D3 &o, const D3 &d, double a, double t_min, int idx, double gx, double gy,
                                                double gz, double r2, ScanCounts &cnt)
{
    if (cnt.pairs) RT_SCAN_CNT(2, 1);
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
    RT_SCAN_CNT(4, 1);
    if (root < fh.closest || (root == fh.closest && idx > fh.hit)) { fh.closest = root; fh.hit = idx; }
}
// ... and as written, for a visit in LIST order (degenerate directions, a NaN t_max: a NaN fails neither comparison and is accepted)
__device__ __forceinline__ void exact_in_order(FirstHit &fh, const D3 &o, const D3 &d, double a, double t_min, const double *geo, int idx)
{
    const double4 g = *reinterpret_cast<const double4 *>(geo + 4 * (size_t)idx);
    const D3 oc = o - mk(g.x, g.y, g.z);
    const double half_b = dot(oc, d);
    const double c = length_squared(oc) - g.w;
    const double disc = half_b * half_b - a * c;
    if (disc < 0.0) return;
    const double sq = __builtin_sqrt(disc);
    double r = (-half_b - sq) / a;                  // sphere.rs:28-34
    if (r < t_min || fh.closest < r) {
        r = (-half_b + sq) / a;
        if (r < t_min || fh.closest < r) return;
    }
    fh.closest = r;                                 // mod.rs:63-64
    fh.hit = idx;
}

// ANY (occlusion): a lane with an accepted root is idle; the wave goes on while a lane is left
template <bool ANY>
__device__ __forceinline__ bool lane_live(bool sane, const FirstHit &fh) { return sane && !(ANY && fh.hit >= 0); }
template <bool ANY>
__device__ __forceinline__ bool wave_live(bool sane, const FirstHit &fh) { return !ANY || __ballot(lane_live<ANY>(sane, fh)) != 0ull; }

// the ray as the f32 filter and the footprint see it (ray_f32)
struct RayF32 { float of[3], df[3], o1; };

// The filter rows of the wave's 64 rays -> A; returns `sane`: the lane has a ray (`ok`: a lane past the end of the work, or a t_max
// that does not compare, has none) inside the filter's analysed range.  Every other lane stays in the wave with rows that keep nothing.
__device__ __forceinline__ bool filter_rows(uint4 *stage, int lane, const D3 &o, const D3 &d, float rho, bool ok, RayF32 &rf, bf16x8 (&A)[4])
{
    ray_f32(o, d, rf.of, rf.df, rf.o1);
    TubeRay T = make_tube<false>(rf.of, rf.df, rf.o1, rho);
    const bool sane = ok && T.sane;
    if (!sane) tube_rows_keep_nothing(T);
    uint32_t w[2][8];
    tube_a_words(T, w);
    tube_stage_operands(stage, lane, w, A);
    return sane;
}

// Before the tiles: a ray in range tests the spheres that skip the filter (the ground); one outside it (zero, NaN and infinite directions)
// the whole list in list order, as written -- occlusion: up to the first accepted root.
template <bool ANY>
__device__ __forceinline__ void exact_prologue(const KParams &P, int lane, const D3 &o, const D3 &d, double a, bool sane, bool valid, FirstHit &fh,
                                               ScanCounts &cnt)
{
    if (lane == 0) RT_SCAN_CNT(0, 1);
    if (sane) RT_SCAN_CNT(3, 1);
    if (sane) {
        for (int e = 0; e < P.n_always; ++e) {
            const int idx = P.always_idx[e];
            const double4 g = *reinterpret_cast<const double4 *>(P.geo + 4 * (size_t)idx);
            exact_any_order(fh, o, d, a, P.t_min, idx, g.x, g.y, g.z, g.w, cnt);
        }
    } else if (valid) {
        for (int k = 0; k < P.n_spheres && !(ANY && fh.hit >= 0); ++k) exact_in_order(fh, o, d, a, P.t_min, P.geo, k);
    }
}

// The filter on one tile of 32 columns, on the matrix pipe.  acc[Gq][8 bb + jj] / acc[Gq][8 bb + 4 + jj]: H_1 / H_2 of ray
// 16 Gq + 8 bb + 4 (lane >> 5) + jj against column lane & 31; the pair is kept iff |H_1| < 2 and |H_2| < 2, i.e. iff bit 30 of both f32
// patterns is clear.  X = AND over the lane's 16 rays of (H_1 | H_2) has bit 30 clear iff one of them keeps this column.
// Returns the ballot of the columns some ray keeps (two lanes per column).
__device__ __forceinline__ unsigned long long filter_tile(const KParams &P, int t, int lane, const bf16x8 (&A)[4], f32x16 (&acc)[4], ScanCounts &cnt)
{
    if (lane == 0) RT_SCAN_CNT(1, 1);
    const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bf16x8 b = __builtin_bit_cast(bf16x8, P.btube[(size_t)t * 64 + lane]);
    uint32_t X = 0xFFFFFFFFu;
#pragma unroll
    for (int Gq = 0; Gq < 4; ++Gq) {
        acc[Gq] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[Gq], b, zero16, 0, 0, 0);
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) X &= __float_as_uint(acc[Gq][8 * bb + jj]) | __float_as_uint(acc[Gq][8 * bb + 4 + jj]);
    }
    return __ballot((X & 0x40000000u) == 0u);
}

// every live lane tests every column of tile t some ray keeps; the sphere is wave-uniform: its records come through scalar loads
template <bool ANY>
__device__ __forceinline__ void test_kept_columns_wave(const KParams &P, int t, unsigned long long kept, int lane, const D3 &o, const D3 &d, double a,
                                                       bool sane, FirstHit &fh, ScanCounts &cnt)
{
    if (kept == 0ull) return;                       // (measured: without this exit the incoherent sets run 0.5-1 % longer, profiles/first_hit_refactor_ab.txt)
    uint32_t cols = (uint32_t)kept | (uint32_t)(kept >> 32);
    while (cols != 0u) {
        const int slot = 32 * t + __builtin_ctz(cols);
        cols &= cols - 1u;
        if (!cnt.pairs && lane == 0) RT_SCAN_CNT(2, 1);
        const uint32_t idx = uniform_ptr(P.slot_orig)[slot];
        if (idx == 0xFFFFFFFFu) continue;           // (padding: never kept by construction)
        const double __attribute__((address_space(4))) *gs = uniform_ptr(P.geo_slot) + 4 * (size_t)slot;
        const double gx = gs[0], gy = gs[1], gz = gs[2], r2 = gs[3];
        if (lane_live<ANY>(sane, fh)) exact_any_order(fh, o, d, a, P.t_min, (int)idx, gx, gy, gz, r2, cnt);
    }
}

// Which grid cells the wave's rays can reach.  The lane's own footprint (has: it has one; the rectangle ix0 .. ix0 + nx - 1 by
// iz0 .. iz0 + nz - 1, and *seg for the runs of its rows) and, wave-uniform, all_tiles ("cannot tell" for some ray, or no grid: every
// tile) and the bounding rectangle of the wave's footprints.
struct Footprint {
    bool all_tiles, has;
    int ix0, nx, iz0, nz;
    int x_lo, x_hi, z_lo, z_hi;
};
__device__ __forceinline__ Footprint wave_footprint(const KParams &P, const RayF32 &rf, bool sane, GridSeg *seg = nullptr)
{
    Footprint f = {P.grid_dim <= 0, false, 0, 0, 0, 0, 0, -1, 0, -1};
    if (P.grid_dim > 0) {
        int verdict = 0;
        if (sane) verdict = grid_cells(rf.of, rf.df, rf.o1, P.grid, P.grid_dim, P.scene_scale, f.ix0, f.nx, f.iz0, f.nz, seg);
        if (__ballot(verdict < 0) != 0ull) f.all_tiles = true;
        f.has = verdict > 0;
        f.x_lo = __builtin_amdgcn_readfirstlane(wave_min(f.has ? f.ix0 : 0x7fffffff));
        f.x_hi = __builtin_amdgcn_readfirstlane(wave_max(f.has ? f.ix0 + f.nx - 1 : -1));
        f.z_lo = __builtin_amdgcn_readfirstlane(wave_min(f.has ? f.iz0 : 0x7fffffff));
        f.z_hi = __builtin_amdgcn_readfirstlane(wave_max(f.has ? f.iz0 + f.nz - 1 : -1));
    }
    return f;
}

// The `wave` scheme, whole: fh (closest = t_max, hit = -1 on entry) becomes the answer of the lane's ray (o, d); lanes that are not
// `valid` have none and stay in the wave.  stage: the wave's 64 * 4 uint4 of LDS.
template <bool ANY>
__device__ __forceinline__ void first_hit_wave(const KParams &P, uint4 *stage, int lane, const D3 &o, const D3 &d, bool valid, FirstHit &fh,
                                               ScanCounts &cnt)
{
    const int ntt = P.n_tiles >> 1;                     // tiles of 32 columns; the tables hold ntt + 1
    RayF32 rf;
    bf16x8 A[4];
    // (a t_max that does not compare: the order-independent form is the loop as written only without it)
    const bool sane = filter_rows(stage, lane, o, d, P.tube_rho, valid && fh.closest == fh.closest, rf, A);
    const double a = length_squared(d);                 // sphere.rs:20
    exact_prologue<ANY>(P, lane, o, d, a, sane, valid, fh, cnt);
    auto scan_tile = [&](int t) {
        f32x16 acc[4];
        const unsigned long long kept = filter_tile(P, t, lane, A, acc, cnt);
        test_kept_columns_wave<ANY>(P, t, kept, lane, o, d, a, sane, fh, cnt);
    };
    const Footprint f = wave_footprint(P, rf, sane);
    if (f.all_tiles) {
        for (int t = 0; t < ntt && wave_live<ANY>(sane, fh); ++t) scan_tile(t);
    } else {
        for (int t = 0; t < P.n_global && t < ntt && wave_live<ANY>(sane, fh); ++t) scan_tile(t);
        for (int iz = f.z_lo; iz <= f.z_hi && wave_live<ANY>(sane, fh); ++iz)
            for (int ix = f.x_lo; ix <= f.x_hi && wave_live<ANY>(sane, fh); ++ix) {
                const int t = P.n_global + iz * P.grid_dim + ix;
                if (t < ntt) scan_tile(t);
            }
    }
}

// sphere.rs:36-37 + mod.rs:20-30 for the winner (fh.hit >= 0): the point, the normal against the ray, and the material record
struct HitRecord {
    D3 p, normal;
    bool front;
    const double *mrec;
};
__device__ __forceinline__ HitRecord hit_record(const KParams &P, const D3 &o, const D3 &d, const FirstHit &fh)
{
    HitRecord r;
    r.mrec = P.mat + kMatStride * (size_t)fh.hit;
    const double4 g = *reinterpret_cast<const double4 *>(P.geo + 4 * (size_t)fh.hit);
    r.p = o + d * fh.closest;                                               // ray.rs:15-17
    const D3 outward = (r.p - mk(g.x, g.y, g.z)) * r.mrec[0];               // / radius = * (1/radius)
    r.front = dot(d, outward) < 0.0;
    r.normal = r.front ? outward : (mk(0.0, 0.0, 0.0) - outward);
    return r;
}

} // namespace rt
