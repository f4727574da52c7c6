// rt_features.hip -- first-hit feature buffers: albedo, normal, depth, hit count and object id (rtiow_hip.h, "feature buffers";
// DESIGN.md section 14).
//
// The third translation unit of librtiow_hip.so.  It owns ONE kernel of its own, rt::features_kernel, which traces the camera rays of a
// dense render -- bounce 0 of ray_color, main.rs:131-134 + HittableList::hit mod.rs:54-70 -- and keeps the hit record the render
// kernel throws away, and the small kernel that turns the exact sums into what a denoiser takes.  It reads the tables rt_upload_scene
// built (rt_host::set_scene_params) and uses the building blocks of rt_device.hpp; rt_kernels.hpp, rt_device.hpp, rt_api.hip and
// rt_diag.hpp are untouched, so every existing kernel keeps its machine code.
//
// Shape of the kernel (simple on purpose): one wave covers an 8 x 8 pixel tile, a lane owns one pixel and loops over its samples
// with the eight sums in registers; no atomics, no LDS sums, no work queue.  Per sample the wave builds the 64 rays' filter rows,
// runs the tube filter over the tiles its rays can reach (four matrix instructions per tile of 32 columns), ORs the keep bits over
// the wave into one 32-bit column mask, and EVERY lane tests every kept column exactly: the filter is conservative and the f64 test
// decides, so a superset is still exact.  The 64 rays of a pixel tile are coherent, which should keep the superset small;
// -DRT_FEATURES_COUNT counts it.
#include <hip/hip_runtime.h>

#include <cstring>

#define RT_RENDER_KERNEL_ONLY       // rt_kernels.hpp: KParams and the constants; rt_api.hip owns the kernels defined there
#include "rt_host.hpp"

using namespace rt_host;

namespace rt {

constexpr int kFeatBlock = 256;                     // four waves, each on pixel tiles of its own
constexpr int kFeatWaves = kFeatBlock / 64;

struct FeatArgs {
    unsigned long long *feat;       // [height][width][8] exact sums
    int32_t *ids;                   // [height][width] list index of the first sample's hit, or NULL
    int32_t accumulate;             // 1: add to feat (RT_FLAG_ACCUMULATE)
    uint32_t tiles_x;               // pixel tiles per row of tiles: ceil(width / 8)
    uint32_t n_wtiles;              // tiles_x * ceil(height / 8)
};

// A wave-uniform address in the constant address space: the compiler selects scalar loads for it.  Legal because the scene's tables
// are written by rt_upload_scene before the launch and only read during it.  Correctness does not depend on the choice: were the
// loads issued as vector loads, every lane would read the same record.
template <typename T>
__device__ __forceinline__ const T __attribute__((address_space(4))) *uniform_ptr(const T *p)
{
    return (const T __attribute__((address_space(4))) *)(uintptr_t)p;
}

// a normal's component on the 2^-32 grid, signed: 0 for a NaN, else floor(clamp(x, -2^16, 2^16) * 2^32) as a two's-complement
// integer (the product with 2^32 is exact; |value| <= 2^48)
__device__ __forceinline__ unsigned long long quantize_signed(double x)
{
    if (x != x) return 0ull;
    x = __builtin_fmin(__builtin_fmax(x, -65536.0), 65536.0);
    return (unsigned long long)(long long)__builtin_floor(x * 4294967296.0);
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

// RT_FEATURES_COUNT (a diagnostic build, never the product: tools/features_bench.py --counts): how large the superset is.  Per wave and
// sample: [0] wave-samples, [1] tiles scanned, [2] columns some ray of the wave kept = exact tests EVERY lane ran, [3] lanes with a
// ray inside the analysed range, [4] (lane, column) pairs whose exact test reached a root >= t_min (the tests that were needed at most).
#ifdef RT_FEATURES_COUNT
__device__ unsigned long long g_feat_counts[8];
#define RT_FEAT_COUNT(k, n) (cnt[k] += (unsigned long long)(n))
#else
#define RT_FEAT_COUNT(k, n) ((void)0)
#endif

__global__ __launch_bounds__(kFeatBlock) void features_kernel(const KParams P, const FeatArgs F)
{
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    __shared__ uint4 s_stage[kFeatWaves][64 * 4];
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    uint4 *stage = s_stage[wave];
    const int ntt = P.n_tiles >> 1;                     // tiles of 32 columns; the tables hold ntt + 1
    const int n = P.n_spheres;
    const int G = P.grid_dim;
    const double wm1 = (double)(P.width - 1), hm1 = (double)(P.height - 1);
    const double t_min = P.t_min;
    const double *__restrict__ geo = P.geo;
    const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t n_waves = gridDim.x * (uint32_t)kFeatWaves;

    for (uint32_t wt = blockIdx.x * (uint32_t)kFeatWaves + (uint32_t)wave; wt < F.n_wtiles; wt += n_waves) {
        const uint32_t ty = wt / F.tiles_x, tx = wt - ty * F.tiles_x;
        const int i = (int)(tx * 8u) + (lane & 7), j = (int)(ty * 8u) + (lane >> 3);
        // lanes past the right or top edge stay in the wave: rows that keep nothing, nothing written
        const bool valid = i < P.width && j < P.height;
        const uint32_t g_pix = (uint32_t)j * (uint32_t)P.width + (uint32_t)i;
        unsigned long long sum[RT_FEATURE_WORDS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
        int first_id = -1;
#ifdef RT_FEATURES_COUNT
        unsigned long long cnt[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
#endif

        for (int s = 0; s < P.spp; ++s) {
            // ---- the camera ray of (pixel, sample): main.rs:131-134, camera.rs:47-54 -- the render kernel's own start of a sample
            D3 o = mk(0.0, 0.0, 0.0), d = mk(0.0, 0.0, 0.0);
            if (valid) {
                const uint32_t g_s = (uint32_t)P.sample_begin + (uint32_t)s;
                U4 w = philox4x32_10(g_pix, g_s, 0u, 0u, P.k0, P.k1);
                uint32_t ev = 1u;
                const double cu = ((double)i + u01(w.x)) / wm1;                 // main.rs:131
                const double cv = ((double)j + u01(w.y)) / hm1;                 // main.rs:132
                // vec3.rs:59-68: block 0 = (u jitter, v jitter, lens x, lens y); every further block holds two tries
                uint32_t wx = w.z, wy = w.w;
                while (!unit_disk_accepts(wx, wy)) {
                    w = philox4x32_10(g_pix, g_s, ev, 0u, P.k0, P.k1);
                    ev++;
                    wx = w.x; wy = w.y;
                    if (!unit_disk_accepts(wx, wy)) { wx = w.z; wy = w.w; }
                }
                const D3 cam_origin = ld3(P.cam.origin);
                const D3 rd = mk(u11(wx), u11(wy), 0.0) * P.cam.lens_radius;
                const D3 offset = ld3(P.cam.u) * rd.x + ld3(P.cam.v) * rd.y;
                o = cam_origin + offset;
                d = (((ld3(P.cam.llc) + ld3(P.cam.horizontal) * cu) + ld3(P.cam.vertical) * cv) - cam_origin) - offset;
            }

            // ---- the filter rows of the wave's 64 rays
            float ray_of[3], ray_df[3], ray_o1;
            ray_f32(o, d, ray_of, ray_df, ray_o1);
            TubeRay T = make_tube<false>(ray_of, ray_df, ray_o1, P.tube_rho);
            const bool sane = valid && T.sane;                  // inside the filter's analysed range
            if (!sane) tube_rows_keep_nothing(T);
            bf16x8 A[4];
            {
                uint32_t w[2][8];
                tube_a_words(T, w);
                tube_stage_operands(stage, lane, w, A);
            }

            // ---- HittableList::hit, mod.rs:54-70, with t_max = +inf
            double closest = __builtin_inf();
            int hit = -1;
            const double a = length_squared(d);                 // sphere.rs:20
            // sphere.rs:16-34 + mod.rs:61-67 in the order-independent form of the render kernel's exact_test: the smallest root
            // r* (the near root if >= t_min, else the far one) wins, among equal roots the LATER sphere of the list
            auto exact_any_order = [&](int idx, double gx, double gy, double gz, double r2) {
                const D3 oc = o - mk(gx, gy, gz);
                const double half_b = dot(oc, d);
                const double c = length_squared(oc) - r2;
                const double disc = half_b * half_b - a * c;
                if (disc < 0.0) return;                         // sphere.rs:25
                if (half_b > 0.0 && c > 0.0) return;            // origin outside, sphere behind the ray: both roots < t_min
                const double sqrtd = __builtin_sqrt(disc);
                double root = (-half_b - sqrtd) / a;
                if (root < t_min) {
                    root = (-half_b + sqrtd) / a;
                    if (root < t_min) return;
                }
                RT_FEAT_COUNT(4, 1);
                if (root < closest || (root == closest && idx > hit)) { closest = root; hit = idx; }
            };
            // ... and as written, for a visit in LIST order (degenerate directions: a NaN root fails neither comparison and is accepted)
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
                // outside the analysed range (zero, NaN and infinite directions): the whole list in list order, as written
                for (int k = 0; k < n; ++k) exact_in_order(k);
            }

            // one tile of 32 columns: the filter on the matrix pipe, then every lane tests every column some ray keeps
            auto scan_tile = [&](int t) {
                if (lane == 0) RT_FEAT_COUNT(1, 1);
                const bf16x8 b = __builtin_bit_cast(bf16x8, P.btube[(size_t)t * 64 + lane]);
                // acc[8 bb + jj] / acc[8 bb + 4 + jj]: H_1 / H_2 of ray 16 Gq + 8 bb + 4 (lane >> 5) + jj against column lane & 31; the pair
                // is kept iff |H_1| < 2 and |H_2| < 2, i.e. iff bit 30 of both f32 patterns is clear.  X = AND over the lane's 16 rays of
                // (H_1 | H_2) has bit 30 clear iff one of them keeps this column.
                uint32_t X = 0xFFFFFFFFu;
#pragma unroll
                for (int Gq = 0; Gq < 4; ++Gq) {
                    const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[Gq], b, zero16, 0, 0, 0);
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) X &= __float_as_uint(acc[8 * bb + jj]) | __float_as_uint(acc[8 * bb + 4 + jj]);
                }
                const unsigned long long kept = __ballot((X & 0x40000000u) == 0u);      // two lanes per column
                uint32_t cols = (uint32_t)kept | (uint32_t)(kept >> 32);
                while (cols != 0u) {
                    const int slot = 32 * t + __builtin_ctz(cols);
                    cols &= cols - 1u;
                    // the sphere is wave-uniform: its records come through scalar loads
                    if (lane == 0) RT_FEAT_COUNT(2, 1);
                    const uint32_t idx = uniform_ptr(P.slot_orig)[slot];
                    if (idx == 0xFFFFFFFFu) continue;           // (padding: never kept by construction)
                    const double __attribute__((address_space(4))) *gs = uniform_ptr(P.geo_slot) + 4 * (size_t)slot;
                    const double gx = gs[0], gy = gs[1], gz = gs[2], r2 = gs[3];
                    if (sane) exact_any_order((int)idx, gx, gy, gz, r2);
                }
            };

            if (lane == 0) RT_FEAT_COUNT(0, 1);
            if (sane) RT_FEAT_COUNT(3, 1);
            // ---- which tiles: the global ones, and the grid cells of the wave-wide union of the rays' footprints
            bool all_tiles = G <= 0;
            int x_lo = 0, x_hi = -1, z_lo = 0, z_hi = -1;
            if (G > 0) {
                int ix0 = 0, nx = 0, iz0 = 0, nz = 0, verdict = 0;
                if (sane) verdict = grid_cells(ray_of, ray_df, ray_o1, P.grid, G, P.scene_scale, ix0, nx, iz0, nz);
                if (__ballot(verdict < 0) != 0ull) all_tiles = true;        // "cannot tell": every tile
                const bool has = verdict > 0;
                x_lo = wave_min(has ? ix0 : 0x7fffffff); x_hi = wave_max(has ? ix0 + nx - 1 : -1);
                z_lo = wave_min(has ? iz0 : 0x7fffffff); z_hi = wave_max(has ? iz0 + nz - 1 : -1);
                x_lo = __builtin_amdgcn_readfirstlane(x_lo); x_hi = __builtin_amdgcn_readfirstlane(x_hi);
                z_lo = __builtin_amdgcn_readfirstlane(z_lo); z_hi = __builtin_amdgcn_readfirstlane(z_hi);
            }
            if (all_tiles) {
                for (int t = 0; t < ntt; ++t) scan_tile(t);
            } else {
                for (int t = 0; t < P.n_global && t < ntt; ++t) scan_tile(t);
                for (int iz = z_lo; iz <= z_hi; ++iz)
                    for (int ix = x_lo; ix <= x_hi; ++ix) {
                        const int t = P.n_global + iz * G + ix;
                        if (t < ntt) scan_tile(t);
                    }
            }

            // ---- the hit record: sphere.rs:36-37 + mod.rs:20-30; the material only for the winner
            if (valid && hit >= 0) {
                const double *mrec = P.mat + kMatStride * (size_t)hit;
                const double4 g = *reinterpret_cast<const double4 *>(geo + 4 * (size_t)hit);
                const D3 p = o + d * closest;                                       // ray.rs:15-17
                const D3 outward = (p - mk(g.x, g.y, g.z)) * mrec[0];               // / radius = * (1/radius)
                const bool front = dot(d, outward) < 0.0;
                const D3 nrm = front ? outward : (mk(0.0, 0.0, 0.0) - outward);
                // by KIND: a Dialectric's attenuation is (1, 1, 1) (materials.rs:103), whatever the flat scene's albedo field holds
                const bool glass = (int)mrec[5] == RT_KIND_DIALECTRIC;
                sum[0] += quantize(glass ? 1.0 : mrec[2]);
                sum[1] += quantize(glass ? 1.0 : mrec[3]);
                sum[2] += quantize(glass ? 1.0 : mrec[4]);
                sum[3] += quantize_signed(nrm.x);
                sum[4] += quantize_signed(nrm.y);
                sum[5] += quantize_signed(nrm.z);
                sum[6] += quantize(closest);
                sum[7] += 1ull;
            }
            if (s == 0) first_id = hit;
        }

        if (valid) {
            unsigned long long *out = F.feat + (size_t)g_pix * RT_FEATURE_WORDS;
#pragma unroll
            for (int k = 0; k < RT_FEATURE_WORDS; ++k) out[k] = F.accumulate ? out[k] + sum[k] : sum[k];
            if (F.ids) F.ids[g_pix] = first_id;
        }
#ifdef RT_FEATURES_COUNT
        for (int k = 0; k < 5; ++k) if (cnt[k] != 0ull) atomicAdd(&g_feat_counts[k], cnt[k]);
#endif
    }
}

// exact sum -> f64 value, hi/lo form (rt_kernels.hpp, fix_to_f64)
__device__ __forceinline__ double feat_fix_to_f64(unsigned long long q)
{
    return ((double)(uint32_t)(q >> 32) * 4294967296.0 + (double)(uint32_t)q) * (1.0 / 4294967296.0);
}

__global__ void features_to_f32_kernel(const unsigned long long *__restrict__ feat, float *__restrict__ out, long long npix, double spp)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; k < npix; k += stride) {
        const unsigned long long *q = feat + RT_FEATURE_WORDS * k;
        float *o = out + RT_FEATURE_WORDS * k;
        for (int c = 0; c < 3; ++c) o[c] = (float)(feat_fix_to_f64(q[c]) / spp);
        for (int c = 3; c < 6; ++c) {
            const bool neg = (long long)q[c] < 0;
            const double v = feat_fix_to_f64(neg ? 0ull - q[c] : q[c]);
            o[c] = (float)((neg ? -v : v) / spp);
        }
        const unsigned long long hits = q[7];
        o[6] = hits ? (float)(feat_fix_to_f64(q[6]) / (double)hits) : 0.0f;
        o[7] = (float)((double)hits / spp);
    }
}

} // namespace rt

namespace {

// What a feature launch accepts beyond validate_params: checked before anything is touched.  The checks that need no context come
// first (a caller without a device still gets the precise message), then the context's own.
int validate_features(const rt_context *ctx, const rt_camera *cam, const rt_params *p, const void *feat)
{
    int rc = validate_params(p);
    if (rc) return rc;
    if (p->flags & (RT_FLAG_UNIFORM53 | RT_FLAG_DIAG_STATS | RT_FLAG_NO_FILTER))
        return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers come from a kernel of their own: RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS and "
                    "RT_FLAG_NO_FILTER are not available on them (flags 0x%x)", p->flags);
    if (p->shard_count != 1)
        return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers are not sharded: shard_count must be 1 (is %d)", p->shard_count);
    if (p->spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers need spp >= 1 (is %d)", p->spp);
    if (!cam) return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers: cam is NULL");
    if (!feat) return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers: the feature buffer is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->scan_mode != 5)
        return fail(RT_ERR_INVALID_ARGUMENT, "feature buffers need the shipped scan mode 5; this context was created under RTIOW_SCAN_MODE=%d", ctx->scan_mode);
    return RT_OK;
}

int validate_to_f32(const rt_context *ctx, const void *feat, int32_t width, int32_t rows, int64_t spp, const void *out)
{
    if (width < 1 || rows < 0 || spp < 1)
        return fail(RT_ERR_INVALID_ARGUMENT, "features to f32: bad width/rows/spp (%d, %d, %lld)", width, rows, (long long)spp);
    if (rows > 0 && (!feat || !out)) return fail(RT_ERR_INVALID_ARGUMENT, "features to f32: a buffer is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return RT_OK;
}

} // namespace

extern "C" {

// bounce 0 of main.rs:122-136: the first hit of every camera ray
int rt_render_features_device(rt_context *ctx, const rt_camera *cam, const rt_params *p, void *d_feat, void *d_ids, void *stream_v)
{
    int rc = validate_features(ctx, cam, p, d_feat);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;

    rt::KParams kp;
    memset(&kp, 0, sizeof(kp));
    static_assert(sizeof(kp.cam) == sizeof(rt_camera), "camera layouts must match");
    memcpy(&kp.cam, cam, sizeof(rt_camera));
    kp.width = p->width; kp.height = p->height;
    kp.spp = p->spp; kp.sample_begin = p->sample_begin;
    kp.t_min = p->t_min;
    kp.k0 = (uint32_t)p->seed; kp.k1 = (uint32_t)(p->seed >> 32);
    kp.rows = p->height; kp.n_spheres = ctx->n_spheres;
    set_scene_params(ctx, kp);
    // (no launch slot: the kernel has no work counter and no statistics words, and rt_last_stats does not report on it)
    rt::FeatArgs fa;
    fa.feat = (unsigned long long *)d_feat;
    fa.ids = (int32_t *)d_ids;
    fa.accumulate = (p->flags & RT_FLAG_ACCUMULATE) ? 1 : 0;
    fa.tiles_x = ((uint32_t)p->width + 7u) / 8u;
    fa.n_wtiles = fa.tiles_x * (((uint32_t)p->height + 7u) / 8u);
    // one wave per pixel tile, handed out by the hardware as workgroups retire (tiles of sky are cheap, tiles of spheres are not: no
    // static split); the kernel's grid-stride loop takes over beyond 2^20 workgroups
    long long grid = ((long long)fa.n_wtiles + rt::kFeatWaves - 1) / rt::kFeatWaves;
    if (grid > (1 << 20)) grid = 1 << 20;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(rt::features_kernel, dim3((unsigned)grid), dim3(rt::kFeatBlock), 0, stream, kp, fa);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_render_features(rt_context *ctx, const rt_camera *cam, const rt_params *p, uint64_t *out_feat, int32_t *out_ids, float *kernel_ms)
{
    int rc = validate_features(ctx, cam, p, out_feat);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)p->width * p->height;
    const size_t feat_bytes = npix * RT_FEATURE_WORDS * sizeof(uint64_t), ids_bytes = out_ids ? npix * sizeof(int32_t) : 0;
    Stage st(ctx);
    const size_t b_feat = st.add(feat_bytes), b_ids = st.add(ids_bytes);
    if ((rc = st.commit())) return rc;
    rt_params q = *p;
    q.flags &= ~RT_FLAG_ACCUMULATE;                     // host form always starts from zero
    return timed_section(ctx, "rt_render_features", kernel_ms,
        [&] { return rt_render_features_device(ctx, cam, &q, st.at(b_feat), out_ids ? st.at(b_ids) : nullptr, ctx->own_stream); },
        [&] {
            const hipError_t he = st.down(out_feat, b_feat, feat_bytes);
            return he == hipSuccess && out_ids ? st.down(out_ids, b_ids, ids_bytes) : he;
        });
}

#ifdef RT_FEATURES_COUNT
// diagnostic builds only: reads the counters and zeroes them
int rt_debug_features_counts(rt_context *ctx, unsigned long long out[8])
{
    if (!ctx || !out) return fail(RT_ERR_INVALID_ARGUMENT, "ctx/out is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rt::g_feat_counts), 8 * sizeof(unsigned long long)));
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_feat_counts), zero, sizeof(zero)));
    return RT_OK;
}
#endif

int rt_features_to_f32_device(rt_context *ctx, const void *d_feat, int32_t width, int32_t rows, int64_t spp, void *d_out, void *stream_v)
{
    int rc = validate_to_f32(ctx, d_feat, width, rows, spp, d_out);
    if (rc) return rc;
    if (rows == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const long long npix = (long long)width * rows;
    hipLaunchKernelGGL(rt::features_to_f32_kernel, dim3(grid_256(npix)), dim3(256), 0, (hipStream_t)stream_v,
                       (const unsigned long long *)d_feat, (float *)d_out, npix, (double)spp);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_features_to_f32(rt_context *ctx, const uint64_t *feat, int32_t width, int32_t rows, int64_t spp, float *out)
{
    int rc = validate_to_f32(ctx, feat, width, rows, spp, out);
    if (rc) return rc;
    if (rows == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const size_t count = (size_t)width * rows * RT_FEATURE_WORDS;
    Stage st(ctx);
    const size_t b_feat = st.add(count * sizeof(uint64_t)), b_out = st.add(count * sizeof(float));
    if ((rc = st.commit())) return rc;
    RT_HIP(st.up(b_feat, feat, count * sizeof(uint64_t)));
    rc = rt_features_to_f32_device(ctx, st.at(b_feat), width, rows, spp, st.at(b_out), ctx->own_stream);
    if (rc) return rc;
    RT_HIP(st.down(out, b_out, count * sizeof(float)));
    RT_HIP(st.sync());
    return RT_OK;
}

} // extern "C"
