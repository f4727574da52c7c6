// rt_adaptive.hip -- adaptive sampling (rtiow_hip.h, "adaptive sampling"): the error estimate and the selection of the
// pixels that get more samples, on the device and on the host, and the driver that renders a frame with them.
//
// A translation unit of librtiow_hip.so with kernels of its own and no render kernel: the selection kernels, the add-back of a pass's
// compact sums, and the two small helpers of the driver.  rt_render_adaptive renders through rt_render_device and
// rt_render_pixels_device (rt_api.hip) like any caller of the C ABI; what it shares with them is rt_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_host.hpp"
#include "rt_adaptive_check.hpp"

using namespace rt_host;

namespace rt {

// ---- adaptive sampling: error estimate, selection, add-back (rtiow_hip.h, rt_select_pixels_device) ----
// The rule, stated once for the device and the host (rt_select_pixels_host compiles this very function): is pixel p, whose sums hold n
// samples of which `half` holds n / 2, still noisy?  Integers for the differences, then binary64 in the written order (-ffp-contract=off).
__host__ __device__ inline bool select_noisy(const unsigned long long *fix, const unsigned long long *half, double sc, double threshold,
                                             double dark_floor)
{
    double D = 0.0, S = 0.0;
    for (int c = 0; c < 3; ++c) {
        const long long t = (long long)(2ull * half[c] - fix[c]);          // fits: n <= 32766 samples of <= 2^48 each
        const unsigned long long d = t < 0 ? (unsigned long long)(-t) : (unsigned long long)t;
        D = c == 0 ? (double)d : D + (double)d;                             // ((d_r + d_g) + d_b)
        S = c == 0 ? (double)fix[c] : S + (double)fix[c];
    }
    const double m = S * sc;
    const double err = (D * sc) / __builtin_sqrt(m > dark_floor ? m : dark_floor);
    return !(err <= threshold);
}

constexpr int kSelBlock = 256;      // pixels per workgroup of the selection kernels (consecutive pixel numbers)

// (1) noisy[p] = candidate && !(err <= threshold)
__global__ __launch_bounds__(kSelBlock) void select_noisy_kernel(const unsigned long long *__restrict__ fix, const unsigned long long *__restrict__ half,
                                                                 const uint32_t *__restrict__ count, uint32_t npix, uint32_t n, double sc,
                                                                 double threshold, double dark_floor, uint8_t *__restrict__ noisy)
{
    const uint32_t p = blockIdx.x * (uint32_t)kSelBlock + threadIdx.x;
    if (p >= npix) return;
    noisy[p] = (count[p] == n && select_noisy(fix + (size_t)p * 3u, half + (size_t)p * 3u, sc, threshold, dark_floor)) ? 1 : 0;
}

// (2) active[p] = candidate && (a pixel of the 3x3 neighbourhood, clipped at the frame's edges, is noisy); block_count[b] = how many in workgroup b
__global__ __launch_bounds__(kSelBlock) void select_active_kernel(const uint8_t *__restrict__ noisy, const uint32_t *__restrict__ count,
                                                                  int width, int height, uint32_t n, uint8_t *__restrict__ active,
                                                                  uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t s_cnt[kSelBlock / 64];
    const uint32_t npix = (uint32_t)width * (uint32_t)height;
    const uint32_t p = blockIdx.x * (uint32_t)kSelBlock + threadIdx.x;
    bool act = false;
    if (p < npix && count[p] == n) {
        const int j = (int)(p / (uint32_t)width), i = (int)(p - (uint32_t)j * (uint32_t)width);
        const int j0 = j > 0 ? j - 1 : 0, j1 = j < height - 1 ? j + 1 : height - 1;
        const int i0 = i > 0 ? i - 1 : 0, i1 = i < width - 1 ? i + 1 : width - 1;
        for (int jj = j0; jj <= j1; ++jj)
            for (int ii = i0; ii <= i1; ++ii) act = act || noisy[(size_t)jj * (size_t)width + (size_t)ii] != 0;
    }
    if (p < npix) active[p] = act ? 1 : 0;
    const unsigned long long m = __ballot(act);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// (3) exclusive scan of the workgroups' counts, in place, by ONE workgroup (chunks of 1 024 with a running carry); the total -> *n_out
__global__ __launch_bounds__(1024) void select_scan_kernel(uint32_t *__restrict__ block_count, uint32_t n_blocks, uint32_t *__restrict__ n_out)
{
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_carry = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < n_blocks; base += 1024u) {
        const uint32_t k = base + tid;
        const uint32_t v = k < n_blocks ? block_count[k] : 0u;
        uint32_t x = v;                                                     // inclusive scan within the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d);
            if (lane >= (uint32_t)d) x += y;
        }
        if (lane == 63u) s_wave[wave] = x;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        if (k < n_blocks) block_count[k] = before + x - v;
        __syncthreads();
        if (tid == 1023u) s_carry = before + x;
        __syncthreads();
    }
    if (tid == 0) *n_out = s_carry;
}

// (4) the active pixels' numbers, ascending: workgroup offset + the waves before this one + the rank within the wave (ballot + v_mbcnt)
__global__ __launch_bounds__(kSelBlock) void select_write_kernel(const uint8_t *__restrict__ active, const uint32_t *__restrict__ block_offset,
                                                                 uint32_t npix, uint32_t *__restrict__ list)
{
    __shared__ uint32_t s_cnt[kSelBlock / 64];
    const uint32_t p = blockIdx.x * (uint32_t)kSelBlock + threadIdx.x;
    const bool act = p < npix && active[p] != 0;
    const unsigned long long m = __ballot(act);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t at = block_offset[blockIdx.x];
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) at += s_cnt[w];
    at += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (act) list[at] = p;                                                  // (at < the total <= npix = the list's capacity)
}

// One pass's compact sums back into the frame's state at the listed pixels (no duplicates in a selection's list): fix += pass,
// half += pass on the even-numbered passes (half != nullptr), count += step.
__global__ void add_back_kernel(const uint32_t *__restrict__ list, uint32_t n_list, const unsigned long long *__restrict__ pass,
                                unsigned long long *__restrict__ fix, unsigned long long *__restrict__ half, uint32_t *__restrict__ count,
                                uint32_t step)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_list) return;
    const size_t g = list[k];
    for (int c = 0; c < 3; ++c) {
        const unsigned long long v = pass[(size_t)k * 3u + c];
        fix[g * 3u + c] += v;
        if (half) half[g * 3u + c] += v;
    }
    count[g] += step;
}

__global__ void fill_u32_kernel(uint32_t *__restrict__ dst, uint32_t value, uint32_t n)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[k] = value;
}

// a launch's counters (KParams::stats [0..4]) added to a running total: rt_render_adaptive reads the total once, at the end
__global__ void stats_accumulate_kernel(const unsigned long long *__restrict__ stats, unsigned long long *__restrict__ total)
{
    if (threadIdx.x < 5) total[threadIdx.x] += stats[threadIdx.x];
}

} // namespace rt

int rt_host::validate_adaptive(const rt_adaptive *a)
{
    if (!a) return fail(RT_ERR_INVALID_ARGUMENT, "rt_adaptive is NULL");
    if (a->step < 1) return fail(RT_ERR_INVALID_ARGUMENT, "rt_adaptive.step must be >= 1 (is %d)", a->step);
    if (a->reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_adaptive.reserved must be 0");
    if (!(a->threshold >= 0.0)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_adaptive.threshold must be >= 0 (and not a NaN)");
    if (!(a->dark_floor > 0.0) || !(a->dark_floor < INFINITY))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_adaptive.dark_floor must be > 0 and finite (with a zero floor a black pixel's error is 0/0)");
    return RT_OK;
}

int rt_host::check_adaptive_frame(const char *what, const rt_params *p, const rt_adaptive *a)
{
    if (p->sample_begin != 0) return fail(RT_ERR_INVALID_ARGUMENT, "%s numbers its own passes: sample_begin must be 0 (is %d)", what, p->sample_begin);
    if (p->spp < 2 * (long long)a->step || p->spp % (2 * (long long)a->step) != 0 || p->spp > kAdaptiveMaxSpp)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: spp = %d (the most samples a pixel may get) must be a multiple of 2 * step = %lld and <= %d", what,
                    p->spp, 2 * (long long)a->step, kAdaptiveMaxSpp);
    return RT_OK;
}

namespace {

int validate_select(const void *fix, const void *half, const void *count, int32_t width, int32_t height, int32_t n, const rt_adaptive *a,
                    const void *list_out, const void *n_out)
{
    if (!fix || !half || !count || !list_out || !n_out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_select_pixels: a buffer is NULL");
    if (width < 1 || height < 1 || (long long)width * height > 0x7fffffffLL)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_select_pixels: bad width/height");
    if (n < 2 || n > kAdaptiveMaxSpp || (n & 1))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_select_pixels: n = %d samples must be even (two halves) and in [2, %d]", n, kAdaptiveMaxSpp);
    return validate_adaptive(a);
}

} // namespace

extern "C" {

int rt_select_pixels_host(const uint64_t *fix, const uint64_t *half, const uint32_t *count, int32_t width, int32_t height,
                          int32_t n, const rt_adaptive *a, uint32_t *list_out, int64_t *n_out)
{
    int rc = validate_select(fix, half, count, width, height, n, a, list_out, n_out);
    if (rc) return rc;
    const size_t npix = (size_t)width * height;
    std::vector<char> noisy(npix);
    const double sc = 1.0 / ((double)n * 4294967296.0);
    for (size_t p = 0; p < npix; ++p)
        noisy[p] = count[p] == (uint32_t)n &&
                   rt::select_noisy((const unsigned long long *)fix + p * 3, (const unsigned long long *)half + p * 3, sc, a->threshold, a->dark_floor);
    int64_t m = 0;
    for (int j = 0; j < height; ++j)
        for (int i = 0; i < width; ++i) {
            const size_t p = (size_t)j * width + i;
            if (count[p] != (uint32_t)n) continue;
            bool act = false;
            for (int jj = std::max(j - 1, 0); jj <= std::min(j + 1, height - 1); ++jj)
                for (int ii = std::max(i - 1, 0); ii <= std::min(i + 1, width - 1); ++ii) act = act || noisy[(size_t)jj * width + ii];
            if (act) list_out[m++] = (uint32_t)p;
        }
    *n_out = m;
    return RT_OK;
}

int rt_select_pixels_device(rt_context *ctx, const void *d_fix, const void *d_half, const void *d_count, int32_t width,
                            int32_t height, int32_t n, const rt_adaptive *a, void *d_list_out, void *d_n_out, void *stream_v)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    int rc = validate_select(d_fix, d_half, d_count, width, height, n, a, d_list_out, d_n_out);
    if (rc) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    const uint32_t npix = (uint32_t)((long long)width * height);
    const uint32_t blocks = (npix + rt::kSelBlock - 1) / rt::kSelBlock;
    // scratch: noisy[npix], active[npix] (bytes, each rounded up to 256), the workgroups' counts [blocks]
    const size_t flags_bytes = ((size_t)npix + 255) / 256 * 256;
    rc = ensure(ctx->sel, 2 * flags_bytes + (size_t)blocks * sizeof(uint32_t));
    if (rc) return rc;
    uint8_t *noisy = (uint8_t *)ctx->sel.ptr, *active = noisy + flags_bytes;
    uint32_t *block_count = (uint32_t *)(active + flags_bytes);
    const double sc = 1.0 / ((double)n * 4294967296.0);
    hipLaunchKernelGGL(rt::select_noisy_kernel, dim3(blocks), dim3(rt::kSelBlock), 0, stream, (const unsigned long long *)d_fix,
                       (const unsigned long long *)d_half, (const uint32_t *)d_count, npix, (uint32_t)n, sc, a->threshold, a->dark_floor, noisy);
    hipLaunchKernelGGL(rt::select_active_kernel, dim3(blocks), dim3(rt::kSelBlock), 0, stream, (const uint8_t *)noisy,
                       (const uint32_t *)d_count, (int)width, (int)height, (uint32_t)n, active, block_count);
    hipLaunchKernelGGL(rt::select_scan_kernel, dim3(1), dim3(1024), 0, stream, block_count, blocks, (uint32_t *)d_n_out);
    hipLaunchKernelGGL(rt::select_write_kernel, dim3(blocks), dim3(rt::kSelBlock), 0, stream, (const uint8_t *)active,
                       (const uint32_t *)block_count, npix, (uint32_t *)d_list_out);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_render_adaptive(rt_context *ctx, const rt_camera *cam, const rt_params *p, const rt_adaptive *a,
                       uint64_t *out_fix, uint64_t *out_half, uint32_t *out_count, rt_stats *stats)
{
    int rc = validate_params(p);
    if (rc) return rc;
    rc = validate_adaptive(a);
    if (rc) return rc;
    rc = check_adaptive_frame("rt_render_adaptive", p, a);
    if (rc) return rc;
    rc = validate_pixel_list(ctx, cam, p, 0);
    if (rc) return rc;
    if (!out_fix || !out_count) return fail(RT_ERR_INVALID_ARGUMENT, "out_fix/out_count is NULL");
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->own_stream;
    const size_t npix = (size_t)p->width * p->height;
    // the frame's state, all on the device: fix | half | one pass's compact sums | count | list | the 64-byte counter block: the running
    // counters (5 x u64), then the list length (one word)
    unsigned long long total[8];
    Stage st(ctx);
    const auto fix = st.out(out_fix, npix * 3);
    const auto half = out_half ? st.out(out_half, npix * 3) : st.scratch<uint64_t>(npix * 3);       // (the selection reads it either way)
    const auto pass = st.scratch<uint64_t>(npix * 3);
    const auto count = st.out(out_count, npix);
    const auto list = st.scratch<uint32_t>(npix);
    const auto counters = st.out(total, 8);
    if ((rc = st.commit())) return rc;
    uint64_t *d_fix = st.ptr(fix), *d_half = st.ptr(half), *d_pass = st.ptr(pass);
    uint32_t *d_count = st.ptr(count), *d_list = st.ptr(list);
    unsigned long long *d_total = st.ptr(counters);
    uint32_t *d_n = (uint32_t *)(d_total + 5);
    RT_HIP(hipMemsetAsync(d_total, 0, sizeof(total), stream));

    const uint32_t step = (uint32_t)a->step;
    float kernel_ms = 0.0f;
    unsigned long long zero_depth = 0;
    rt_stats shape{};                                                    // grid, variant ... of the latest launch
    int round_slots[2] = {0, 0};
    auto after_pass = [&](int k) -> int {                                // the launch's counters -> the running total; remember its events
        hipLaunchKernelGGL(rt::stats_accumulate_kernel, dim3(1), dim3(64), 0, stream, (const unsigned long long *)ctx->d_stats, d_total);
        RT_HIP(hipGetLastError());
        zero_depth += ctx->zero_depth_samples;
        round_slots[k] = ctx->cur;
        shape = ctx->last;
        return RT_OK;
    };
    auto round_time = [&]() -> int {                                     // (after the round's synchronise: both passes have finished)
        for (int k = 0; k < 2; ++k) {
            float ms = 0.0f;
            RT_HIP(hipEventElapsedTime(&ms, ctx->e0_slots[round_slots[k]], ctx->e1_slots[round_slots[k]]));
            kernel_ms += ms;
        }
        return RT_OK;
    };
    rt_params q = *p;
    q.spp = (int32_t)step;
    // round 1: every pixel, through the dense kernel.  Pass 0 -> fix, a copy of it is `half`, pass 1 is added to fix.
    q.sample_begin = 0; q.flags = p->flags & ~RT_FLAG_ACCUMULATE;
    rc = rt_render_device(ctx, cam, &q, d_fix, stream);
    if (rc) return rc;
    if ((rc = after_pass(0))) return rc;
    RT_HIP(hipMemcpyAsync(d_half, d_fix, npix * 3 * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    q.sample_begin = (int32_t)step; q.flags = p->flags | RT_FLAG_ACCUMULATE;
    rc = rt_render_device(ctx, cam, &q, d_fix, stream);
    if (rc) return rc;
    if ((rc = after_pass(1))) return rc;
    hipLaunchKernelGGL(rt::fill_u32_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, d_count, 2u * step, (uint32_t)npix);
    RT_HIP(hipGetLastError());
    q.flags = p->flags & ~RT_FLAG_ACCUMULATE;
    for (uint32_t n = 2u * step; ; n += 2u * step) {
        uint32_t n_list = 0;
        if (n < (uint32_t)p->spp) {
            rc = rt_select_pixels_device(ctx, d_fix, d_half, d_count, p->width, p->height, (int32_t)n, a, d_list, d_n, stream);
            if (rc) return rc;
            RT_HIP(hipMemcpyAsync(&n_list, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));    // the round's ONE word
        }
        RT_HIP(st.sync());
        if ((rc = round_time())) return rc;
        if (n_list == 0u) break;
        for (int k = 0; k < 2; ++k) {                                    // passes n / step (even: also into half) and n / step + 1
            q.sample_begin = (int32_t)(n + (uint32_t)k * step);
            rc = rt_render_pixels_device(ctx, cam, &q, d_list, (int64_t)n_list, d_pass, stream);
            if (rc) return rc;
            if ((rc = after_pass(k))) return rc;
            hipLaunchKernelGGL(rt::add_back_kernel, dim3((n_list + 255u) / 256u), dim3(256), 0, stream, (const uint32_t *)d_list, n_list,
                               (const unsigned long long *)d_pass, (unsigned long long *)d_fix,
                               k == 0 ? (unsigned long long *)d_half : (unsigned long long *)nullptr, d_count, step);
            RT_HIP(hipGetLastError());
        }
    }
    RT_HIP(st.finish());                                // the sums, half if asked for, the counts and the counter block
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->n_spheres = shape.n_spheres; stats->grid_blocks = shape.grid_blocks; stats->block_threads = shape.block_threads;
        stats->scan_mode = shape.scan_mode; stats->kernel_variant = shape.kernel_variant;
        stats->rays_traced = total[0];
        stats->samples = total[1] + zero_depth;
        stats->direct_samples = total[4];
        stats->sphere_tests = total[0] * (unsigned long long)(shape.n_spheres > 0 ? shape.n_spheres : 0);
        stats->kernel_ms = kernel_ms;
    }
    return RT_OK;
}

} // extern "C"
