// rt_selftest.hip -- the known-answer hooks of the product library (rtiow_hip.h, "test hooks"): each runs ONE building block of the render
// kernel -- Philox, the f64 division and square root, quantize, the rejection tests -- on the caller's inputs, through the very functions
// of rt_device.hpp the kernel calls, and hands the results back for the tests to compare with known answers.  (The fifth hook,
// rt_filter_tube_device, stays in rt_api.hip with its kernel: see there.)
//
// A translation unit of librtiow_hip.so with kernels of its own and no render kernel.  The cross-check build
// (-DRTIOW_CROSSCHECK_MODES) adds the hooks of scan modes 2-4 and of the grid footprint here as well (xcheck/).
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_host.hpp"
#include "rt_device.hpp"

using namespace rt_host;

namespace rt {

__global__ void philox_kat_kernel(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                  uint32_t k0, uint32_t k1, uint32_t *out)
{
    const U4 r = philox4x32_10(c0, c1, c2, c3, k0, k1);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

__global__ void f64_div_sqrt_kernel(const double *a, const double *b, int n, double *q, double *r)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) { q[k] = a[k] / b[k]; r[k] = __builtin_sqrt(a[k]); }
}

// known-answer hook: the kernel's own quantize() (contract C5) on n radiance values
__global__ void quantize_kernel(const double *x, int n, unsigned long long *q)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) q[k] = quantize(x[k]);
}

// known-answer hook: the kernel's own rejection tests and word -> uniform conversions on n triples of Philox words.
// acc[k] = unit_sphere_accepts(w) | unit_disk_accepts(w.x, w.y) << 1; uni[k] = (u01(w.x), u11(w.x), u11(w.y), u11(w.z))
__global__ void unit_accept_kernel(const uint32_t *w, int n, uint32_t *acc, double *uni)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) {
        const uint32_t x = w[3 * k], y = w[3 * k + 1], z = w[3 * k + 2];
        acc[k] = (unit_sphere_accepts(x, y, z) ? 1u : 0u) | (unit_disk_accepts(x, y) ? 2u : 0u);
        uni[4 * k] = u01(x); uni[4 * k + 1] = u11(x); uni[4 * k + 2] = u11(y); uni[4 * k + 3] = u11(z);
    }
}

} // namespace rt

#ifdef RTIOW_CROSSCHECK_MODES
#include "xcheck/rt_xcheck_kernels.hpp"    // known-answer kernels of modes 2-4
#endif

extern "C" {

int rt_f64_div_sqrt_device(rt_context *ctx, const double *a, const double *b, int32_t n,
                           double *out_div, double *out_sqrt)
{
    if (!ctx || !a || !b || !out_div || !out_sqrt || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const auto d_a = st.in(a, (size_t)n), d_b = st.in(b, (size_t)n);
    const auto d_q = st.out(out_div, (size_t)n), d_r = st.out(out_sqrt, (size_t)n);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    hipLaunchKernelGGL(rt::f64_div_sqrt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->own_stream,
                       st.ptr(d_a), st.ptr(d_b), (int)n, st.ptr(d_q), st.ptr(d_r));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
    return RT_OK;
}

int rt_quantize_device(rt_context *ctx, const double *x, int32_t n, uint64_t *out)
{
    if (!ctx || !x || !out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const auto d_x = st.in(x, (size_t)n);
    const auto d_q = st.out(reinterpret_cast<unsigned long long *>(out), (size_t)n);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    hipLaunchKernelGGL(rt::quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->own_stream, st.ptr(d_x), (int)n, st.ptr(d_q));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
    return RT_OK;
}

int rt_unit_accept_device(rt_context *ctx, const uint32_t *words, int32_t n, uint32_t *out_accept, double *out_uniforms)
{
    if (!ctx || !words || !out_accept || !out_uniforms || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const auto d_u = st.out(out_uniforms, (size_t)n * 4);
    const auto d_w = st.in(words, (size_t)n * 3);
    const auto d_a = st.out(out_accept, (size_t)n);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    hipLaunchKernelGGL(rt::unit_accept_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->own_stream, st.ptr(d_w), (int)n, st.ptr(d_a),
                       st.ptr(d_u));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
    return RT_OK;
}

#ifdef RTIOW_CROSSCHECK_MODES
#include "xcheck/rt_xcheck_hooks.inc"      // rt_filter_products_device, rt_filter_lifted_device
#endif

int rt_philox_device(rt_context *ctx, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    if (!ctx || !ctr || !key || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const auto d_out = st.out(out, 4);
    int rc = st.commit();
    if (rc) return rc;
    hipLaunchKernelGGL(rt::philox_kat_kernel, dim3(1), dim3(1), 0, ctx->own_stream, ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], st.ptr(d_out));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
    return RT_OK;
}

} // extern "C"
