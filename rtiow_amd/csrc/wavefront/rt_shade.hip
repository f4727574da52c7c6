// rt_shade.hip -- wavefront path steps: camera rays, material scatter, accumulate (rtiow_hip.h, "wavefront path steps").
//
// The tenth translation unit of librtiow_hip.so.  Three kernels of its own, one lane per path, grid-stride over the batch: what a path needs
// besides its closest hit (rt_trace.hip) and what until now lived only inside render_kernel -- the camera ray of a (pixel, sample), Scatter::scatter
// of the three materials on the keyed Philox stream, and the sky term quantised into the exact sums.  The per-path bodies are rt_shade_core.hpp,
// which the fused bounce step of rt_paths.hip shares; the kernels here are load -> call -> store.  The bodies COMPOSE rt_device.hpp and state none of it again;
// rt_kernels.hpp, rt_device.hpp, rt_params.hpp, rt_launch.hpp, rt_api.hip, rt_dense.hip and rt_first_hit.hpp are untouched, so every other kernel
// keeps its machine code.  No LDS, no work queue, no scratch, no launch slot.  The sphere's material record is read through vector loads: the
// index diverges over the wave.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "rt_host.hpp"
#include "rt_shade_core.hpp"

using namespace rt_host;

namespace rt {

constexpr int kShadeBlock = 256;

struct CameraRayArgs {
    const uint32_t *pixel, *sample;     // [n]
    double *origin, *dir;               // [n][3]
    uint32_t *event;                    // [n]
    long long n;
    int32_t width, height;
    uint32_t k0, k1;
};

struct ScatterArgs {
    const double *dir;                  // [n][3]
    const int32_t *index;               // [n]
    const double *point, *normal;       // [n][3]
    const uint8_t *front;               // [n]
    const uint32_t *pixel, *sample;     // [n]
    uint32_t *event;                    // [n] in and out
    double *out_origin, *out_dir, *attenuation;     // [n][3]
    uint8_t *status;                    // [n]
    long long n;
    const double *mat;                  // [n_spheres][kMatStride]: the records rt_upload_scene keeps (rt_scene_core.hpp)
    int32_t n_spheres;
    uint32_t k0, k1;
};

struct AccumulateArgs {
    const uint32_t *pixel;              // [n]
    const double *weight;               // [n][3]
    const double *sky_dir;              // [n][3] or NULL
    const uint8_t *select;              // [n] or NULL
    long long n;
    unsigned long long *fix;            // [npix][3]
    unsigned long long npix;
};

// ---- sample_ray (rt_shade_core.hpp) -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kShadeBlock) void camera_rays_kernel(const KCamera cam, const CameraRayArgs A)
{
    const double wm1 = (double)(A.width - 1), hm1 = (double)(A.height - 1);
    const long long stride = (long long)gridDim.x * kShadeBlock;
    for (long long k = (long long)blockIdx.x * kShadeBlock + threadIdx.x; k < A.n; k += stride) {
        D3 origin, dir;
        const uint32_t ev = sample_ray(cam, (uint32_t)A.width, wm1, hm1, A.pixel[k], A.sample[k], A.k0, A.k1, origin, dir);
        store3(A.origin, k, origin);
        store3(A.dir, k, dir);
        A.event[k] = ev;
    }
}

// ---- Scatter::scatter (rt_shade_core.hpp) -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kShadeBlock) void scatter_kernel(const ScatterArgs A)
{
    const long long stride = (long long)gridDim.x * kShadeBlock;
    for (long long k = (long long)blockIdx.x * kShadeBlock + threadIdx.x; k < A.n; k += stride) {
        const int32_t hit = A.index[k];
        if (hit == -1) { A.status[k] = (uint8_t)RT_SCATTER_MISS; continue; }
        if (hit < -1 || hit >= A.n_spheres) { A.status[k] = (uint8_t)RT_SCATTER_BAD_INDEX; continue; }
        // the path's own elements, all read before anything is written (out_dir may be dir)
        const D3 d = ld3(A.dir + 3 * k), p = ld3(A.point + 3 * k), nrm = ld3(A.normal + 3 * k);
        const bool front = A.front[k] != 0;
        const uint32_t g_pix = A.pixel[k], g_s = A.sample[k];
        uint32_t ev = A.event[k];
        D3 ndir, albedo;
        const bool absorbed = scatter_path(A.mat + kMatStride * (size_t)hit, d, nrm, front, g_pix, g_s, ev, A.k0, A.k1, ndir, albedo);

        A.event[k] = ev;
        if (absorbed) {
            A.attenuation[3 * k] = 0.0; A.attenuation[3 * k + 1] = 0.0; A.attenuation[3 * k + 2] = 0.0;
            A.status[k] = (uint8_t)RT_SCATTER_ABSORBED;
        } else {
            store3(A.out_origin, k, p);
            store3(A.out_dir, k, ndir);
            store3(A.attenuation, k, albedo);
            A.status[k] = (uint8_t)RT_SCATTER_SCATTERED;
        }
    }
}

// ---- contract C5: quantize(weight * sky) into the exact sums ------------------------------------------------------------------------
__global__ __launch_bounds__(kShadeBlock) void accumulate_kernel(const AccumulateArgs A)
{
    const long long stride = (long long)gridDim.x * kShadeBlock;
    for (long long k = (long long)blockIdx.x * kShadeBlock + threadIdx.x; k < A.n; k += stride) {
        if (A.select && A.select[k] == 0) continue;
        const unsigned long long pix = A.pixel[k];
        if (pix >= A.npix) continue;
        D3 v = ld3(A.weight + 3 * k);
        if (A.sky_dir) v = sky_sample(v, ld3(A.sky_dir + 3 * k));
        unsigned long long *px = A.fix + (size_t)pix * 3u;
        atomicAdd(px + 0, quantize(v.x)); atomicAdd(px + 1, quantize(v.y)); atomicAdd(px + 2, quantize(v.z));
    }
}

} // namespace rt

namespace {

// RTIOW_SHADE_GRID_BLOCKS=k (diagnostic, read per call): at most k workgroups, so that the kernels' grid-stride trip runs at a test's size
unsigned shade_grid(long long n)
{
    unsigned grid = grid_256(n);
    const char *e = getenv("RTIOW_SHADE_GRID_BLOCKS");
    const long long cap = e && *e ? atoll(e) : 0;
    if (cap > 0 && (long long)grid > cap) grid = (unsigned)cap;
    return grid;
}

int check_n(const char *what, int64_t n)
{
    if (n < 0 || n > (int64_t)1 << 31) return fail(RT_ERR_INVALID_ARGUMENT, "%s: n must be in [0, 2^31] (is %lld)", what, (long long)n);
    return RT_OK;
}
int check_flags(const char *what, uint32_t flags)
{
    if (flags & RT_FLAG_UNIFORM53)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: RT_FLAG_UNIFORM53 is not built for the wavefront steps (flags 0x%x; only 0 is legal)", what, flags);
    if (flags) return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x (only 0 is legal)", what, flags);
    return RT_OK;
}
#define RT_NEED(ptr, what, name) \
    do { if (!(ptr)) return fail(RT_ERR_INVALID_ARGUMENT, "%s: %s is NULL", what, name); } while (0)

// What each step accepts, checked before anything is touched: the checks that need no context first, then the context's own, then the
// device.  *go: there are paths to run (an empty batch is RT_OK with nothing done).
int begin_camera_rays(const rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint32_t flags, const rt_camera_batch *b, bool *go)
{
    const char *what = "rt_camera_rays";
    *go = false;
    RT_NEED(cam, what, "cam");
    RT_NEED(b, what, "batch");
    if (int rc = check_n(what, b->n)) return rc;
    if (b->n > 0) {
        RT_NEED(b->pixel, what, "batch->pixel"); RT_NEED(b->sample, what, "batch->sample");
        RT_NEED(b->origin, what, "batch->origin"); RT_NEED(b->dir, what, "batch->dir"); RT_NEED(b->event, what, "batch->event");
    }
    if (width < 2 || height < 2) return fail(RT_ERR_INVALID_ARGUMENT, "%s: width and height must be >= 2 (are %d, %d)", what, width, height);
    if (int rc = check_flags(what, flags)) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (b->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    *go = true;
    return RT_OK;
}

int begin_scatter(const rt_context *ctx, uint32_t flags, const rt_scatter_batch *b, bool *go)
{
    const char *what = "rt_scatter";
    *go = false;
    RT_NEED(b, what, "batch");
    if (int rc = check_n(what, b->n)) return rc;
    if (b->n > 0) {
        RT_NEED(b->dir, what, "batch->dir"); RT_NEED(b->index, what, "batch->index"); RT_NEED(b->point, what, "batch->point");
        RT_NEED(b->normal, what, "batch->normal"); RT_NEED(b->front_face, what, "batch->front_face");
        RT_NEED(b->pixel, what, "batch->pixel"); RT_NEED(b->sample, what, "batch->sample"); RT_NEED(b->event, what, "batch->event");
        RT_NEED(b->out_origin, what, "batch->out_origin"); RT_NEED(b->out_dir, what, "batch->out_dir");
        RT_NEED(b->attenuation, what, "batch->attenuation"); RT_NEED(b->status, what, "batch->status");
    }
    if (int rc = check_flags(what, flags)) return rc;
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (b->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    *go = true;
    return RT_OK;
}

int begin_accumulate(const rt_context *ctx, const rt_accumulate_batch *b, const void *fix, int64_t npix, bool *go)
{
    const char *what = "rt_accumulate";
    *go = false;
    RT_NEED(b, what, "batch");
    RT_NEED(fix, what, "fix");
    if (int rc = check_n(what, b->n)) return rc;
    if (b->n > 0) { RT_NEED(b->pixel, what, "batch->pixel"); RT_NEED(b->weight, what, "batch->weight"); }
    if (npix <= 0 || npix > (int64_t)1 << 32) return fail(RT_ERR_INVALID_ARGUMENT, "%s: npix must be in [1, 2^32] (is %lld)", what, (long long)npix);
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (b->n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    *go = true;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_camera_rays_device(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags,
                          const rt_camera_batch *b, void *stream_v)
{
    bool go;
    int rc = begin_camera_rays(ctx, cam, width, height, flags, b, &go);
    if (rc || !go) return rc;
    rt::KCamera kc;
    static_assert(sizeof(rt::KCamera) == sizeof(rt_camera), "camera layouts must match");
    memcpy(&kc, cam, sizeof(rt_camera));
    rt::CameraRayArgs a;
    memset(&a, 0, sizeof(a));
    a.pixel = b->pixel; a.sample = b->sample; a.origin = b->origin; a.dir = b->dir; a.event = b->event; a.n = (long long)b->n;
    a.width = width; a.height = height;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(rt::camera_rays_kernel, dim3(shade_grid(a.n)), dim3(rt::kShadeBlock), 0, (hipStream_t)stream_v, kc, a);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_camera_rays(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags,
                   const rt_camera_batch *b, float *kernel_ms)
{
    bool go;
    int rc = begin_camera_rays(ctx, cam, width, height, flags, b, &go);
    if (rc || !go) return rc;
    const size_t n = (size_t)b->n, w32 = n * sizeof(uint32_t), v3 = n * 3 * sizeof(double);
    Stage st(ctx);
    const size_t b_pixel = st.add(w32), b_sample = st.add(w32), b_origin = st.add(v3), b_dir = st.add(v3), b_event = st.add(w32);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.up(b_pixel, b->pixel, w32));
    RT_HIP(st.up(b_sample, b->sample, w32));
    rt_camera_batch d;
    d.pixel = st.at<uint32_t>(b_pixel); d.sample = st.at<uint32_t>(b_sample);
    d.origin = st.at<double>(b_origin); d.dir = st.at<double>(b_dir); d.event = st.at<uint32_t>(b_event); d.n = b->n;
    return timed_section(ctx, "rt_camera_rays", kernel_ms,
        [&] { return rt_camera_rays_device(ctx, cam, width, height, seed, flags, &d, ctx->own_stream); },
        [&] {
            hipError_t he = st.down(b->origin, b_origin, v3);
            if (he == hipSuccess) he = st.down(b->dir, b_dir, v3);
            if (he == hipSuccess) he = st.down(b->event, b_event, w32);
            return he;
        });
}

int rt_scatter_device(rt_context *ctx, uint64_t seed, uint32_t flags, const rt_scatter_batch *b, void *stream_v)
{
    bool go;
    int rc = begin_scatter(ctx, flags, b, &go);
    if (rc || !go) return rc;
    rt::ScatterArgs a;
    memset(&a, 0, sizeof(a));
    a.dir = b->dir; a.index = b->index; a.point = b->point; a.normal = b->normal; a.front = b->front_face;
    a.pixel = b->pixel; a.sample = b->sample; a.event = b->event;
    a.out_origin = b->out_origin; a.out_dir = b->out_dir; a.attenuation = b->attenuation; a.status = b->status; a.n = (long long)b->n;
    a.mat = ctx->d_mat; a.n_spheres = ctx->n_spheres;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(rt::scatter_kernel, dim3(shade_grid(a.n)), dim3(rt::kShadeBlock), 0, (hipStream_t)stream_v, a);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_scatter(rt_context *ctx, uint64_t seed, uint32_t flags, const rt_scatter_batch *b, float *kernel_ms)
{
    bool go;
    int rc = begin_scatter(ctx, flags, b, &go);
    if (rc || !go) return rc;
    const size_t n = (size_t)b->n, w32 = n * sizeof(uint32_t), v3 = n * 3 * sizeof(double);
    const bool in_place = b->out_dir == b->dir;
    Stage st(ctx);
    const size_t b_dir = st.add(v3), b_index = st.add(n * sizeof(int32_t)), b_point = st.add(v3), b_normal = st.add(v3), b_front = st.add(n);
    const size_t b_pixel = st.add(w32), b_sample = st.add(w32), b_event = st.add(w32);
    const size_t b_oorg = st.add(v3), b_odir = in_place ? b_dir : st.add(v3), b_att = st.add(v3), b_status = st.add(n);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.up(b_dir, b->dir, v3));
    RT_HIP(st.up(b_index, b->index, n * sizeof(int32_t)));
    RT_HIP(st.up(b_point, b->point, v3));
    RT_HIP(st.up(b_normal, b->normal, v3));
    RT_HIP(st.up(b_front, b->front_face, n));
    RT_HIP(st.up(b_pixel, b->pixel, w32));
    RT_HIP(st.up(b_sample, b->sample, w32));
    RT_HIP(st.up(b_event, b->event, w32));
    // what the step leaves unwritten keeps the caller's bytes: the outputs go up as they are
    RT_HIP(st.up(b_oorg, b->out_origin, v3));
    if (!in_place) RT_HIP(st.up(b_odir, b->out_dir, v3));
    RT_HIP(st.up(b_att, b->attenuation, v3));
    rt_scatter_batch d;
    d.dir = st.at<double>(b_dir); d.index = st.at<int32_t>(b_index); d.point = st.at<double>(b_point); d.normal = st.at<double>(b_normal);
    d.front_face = st.at<uint8_t>(b_front); d.pixel = st.at<uint32_t>(b_pixel); d.sample = st.at<uint32_t>(b_sample);
    d.event = st.at<uint32_t>(b_event); d.out_origin = st.at<double>(b_oorg); d.out_dir = st.at<double>(b_odir);
    d.attenuation = st.at<double>(b_att); d.status = st.at<uint8_t>(b_status); d.n = b->n;
    return timed_section(ctx, "rt_scatter", kernel_ms,
        [&] { return rt_scatter_device(ctx, seed, flags, &d, ctx->own_stream); },
        [&] {
            hipError_t he = st.down(b->event, b_event, w32);
            if (he == hipSuccess) he = st.down(b->out_origin, b_oorg, v3);
            if (he == hipSuccess) he = st.down(b->out_dir, b_odir, v3);
            if (he == hipSuccess) he = st.down(b->attenuation, b_att, v3);
            if (he == hipSuccess) he = st.down(b->status, b_status, n);
            return he;
        });
}

int rt_accumulate_device(rt_context *ctx, const rt_accumulate_batch *b, void *d_fix, int64_t npix, void *stream_v)
{
    bool go;
    int rc = begin_accumulate(ctx, b, d_fix, npix, &go);
    if (rc || !go) return rc;
    rt::AccumulateArgs a;
    memset(&a, 0, sizeof(a));
    a.pixel = b->pixel; a.weight = b->weight; a.sky_dir = b->sky_dir; a.select = b->select; a.n = (long long)b->n;
    a.fix = (unsigned long long *)d_fix; a.npix = (unsigned long long)npix;
    hipLaunchKernelGGL(rt::accumulate_kernel, dim3(shade_grid(a.n)), dim3(rt::kShadeBlock), 0, (hipStream_t)stream_v, a);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_accumulate(rt_context *ctx, const rt_accumulate_batch *b, uint64_t *fix, int64_t npix, float *kernel_ms)
{
    bool go;
    int rc = begin_accumulate(ctx, b, fix, npix, &go);
    if (rc || !go) return rc;
    const size_t n = (size_t)b->n, w32 = n * sizeof(uint32_t), v3 = n * 3 * sizeof(double), fb = (size_t)npix * 3 * sizeof(uint64_t);
    Stage st(ctx);
    const size_t b_pixel = st.add(w32), b_weight = st.add(v3), b_sky = st.add(b->sky_dir ? v3 : 0), b_select = st.add(b->select ? n : 0);
    const size_t b_fix = st.add(fb);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.up(b_pixel, b->pixel, w32));
    RT_HIP(st.up(b_weight, b->weight, v3));
    if (b->sky_dir) RT_HIP(st.up(b_sky, b->sky_dir, v3));
    if (b->select) RT_HIP(st.up(b_select, b->select, n));
    RT_HIP(st.up(b_fix, fix, fb));
    rt_accumulate_batch d;
    d.pixel = st.at<uint32_t>(b_pixel); d.weight = st.at<double>(b_weight);
    d.sky_dir = b->sky_dir ? st.at<double>(b_sky) : nullptr; d.select = b->select ? st.at<uint8_t>(b_select) : nullptr; d.n = b->n;
    return timed_section(ctx, "rt_accumulate", kernel_ms,
        [&] { return rt_accumulate_device(ctx, &d, st.at(b_fix), npix, ctx->own_stream); },
        [&] { return st.down(fix, b_fix, fb); });
}

} // extern "C"
