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

// RTIOW_SHADE_GRID_BLOCKS: the diagnostic cap on the kernels' grids
unsigned shade_grid(long long n) { return (unsigned)capped_grid("RTIOW_SHADE_GRID_BLOCKS", grid_256(n)); }

const char *const kNoun = "the wavefront steps";

// What each step accepts, checked before anything is touched: the checks that need no context first, then the context's own, then the
// device.  *go: there are paths to run (an empty batch is RT_OK with nothing done).
int begin_camera_rays(const rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint32_t flags, const rt_camera_batch *b, bool *go)
{
    const char *what = "rt_camera_rays";
    *go = false;
    RT_NEED(cam, what, "cam");
    RT_NEED(b, what, "batch");
    if (int rc = check_count(what, b->n)) return rc;
    if (b->n > 0) {
        RT_NEED(b->pixel, what, "batch->pixel"); RT_NEED(b->sample, what, "batch->sample");
        RT_NEED(b->origin, what, "batch->origin"); RT_NEED(b->dir, what, "batch->dir"); RT_NEED(b->event, what, "batch->event");
    }
    if (int rc = check_frame_dims(what, width, height)) return rc;
    if (int rc = check_no_flags(what, flags, kNoun)) return rc;
    if (int rc = check_context(ctx, what, false, false)) return rc;
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
    if (int rc = check_count(what, b->n)) return rc;
    if (b->n > 0) {
        RT_NEED(b->dir, what, "batch->dir"); RT_NEED(b->index, what, "batch->index"); RT_NEED(b->point, what, "batch->point");
        RT_NEED(b->normal, what, "batch->normal"); RT_NEED(b->front_face, what, "batch->front_face");
        RT_NEED(b->pixel, what, "batch->pixel"); RT_NEED(b->sample, what, "batch->sample"); RT_NEED(b->event, what, "batch->event");
        RT_NEED(b->out_origin, what, "batch->out_origin"); RT_NEED(b->out_dir, what, "batch->out_dir");
        RT_NEED(b->attenuation, what, "batch->attenuation"); RT_NEED(b->status, what, "batch->status");
    }
    if (int rc = check_no_flags(what, flags, kNoun)) return rc;
    if (int rc = check_context(ctx, what, false, true)) return rc;
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
    if (int rc = check_count(what, b->n)) return rc;
    if (b->n > 0) { RT_NEED(b->pixel, what, "batch->pixel"); RT_NEED(b->weight, what, "batch->weight"); }
    if (int rc = check_npix(what, npix)) return rc;
    if (int rc = check_context(ctx, what, false, false)) return rc;
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
    rt::CameraRayArgs a;
    memset(&a, 0, sizeof(a));
    a.pixel = b->pixel; a.sample = b->sample; a.origin = b->origin; a.dir = b->dir; a.event = b->event; a.n = (long long)b->n;
    a.width = width; a.height = height;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(rt::camera_rays_kernel, dim3(shade_grid(a.n)), dim3(rt::kShadeBlock), 0, (hipStream_t)stream_v, to_kcamera(cam), a);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_camera_rays(rt_context *ctx, const rt_camera *cam, int32_t width, int32_t height, uint64_t seed, uint32_t flags,
                   const rt_camera_batch *b, float *kernel_ms)
{
    bool go;
    int rc = begin_camera_rays(ctx, cam, width, height, flags, b, &go);
    if (rc || !go) return rc;
    const size_t n = (size_t)b->n;
    Stage st(ctx);
    const auto pixel = st.in(b->pixel, n), sample = st.in(b->sample, n);
    const auto origin = st.out(b->origin, 3 * n), dir = st.out(b->dir, 3 * n);
    const auto event = st.out(b->event, n);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    const rt_camera_batch d = {st.ptr(pixel), st.ptr(sample), st.ptr(origin), st.ptr(dir), st.ptr(event), b->n};
    return timed_section(ctx, "rt_camera_rays", kernel_ms, st,
        [&] { return rt_camera_rays_device(ctx, cam, width, height, seed, flags, &d, ctx->own_stream); });
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
    const size_t n = (size_t)b->n;
    // out_dir == dir: ONE block serves both fields -- the directions go up, the step writes the scattered ones over their own, and the
    // block comes down into out_dir
    const bool in_place = b->out_dir == b->dir;
    Stage st(ctx);
    Staged<const double> dir;
    Staged<double> out_dir;
    if (in_place) out_dir = st.inout(b->out_dir, 3 * n);
    else dir = st.in(b->dir, 3 * n);
    const auto index = st.in(b->index, n);
    const auto point = st.in(b->point, 3 * n), normal = st.in(b->normal, 3 * n);
    const auto front = st.in(b->front_face, n);
    const auto pixel = st.in(b->pixel, n), sample = st.in(b->sample, n);
    const auto event = st.inout(b->event, n);
    // what the step leaves unwritten keeps the caller's bytes: the outputs go up as they are (inout), all but the status
    const auto out_origin = st.inout(b->out_origin, 3 * n);
    if (!in_place) out_dir = st.inout(b->out_dir, 3 * n);
    const auto attenuation = st.inout(b->attenuation, 3 * n);
    const auto status = st.out(b->status, n);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    const rt_scatter_batch d = {in_place ? st.ptr(out_dir) : st.ptr(dir), st.ptr(index), st.ptr(point), st.ptr(normal), st.ptr(front), st.ptr(pixel), st.ptr(sample),
                                st.ptr(event), st.ptr(out_origin), st.ptr(out_dir), st.ptr(attenuation), st.ptr(status), b->n};
    return timed_section(ctx, "rt_scatter", kernel_ms, st, [&] { return rt_scatter_device(ctx, seed, flags, &d, ctx->own_stream); });
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
    const size_t n = (size_t)b->n;
    Stage st(ctx);
    const auto pixel = st.in(b->pixel, n);
    const auto weight = st.in(b->weight, 3 * n), sky_dir = st.in(b->sky_dir, 3 * n);
    const auto select = st.in(b->select, n);
    const auto sums = st.inout(fix, (size_t)npix * 3);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    const rt_accumulate_batch d = {st.ptr(pixel), st.ptr(weight), st.ptr(sky_dir), st.ptr(select), b->n};
    return timed_section(ctx, "rt_accumulate", kernel_ms, st,
        [&] { return rt_accumulate_device(ctx, &d, st.ptr(sums), npix, ctx->own_stream); });
}

} // extern "C"
