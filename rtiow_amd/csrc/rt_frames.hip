// rt_frames.hip -- frame batches: n_frames cameras over the uploaded scene in ONE launch (rtiow_hip.h, "frame batches").
//
// The second translation unit of librtiow_hip.so.  It owns the frame-batch instantiations of the render kernel,
// rt::render_kernel<5, false, SMALLGRID, false, rt::kItemBlockFrames> (rt_kernels.hpp), and the three entry points that launch
// them: their validation, the frame fields of KParams and the kernel choice.  The context, validate_params and the launch path that
// the dense and the pixel-list renders take as well (plan_launch, fill_common_params, run_launch) are shared through rt_host.hpp and
// rt_launch.hpp.  This file defines no other kernel (the resolve of its rgba8 form is rt_api.hip's).
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_launch.hpp"

using namespace rt_host;

namespace {

// work blocks as rt_render_pixels_device takes them: the shipped kernel's ring of 2 x 16 pixel slots, never the blocks of 1 024
LaunchPlan frames_plan(int spp, int ring_min_spp) { return plan_launch(spp, ring_min_spp, true, false, false, 0, 0); }

// What a frame batch accepts beyond validate_params: checked before anything is touched.  The checks that need no context come first
// (a caller without a device still gets the precise message), then the context's own.
int validate_frames(const rt_context *ctx, int32_t n_frames, int32_t sample_stride, const rt_params *p)
{
    int rc = validate_params(p);
    if (rc) return rc;
    if (p->flags & (RT_FLAG_UNIFORM53 | RT_FLAG_DIAG_STATS | RT_FLAG_NO_FILTER))
        return fail(RT_ERR_INVALID_ARGUMENT, "frame batches run the shipped kernel only: RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS and "
                    "RT_FLAG_NO_FILTER are not available on them (flags 0x%x)", p->flags);
    if (p->shard_count != 1)
        return fail(RT_ERR_INVALID_ARGUMENT, "frame batches are not sharded: shard_count must be 1 (is %d)", p->shard_count);
    if (n_frames < 0) return fail(RT_ERR_INVALID_ARGUMENT, "n_frames must be >= 0 (is %d)", n_frames);
    if (sample_stride < 0) return fail(RT_ERR_INVALID_ARGUMENT, "sample_stride must be >= 0 (is %d)", sample_stride);
    const long long frame_pix = (long long)p->width * p->height;
    if ((long long)n_frames * frame_pix > 0x80000000LL)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_frames*width*height = %lld pixels in one batch: at most 2^31", (long long)n_frames * frame_pix);
    if (n_frames > 0 && (long long)p->sample_begin + (long long)(n_frames - 1) * sample_stride + p->spp > 0x7fffffffLL)
        return fail(RT_ERR_INVALID_ARGUMENT, "sample_begin + (n_frames-1)*sample_stride + spp = %lld: the last frame's sample indices must stay "
                    "below 2^31", (long long)p->sample_begin + (long long)(n_frames - 1) * sample_stride + p->spp);
    const unsigned item_block = frames_plan(p->spp, ctx ? ctx->ring_min_spp : 0).block_items;
    const unsigned long long frame_blocks = ((unsigned long long)frame_pix * (unsigned long long)p->spp + item_block - 1) / item_block;
    if (frame_blocks * (unsigned long long)n_frames > 0x7fffffffULL)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_frames*ceil(width*height*spp / %u) = %llu work blocks in one batch: at most 2^31 - 1 "
                    "(split the batch, or the samples with sample_begin and RT_FLAG_ACCUMULATE)", item_block, frame_blocks * (unsigned long long)n_frames);
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->scan_mode != 5)
        return fail(RT_ERR_INVALID_ARGUMENT, "frame batches need the shipped scan mode 5; this context was created under RTIOW_SCAN_MODE=%d", ctx->scan_mode);
    return RT_OK;
}

} // namespace

extern "C" {

// main.rs:108-139, once per camera, in one launch
int rt_render_frames_device(rt_context *ctx, const rt_camera *d_cams, int32_t n_frames, int32_t sample_stride,
                            const rt_params *p, void *d_fix, void *stream_v)
{
    int rc = validate_frames(ctx, n_frames, sample_stride, p);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (n_frames == 0) return RT_OK;
    if (!d_cams || !d_fix) return fail(RT_ERR_INVALID_ARGUMENT, "d_cams/d_fix is NULL");
    const unsigned long long frame_pix = (unsigned long long)p->width * (unsigned long long)p->height;
    const unsigned long long frame_items = frame_pix * (unsigned long long)p->spp;
    const unsigned long long total_items = frame_items * (unsigned long long)n_frames;
    const LaunchPlan plan = frames_plan(p->spp, ctx->ring_min_spp);
    // a work block never straddles two frames: every frame has its own ceil(frame_items / block_items) blocks, the last one short
    const unsigned long long frame_blocks = (frame_items + plan.block_items - 1) / plan.block_items;
    const unsigned long long n_blocks = frame_blocks * (unsigned long long)n_frames;      // (<= 2^31 - 1: validate_frames)
    RT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;

    rt::KParams kp;
    static_assert(sizeof(rt::KCamera) == sizeof(rt_camera) && sizeof(rt_camera) == 19 * sizeof(double), "camera layouts must match");
    fill_common_params(ctx, p, plan, frame_pix * (unsigned long long)n_frames, total_items, n_blocks, d_fix, kp);   // (the kernel does not read npix)
    kp.rows = p->height;                                                 // (rows and the sharding fields are unused by the variant; no magic_tile)
    kp.magic_width = magic_for(p->width);
    kp.cams = reinterpret_cast<const rt::KCamera *>(d_cams);
    kp.frame_items = frame_items;
    kp.frame_blocks = (uint32_t)frame_blocks;
    kp.inv_frame_blocks = frame_blocks > 0 ? 1.0 / (double)frame_blocks : 0.0;
    kp.frame_pix = (uint32_t)frame_pix;
    kp.sample_stride = sample_stride;
    const size_t clear_bytes = (p->flags & RT_FLAG_ACCUMULATE) ? 0 : (size_t)(frame_pix * (unsigned long long)n_frames) * 3 * sizeof(unsigned long long);
    // The untraced exit (max_depth 0) reports scan_mode 5 here, where the dense and the pixel-list launches report 0: nobody chose the
    // difference, and rt_last_stats keeps it.
    return run_launch(ctx, stream, kp, p->max_depth, clear_bytes, 5, [&](int *grid) {
        const bool small_grid = small_grid_scene(ctx);
        ctx->last.scan_mode = 5;
        ctx->last.kernel_variant = 16 | (small_grid ? 1 : 0);
        return small_grid ? launch_render<5, false, true, false, rt::kItemBlockFrames>(ctx, kp, stream, grid)      // (the frame-batch instantiations)
                          : launch_render<5, false, false, false, rt::kItemBlockFrames>(ctx, kp, stream, grid);
    });
}

int rt_render_frames(rt_context *ctx, const rt_camera *cams, int32_t n_frames, int32_t sample_stride,
                     const rt_params *p, uint64_t *out_fix, rt_stats *stats)
{
    int rc = validate_frames(ctx, n_frames, sample_stride, p);
    if (rc) return rc;
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (n_frames == 0) return RT_OK;
    if (!cams || !out_fix) return fail(RT_ERR_INVALID_ARGUMENT, "cams/out_fix is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t count = (size_t)n_frames * p->width * p->height * 3;
    Stage st(ctx);
    const auto sums = st.out(out_fix, count);
    const auto d_cams = st.in(cams, (size_t)n_frames);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    rt_params q = *p;
    q.flags &= ~RT_FLAG_ACCUMULATE;                     // host form always starts from zero
    rc = rt_render_frames_device(ctx, st.ptr(d_cams), n_frames, sample_stride, &q, st.ptr(sums), ctx->own_stream);
    if (rc) return rc;
    RT_HIP(st.finish());
    if (stats) return rt_last_stats(ctx, stats);
    return RT_OK;
}

// main.rs:108-145 once per camera: the sums stay on the device, 4 bytes per pixel come back
int rt_render_frames_rgba8(rt_context *ctx, const rt_camera *cams, int32_t n_frames, int32_t sample_stride,
                           const rt_params *p, int32_t flip, uint8_t *out_rgba, rt_stats *stats)
{
    int rc = validate_frames(ctx, n_frames, sample_stride, p);
    if (rc) return rc;
    if (p->spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_frames_rgba8 needs spp >= 1 (to_rgba divides by the sample count, vec3.rs:409)");
    if (ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (n_frames == 0) return RT_OK;
    if (!cams || !out_rgba) return fail(RT_ERR_INVALID_ARGUMENT, "cams/out_rgba is NULL");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t frame_pix = (size_t)p->width * p->height;
    const size_t npix = frame_pix * (size_t)n_frames;
    Stage st(ctx);
    const auto sums = st.scratch<uint64_t>(npix * 3);
    const auto rgba = st.out(out_rgba, npix * 4);
    const auto d_cams = st.in(cams, (size_t)n_frames);
    if ((rc = st.commit())) return rc;
    RT_HIP(st.upload());
    rt_params q = *p;
    q.flags &= ~RT_FLAG_ACCUMULATE;                     // host form always starts from zero
    rc = rt_render_frames_device(ctx, st.ptr(d_cams), n_frames, sample_stride, &q, st.ptr(sums), ctx->own_stream);
    if (rc) return rc;
    // Color::to_rgba is per pixel; only the flip knows about frames.  Unflipped, the batch is one image of n_frames * height rows;
    // flipped, every frame is resolved on its own (the resolve kernel is rt_api.hip's: this file adds none)
    if (!flip && (long long)n_frames * p->height <= 0x7fffffffLL) {
        rc = rt_resolve_rgba8_device(ctx, st.ptr(sums), p->width, n_frames * p->height, (int64_t)p->spp, 0, st.ptr(rgba), ctx->own_stream);
        if (rc) return rc;
    } else {
        for (int32_t f = 0; f < n_frames; ++f) {
            rc = rt_resolve_rgba8_device(ctx, st.ptr(sums) + (size_t)f * frame_pix * 3, p->width, p->height, (int64_t)p->spp, flip,
                                         st.ptr(rgba) + (size_t)f * frame_pix * 4, ctx->own_stream);
            if (rc) return rc;
        }
    }
    RT_HIP(st.finish());
    if (stats) return rt_last_stats(ctx, stats);
    return RT_OK;
}

} // extern "C"
