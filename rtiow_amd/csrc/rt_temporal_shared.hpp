// rt_temporal_shared.hpp -- what the two temporal accumulations share beyond their arithmetic (DESIGN.md sections 16 and 26), stated
// ONCE for rt_temporal.hip and denoise/rt_temporal_var.hip, which include it behind rt_host.hpp and rt_temporal_core.hpp: the launch
// geometry, the tiling of the frame, the camera's four vectors, and the checks that follow the NULL pointers and the history count --
// which each unit makes itself, over its own buffers -- with the constants of the call.  Host code and plain data only: the kernels stay
// in their units.
#pragma once

namespace rt {

constexpr int kTpBlock = 256;                       // four waves, each on pixel tiles of its own
constexpr int kTpWaves = kTpBlock / 64;
constexpr long long kTpMaxBlocks = 1 << 20;         // the grid-stride loop takes over beyond

struct TpTiling {
    uint32_t tiles_x;               // pixel tiles per row of tiles: ceil(width / 8)
    uint32_t n_tiles;               // tiles_x * ceil(height / 8) <= 2^31 / 64 + 2^16
};

// the tiling of a width x height frame and the grid that walks it
inline unsigned tp_grid(int32_t width, int32_t height, TpTiling *T)
{
    T->tiles_x = ((uint32_t)width + 7u) / 8u;
    const unsigned long long n_tiles = (unsigned long long)T->tiles_x * (((unsigned long long)height + 7ull) / 8ull);
    T->n_tiles = (uint32_t)n_tiles;                             // width * height <= 2^31: at most 2^31 / 8 + 2^28 tiles of one row or column
    unsigned long long grid = (n_tiles + kTpWaves - 1) / kTpWaves;
    if (grid > (unsigned long long)kTpMaxBlocks) grid = (unsigned long long)kTpMaxBlocks;
    return (unsigned)grid;
}

inline rt_tp::Cam tp_cam_of(const rt_camera *c)
{
    rt_tp::Cam k;
    for (int a = 0; a < 3; ++a) {
        k.origin[a] = c->origin[a]; k.llc[a] = c->lower_left_corner[a];
        k.horizontal[a] = c->horizontal[a]; k.vertical[a] = c->vertical[a];
    }
    return k;
}

// What every form of both accumulations checks behind its NULL pointers and its history count, in this order; none of it needs a
// context.  who: "temporal", "temporal_var"; hist: the call has a history.  *K: the constants of the call.
inline int tp_check_settings(const char *who, const struct rt_temporal *tp, bool has_count, int64_t spp, int64_t feat_spp, const rt_camera *cam,
                             bool hist, int64_t prev_feat_spp, const rt_camera *prev_cam, int32_t width, int32_t height, rt_tp::Const *K)
{
    using rt_host::fail;
    if (tp->flags & ~RT_TEMPORAL_CLAMP) return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", who, tp->flags);
    if (!(tp->alpha_min > 0.0) || !(tp->alpha_min <= 1.0))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: alpha_min must be in (0, 1] (is %g)", who, tp->alpha_min);
    if (!(tp->sigma_normal > 0.0) || !(tp->sigma_depth > 0.0) || !std::isfinite(tp->sigma_normal) || !std::isfinite(tp->sigma_depth))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: every sigma must be > 0 and finite (%g, %g)", who, tp->sigma_normal, tp->sigma_depth);
    if (!(tp->clamp_scale >= 0.0) || !std::isfinite(tp->clamp_scale))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: clamp_scale must be >= 0 and finite (is %g)", who, tp->clamp_scale);
    if (width < 2 || height < 2) return fail(RT_ERR_INVALID_ARGUMENT, "%s: width and height must be >= 2 (%d, %d)", who, width, height);
    if ((long long)width * height > (1ll << 31))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: width * height must be <= 2^31 (is %lld)", who, (long long)width * height);
    if (!has_count && spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "%s: spp >= 1 without a count buffer (is %lld)", who, (long long)spp);
    if (feat_spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "%s: feat_spp >= 1 (is %lld)", who, (long long)feat_spp);
    if (hist && prev_feat_spp < 1)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: prev_feat_spp >= 1 with a history (is %lld)", who, (long long)prev_feat_spp);
    const rt_tp::Cam cur = tp_cam_of(cam);
    rt_tp::Cam prev;
    if (hist) prev = tp_cam_of(prev_cam);
    *K = rt_tp::constants(cur, hist ? &prev : nullptr, width, height, has_count ? 1 : (long long)spp, (long long)feat_spp,
                          hist ? (long long)prev_feat_spp : 1, tp->flags, tp->alpha_min, tp->sigma_normal, tp->sigma_depth, tp->clamp_scale);
    return RT_OK;
}

} // namespace rt
