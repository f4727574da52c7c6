// rt_dense.hip -- the dense launch's kernels with the CAPPED unit-sphere redraw (rt_kernels.hpp, ITEMS = kItemBlockDense / kItemBlockDenseLarge;
// DESIGN.md section 5.3).
//
// The fourth translation unit of librtiow_hip.so.  It owns four instantiations of the render kernel,
// rt::render_kernel<5, false, SMALLGRID, false, rt::kItemBlockDense | rt::kItemBlockDenseLarge>, the function the dense launch's one dispatch
// (launch_dense, rt_api.hip) reaches them through, and the diagnostic that says which body the last dense launch ran (rtiow_hip_diag.h).  The
// launch itself -- plan, KParams, slot, clears, tail -- is the shared path of rt_launch.hpp: nothing of it is here.  Every other kernel of the library stays
// where it was: rt_api.hip's and rt_frames.hip's device code is untouched, and the classic dense kernels remain in the library
// (RTIOW_DENSE_BODY=classic runs them for the same launch: the same frame, the A/B baseline).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "rt_launch.hpp"
#include "rtiow_hip_diag.h"

namespace rt_host {

// Which launches take the capped body when RTIOW_DENSE_BODY is not set: decided per instantiation by the interleaved A/B of
// profiles/capped_redraw_ab.txt (tools/dense_body_ab.py) -- a default only where the capped body is faster by at least three times the
// rebuild-to-rebuild band of +-0.3 % in both orders: the headline shape (small grid, blocks of 1 024) alone (rt_launch.hpp, kDenseCappedDefault).
static bool capped_by_default(bool small_grid, bool large_blocks)
{
    return kDenseCappedDefault[small_grid ? 1 : 0][large_blocks ? 1 : 0];
}

bool dense_body_is_capped(bool small_grid, bool large_blocks)
{
    // RTIOW_DENSE_BODY (diagnostic, read per launch): classic = the dense kernels of rt_api.hip, capped = the ones of this file
    // wherever they exist; anything else, or unset: the measured defaults
    const char *v = getenv("RTIOW_DENSE_BODY");
    if (v && !strcmp(v, "classic")) return false;
    if (v && !strcmp(v, "capped")) return true;
    return capped_by_default(small_grid, large_blocks);
}

int launch_dense_capped(rt_context *ctx, const rt::KParams &kp_in, hipStream_t stream, bool small_grid, bool large_blocks, int *grid_out)
{
    // lane-striped block sums: the three capped kernels whose ring has 16 pixel slots (the large-grid one on blocks of 1 024 keeps 4 x 8 and its code)
    rt::KParams kp = kp_in;
    const StripePlan sp = plan_stripes(kp.use_ring != 0, kp.block_items, kp.spp, small_grid || !large_blocks);
    kp.stripe_mask = sp.mask;
    if (small_grid)
        return large_blocks ? launch_render<5, false, true, false, rt::kItemBlockDenseLarge>(ctx, kp, stream, grid_out)
                            : launch_render<5, false, true, false, rt::kItemBlockDense>(ctx, kp, stream, grid_out);
    return large_blocks ? launch_render<5, false, false, false, rt::kItemBlockDenseLarge>(ctx, kp, stream, grid_out)
                        : launch_render<5, false, false, false, rt::kItemBlockDense>(ctx, kp, stream, grid_out);
}

} // namespace rt_host

extern "C" int32_t rt_last_dense_body(const rt_context *ctx)
{
    return ctx ? ctx->last_dense_body : -1;
}
