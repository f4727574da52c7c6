/* rtiow_hip_diag.h -- diagnostics of librtiow_hip.so that are NOT part of the C ABI of rtiow_hip.h (no ABI version, no binding
 * promise): what the tests and the measurement tools ask the library about itself. */
#ifndef RTIOW_HIP_DIAG_H
#define RTIOW_HIP_DIAG_H

#include "rtiow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which body of the dense kernel the context's latest rt_render_device launch ran: 1 = the capped unit-sphere redraw (at most four
 * tries per scatter and pass; a lane that accepts none keeps its ray and draws on in the next pass), 0 = the classic body (the
 * unbounded redraw loop) or any launch the capped body does not exist for (RT_FLAG_NO_FILTER, RT_FLAG_DIAG_STATS,
 * RT_FLAG_UNIFORM53, the cross-check scan modes, RTIOW_DENSE_BODY=classic); -1: ctx is NULL.  Both bodies give the same sums and
 * the same rt_stats; kernel_variant does not tell them apart.  Pixel-list and frame-batch launches leave the value alone. */
int32_t rt_last_dense_body(const rt_context *ctx);

#ifdef __cplusplus
}
#endif

#endif
