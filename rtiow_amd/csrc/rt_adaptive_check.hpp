// rt_adaptive_check.hpp -- what the two adaptive drivers share on the host: rt_render_adaptive (rt_adaptive.hip, which defines the
// functions declared here) and rt_render_wavefront_adaptive (wavefront/rt_paths.hip).  No kernel, no HIP call.
#pragma once
#include "rtiow_hip.h"

namespace rt_host {

constexpr int kAdaptiveMaxSpp = 32766;     // n * 2^48 < 2^63: the half-buffer differences fit a signed 64-bit integer whatever the scene

int validate_adaptive(const rt_adaptive *a);

// The frame a driver (`what`: its name) was handed, after validate_params and validate_adaptive have passed: it numbers its own passes
// from 0, in rounds of 2 * step samples, up to p->spp.
int check_adaptive_frame(const char *what, const rt_params *p, const rt_adaptive *a);

} // namespace rt_host
