// rt_adaptive_check.hpp -- what the two adaptive drivers share on the host: rt_render_adaptive (rt_adaptive.hip, which defines the
// function declared here) and rt_render_wavefront_adaptive (wavefront/rt_paths.hip).  No kernel, no HIP call.
#pragma once
#include "rtiow_hip.h"

namespace rt_host {

constexpr int kAdaptiveMaxSpp = 32766;     // n * 2^48 < 2^63: the half-buffer differences fit a signed 64-bit integer whatever the scene

int validate_adaptive(const rt_adaptive *a);

} // namespace rt_host
