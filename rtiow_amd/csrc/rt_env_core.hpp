// rt_env_core.hpp -- the sampling table of an environment cube map (rtiow_hip.h, "environment"), built on the host
// from the caller's texels: per texel the largest positive channel times the solid angle its square subtends, as running sums in index
// order.  Pure: plain C++17 and the standard library only -- no HIP, no environment variable, no context.  wavefront/rt_paths.hip's
// rt_environment_cdf validates with valid_size() and calls cdf(); rt_render_wavefront_env builds its own table with it;
// tests/env_cdf_san_main.cpp compiles this header alone under ASan + UBSan.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_env {

constexpr int32_t kMaxSize = 1024;                  // RT_ENV_MAX_SIZE (pinned by a static_assert where both are seen)

// texels per face edge: a power of two in [1, kMaxSize]
inline bool valid_size(int32_t size) { return size >= 1 && size <= kMaxSize && (size & (size - 1)) == 0; }

// texels of a map: 6 faces of size x size
inline size_t texel_count(int32_t size) { return (size_t)6 * (size_t)size * (size_t)size; }

// The weight of texel (i, j) of a face: mx / r^3 with r^2 = 1 + ac^2 + bc^2 at the texel's centre (the solid angle of its square, up to
// the factor s^2 every texel shares) and mx the largest channel that compares > 0.0 -- a NaN or a negative channel counts as 0.
inline double texel_weight(const double *rgb, int32_t i, int32_t j, double s)
{
    const double ac = ((double)i + 0.5) * s - 1.0;
    const double bc = ((double)j + 0.5) * s - 1.0;
    const double r2 = (1.0 + ac * ac) + bc * bc;
    double mx = 0.0;
    for (int c = 0; c < 3; ++c)
        if (rgb[c] > mx) mx = rgb[c];
    return mx / (r2 * std::sqrt(r2));
}

// texels: [6][size][size][3]; out: [6 * size * size] running sums, out[k] = (k ? out[k - 1] : 0.0) + W_k in index order.  size: valid.
inline void cdf(const double *texels, int32_t size, double *out)
{
    const double s = 2.0 / (double)size;
    double run = 0.0;
    size_t k = 0;
    for (int32_t f = 0; f < 6; ++f)
        for (int32_t i = 0; i < size; ++i)
            for (int32_t j = 0; j < size; ++j, ++k) {
                run = run + texel_weight(texels + 3 * k, i, j, s);
                out[k] = run;
            }
}

} // namespace rt_env
