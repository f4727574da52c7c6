// rt_denoise_var_core.hpp -- the arithmetic of the variance-guided a-trous denoiser (rtiow_hip.h, "variance-guided denoiser"; DESIGN.md
// section 25), stated ONCE on top of rt_denoise_core.hpp: the value of a sum, quantize, prepare, the 3x3 box mean, the edge-stop, finish and
// the level constants are that header's and are not restated, and so are the 5x5 taps of one pixel, the workspace (kVarWorkDoubles) and the
// walk over host arrays, which that header writes for either record.  Added here: the record with a variance (TapVar), the variance a
// pixel's half-sample sums give (prepare_var), its 3x3 Gaussian (gauss_var), and under their names one pixel of one level with the colour
// stop in units of the local standard deviation and the variance carried along with the squared weights (level_pixel_var) and the whole
// filter on host arrays (filter_var_host); and, for rt_denoise_var_given, the same variance from one the caller
// gives (prepare_var_given) and the filter behind it (filter_var_given_host).  rt_denoise_var_host, the kernels of denoise/rt_denoise_var.hip and the stand-alone sanitizer
// program tests/denoise_var_san_main.cpp compile these very functions.
//
// A pure header: no HIP header, no library call.  IEEE binary64 throughout, in the written operation order; the translation units that
// include it are compiled with -ffp-contract=off, so no product is fused into a sum.
#pragma once
#include "rt_denoise_core.hpp"

namespace rt_dn {

// what a tap reads of a pixel here: rt_denoise's record and the level's input variance
struct TapVar : Tap {
    static constexpr bool kVar = true;
    double var;
};

// The variance of the pixel's demodulated mean, summed over the channels: d_ch = |2 half_ch - fix_ch| (wrapping uint64 arithmetic, read as
// two's complement: the selection rule's d_c), e_ch = (v(d_ch) / samples) / m_ch, var = (e_r e_r + e_g e_g) + e_b e_b.
RT_DN_FN double prepare_var(const uint64_t *fix, const uint64_t *half, double samples, const double m[3])
{
    double e[3];
    for (int ch = 0; ch < 3; ++ch) {
        uint64_t d = 2ull * half[ch] - fix[ch];
        if ((int64_t)d < 0) d = 0ull - d;
        e[ch] = (value(d) / samples) / m[ch];
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// The same quantity from a variance the caller gives (rt_denoise_var_given): var[ch] = the variance of the pixel's mean c_ch in radiance
// units; x_ch = (var_ch / m_ch) / m_ch, a NaN or a negative counts 0, (x_r + x_g) + x_b.
RT_DN_FN double prepare_var_given(const double var[3], const double m[3])
{
    double x[3];
    for (int ch = 0; ch < 3; ++ch) {
        x[ch] = (var[ch] / m[ch]) / m[ch];
        x[ch] = x[ch] > 0.0 ? x[ch] : 0.0;
    }
    return (x[0] + x[1]) + x[2];
}

// The 3x3 Gaussian of the level's input variance at pixel (i, j): the in-frame neighbours, dy = -1..1 outer, dx = -1..1 inner, weights
// (1,2,1; 2,4,2; 1,2,1) / 16, sv = sv + kk * var_q and sk = sk + kk from 0.0, sv / sk.  var_at(ii, jj) loads an in-frame pixel's variance.
template <class VarAt>
RT_DN_FN double gauss_var(long long i, long long j, long long width, long long height, VarAt var_at)
{
    const double g3[3] = {0.25, 0.5, 0.25};
    double sv = 0.0, sk = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const long long ii = i + dx, jj = j + dy;
            if (ii < 0 || ii >= width || jj < 0 || jj >= height) continue;
            const double kk = g3[dy + 1] * g3[dx + 1];              // 1/16, 1/8 or 1/4: exact
            sv = sv + kk * var_at(ii, jj);
            sk = sk + kk;
        }
    return sv / sk;
}

// One pixel of one level: rt_denoise's taps, order and skip rule (level_pixel_of, stated there for both records).  L: level_const's in,
// sz2 and step (its ic is rt_denoise's and is not used); sc2 = sigma_color * sigma_color, the same at every level; gv: the centre's
// Gaussian-filtered variance.
template <class TapAt>
RT_DN_FN void level_pixel_var(long long i, long long j, long long width, long long height, const LevelConst &L, double sc2, double gv,
                              const TapVar &centre, TapAt tap, double out[3], double *out_var)
{
    level_pixel_of(i, j, width, height, L, sc2, gv, centre, tap, out, out_var);
}

// The whole filter on host arrays -- rt_denoise_var_host and the stand-alone program.  work: kVarWorkDoubles per pixel.
inline void filter_var_host(const uint64_t *fix, const uint64_t *half, const uint32_t *count, long long spp, const uint64_t *feat,
                            long long feat_spp, long long width, long long height, int levels, bool demodulate, double sigma_color,
                            double sigma_normal, double sigma_depth, double *work, uint64_t *out_fix)
{
    filter_walk<TapVar>(fix, half, count, spp, feat, feat_spp, width, height, levels, demodulate, sigma_color, sigma_normal, sigma_depth, work,
                        out_fix);
}

// ... and with the variance given -- rt_denoise_var_given_host and the stand-alone program tests/temporal_var_san_main.cpp.
inline void filter_var_given_host(const uint64_t *fix, const double *var, const uint32_t *count, long long spp, const uint64_t *feat,
                                  long long feat_spp, long long width, long long height, int levels, bool demodulate, double sigma_color,
                                  double sigma_normal, double sigma_depth, double *work, uint64_t *out_fix)
{
    const long long npix = width * height;
    Work k = partition(work, (unsigned long long)npix, true);
    for (long long p = 0; p < npix; ++p) {
        prepare(fix + 3 * p, count ? (double)count[p] : (double)spp, feat + 8 * p, (double)feat_spp, demodulate, k.ca + 3 * p, k.mod + 3 * p,
                k.guide + 4 * p, k.guide + 4 * p + 3);
        k.va[p] = prepare_var_given(var + 3 * p, k.mod + 3 * p);
    }
    filter_levels<TapVar>(k, width, height, levels, sigma_color, sigma_normal, sigma_depth, out_fix);
}

} // namespace rt_dn
