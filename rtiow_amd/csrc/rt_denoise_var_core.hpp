// rt_denoise_var_core.hpp -- the arithmetic of the variance-guided a-trous denoiser (rtiow_hip.h, "variance-guided denoiser"; DESIGN.md
// section 25), stated ONCE on top of rt_denoise_core.hpp: the value of a sum, quantize, prepare, the 3x3 box mean, the edge-stop, finish and
// the level constants are that header's and are not restated.  Added here: the variance a pixel's half-sample sums give (prepare_var), its
// 3x3 Gaussian (gauss_var), one pixel of one level with the colour stop in units of the local standard deviation and the variance carried
// along with the squared weights (level_pixel_var), and the whole filter on host arrays (filter_var_host).  rt_denoise_var_host, the
// kernels of denoise/rt_denoise_var.hip and the stand-alone sanitizer program tests/denoise_var_san_main.cpp compile these very functions.
//
// A pure header: no HIP header, no library call.  IEEE binary64 throughout, in the written operation order; the translation units that
// include it are compiled with -ffp-contract=off, so no product is fused into a sum.
#pragma once
#include "rt_denoise_core.hpp"

namespace rt_dn {

constexpr int kVarWorkDoubles = 19;                 // per pixel: rt_denoise's 16, two variance planes, the variance's 3x3 Gaussian

// what a tap reads of a pixel here: rt_denoise's record and the level's input variance
struct TapVar : Tap {
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

// One pixel of one level.  L: level_const's in, sz2 and step (its ic is rt_denoise's and is not used); sc2 = sigma_color * sigma_color, the
// same at every level; gv: the centre's Gaussian-filtered variance.  The taps, their order and the skip rule are level_pixel's; the colour
// stop divides by sc2 * gv, and the variance leaves as the sum of (w w) var_q over (ws ws).
template <class TapAt>
RT_DN_FN void level_pixel_var(long long i, long long j, long long width, long long height, const LevelConst &L, double sc2, double gv,
                              const TapVar &centre, TapAt tap, double out[3], double *out_var)
{
    const double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    const double izp = 1.0 / (L.sz2 * (centre.z * centre.z) + 1e-12);
    const double icv = 1.0 / (sc2 * gv + 1e-12);
    double acc[3] = {0.0, 0.0, 0.0};
    double ws = 0.0, va = 0.0;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const long long ii = i + L.step * dx, jj = j + L.step * dy;
            if (ii < 0 || ii >= width || jj < 0 || jj >= height) continue;
            TapVar q;
            tap(dx, dy, &q);
            const double k = h[dy + 2] * h[dx + 2];
            const double dr = centre.g[0] - q.g[0], dg = centre.g[1] - q.g[1], db = centre.g[2] - q.g[2];
            const double xc = ((dr * dr + dg * dg) + db * db) * icv;
            const double nx = centre.n[0] - q.n[0], ny = centre.n[1] - q.n[1], nz = centre.n[2] - q.n[2];
            const double xn = ((nx * nx + ny * ny) + nz * nz) * L.in;
            const double dz = centre.z - q.z;
            const double xz = (dz * dz) * izp;
            const double tc = edge_stop(xc), tn = edge_stop(xn), tz = edge_stop(xz);
            const double w = ((k * (tc * tc)) * (tn * tn)) * (tz * tz);
            acc[0] = acc[0] + w * q.c[0]; acc[1] = acc[1] + w * q.c[1]; acc[2] = acc[2] + w * q.c[2];
            ws = ws + w;
            va = va + (w * w) * q.var;
        }
    out[0] = acc[0] / ws; out[1] = acc[1] / ws; out[2] = acc[2] / ws;         // the centre tap contributes 9/64: ws > 0
    *out_var = va / (ws * ws);
}

// The whole filter on host arrays, one pixel after the other -- rt_denoise_var_host and the stand-alone program.  work: kVarWorkDoubles
// per pixel (guides n, z: 4; m: 3; colour in: 3; colour out: 3; box mean: 3; variance in: 1; variance out: 1; its Gaussian: 1).  count
// may be null (every pixel has spp samples).
inline void filter_var_host(const uint64_t *fix, const uint64_t *half, const uint32_t *count, long long spp, const uint64_t *feat,
                            long long feat_spp, long long width, long long height, int levels, bool demodulate, double sigma_color,
                            double sigma_normal, double sigma_depth, double *work, uint64_t *out_fix)
{
    const long long npix = width * height;
    double *guide = work, *mod = guide + 4 * npix, *ca = mod + 3 * npix, *cb = ca + 3 * npix, *box = cb + 3 * npix;
    double *va = box + 3 * npix, *vb = va + npix, *gv = vb + npix;
    for (long long p = 0; p < npix; ++p) {
        const double samples = count ? (double)count[p] : (double)spp;
        prepare(fix + 3 * p, samples, feat + 8 * p, (double)feat_spp, demodulate, ca + 3 * p, mod + 3 * p, guide + 4 * p, guide + 4 * p + 3);
        va[p] = prepare_var(fix + 3 * p, half + 3 * p, samples, mod + 3 * p);
    }
    const double sc2 = sigma_color * sigma_color;
    for (int l = 0; l < levels; ++l) {
        const LevelConst L = level_const(sigma_color, sigma_normal, sigma_depth, l);
        const double *cin = ca, *vin = va;
        auto colour = [cin, width](long long ii, long long jj, double c[3]) {
            const double *s = cin + 3 * (jj * width + ii);
            c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
        };
        auto var_at = [vin, width](long long ii, long long jj) { return vin[jj * width + ii]; };
        for (long long j = 0; j < height; ++j)
            for (long long i = 0; i < width; ++i) {
                box_mean(i, j, width, height, colour, box + 3 * (j * width + i));
                gv[j * width + i] = gauss_var(i, j, width, height, var_at);
            }
        auto load = [cin, vin, box, guide](long long p, TapVar *t) {
            for (int ch = 0; ch < 3; ++ch) { t->c[ch] = cin[3 * p + ch]; t->g[ch] = box[3 * p + ch]; t->n[ch] = guide[4 * p + ch]; }
            t->z = guide[4 * p + 3];
            t->var = vin[p];
        };
        for (long long j = 0; j < height; ++j)
            for (long long i = 0; i < width; ++i) {
                TapVar centre;
                load(j * width + i, &centre);
                auto tap = [&](int dx, int dy, TapVar *t) { load((j + L.step * dy) * width + (i + L.step * dx), t); };
                level_pixel_var(i, j, width, height, L, sc2, gv[j * width + i], centre, tap, cb + 3 * (j * width + i), vb + (j * width + i));
            }
        double *t = ca; ca = cb; cb = t;
        t = va; va = vb; vb = t;
    }
    for (long long p = 0; p < npix; ++p) finish(ca + 3 * p, mod + 3 * p, out_fix + 3 * p);
}

} // namespace rt_dn
