// rt_denoise_core.hpp -- the arithmetic of the edge-avoiding a-trous denoiser (rtiow_hip.h, "denoiser"), stated
// ONCE: the value of an exact sum, prepare, the 3x3 box mean, one pixel of one level, finish.  rt_denoise_host and the kernels of
// rt_denoise.hip both compile these very functions (as rt_select_pixels_host and its kernels share rt::select_noisy), and so does the
// stand-alone sanitizer program tests/denoise_san_main.cpp.  The pixel function, the workspace and the walk over host arrays are written for
// either record -- Tap here, TapVar of the variance-guided denoiser (rt_denoise_var_core.hpp, which adds only what a variance needs).
//
// A pure header: no HIP header, no library call.  IEEE binary64 throughout, in the written operation order; the translation units that
// include it are compiled with -ffp-contract=off, so no product is fused into a sum.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_DN_FN __host__ __device__ inline
#else
#define RT_DN_FN inline
#endif

namespace rt_dn {

constexpr int kMaxLevels = 8;                       // RT_DENOISE_MAX_LEVELS
constexpr double kAlbedoFloor = 0.015625;           // RT_DENOISE_ALBEDO_FLOOR

// what a tap reads of a pixel: the level's input colour c, its 3x3 box mean g, and the guides (normal, depth)
struct Tap {
    static constexpr bool kVar = false;             // (no variance rides along: rt_denoise_var_core.hpp's record has one)
    double c[3], g[3], n[3], z;
};

// the constants of level l: scl = sigma_color * 0.5^l, ic = 1 / scl^2, in = 1 / sigma_normal^2, sz2 = sigma_depth^2
struct LevelConst {
    double ic, in, sz2;
    long long step;                                 // the hole step s = 2^l
};

RT_DN_FN LevelConst level_const(double sigma_color, double sigma_normal, double sigma_depth, int l)
{
    double half_l = 1.0;
    for (int k = 0; k < l; ++k) half_l = half_l * 0.5;          // 0.5^l, exact
    const double scl = sigma_color * half_l;
    LevelConst k;
    k.ic = 1.0 / (scl * scl);
    k.in = 1.0 / (sigma_normal * sigma_normal);
    k.sz2 = sigma_depth * sigma_depth;
    k.step = 1ll << l;
    return k;
}

// exact sum -> f64 value, hi/lo form (rt_api.hip, fix_to_f64)
RT_DN_FN double value(uint64_t q)
{
    return ((double)(uint32_t)(q >> 32) * 4294967296.0 + (double)(uint32_t)q) * (1.0 / 4294967296.0);
}

// contract C5 (rt_device.hpp, quantize): floor(min(x, 65536) * 2^32) for x >= 0, 0 for negatives and NaN
RT_DN_FN uint64_t quantize(double x)
{
    x = x > 0.0 ? x : 0.0;                                      // a NaN fails the comparison: 0
    x = x < 65536.0 ? x : 65536.0;
    const uint32_t hi = (uint32_t)x;
    const uint32_t lo = (uint32_t)((x - (double)hi) * 4294967296.0);
    return ((uint64_t)hi << 32) | (uint64_t)lo;
}

// Prepare: the pixel's sums -> the filter's input c0 = c / m, the modulation m, and the guides.  samples = (double)count_p (or spp).
RT_DN_FN void prepare(const uint64_t *fix, double samples, const uint64_t *feat, double feat_spp, bool demodulate, double c0[3], double m[3],
                      double n[3], double *z)
{
    const uint64_t hits = feat[7];
    const double alpha = (double)hits / feat_spp;
    *z = hits ? value(feat[6]) / (double)hits : 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        const uint64_t qn = feat[3 + ch];
        const bool neg = (int64_t)qn < 0;                       // two's complement: the rule of rt_features_to_f32
        const double v = value(neg ? 0ull - qn : qn);
        n[ch] = (neg ? -v : v) / feat_spp;
        double mod = 1.0;
        if (demodulate) {
            const double alb = value(feat[ch]) / feat_spp;
            mod = alb + (1.0 - alpha);                          // the part of the pixel that sees the sky counts as albedo 1
            mod = mod < kAlbedoFloor ? kAlbedoFloor : mod;
        }
        m[ch] = mod;
        const double c = value(fix[ch]) / samples;
        c0[ch] = c / mod;
    }
}

// The 3x3 box mean of pixel (i, j): the in-frame neighbours summed dy = -1..1 outer, dx = -1..1 inner from 0.0, over their number.
// colour(ii, jj, out[3]) loads the level's input colour of an in-frame pixel.
template <class Colour>
RT_DN_FN void box_mean(long long i, long long j, long long width, long long height, Colour colour, double g[3])
{
    double sum[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const long long ii = i + dx, jj = j + dy;
            if (ii < 0 || ii >= width || jj < 0 || jj >= height) continue;
            double c[3];
            colour(ii, jj, c);
            sum[0] = sum[0] + c[0]; sum[1] = sum[1] + c[1]; sum[2] = sum[2] + c[2];
            ++cnt;
        }
    const double d = (double)cnt;
    g[0] = sum[0] / d; g[1] = sum[1] / d; g[2] = sum[2] / d;
}

// the edge-stop: 1 - x below 1, else 0; a NaN gives 0
RT_DN_FN double edge_stop(double x) { return x < 1.0 ? 1.0 - x : 0.0; }

// One pixel of one level: the 5x5 taps q = p + s (dx, dy), dy outer, dx inner, in-frame taps only.  centre = the pixel's own record;
// tap(dx, dy, &t) loads the record of an in-frame tap -- from global memory, from a staged tile or from host arrays: the order of the
// taps, and with it every bit of the result, is fixed here and not by where the records come from.  Stated once for both records.  Tap:
// the colour stop is L.ic, and sc2, gv and out_var are not looked at.  TapVar (rt_denoise_var_core.hpp): the colour stop divides by
// sc2 * gv, and the variance leaves as the sum of (w w) var_q over (ws ws).
template <class Rec, class TapAt>
RT_DN_FN void level_pixel_of(long long i, long long j, long long width, long long height, const LevelConst &L, [[maybe_unused]] double sc2,
                             [[maybe_unused]] double gv, const Rec &centre, TapAt tap, double out[3], [[maybe_unused]] double *out_var)
{
    const double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    const double izp = 1.0 / (L.sz2 * (centre.z * centre.z) + 1e-12);
    double ic = L.ic;
    if constexpr (Rec::kVar) ic = 1.0 / (sc2 * gv + 1e-12);
    double acc[3] = {0.0, 0.0, 0.0};
    double ws = 0.0;
    [[maybe_unused]] double va = 0.0;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const long long ii = i + L.step * dx, jj = j + L.step * dy;
            if (ii < 0 || ii >= width || jj < 0 || jj >= height) continue;
            Rec q;
            tap(dx, dy, &q);
            const double k = h[dy + 2] * h[dx + 2];
            const double dr = centre.g[0] - q.g[0], dg = centre.g[1] - q.g[1], db = centre.g[2] - q.g[2];
            const double xc = ((dr * dr + dg * dg) + db * db) * ic;
            const double nx = centre.n[0] - q.n[0], ny = centre.n[1] - q.n[1], nz = centre.n[2] - q.n[2];
            const double xn = ((nx * nx + ny * ny) + nz * nz) * L.in;
            const double dz = centre.z - q.z;
            const double xz = (dz * dz) * izp;
            const double tc = edge_stop(xc), tn = edge_stop(xn), tz = edge_stop(xz);
            const double w = ((k * (tc * tc)) * (tn * tn)) * (tz * tz);
            acc[0] = acc[0] + w * q.c[0]; acc[1] = acc[1] + w * q.c[1]; acc[2] = acc[2] + w * q.c[2];
            ws = ws + w;
            if constexpr (Rec::kVar) va = va + (w * w) * q.var;
        }
    out[0] = acc[0] / ws; out[1] = acc[1] / ws; out[2] = acc[2] / ws;         // the centre tap contributes 9/64: ws > 0
    if constexpr (Rec::kVar) *out_var = va / (ws * ws);
}

template <class TapAt>
RT_DN_FN void level_pixel(long long i, long long j, long long width, long long height, const LevelConst &L, const Tap &centre, TapAt tap,
                          double out[3])
{
    level_pixel_of(i, j, width, height, L, 0.0, 0.0, centre, tap, out, nullptr);
}

// Finish: the filtered c0 times the modulation, back on the 2^-32 grid (a one-sample frame)
RT_DN_FN void finish(const double c[3], const double m[3], uint64_t out[3])
{
    for (int ch = 0; ch < 3; ++ch) out[ch] = quantize(c[ch] * m[ch]);
}

// The workspace of one denoise, kWorkDoubles per pixel: the guides (n, z: 4), the modulation m (3), two colour frames (a level reads one
// and writes the other: 3 + 3) and the box mean (3).  The variance-guided filter's has kVarWorkDoubles: behind those, two variance
// planes (in, out) and the variance's 3x3 Gaussian.  Without them (var false) va, vb and gv point at the workspace's end.
constexpr int kWorkDoubles = 16, kVarWorkDoubles = 19;

struct Work {
    double *guide, *mod, *ca, *cb, *box, *va, *vb, *gv;
};

inline Work partition(double *work, unsigned long long npix, bool var)
{
    Work k;
    k.guide = work; k.mod = k.guide + 4 * npix; k.ca = k.mod + 3 * npix; k.cb = k.ca + 3 * npix; k.box = k.cb + 3 * npix;
    k.va = k.box + 3 * npix; k.vb = k.va + (var ? npix : 0); k.gv = k.vb + (var ? npix : 0);
    return k;
}

// (rt_denoise_var_core.hpp defines them; the walk below names them for a record with a variance only)
RT_DN_FN double prepare_var(const uint64_t *fix, const uint64_t *half, double samples, const double m[3]);
template <class VarAt>
RT_DN_FN double gauss_var(long long i, long long j, long long width, long long height, VarAt var_at);

// What follows prepare on host arrays, one pixel after the other, for either record: per level the statistics (the box mean; with a
// variance, its Gaussian too) and the taps, then finish.  k: the partitioned workspace, prepared (guide, mod, ca; with a variance, va).
template <class Rec>
inline void filter_levels(Work k, long long width, long long height, int levels, double sigma_color, double sigma_normal, double sigma_depth,
                          uint64_t *out_fix)
{
    const long long npix = width * height;
    for (int l = 0; l < levels; ++l) {
        const LevelConst L = level_const(sigma_color, sigma_normal, sigma_depth, l);
        const double *cin = k.ca, *vin = k.va, *box = k.box, *guide = k.guide;
        auto colour = [cin, width](long long ii, long long jj, double c[3]) {
            const double *s = cin + 3 * (jj * width + ii);
            c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
        };
        for (long long j = 0; j < height; ++j)
            for (long long i = 0; i < width; ++i) {
                box_mean(i, j, width, height, colour, k.box + 3 * (j * width + i));
                if constexpr (Rec::kVar)
                    k.gv[j * width + i] = gauss_var(i, j, width, height, [vin, width](long long ii, long long jj) { return vin[jj * width + ii]; });
            }
        auto load = [=](long long p, Rec *t) {
            for (int ch = 0; ch < 3; ++ch) { t->c[ch] = cin[3 * p + ch]; t->g[ch] = box[3 * p + ch]; t->n[ch] = guide[4 * p + ch]; }
            t->z = guide[4 * p + 3];
            if constexpr (Rec::kVar) t->var = vin[p];
        };
        for (long long j = 0; j < height; ++j)
            for (long long i = 0; i < width; ++i) {
                const long long p = j * width + i;
                Rec centre;
                load(p, &centre);
                auto tap = [&](int dx, int dy, Rec *t) { load((j + L.step * dy) * width + (i + L.step * dx), t); };
                if constexpr (Rec::kVar)
                    level_pixel_of(i, j, width, height, L, sigma_color * sigma_color, k.gv[p], centre, tap, k.cb + 3 * p, k.vb + p);
                else
                    level_pixel(i, j, width, height, L, centre, tap, k.cb + 3 * p);
            }
        double *t = k.ca; k.ca = k.cb; k.cb = t;
        if constexpr (Rec::kVar) { t = k.va; k.va = k.vb; k.vb = t; }
    }
    for (long long p = 0; p < npix; ++p) finish(k.ca + 3 * p, k.mod + 3 * p, out_fix + 3 * p);
}

// The whole filter on host arrays for either record: prepare, then filter_levels.  count may be null (every pixel has spp samples);
// half is read with a variance only.
template <class Rec>
inline void filter_walk(const uint64_t *fix, [[maybe_unused]] const uint64_t *half, const uint32_t *count, long long spp, const uint64_t *feat,
                        long long feat_spp, long long width, long long height, int levels, bool demodulate, double sigma_color,
                        double sigma_normal, double sigma_depth, double *work, uint64_t *out_fix)
{
    const long long npix = width * height;
    Work k = partition(work, (unsigned long long)npix, Rec::kVar);
    for (long long p = 0; p < npix; ++p) {
        const double samples = count ? (double)count[p] : (double)spp;
        prepare(fix + 3 * p, samples, feat + 8 * p, (double)feat_spp, demodulate, k.ca + 3 * p, k.mod + 3 * p, k.guide + 4 * p,
                k.guide + 4 * p + 3);
        if constexpr (Rec::kVar) k.va[p] = prepare_var(fix + 3 * p, half + 3 * p, samples, k.mod + 3 * p);
    }
    filter_levels<Rec>(k, width, height, levels, sigma_color, sigma_normal, sigma_depth, out_fix);
}

// rt_denoise_host and the stand-alone program
inline void filter_host(const uint64_t *fix, const uint32_t *count, long long spp, const uint64_t *feat, long long feat_spp, long long width,
                        long long height, int levels, bool demodulate, double sigma_color, double sigma_normal, double sigma_depth,
                        double *work, uint64_t *out_fix)
{
    filter_walk<Tap>(fix, nullptr, count, spp, feat, feat_spp, width, height, levels, demodulate, sigma_color, sigma_normal, sigma_depth, work,
                     out_fix);
}

} // namespace rt_dn
