// rt_temporal_core.hpp -- the arithmetic of temporal accumulation by first-hit reprojection (rtiow_hip.h, "temporal accumulation";
// DESIGN.md section 16), stated ONCE: the constants of a call, one pixel of the filter, and the whole frame on host arrays.
// rt_temporal_host and the kernel of rt_temporal.hip both compile these very functions, and so does the stand-alone sanitizer program
// tests/temporal_san_main.cpp.  The value of a sum and the C5 quantisation are rt_denoise_core.hpp's.
//
// A pure header: no HIP header, no library call.  IEEE binary64 throughout, in the written operation order; the translation units that
// include it are compiled with -ffp-contract=off, so no product is fused into a sum.
#pragma once
#include <stdint.h>

#include "rt_denoise_core.hpp"

#if defined(__HIPCC__)
#define RT_TP_FN __host__ __device__ inline
#else
#define RT_TP_FN inline
#endif

namespace rt_tp {

constexpr uint32_t kClamp = 0x1u;                   // RT_TEMPORAL_CLAMP
constexpr uint32_t kMaxLen = 65535u;                // RT_TEMPORAL_MAX_LEN

// the four vectors of an rt_camera that reprojection reads (the lens plays no part: the world point lies on the ray through its centre)
struct Cam {
    double origin[3], llc[3], horizontal[3], vertical[3];
};

// Everything of a call that is the same for every pixel: computed on the host, once, and handed to the kernel as an argument.
struct Const {
    Cam cur, prev;
    double nrm[3];                                  // cross(prev.horizontal, prev.vertical)
    double iLn, LH, LV, iHH, iVV;                   // with L = prev.llc - prev.origin
    double wm1, hm1, sz2, in;
    double alpha_min, clamp_scale;
    double samples, feat_spp, prev_feat_spp;        // (double) of spp (unused with a count buffer), feat_spp, prev_feat_spp
    long long width, height;
    uint32_t flags;
    uint32_t has_prev;                              // 0: the first frame, nothing of `prev` or the history is read
};

RT_TP_FN double dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RT_TP_FN void cross(const double a[3], const double b[3], double out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

RT_TP_FN Const constants(const Cam &cur, const Cam *prev, long long width, long long height, long long spp, long long feat_spp,
                         long long prev_feat_spp, uint32_t flags, double alpha_min, double sigma_normal, double sigma_depth, double clamp_scale)
{
    Const K;
    K.cur = cur;
    K.has_prev = prev ? 1u : 0u;
    K.prev = prev ? *prev : cur;
    double L[3];
    for (int k = 0; k < 3; ++k) L[k] = K.prev.llc[k] - K.prev.origin[k];
    cross(K.prev.horizontal, K.prev.vertical, K.nrm);
    K.iLn = 1.0 / dot(L, K.nrm);
    K.LH = dot(L, K.prev.horizontal);
    K.LV = dot(L, K.prev.vertical);
    K.iHH = 1.0 / dot(K.prev.horizontal, K.prev.horizontal);
    K.iVV = 1.0 / dot(K.prev.vertical, K.prev.vertical);
    K.wm1 = (double)(width - 1);
    K.hm1 = (double)(height - 1);
    K.sz2 = sigma_depth * sigma_depth;
    K.in = 1.0 / (sigma_normal * sigma_normal);
    K.alpha_min = alpha_min;
    K.clamp_scale = clamp_scale;
    K.samples = (double)spp;
    K.feat_spp = (double)feat_spp;
    K.prev_feat_spp = (double)prev_feat_spp;
    K.width = width;
    K.height = height;
    K.flags = flags;
    return K;
}

// the guides of a pixel from its eight feature sums: hits = word 7, z = the mean depth over the hitting samples, n = the mean normal
RT_TP_FN uint64_t guides(const uint64_t *feat, double feat_spp, double n[3], double *z)
{
    const uint64_t hits = feat[7];
    *z = hits ? rt_dn::value(feat[6]) / (double)hits : 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        const uint64_t qn = feat[3 + ch];
        const bool neg = (int64_t)qn < 0;                       // two's complement: the rule of rt_features_to_f32
        const double v = rt_dn::value(neg ? 0ull - qn : qn);
        n[ch] = (neg ? -v : v) / feat_spp;
    }
    return hits;
}

// the colour of a current-frame pixel: c_ch = v(fix_ch) / samples
RT_TP_FN void colour_of(const uint64_t *fix, double samples, double c[3])
{
    for (int ch = 0; ch < 3; ++ch) c[ch] = rt_dn::value(fix[ch]) / samples;
}

// floor of x for |x| < 2^62, by cast and correction
RT_TP_FN long long floor_ll(double x)
{
    long long k = (long long)x;
    if ((double)k > x) k -= 1;
    return k;
}

// what a tap reads of a previous-frame pixel: its history length, its hit count, its guides and its accumulated colour
struct Tap {
    uint32_t len;
    uint64_t hits;
    double n[3], z, c[3];
};

// One pixel.  c, hits, n, z: the pixel's own prepared values.  tap(ii, jj, &t) loads an in-frame pixel of the previous frame;
// colour(ii, jj, out[3]) the colour c of an in-frame pixel of the current frame.  Returns the history length; out[3] the sums.
template <class TapAt, class Colour>
RT_TP_FN uint32_t pixel(long long i, long long j, const Const &K, const double c[3], uint64_t hits, const double n[3], double z, TapAt tap,
                        Colour colour, uint64_t out[3])
{
    const long long W = K.width, H = K.height;
    bool have = K.has_prev != 0u && hits != 0;
    double h[3] = {0.0, 0.0, 0.0};
    unsigned long long N = 0xFFFFFFFFull;
    if (have) {
        // the world point of the pixel centre through the lens centre
        const double u = ((double)i + 0.5) / K.wm1, v = ((double)j + 0.5) / K.hm1;
        double e[3];
        for (int k = 0; k < 3; ++k) {
            const double d = ((K.cur.llc[k] + u * K.cur.horizontal[k]) + v * K.cur.vertical[k]) - K.cur.origin[k];
            const double P = K.cur.origin[k] + z * d;
            e[k] = P - K.prev.origin[k];
        }
        // into the previous image
        const double s = dot(e, K.nrm) * K.iLn;
        have = s > 0.0;
        if (have) {
            const double is = 1.0 / s;
            const double up = (dot(e, K.prev.horizontal) * is - K.LH) * K.iHH;
            const double vp = (dot(e, K.prev.vertical) * is - K.LV) * K.iVV;
            const double fx = up * K.wm1 - 0.5, fy = vp * K.hm1 - 0.5;
            have = fx >= -1.0 && fx < (double)W && fy >= -1.0 && fy < (double)H;          // a NaN fails
            if (have) {
                const long long i0 = floor_ll(fx), j0 = floor_ll(fy);
                const double a = fx - (double)i0, b = fy - (double)j0;
                const double kws[4] = {(1.0 - a) * (1.0 - b), a * (1.0 - b), (1.0 - a) * b, a * b};
                const double lim = K.sz2 * (s * s) + 1e-12;
                double acc[3] = {0.0, 0.0, 0.0};
                double ws = 0.0;
                for (int t = 0; t < 4; ++t) {
                    const long long ii = i0 + (t & 1), jj = j0 + (t >> 1);
                    const double kw = kws[t];
                    if (ii < 0 || ii >= W || jj < 0 || jj >= H || !(kw > 0.0)) continue;
                    Tap q;
                    tap(ii, jj, &q);
                    if (q.len == 0u || q.hits == 0) continue;
                    const double dz = q.z - s;
                    if (!((dz * dz) < lim)) continue;
                    const double d0 = n[0] - q.n[0], d1 = n[1] - q.n[1], d2 = n[2] - q.n[2];
                    if (!(((d0 * d0 + d1 * d1) + d2 * d2) * K.in < 1.0)) continue;
                    acc[0] = acc[0] + kw * q.c[0]; acc[1] = acc[1] + kw * q.c[1]; acc[2] = acc[2] + kw * q.c[2];
                    ws = ws + kw;
                    N = (unsigned long long)q.len < N ? (unsigned long long)q.len : N;
                }
                have = ws > 0.0;
                if (have) { h[0] = acc[0] / ws; h[1] = acc[1] / ws; h[2] = acc[2] / ws; }
            }
        }
    }
    if (!have) {
        out[0] = rt_dn::quantize(c[0]); out[1] = rt_dn::quantize(c[1]); out[2] = rt_dn::quantize(c[2]);
        return 1u;
    }
    if (K.flags & kClamp) {
        // the box of the current frame's 3 x 3 neighbourhood (the pixel itself first), dy outer, dx inner
        double lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const long long ii = i + dx, jj = j + dy;
                if (ii < 0 || ii >= W || jj < 0 || jj >= H || (dx == 0 && dy == 0)) continue;
                double cq[3];
                colour(ii, jj, cq);
                for (int ch = 0; ch < 3; ++ch) {
                    lo[ch] = cq[ch] < lo[ch] ? cq[ch] : lo[ch];
                    hi[ch] = cq[ch] > hi[ch] ? cq[ch] : hi[ch];
                }
            }
        for (int ch = 0; ch < 3; ++ch) {
            const double mid = (lo[ch] + hi[ch]) * 0.5, ext = ((hi[ch] - lo[ch]) * 0.5) * K.clamp_scale;
            h[ch] = h[ch] < mid - ext ? mid - ext : h[ch];
            h[ch] = h[ch] > mid + ext ? mid + ext : h[ch];
        }
    }
    double at = 1.0 / (double)(N + 1ull);
    at = at < K.alpha_min ? K.alpha_min : at;
    for (int ch = 0; ch < 3; ++ch) out[ch] = rt_dn::quantize(h[ch] + at * (c[ch] - h[ch]));
    return (uint32_t)(N + 1ull < (unsigned long long)kMaxLen ? N + 1ull : (unsigned long long)kMaxLen);
}

// The buffers of a call, on the host or on the device: pixel_at() is the one way from them to a pixel's result.
struct Buffers {
    const uint64_t *fix;            // [H][W][3]
    const uint32_t *count;          // [H][W] or null
    const uint64_t *feat;           // [H][W][8]
    const uint64_t *prev_fix;       // [H][W][3] the previous call's out_fix, or null
    const uint32_t *prev_len;       // [H][W]
    const uint64_t *prev_feat;      // [H][W][8]
};

RT_TP_FN uint32_t pixel_at(long long i, long long j, const Const &K, const Buffers &B, uint64_t out[3])
{
    const long long W = K.width;
    const long long p = j * W + i;
    double c[3], n[3], z;
    colour_of(B.fix + 3 * p, B.count ? (double)B.count[p] : K.samples, c);
    const uint64_t hits = guides(B.feat + 8 * p, K.feat_spp, n, &z);
    auto tap = [&](long long ii, long long jj, Tap *t) {
        const long long q = jj * W + ii;
        t->len = B.prev_len[q];
        t->hits = 0;
        if (t->len == 0u) return;                               // (pixel() reads nothing else of such a tap)
        t->hits = guides(B.prev_feat + 8 * q, K.prev_feat_spp, t->n, &t->z);
        t->c[0] = rt_dn::value(B.prev_fix[3 * q + 0]); t->c[1] = rt_dn::value(B.prev_fix[3 * q + 1]); t->c[2] = rt_dn::value(B.prev_fix[3 * q + 2]);
    };
    auto colour = [&](long long ii, long long jj, double cq[3]) {
        const long long q = jj * W + ii;
        colour_of(B.fix + 3 * q, B.count ? (double)B.count[q] : K.samples, cq);
    };
    return pixel(i, j, K, c, hits, n, z, tap, colour, out);
}

// The whole frame on host arrays, one pixel after the other -- rt_temporal_host and the stand-alone program.
inline void accumulate_host(const Const &K, const Buffers &B, uint64_t *out_fix, uint32_t *out_len)
{
    for (long long j = 0; j < K.height; ++j)
        for (long long i = 0; i < K.width; ++i) {
            const long long p = j * K.width + i;
            out_len[p] = pixel_at(i, j, K, B, out_fix + 3 * p);
        }
}

} // namespace rt_tp
