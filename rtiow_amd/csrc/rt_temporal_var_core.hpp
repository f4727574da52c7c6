// rt_temporal_var_core.hpp -- the arithmetic of temporal accumulation with second moments (rtiow_hip.h, "temporal accumulation with
// second moments"), stated ONCE on top of rt_temporal_core.hpp: the constants of a call, the guides, the colour of a
// pixel, floor and the four vectors of a camera are that header's and are not restated.  Added here: the tap that also reads the history's
// second moment, one pixel -- rt_temporal's steps 1-7 in rt_temporal's operation order (tests/test_temporal_var_host.py holds out_fix and
// out_len to rt_temporal's bits) with the moment carried beside the colour, the 3 x 3 walk that feeds both the clamp's box and the spatial
// moments, and the variance of the accumulated value -- and the whole frame on host arrays.  rt_temporal_var_host, the kernel of
// denoise/rt_temporal_var.hip and the stand-alone sanitizer program tests/temporal_var_san_main.cpp compile these very functions.
//
// A pure header: no HIP header, no library call.  IEEE binary64 throughout, in the written operation order; the translation units that
// include it are compiled with -ffp-contract=off, so no product is fused into a sum.
#pragma once
#include "rt_temporal_core.hpp"

namespace rt_tp {

constexpr uint32_t kVarMinLen = 4u;                 // RT_TEMPORAL_VAR_MIN_LEN

// what a tap reads of a previous-frame pixel here: rt_temporal's record and the accumulated second moment
struct TapVar : Tap {
    double m2[3];
};

// x > 0 ? x : 0 -- a NaN and a negative give 0
RT_TP_FN double clip0(double x) { return x > 0.0 ? x : 0.0; }

// One pixel.  c, hits, n, z: the pixel's own prepared values.  tap(ii, jj, &t) loads an in-frame pixel of the previous frame;
// colour(ii, jj, out[3]) the colour c of an in-frame pixel of the current frame OTHER than (i, j).  Returns the history length; out[3] the
// sums, m2[3] the accumulated second moment, var[3] the variance of the accumulated value.
template <class TapAt, class Colour>
RT_TP_FN uint32_t pixel_var(long long i, long long j, const Const &K, const double c[3], uint64_t hits, const double n[3], double z, TapAt tap,
                            Colour colour, uint64_t out[3], double m2[3], double var[3])
{
    const long long W = K.width, H = K.height;
    // the 3 x 3 neighbourhood of the current frame, once: the spatial moments (centre in its place) and the clamp's box (which starts
    // from the centre, so that visiting it changes nothing), dy outer, dx inner
    double lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
    double a1[3] = {0.0, 0.0, 0.0}, a2[3] = {0.0, 0.0, 0.0}, cnt = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const long long ii = i + dx, jj = j + dy;
            if (ii < 0 || ii >= W || jj < 0 || jj >= H) continue;
            double cq[3] = {c[0], c[1], c[2]};
            if (dx != 0 || dy != 0) colour(ii, jj, cq);
            for (int ch = 0; ch < 3; ++ch) {
                a1[ch] = a1[ch] + cq[ch];
                a2[ch] = a2[ch] + cq[ch] * cq[ch];
                lo[ch] = cq[ch] < lo[ch] ? cq[ch] : lo[ch];
                hi[ch] = cq[ch] > hi[ch] ? cq[ch] : hi[ch];
            }
            cnt = cnt + 1.0;
        }
    double vs[3], s2[3];
    for (int ch = 0; ch < 3; ++ch) {
        const double mu = a1[ch] / cnt;
        vs[ch] = clip0(a2[ch] / cnt - mu * mu);
        s2[ch] = c[ch] * c[ch];
    }
    // steps 2-5 of rt_temporal, the moment beside the colour
    bool have = K.has_prev != 0u && hits != 0;
    double h[3] = {0.0, 0.0, 0.0}, h2[3] = {0.0, 0.0, 0.0};
    unsigned long long N = 0xFFFFFFFFull;
    if (have) {
        const double u = ((double)i + 0.5) / K.wm1, v = ((double)j + 0.5) / K.hm1;
        double e[3];
        for (int k = 0; k < 3; ++k) {
            const double d = ((K.cur.llc[k] + u * K.cur.horizontal[k]) + v * K.cur.vertical[k]) - K.cur.origin[k];
            const double P = K.cur.origin[k] + z * d;
            e[k] = P - K.prev.origin[k];
        }
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
                double acc[3] = {0.0, 0.0, 0.0}, acc2[3] = {0.0, 0.0, 0.0};
                double ws = 0.0;
                for (int t = 0; t < 4; ++t) {
                    const long long ii = i0 + (t & 1), jj = j0 + (t >> 1);
                    const double kw = kws[t];
                    if (ii < 0 || ii >= W || jj < 0 || jj >= H || !(kw > 0.0)) continue;
                    TapVar q;
                    tap(ii, jj, &q);
                    if (q.len == 0u || q.hits == 0) continue;
                    const double dz = q.z - s;
                    if (!((dz * dz) < lim)) continue;
                    const double d0 = n[0] - q.n[0], d1 = n[1] - q.n[1], d2 = n[2] - q.n[2];
                    if (!(((d0 * d0 + d1 * d1) + d2 * d2) * K.in < 1.0)) continue;
                    acc[0] = acc[0] + kw * q.c[0]; acc[1] = acc[1] + kw * q.c[1]; acc[2] = acc[2] + kw * q.c[2];
                    acc2[0] = acc2[0] + kw * q.m2[0]; acc2[1] = acc2[1] + kw * q.m2[1]; acc2[2] = acc2[2] + kw * q.m2[2];
                    ws = ws + kw;
                    N = (unsigned long long)q.len < N ? (unsigned long long)q.len : N;
                }
                have = ws > 0.0;
                if (have)
                    for (int ch = 0; ch < 3; ++ch) { h[ch] = acc[ch] / ws; h2[ch] = acc2[ch] / ws; }
            }
        }
    }
    if (!have) {
        // no history: the frame's own mean and square, at = 1, len = 1 < kVarMinLen, so the spatial estimate
        for (int ch = 0; ch < 3; ++ch) {
            out[ch] = rt_dn::quantize(c[ch]);
            m2[ch] = s2[ch];
            var[ch] = vs[ch] * 1.0;
        }
        return 1u;
    }
    if (K.flags & kClamp) {
        // step 6: the clamp moves the history's mean and keeps its central variance
        for (int ch = 0; ch < 3; ++ch) {
            const double hb = h[ch];
            const double mid = (lo[ch] + hi[ch]) * 0.5, ext = ((hi[ch] - lo[ch]) * 0.5) * K.clamp_scale;
            h[ch] = h[ch] < mid - ext ? mid - ext : h[ch];
            h[ch] = h[ch] > mid + ext ? mid + ext : h[ch];
            h2[ch] = (h2[ch] - hb * hb) + h[ch] * h[ch];
        }
    }
    double at = 1.0 / (double)(N + 1ull);
    at = at < K.alpha_min ? K.alpha_min : at;
    const uint32_t len = (uint32_t)(N + 1ull < (unsigned long long)kMaxLen ? N + 1ull : (unsigned long long)kMaxLen);
    for (int ch = 0; ch < 3; ++ch) {
        const double o = h[ch] + at * (c[ch] - h[ch]);
        out[ch] = rt_dn::quantize(o);
        m2[ch] = h2[ch] + at * (s2[ch] - h2[ch]);
        const double vt = clip0(m2[ch] - o * o);
        const double vf = len < kVarMinLen ? vs[ch] : vt;
        var[ch] = vf * at;
    }
    return len;
}

// The buffers of a call, on the host or on the device: rt_temporal's and the history's second moment.
struct BuffersVar : Buffers {
    const double *prev_m2;          // [H][W][3] the previous call's out_m2, or null
};

RT_TP_FN uint32_t pixel_var_at(long long i, long long j, const Const &K, const BuffersVar &B, uint64_t out[3], double m2[3], double var[3])
{
    const long long W = K.width;
    const long long p = j * W + i;
    double c[3], n[3], z;
    colour_of(B.fix + 3 * p, B.count ? (double)B.count[p] : K.samples, c);
    const uint64_t hits = guides(B.feat + 8 * p, K.feat_spp, n, &z);
    auto tap = [&](long long ii, long long jj, TapVar *t) {
        const long long q = jj * W + ii;
        t->len = B.prev_len[q];
        t->hits = 0;
        if (t->len == 0u) return;                               // (pixel_var() reads nothing else of such a tap)
        t->hits = guides(B.prev_feat + 8 * q, K.prev_feat_spp, t->n, &t->z);
        for (int ch = 0; ch < 3; ++ch) { t->c[ch] = rt_dn::value(B.prev_fix[3 * q + ch]); t->m2[ch] = B.prev_m2[3 * q + ch]; }
    };
    auto colour = [&](long long ii, long long jj, double cq[3]) {
        const long long q = jj * W + ii;
        colour_of(B.fix + 3 * q, B.count ? (double)B.count[q] : K.samples, cq);
    };
    return pixel_var(i, j, K, c, hits, n, z, tap, colour, out, m2, var);
}

// The whole frame on host arrays, one pixel after the other -- rt_temporal_var_host and the stand-alone program.
inline void accumulate_var_host(const Const &K, const BuffersVar &B, uint64_t *out_fix, uint32_t *out_len, double *out_m2, double *out_var)
{
    for (long long j = 0; j < K.height; ++j)
        for (long long i = 0; i < K.width; ++i) {
            const long long p = j * K.width + i;
            out_len[p] = pixel_var_at(i, j, K, B, out_fix + 3 * p, out_m2 + 3 * p, out_var + 3 * p);
        }
}

} // namespace rt_tp
