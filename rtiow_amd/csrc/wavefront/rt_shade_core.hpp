// rt_shade_core.hpp -- the per-path bodies of the wavefront steps: the camera ray of a (pixel, sample), Scatter::scatter of the three
// materials on the keyed Philox stream, the sky sample, and the light sample of next-event estimation.  Values in, values out: no global
// load except the material record (the light sample: one entry each of the light list, the geometry and the emission table; the weighted choice: one per list entry), no store.
// wavefront/rt_shade.hip (one step per kernel: load -> call -> store) and wavefront/rt_paths.hip (the fused bounce step of the device path
// queue) call the same functions, so the arithmetic is stated once.  They COMPOSE rt_device.hpp (philox4x32_10, u01, u11,
// unit_sphere_accepts, unit_disk_accepts, reflect, refract, reflectance, min_1, unit_vector) and state none of it again.
#pragma once
#include "rt_params.hpp"
#include "rt_device.hpp"

namespace rt {

// a NaN result leaves as THE quiet NaN 0x7FF8000000000000, as the ray queries write it (IEEE 754 leaves sign and payload of a generated NaN open)
__device__ __forceinline__ double shade_canonical_nan(double x)
{
    return x != x ? __longlong_as_double(0x7FF8000000000000ll) : x;
}
__device__ __forceinline__ void store3(double *p, long long k, D3 v)
{
    p[3 * k] = shade_canonical_nan(v.x); p[3 * k + 1] = shade_canonical_nan(v.y); p[3 * k + 2] = shade_canonical_nan(v.z);
}

// ---- sample_ray: main.rs:131-134 + camera.rs:47-54, the render kernel's own start of a sample -----------------------------------------
// wm1, hm1: (double)(width - 1), (double)(height - 1).  Returns the next unused Philox block of the path's stream.
__device__ __forceinline__ uint32_t sample_ray(const KCamera &cam, uint32_t width, double wm1, double hm1, uint32_t g_pix, uint32_t g_s, uint32_t k0,
                                               uint32_t k1, D3 &origin, D3 &dir)
{
    const uint32_t j = g_pix / width, i = g_pix - j * width;
    U4 w = philox4x32_10(g_pix, g_s, 0u, 0u, k0, k1);
    uint32_t ev = 1u;
    const double cu = ((double)i + u01(w.x)) / wm1;                 // main.rs:131
    const double cv = ((double)j + u01(w.y)) / hm1;                 // main.rs:132
    // vec3.rs:59-68: block 0 = (u jitter, v jitter, lens x, lens y); every further block holds two tries
    uint32_t wx = w.z, wy = w.w;
    while (!unit_disk_accepts(wx, wy)) {
        w = philox4x32_10(g_pix, g_s, ev, 0u, k0, k1);
        ev++;
        wx = w.x; wy = w.y;
        if (!unit_disk_accepts(wx, wy)) { wx = w.z; wy = w.w; }
    }
    const D3 cam_origin = ld3(cam.origin);
    const D3 rd = mk(u11(wx), u11(wy), 0.0) * cam.lens_radius;
    const D3 offset = ld3(cam.u) * rd.x + ld3(cam.v) * rd.y;
    origin = cam_origin + offset;
    dir = (((ld3(cam.llc) + ld3(cam.horizontal) * cu) + ld3(cam.vertical) * cv) - cam_origin) - offset;
    return ev;
}

// ---- Scatter::scatter, materials.rs:21-31, 48-62, 76-105 ------------------------------------------------------------------------------
// The hit (d: the incoming direction; nrm, front: the record's normal and face) on the sphere whose material record is mrec.  ev: the
// path's next unused block, advanced.  Returns `absorbed`; otherwise ndir is the scattered direction and albedo the attenuation.
__device__ __forceinline__ bool scatter_path(const double *mrec, const D3 &d, const D3 &nrm, bool front, uint32_t g_pix, uint32_t g_s, uint32_t &ev,
                                             uint32_t k0, uint32_t k1, D3 &ndir, D3 &albedo)
{
    const double2 mA = *reinterpret_cast<const double2 *>(mrec);          // 1/r, param
    const double2 mB = *reinterpret_cast<const double2 *>(mrec + 2);      // albedo r, g
    const double2 mC = *reinterpret_cast<const double2 *>(mrec + 4);      // albedo b, kind
    const int kind = (int)mC.y;
    const double param = mA.y;
    albedo = mk(mB.x, mB.y, mC.x);                                        // (a Dialectric's record holds (1, 1, 1), materials.rs:103)

    bool absorbed = false;
    if (kind != RT_KIND_DIALECTRIC) {
        // vec3.rs:37-45: redraw until |p|^2 < 1, a plain loop to acceptance.  The tries of one scatter take consecutive words of consecutive
        // blocks: four tries per three blocks.
        U4 b = philox4x32_10(g_pix, g_s, ev, 0u, k0, k1);
        uint32_t nblk = 1u;
        uint32_t tx = b.x, ty = b.y, tz = b.z, c0 = b.w;
        bool ok = unit_sphere_accepts(tx, ty, tz);                                       // try 4m
        while (!ok) {
            b = philox4x32_10(g_pix, g_s, ev + nblk, 0u, k0, k1);
            nblk++;
            tx = c0; ty = b.x; tz = b.y;                                                 // try 4m+1
            ok = unit_sphere_accepts(tx, ty, tz);
            if (!ok) {
                const uint32_t c1 = b.z, c2 = b.w;
                b = philox4x32_10(g_pix, g_s, ev + nblk, 0u, k0, k1);
                nblk++;
                tx = c1; ty = c2; tz = b.x;                                              // try 4m+2
                ok = unit_sphere_accepts(tx, ty, tz);
                if (!ok) {
                    tx = b.y; ty = b.z; tz = b.w;                                        // try 4m+3: no new block
                    ok = unit_sphere_accepts(tx, ty, tz);
                    if (!ok) {
                        b = philox4x32_10(g_pix, g_s, ev + nblk, 0u, k0, k1);
                        nblk++;
                        tx = b.x; ty = b.y; tz = b.z; c0 = b.w;                          // try 4m+4 = try 0 of the next three blocks
                        ok = unit_sphere_accepts(tx, ty, tz);
                    }
                }
            }
        }
        ev += nblk;
        const D3 sp = mk(u11(tx), u11(ty), u11(tz));
        if (kind == RT_KIND_LAMBERTIAN) {                                                // materials.rs:21-31
            ndir = nrm + unit_vector(sp);
            const double eps = 1e-8;                                                     // vec3.rs:111-114
            if (__builtin_fabs(ndir.x) < eps && __builtin_fabs(ndir.y) < eps && __builtin_fabs(ndir.z) < eps) ndir = nrm;
        } else {                                                                         // materials.rs:48-62
            ndir = unit_vector(reflect(d, nrm)) + sp * param;
            absorbed = dot(ndir, nrm) <= 0.0;
        }
    } else {                                                                             // materials.rs:76-105
        const double ratio = front ? mrec[6] : param;                                    // 1.0 / ir, hoisted by the upload: the same operation
        const D3 ud = unit_vector(d);
        const double cos_theta = min_1(-dot(ud, nrm));
        const double sin_theta = __builtin_sqrt(1.0 - cos_theta * cos_theta);
        bool do_refract = false;
        if (ratio * sin_theta <= 1.0) {                                                  // && short-circuit: the draw only if it can refract
            const U4 w = philox4x32_10(g_pix, g_s, ev, 0u, k0, k1);
            ev++;
            do_refract = reflectance(cos_theta, ratio) <= u01(w.x);
        }
        ndir = do_refract ? refract(ud, nrm, ratio) : reflect(ud, nrm);
    }
    return absorbed;
}

// ---- contract C3: mulv(throughput, sky(dir)), main.rs:54-56 ---------------------------------------------------------------------------
// ... for a sky whose colour is `bottom` where unit_vector(dir).y = -1 and `top` where it is +1
__device__ __forceinline__ D3 sky_blend(const D3 &weight, const D3 &dir, const D3 &bottom, const D3 &top)
{
    const D3 ud = unit_vector(dir);                                                      // main.rs:54-56
    const double t = 0.5 * (ud.y + 1.0);
    const D3 sky = bottom * (1.0 - t) + top * t;
    return weight * sky;                                                                 // contract C3: mulv(throughput, sky)
}
__device__ __forceinline__ D3 sky_sample(const D3 &weight, const D3 &dir)
{
    return sky_blend(weight, dir, mk(1.0, 1.0, 1.0), mk(0.5, 0.7, 1.0));
}

// ---- next-event estimation: one light sampled by area at a Lambertian hit (rtiow_hip.h, "direct lighting") ---------
// Stated HERE and nowhere else.  Everything is + - * / and one sqrt in binary64, no contraction: the Lambertian BRDF albedo / pi and the
// area pdf 1 / (4 pi r^2 n_lights) leave no pi.

// Which face of sphere `hit` the ray (o, d) meets at the root t: the sign of dot(d, p - centre); the radius is not multiplied in.
__device__ __forceinline__ bool light_front(const KParams &P, const D3 &o, const D3 &d, int hit, double t)
{
    const double4 g = *reinterpret_cast<const double4 *>(P.geo + 4 * (size_t)hit);
    const D3 p = o + d * t;                                                              // ray.rs:15-17, as hit_record
    return dot(d, p - mk(g.x, g.y, g.z)) < 0.0;
}

// List entry s names no sphere of both tables: no contribution (no content of the list makes a read leave the tables).  A macro, not a
// function: bounce_nee_kernel's machine code is pinned (profiles/isa_fingerprint_nee.txt), and behind an inlined call the compiler
// schedules that kernel's Philox rounds in another order.
#define RT_NAMES_NO_LIGHT(P, emission, n_emission, s) ((s) < 0 || (s) >= (P).n_spheres || !(emission) || (s) >= (n_emission))

// The uniform choice among n list entries from one Philox word: floor(word * n / 2^32).
__device__ __forceinline__ uint32_t uniform_pick(uint32_t word, int32_t n)
{
    return (uint32_t)(((unsigned long long)word * (unsigned long long)(uint32_t)n) >> 32);
}

// The light sample of the path (g_pix, g_s) whose event on entry -- DIRECT bit masked off -- was ev_in, at the hit point p with the
// record's normal n; weight: throughput * albedo, the path's new throughput.  The draws are the blocks (g_pix, g_s, ev_in, 1 + m), m = 0,
// 1, ...: word 3 >= 1 is used by nothing else and ev_in is unique per bounce, so the path's own stream is not touched.  Block 0: x chooses
// the light, (y, z, w) is the first unit-sphere try; every further block holds one try (x, y, z).  Returns whether there is a shadow ray
// to trace -- (p, dv), not normalised -- and then c, the radiance to add if the closest hit along it is sphere li.
__device__ __forceinline__ bool nee_sample(const KParams &P, const double *emission, int32_t n_emission, const int32_t *lights, int32_t n_lights,
                                           const D3 &p, const D3 &n, const D3 &weight, uint32_t g_pix, uint32_t g_s, uint32_t ev_in, D3 &dv, D3 &c,
                                           int &li)
{
    U4 b = philox4x32_10(g_pix, g_s, ev_in, 1u, P.k0, P.k1);
    li = lights[uniform_pick(b.x, n_lights)];
    if (RT_NAMES_NO_LIGHT(P, emission, n_emission, li)) return false;
    uint32_t tx = b.y, ty = b.z, tz = b.w;
    for (uint32_t m = 1u; !unit_sphere_accepts(tx, ty, tz); ++m) {                       // vec3.rs:37-45: a plain loop to acceptance
        b = philox4x32_10(g_pix, g_s, ev_in, 1u + m, P.k0, P.k1);
        tx = b.x; ty = b.y; tz = b.z;
    }
    const D3 u = unit_vector(mk(u11(tx), u11(ty), u11(tz)));
    const double4 g = *reinterpret_cast<const double4 *>(P.geo + 4 * (size_t)li);        // centre, r^2
    const D3 q = mk(g.x, g.y, g.z) + u * __builtin_sqrt(g.w);                            // a uniform point of the light's surface
    dv = q - p;
    const double ns = dot(n, dv);
    const double nl = 0.0 - dot(u, dv);
    const double dd = dot(dv, dv);
    if (!(ns > 0.0 && nl > 0.0)) return false;                                           // below either horizon; a NaN fails this
    const double w = ((4.0 * g.w) * (double)n_lights) * ((ns * nl) / (dd * dd));
    c = (weight * ld3(emission + 3 * (size_t)li)) * w;
    return true;
}

// ---- ... or by solid angle: a uniform direction of the cone the light subtends from p (RT_DIRECT_CONE) -------------
// Steps 2 to 9 of the cone sample, for the light li (a sphere of the geometry table) whatever chose it: nee_sample_cone's and
// nee_sample_weighted's, stated HERE and nowhere else.  b: block 0 of the sample, of which y is the polar draw and (z, w) the first
// unit-disk try, whose normalised point is (cos phi, sin phi); every further block holds one try (x, y).  + - * / and sqrt in binary64, no
// contraction, in this order.  Returns whether there is a shadow ray (p, dv) -- dv a unit vector up to rounding --, and then k = 1 - cos
// theta_max and ns = dot(n, dv) for the caller's weight.
__device__ __forceinline__ bool cone_toward(const KParams &P, int li, const D3 &p, const D3 &n, U4 b, uint32_t g_pix, uint32_t g_s, uint32_t ev_in,
                                            D3 &dv, double &k, double &ns)
{
    const double4 g = *reinterpret_cast<const double4 *>(P.geo + 4 * (size_t)li);        // centre, r^2
    const D3 wv = mk(g.x, g.y, g.z) - p;
    const double d2 = (wv.x * wv.x + wv.y * wv.y) + wv.z * wv.z;
    if (!(d2 > g.w)) return false;                                                       // p inside or on the light; a NaN fails this
    const double q = g.w / d2;
    const double cm = __builtin_sqrt(1.0 - q);                                           // cos theta_max
    k = q / (1.0 + cm);                                                                  // 1 - cos theta_max, without the cancellation
    const double s = u01(b.y) * k;
    const double ct = 1.0 - s;
    const double st = __builtin_sqrt(s * (1.0 + ct));
    uint32_t tx = b.z, ty = b.w;
    for (uint32_t m = 1u; !unit_disk_accepts(tx, ty); ++m) {                             // vec3.rs:59-68: a plain loop to acceptance
        b = philox4x32_10(g_pix, g_s, ev_in, 1u + m, P.k0, P.k1);
        tx = b.x; ty = b.y;
    }
    const double hx = u11(tx), hy = u11(ty);
    const double il = 1.0 / __builtin_sqrt(hx * hx + hy * hy);                           // (the all-zero try: NaNs, which ns > 0.0 drops)
    const double cphi = hx * il, sphi = hy * il;
    const D3 w = wv * (1.0 / __builtin_sqrt(d2));
    const D3 a = __builtin_fabs(w.x) > 0.9 ? mk(0.0, 1.0, 0.0) : mk(1.0, 0.0, 0.0);
    const D3 t0 = mk(a.y * w.z - a.z * w.y, a.z * w.x - a.x * w.z, a.x * w.y - a.y * w.x);
    const D3 t = t0 * (1.0 / __builtin_sqrt(dot(t0, t0)));
    const D3 bt = mk(w.y * t.z - w.z * t.y, w.z * t.x - w.x * t.z, w.x * t.y - w.y * t.x);
    dv = (t * (st * cphi) + bt * (st * sphi)) + w * ct;
    ns = dot(n, dv);
    return ns > 0.0;                                                                     // below the hit's horizon: none; a NaN fails this
}

// nee_sample's arguments, blocks and result.  Block 0: x chooses the light (step 1), the rest is cone_toward's.  The BRDF albedo / pi and
// the cone pdf 1 / (2 pi (1 - cos theta_max) n_lights) leave no pi, and the weight 2 k n_lights ns (step 10) is bounded by 2 n_lights
// whatever the geometry (k <= 1, ns <= 1).
__device__ __forceinline__ bool nee_sample_cone(const KParams &P, const double *emission, int32_t n_emission, const int32_t *lights, int32_t n_lights,
                                                const D3 &p, const D3 &n, const D3 &weight, uint32_t g_pix, uint32_t g_s, uint32_t ev_in, D3 &dv, D3 &c,
                                                int &li)
{
    const U4 b = philox4x32_10(g_pix, g_s, ev_in, 1u, P.k0, P.k1);
    li = lights[uniform_pick(b.x, n_lights)];
    if (RT_NAMES_NO_LIGHT(P, emission, n_emission, li)) return false;
    double k, ns;
    if (!cone_toward(P, li, p, n, b, g_pix, g_s, ev_in, dv, k, ns)) return false;
    const double wgt = ((2.0 * k) * (double)n_lights) * ns;
    c = (weight * ld3(emission + 3 * (size_t)li)) * wgt;
    return true;
}

// ---- ... with the light chosen by what it can contribute at p (RT_DIRECT_WEIGHTED | RT_DIRECT_CONE) ---------------
// The importance of list entry i at p: (r^2 / d^2) max(e) for an entry that names a sphere of both tables, emits, and does not contain p;
// else 0.  One division, no sqrt.  i, the list, the geometry and the emission table are wave-uniform: only p is the lane's own.
__device__ __forceinline__ double light_importance(const KParams &P, const double *emission, int32_t n_emission, const int32_t *lights, int32_t i,
                                                   const D3 &p)
{
    const int s = lights[i];
    if (RT_NAMES_NO_LIGHT(P, emission, n_emission, s)) return 0.0;
    const double4 g = *reinterpret_cast<const double4 *>(P.geo + 4 * (size_t)s);         // centre, r^2
    const D3 e = ld3(emission + 3 * (size_t)s);
    const D3 wv = mk(g.x, g.y, g.z) - p;
    const double d2 = (wv.x * wv.x + wv.y * wv.y) + wv.z * wv.z;
    double em = e.x > e.y ? e.x : e.y;                                                   // (a NaN on the left of > is dropped, one on the
    em = em > e.z ? em : e.z;                                                            //  right is taken and fails v > 0.0)
    const double v = (g.w / d2) * em;
    return (d2 > g.w && v > 0.0) ? v : 0.0;                                              // a NaN fails either test
}

// nee_sample_cone's arguments, blocks and result.  Word x of block 0 chooses the light with probability imp_j / tot instead of 1 / n_lights:
// two walks over the list, the first for the total, the second -- the same expressions, the same running sum -- for the first entry whose
// partial sum exceeds u01(x) tot.  Then cone_toward for that light (imp_j > 0.0 has decided its d2 > r^2 already), and the weight
// 2 k ns (tot / imp_j) in the place of 2 k n_lights ns: k <= r^2 / d^2 and e / max(e) <= 1, so one sample adds at most 2 sum_i max(e_i) per
// unit of throughput, and with one valid light tot / imp_j is exactly 1.0 and the sample is nee_sample_cone's, bit for bit.
__device__ __forceinline__ bool nee_sample_weighted(const KParams &P, const double *emission, int32_t n_emission, const int32_t *lights, int32_t n_lights,
                                                    const D3 &p, const D3 &n, const D3 &weight, uint32_t g_pix, uint32_t g_s, uint32_t ev_in, D3 &dv,
                                                    D3 &c, int &li)
{
    const U4 b = philox4x32_10(g_pix, g_s, ev_in, 1u, P.k0, P.k1);
    double tot = 0.0;
    for (int32_t i = 0; i < n_lights; ++i) {
        const double imp = light_importance(P, emission, n_emission, lights, i, p);
        if (imp > 0.0) tot += imp;
    }
    if (!(tot > 0.0)) return false;                                                      // no light can contribute at p
    const double x = u01(b.x) * tot;
    double acc = 0.0, imp_j = 0.0;
    int32_t j = -1;
    bool found = false;
    for (int32_t i = 0; i < n_lights; ++i) {
        const double imp = light_importance(P, emission, n_emission, lights, i, p);
        if (imp > 0.0) {
            acc += imp;
            if (!found) { j = i; imp_j = imp; found = x < acc; }                         // (x rounded up to tot: the last positive entry stays)
        }
    }
    if (j < 0) return false;                                                             // (tot > 0.0 has decided this already)
    li = lights[j];
    double k, ns;
    if (!cone_toward(P, li, p, n, b, g_pix, g_s, ev_in, dv, k, ns)) return false;
    const double wgt = ((2.0 * k) * ns) * (tot / imp_j);
    c = (weight * ld3(emission + 3 * (size_t)li)) * wgt;
    return true;
}

// bounce_trip's MODE (wavefront/rt_paths.hip); from kNee on, which sampler a Lambertian hit calls
constexpr int kUnlit = 0, kLit = 1, kNee = 2, kNeeCone = 3, kNeeWeighted = 4;

// the sampler of MODE: nee_sample's arguments and result
template <int MODE>
__device__ __forceinline__ bool nee_sample_for(const KParams &P, const double *emission, int32_t n_emission, const int32_t *lights, int32_t n_lights,
                                               const D3 &p, const D3 &n, const D3 &weight, uint32_t g_pix, uint32_t g_s, uint32_t ev_in, D3 &dv, D3 &c,
                                               int &li)
{
    static_assert(MODE == kNee || MODE == kNeeCone || MODE == kNeeWeighted, "a mode without direct lighting has no sampler");
    if constexpr (MODE == kNeeWeighted) return nee_sample_weighted(P, emission, n_emission, lights, n_lights, p, n, weight, g_pix, g_s, ev_in, dv, c, li);
    else if constexpr (MODE == kNeeCone) return nee_sample_cone(P, emission, n_emission, lights, n_lights, p, n, weight, g_pix, g_s, ev_in, dv, c, li);
    else return nee_sample(P, emission, n_emission, lights, n_lights, p, n, weight, g_pix, g_s, ev_in, dv, c, li);
}

#undef RT_NAMES_NO_LIGHT

// ---- the environment: a cube map the path queue looks up on a miss and samples at a Lambertian hit (rtiow_hip.h, "environment"; DESIGN.md
// section 27).  Stated HERE and nowhere else.  Everything is + - * / in binary64, no contraction, and one constant for pi: no sqrt, no
// atan2.  size: texels per face edge, a power of two (the host has checked it); texels: [6][size][size][3]; cdf: [6 size^2] running sums.
constexpr int kEnv = 5;                                                                  // bounce_trip's MODE of the environment step

// one in-face coordinate c in [-1, 1] -> its texel row: a NaN fails both comparisons and gives 0
__device__ __forceinline__ int env_row(double c, int size)
{
    const double x = ((c + 1.0) * 0.5) * (double)size;
    return x >= (double)size ? size - 1 : (x >= 0.0 ? (int)x : 0);
}

// The texel a direction names, d not normalised: the face by strict comparisons (x wins ties over y, y over z; a NaN never wins), the
// texel by one division per coordinate.  Every bit pattern of d names a texel inside the table.
__device__ __forceinline__ int env_lookup(const D3 &d, int size)
{
    int ax = 0;
    double m = __builtin_fabs(d.x);
    if (__builtin_fabs(d.y) > m) { ax = 1; m = __builtin_fabs(d.y); }
    if (__builtin_fabs(d.z) > m) { ax = 2; m = __builtin_fabs(d.z); }
    const double on = ax == 0 ? d.x : ax == 1 ? d.y : d.z;
    const int f = 2 * ax + (on < 0.0 ? 1 : 0);
    const double a = (ax == 0 ? d.y : d.x) / m;                                          // the other two components, in axis order
    const double b = (ax == 2 ? d.y : d.z) / m;
    return (f * size + env_row(a, size)) * size + env_row(b, size);
}

// The environment sample of the path (g_pix, g_s) whose event on entry -- DIRECT bit masked off -- was ev_in, at the hit point with the
// record's normal n; weight: throughput * albedo; tot = cdf[6 size^2 - 1], > 0 and finite (the caller has decided that).  ONE block,
// (g_pix, g_s, ev_in, 1): x chooses the texel by a binary search of the running sums -- the first entry above u01(x) tot; NaNs send it
// right, it never leaves the table --, (y, z) a point of the texel's square.  A direction uniform over that square has the solid-angle
// density r^3 / s^2, so with the Lambertian BRDF albedo / pi the weight is ns s^2 / (pi P dd^2), dd = r^2 = dot(dv, dv): no sqrt.
// Returns whether there is a shadow ray to trace -- dv from the hit point, not normalised -- and then c, the radiance to add if that ray
// meets no sphere.
__device__ __forceinline__ bool env_sample(const KParams &P, const double *texels, const double *cdf, int size, double tot, const D3 &n,
                                           const D3 &weight, uint32_t g_pix, uint32_t g_s, uint32_t ev_in, D3 &dv, D3 &c)
{
    const U4 b = philox4x32_10(g_pix, g_s, ev_in, 1u, P.k0, P.k1);
    const double x = u01(b.x) * tot;
    int lo = 0, hi = 6 * size * size - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > x) hi = mid; else lo = mid + 1;
    }
    const int k = lo;
    const double pk = (cdf[k] - (k ? cdf[k - 1] : 0.0)) / tot;
    if (!(pk > 0.0)) return false;                                                       // a texel of no weight, or a NaN
    const int sh = __builtin_ctz((unsigned)size);
    const int f = k >> (2 * sh), i = (k >> sh) & (size - 1), j = k & (size - 1);
    const double s = 2.0 / (double)size;
    const double ta = ((double)i + u01(b.y)) * s - 1.0;
    const double tb = ((double)j + u01(b.z)) * s - 1.0;
    const double on = (f & 1) ? -1.0 : 1.0;
    const int ax = f >> 1;
    dv = ax == 0 ? mk(on, ta, tb) : ax == 1 ? mk(ta, on, tb) : mk(ta, tb, on);
    const double ns = dot(n, dv);
    const double dd = dot(dv, dv);
    if (!(ns > 0.0)) return false;                                                       // below the hit's horizon; a NaN fails this
    const double pi = __longlong_as_double(0x400921FB54442D18ll);
    const double w = (ns * (s * s)) / ((pi * pk) * (dd * dd));
    c = (weight * ld3(texels + 3 * (size_t)k)) * w;
    return true;
}

} // namespace rt
