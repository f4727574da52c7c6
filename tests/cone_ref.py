"""CPU statement of direct lighting by solid angle in the lit path queue (include/rtiow_hip.h "direct lighting by solid angle", DESIGN.md
section 22) -- a test helper.

Composed from tests/nee_ref.py (the DIRECT bit, the face a path that carries it does not count again, which paths sample), through it
tests/lights_ref.py and tests/paths_ref.py, and tests/trace_ref.py (fast_hit: the closest hit of the shadow ray), restating none of them:
here is only the light sample -- a uniform direction of the cone the sphere subtends from the hit point -- and nee_ref's loop with that
sampler in the place of its own.  The arithmetic is IEEE binary64 without fused multiply-add, in exactly the order the contract writes.
"""
import functools

import numpy as np

import lights_ref as lr
import nee_ref as nr
import oracle
import paths_ref as pr
import wavefront_ref as wr
from trace_ref import Scene, fast_hit

CONE = 2                                           # RT_DIRECT_CONE
DIRECT, MASK64 = nr.DIRECT, nr.MASK64
F = np.float64


def cross(a, b):
    """The general form, every product written out (a zero component of `a` still multiplies)."""
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def sample_light_cone(scene, seed, light, lights, pixel, sample, ev_in, p, n, weight, t_min=1e-4):
    """Steps 1 .. 11 of the contract for one Lambertian hit -> dict(j, li, tries, d2, r2, k, wx, ns, shadow: a shadow ray is traced, dv:
    its direction, visible, front: the face of the closest hit, c: what the path adds per channel if visible, else None).  weight:
    throughput * albedo, the path's new throughput."""
    key = wr.key_of(seed)
    block = lambda m: oracle.philox((int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF, int(ev_in) & 0xFFFFFFFF, 1 + m), key)
    b0 = block(0)
    j = (int(b0[0]) * len(lights)) >> 32                                              # 1
    li = int(lights[j])
    out = dict(j=j, li=li, tries=0, d2=None, r2=None, k=None, wx=None, ns=None, shadow=False, visible=False, front=None, c=None, word=int(b0[0]))
    if li < 0 or li >= scene.n or light.emission is None or li >= len(light.emission):
        return out
    with np.errstate(all="ignore"):
        c_li, radius = scene.flat[li]["center"], F(scene.flat[li]["radius"])
        r2 = radius * radius                                                          # as the upload builds the geometry table
        wv = [F(c_li[k]) - F(p[k]) for k in range(3)]                                 # 2
        d2 = (wv[0] * wv[0] + wv[1] * wv[1]) + wv[2] * wv[2]
        out["d2"], out["r2"] = float(d2), float(r2)
        if not d2 > r2:                                                               # inside or on the light; a NaN fails this
            return out
        q = r2 / d2                                                                   # 3
        cm = np.sqrt(F(1.0) - q)
        k = q / (F(1.0) + cm)
        out["k"] = float(k)
        s = F(wr.u01(b0[1])) * k                                                      # 4
        ct = F(1.0) - s
        st = np.sqrt(s * (F(1.0) + ct))
        tx, ty = b0[2], b0[3]                                                         # 5
        m = 0
        while True:
            hx, hy = F(wr.u11(tx)), F(wr.u11(ty))
            if hx * hx + hy * hy < 1.0:                                               # vec3.rs:59-68
                break
            m += 1
            tx, ty = block(m)[:2]
        out["tries"] = m + 1
        il = F(1.0) / np.sqrt(hx * hx + hy * hy)
        cphi, sphi = hx * il, hy * il
        inv = F(1.0) / np.sqrt(d2)                                                    # 6
        w = [wv[k] * inv for k in range(3)]
        out["wx"] = float(w[0])
        a = [F(0.0), F(1.0), F(0.0)] if np.fabs(w[0]) > 0.9 else [F(1.0), F(0.0), F(0.0)]      # 7
        t0 = cross(a, w)
        it = F(1.0) / np.sqrt(t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2])
        t = [t0[k] * it for k in range(3)]
        b = cross(w, t)
        sc, ss = st * cphi, st * sphi                                                 # 8
        dv = [(t[k] * sc + b[k] * ss) + w[k] * ct for k in range(3)]
        ns = nr.dot([F(x) for x in n], dv)                                            # 9
        out["ns"] = float(ns)
        if not ns > 0.0:                                                              # a NaN fails this
            return out
        wgt = ((F(2.0) * k) * F(len(lights))) * ns                                    # 10
        out["c"] = [float((F(weight[k]) * F(light.emission[li][k])) * wgt) for k in range(3)]
    out["shadow"] = True
    out["dv"] = [float(x) for x in dv]
    hit = fast_hit(scene, [float(x) for x in p], out["dv"], t_min)                   # 11
    out["visible"] = hit[0] == li                                                     # the CLOSEST hit is the light itself, either face
    out["front"] = hit[4] if hit[0] >= 0 else None
    return out


def sampler_of(flags):
    """The light sample of direct->flags: CONE: sample_light_cone; 0: nee_ref.sample_light."""
    assert flags in (0, CONE)
    return sample_light_cone if flags & CONE else nr.sample_light


def bounce_cone(scene, queue, seed, npix, light, lights, no_direct=False, t_min=1e-4, flags=CONE):
    """nee_ref.bounce_direct with the light sample of direct->flags."""
    return nr.bounce_direct(scene, queue, seed, npix, light, lights, sampler_of(flags), no_direct, t_min)


def step_cone(scene, queue, seed, npix, light, lights, no_direct=False, t_min=1e-4, flags=CONE):
    """nee_ref.step_direct with the light sample of direct->flags."""
    return nr.step_direct(scene, queue, seed, npix, light, lights, sampler_of(flags), no_direct, t_min)


def render_cone(flat, ocam, width, height, spp, light, *, flags=CONE, **frame):
    """rt_render_wavefront_nee_sampled: nee_ref.render_direct (whose keywords `frame` holds) with the light sample of direct_flags."""
    return nr.render_direct(flat, ocam, width, height, spp, light, sampler_of(flags), **frame)


# ---- the hand-built cone queue of the GPU tests: hard by construction, checked by tests/test_cone_host.py -----------------------------------

SEED, HAND_N, HAND_NPIX = nr.SEED, nr.HAND_N, nr.HAND_NPIX
T_MIN = 1e-4
# the slot whose hit point the last sphere is built around: an oblique ray onto sphere 0 (centre (-6, 1, 0), radius 1) at (-6, 1.8, 0.6),
# 45 degrees from the normal; NEAR_AXIS is perpendicular to it and 45 degrees from the normal on the other side
NEAR_SLOT, NEAR_ORIGIN, NEAR_DIR = 55, (-6.0, 1.8 + 2.1, 0.6 - 0.3), (0.0, -1.4, 0.2)
NEAR_AXIS, NEAR_RADIUS, NEAR_GAP = (0.0, 0.2, 1.4), 0.05, 5.0e-5
# four more spheres over nee_ref.hand_queue()'s seventeen: sphere -> (centre, radius, emission); all Lambertian, albedo 0.5
EXTRA = [
    ((594.0, 802.0, 0.0), 1.0e-3, (1.0e6, 2.0e6, 5.0e5)),      # 17: a light at r / d = 1e-6 from sphere 0: k = 5e-13 only by the stable form
    ((-10.0, 2.5, 0.0), 0.5, (2.0, 3.0, 1.0)),                 # 18: a light beside sphere 0: |w.x| > 0.9
    ((-6.8, 1.6, 0.0), 0.3, (1.0, 1.0, 2.0)),                  # 19: a light that holds a piece of sphere 0's surface
    (None, NEAR_RADIUS, (5.0, 1.0, 1.0)),                      # 20: a light whose surface passes NEAR_GAP (< t_min) from NEAR_SLOT's hit point
]
LIGHTS = nr.LIGHTS + (17, 18, 19, 20)
# slot -> what it was rebuilt to do (test_cone_host.py checks each with the statement); every slot below 63
CASES = {1: "inside_light", 19: "below_horizon", 23: "wx_below", 25: "blocked", 31: "first_try", 37: "later_block", 43: "wx_above", 49: "out_of_range",
         NEAR_SLOT: "inner_face", 61: "far_light"}
DIRECT_SLOTS = nr.DIRECT_SLOTS                             # these carry the DIRECT bit on entry: 6 a light's front face, 7 a back face
ALL_WAVE, LAST_LANE_WAVE = nr.ALL_WAVE, nr.LAST_LANE_WAVE  # every lane a shadow ray; only lane 63


def _matches(what, s):
    if what == "inside_light":
        return s["li"] == 19 and s["d2"] is not None and s["d2"] <= s["r2"] and not s["shadow"]
    if what == "below_horizon":
        return s["ns"] is not None and s["ns"] <= 0.0
    if what == "wx_below":
        return s["li"] == 14 and abs(s["wx"]) < 0.9 and s["visible"]
    if what == "blocked":
        return s["li"] == 14 and s["shadow"] and not s["visible"]
    if what == "first_try":
        return s["tries"] == 1 and s["visible"]
    if what == "later_block":
        return s["tries"] >= 3 and s["visible"]
    if what == "wx_above":
        return s["li"] == 18 and abs(s["wx"]) > 0.9 and s["visible"]
    if what == "out_of_range":
        return s["li"] in (99, -1)
    if what == "inner_face":
        return s["li"] == 20 and s["visible"] and s["front"] == 0
    if what == "far_light":
        return s["li"] == 17 and s["visible"]
    if what == "shadow":
        return s["shadow"]
    raise KeyError(what)


@functools.lru_cache(None)
def hand_queue():
    """(flat, queue, light, lights): nee_ref.hand_queue()'s scene with EXTRA (no path of the original comes near: 17 is far away, 18 and 19
    sit beside the rays that come down onto sphere 0, 20 is 5 cm wide), its 513 paths with the slots of CASES and the two waves of the
    second workgroup searched again -- with the statement alone -- so that the CONE sample of each is the named case, and the list LIGHTS.
    Slots 1 and NEAR_SLOT get rays of their own.  Read-only."""
    import rtiow_amd as rt
    base_flat, base_q, base_light, _ = nr.hand_queue()
    q = {f: np.array(base_q[f], copy=True) for f in pr.FIELDS}
    # slot 1 starts INSIDE light 19 and runs to sphere 0's centre: its hit point lies inside the light, which it never meets
    q["origin"][1], q["dir"][1] = (-6.92, 1.69, 0.1), (0.92, -0.69, -0.1)
    q["origin"][NEAR_SLOT], q["dir"][NEAR_SLOT] = NEAR_ORIGIN, NEAR_DIR
    hit = fast_hit(Scene(base_flat), list(NEAR_ORIGIN), list(NEAR_DIR), T_MIN)
    assert hit[0] == 0
    axis = np.array(NEAR_AXIS) / np.linalg.norm(NEAR_AXIS)
    assert abs(float(np.dot(axis, NEAR_DIR))) < 1e-12                                 # the ray passes the light at NEAR_RADIUS + NEAR_GAP: no hit
    near_centre = tuple(float(x) for x in np.array(hit[2]) + axis * (NEAR_RADIUS + NEAR_GAP))
    flat = np.zeros(len(base_flat) + len(EXTRA), dtype=rt.SPHERE_DTYPE)
    flat[:len(base_flat)] = base_flat
    for k, (centre, radius, _) in enumerate(EXTRA, start=len(base_flat)):
        flat[k]["center"], flat[k]["radius"] = near_centre if centre is None else centre, radius
        flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = (0.5, 0.5, 0.5), 0.0, wr.LAMBERTIAN
    emission = np.concatenate([base_light.emission, np.array([e for *_, e in EXTRA], dtype=np.float64)])
    light = lr.Light(base_light.sky_bottom, base_light.sky_top, emission)
    scene = Scene(flat)

    def search(k, what):
        """Slot k, a path that ends on Lambertian sphere 0: the sample below 4000 that makes its light sample `what`."""
        idx, _, p, nrm, _ = fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), T_MIN)
        assert idx == 0, (k, idx)
        q["pixel"][k] = k % HAND_NPIX
        ev_in = int(q["event"][k]) & 0x7FFFFFFF
        with np.errstate(all="ignore"):
            weight = [float(F(q["throughput"][k][c]) * F(flat[0]["albedo"][c])) for c in range(3)]
        for sample in range(4000):
            if _matches(what, sample_light_cone(scene, SEED, light, LIGHTS, k % HAND_NPIX, sample, ev_in, p, nrm, weight, T_MIN)):
                q["sample"][k] = sample
                return
        raise AssertionError(f"no sample below 4000 makes slot {k} the case {what}")

    for k, what in CASES.items():
        search(k, what)
    for k in ALL_WAVE:
        search(k, "shadow")
    search(LAST_LANE_WAVE[-1], "shadow")
    for a in list(q.values()) + [emission]:
        a.setflags(write=False)
    return flat, q, light, LIGHTS


@functools.lru_cache(None)
def hand_step(count, no_direct=False, flags=CONE):
    """The statement's answer for the first `count` paths of hand_queue() (computed once per setting, read-only)."""
    flat, q, light, lights = hand_queue()
    out, adds, live, shadow = step_cone(flat, pr.prefix(q, count), SEED, HAND_NPIX, light, lights, no_direct, T_MIN, flags)
    for a in list(out.values()) + [adds]:
        a.setflags(write=False)
    return out, adds, live, shadow


# ---- the cone book frame ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def book_frame(max_depth, batch=257):
    """The statement's cone frame of lights_ref.book_case() at `max_depth` -> (fix, rays, shadow rays), read-only."""
    flat, light, _ = lr.book_case()
    fix, rays, shadow = render_cone(flat, oracle.book1_camera(lr.BW, lr.BH), lr.BW, lr.BH, lr.BSPP, light, max_depth=max_depth, seed=1, batch=batch)
    fix.setflags(write=False)
    return fix, rays, shadow


# ---- the big-light scene: where area sampling is worse than none ---------------------------------------------------------------------------------

BIG_W, BIG_H, BIG_SPP, BIG_DEPTH = 16, 12, 64, 8
BIG_SEEDS = nr.STAT_SEEDS
BIG_LIGHT = 1
BIG_EMISSION = (4.0, 3.2, 2.4)


def big_light_scene():
    """(flat, light): a Lambertian ground and, resting on it, a light of radius 1 -- the shape of a night frame lit by the book scene's
    large sphere --, a Lambertian, a Metal and a Dialectric sphere beside it; a black sky.  Every hit point of the ground near the light
    sees it under a large solid angle and from close by, where the area sample's weight 4 r^2 n (ns nl) / dd^2 has no bound."""
    import rtiow_amd as rt
    spheres = [((0.0, -1000.0, 0.0), 1000.0, wr.LAMBERTIAN, (0.6, 0.6, 0.6), 0.0),
               ((0.0, 1.0, 0.0), 1.0, wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0),
               ((1.6, 0.5, 0.3), 0.5, wr.LAMBERTIAN, (0.7, 0.3, 0.3), 0.0),
               ((-1.7, 0.5, 0.6), 0.5, wr.METAL, (0.8, 0.8, 0.8), 0.0),
               ((1.1, 0.3, 1.4), 0.3, wr.DIALECTRIC, (1.0, 1.0, 1.0), 1.5)]
    flat = np.zeros(len(spheres), dtype=rt.SPHERE_DTYPE)
    for k, (centre, radius, kind, albedo, param) in enumerate(spheres):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = centre, radius, albedo, param, kind
    emission = np.zeros((len(spheres), 3))
    emission[BIG_LIGHT] = BIG_EMISSION
    return flat, lr.Light((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), emission)


def big_light_camera():
    from rtiow_amd.scene import Camera
    return Camera((0.0, 2.5, 7.0), (0.6, 0.4, 0.0), (0.0, 1.0, 0.0), 35.0, BIG_W / BIG_H, 0.0, 7.0)


def cone_sample_bound(emission=None):
    """The largest value one sample can add in one channel under cone sampling, whatever the geometry, per unit of throughput: a light hit
    adds throughput * e; a light sample adds (throughput * albedo) * e * wgt with albedo <= 1 and wgt = 2 k n_lights ns <= 2 n_lights,
    because k = 1 - cos(theta_max) <= 1 and ns is the dot product of two unit vectors."""
    if emission is None:
        emission = big_light_scene()[1].emission
    e = np.array(emission, dtype=np.float64)
    return float(e.max()) * max(1.0, 2.0 * len(nr.light_list(e)))
