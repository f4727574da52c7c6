"""CPU statement of next-event estimation in the lit path queue (include/rtiow_hip.h "direct lighting") -- a test helper.

Composed from tests/lights_ref.py (bounce_lit: the sky, which sphere is a light, what a path adds there and that it ends; through it
tests/paths_ref.py: what a path that scatters does, and the queue) and tests/trace_ref.py (fast_hit: the closest hit, of the path's ray and
of the shadow ray) and restating none of them: here is only what direct lighting adds -- the DIRECT bit of the event word, the light's face a
path that carries it does not count again, the light sample at a Lambertian hit and the shadow ray that decides it.  The arithmetic is
IEEE binary64 without fused multiply-add, left to right as dot and length_squared write it.
"""
import functools
import math

import numpy as np

import lights_ref as lr
import oracle
import paths_ref as pr
import wavefront_ref as wr
from trace_ref import Scene, fast_hit

DIRECT = 0x80000000                                # RT_PATH_EVENT_DIRECT
NO_DIRECT = 1                                      # RT_STEP_NO_DIRECT
OUTSIDE = 0xFFFFFFFF                               # a pixel outside every frame: such a path adds nothing
MASK64 = lr.MASK64
F = np.float64


def light_list(emission):
    """rt_light_list: the indices whose entry lights_ref.is_light takes for a light, ascending."""
    return [] if emission is None else [s for s in range(len(emission)) if lr.is_light(emission[s])]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def light_front(scene, idx, d, p):
    """Which face of sphere idx the ray of direction d meets at p: dot(d, p - centre) < 0.0; the radius is not multiplied in."""
    c = scene.flat[idx]["center"]
    with np.errstate(all="ignore"):
        return bool(dot([F(x) for x in d], [F(p[k]) - F(c[k]) for k in range(3)]) < 0.0)


def sample_light(scene, seed, light, lights, pixel, sample, ev_in, p, n, weight, t_min=1e-4):
    """Steps 1 .. 15 of the contract for one Lambertian hit -> dict(j, li, tries, ns, nl, shadow: a shadow ray is traced, visible, c: what
    the path adds per channel if visible, else None).  weight: throughput * albedo, the path's new throughput."""
    key = wr.key_of(seed)
    block = lambda m: oracle.philox((int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF, int(ev_in) & 0xFFFFFFFF, 1 + m), key)
    b0 = block(0)
    j = (int(b0[0]) * len(lights)) >> 32
    li = int(lights[j])
    out = dict(j=j, li=li, tries=0, ns=None, nl=None, shadow=False, visible=False, c=None, word=int(b0[0]))
    if li < 0 or li >= scene.n or light.emission is None or li >= len(light.emission):
        return out
    tx, ty, tz = b0[1], b0[2], b0[3]
    m = 0
    while True:
        x, y, z = wr.u11(tx), wr.u11(ty), wr.u11(tz)
        if x * x + y * y + z * z < 1.0:                                           # vec3.rs:37-45, as wavefront_ref.unit_sphere_run
            break
        m += 1
        tx, ty, tz = block(m)[:3]
    out["tries"] = m + 1
    with np.errstate(all="ignore"):
        v = [F(x), F(y), F(z)]
        inv = F(1.0) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])           # unit_vector: v * (1 / length)
        u = [v[k] * inv for k in range(3)]
        c_li, radius = scene.flat[li]["center"], F(scene.flat[li]["radius"])
        r2 = radius * radius                                                      # as the upload builds the geometry table
        root = np.sqrt(r2)
        q = [F(c_li[k]) + u[k] * root for k in range(3)]
        dv = [q[k] - F(p[k]) for k in range(3)]
        ns = dot([F(a) for a in n], dv)
        nl = F(0.0) - dot(u, dv)
        dd = dot(dv, dv)
        out["ns"], out["nl"] = float(ns), float(nl)
        if not (ns > 0.0 and nl > 0.0):                                            # a NaN fails this
            return out
        w = ((F(4.0) * r2) * F(len(lights))) * ((ns * nl) / (dd * dd))
        out["c"] = [float(((F(weight[k])) * F(light.emission[li][k])) * w) for k in range(3)]
    out["shadow"] = True
    out["dv"] = [float(a) for a in dv]
    out["visible"] = fast_hit(scene, [float(a) for a in p], out["dv"], t_min)[0] == li      # the CLOSEST hit is the light itself: no epsilon
    return out


def bounce_direct(scene, queue, seed, npix, light, lights, sampler, no_direct=False, t_min=1e-4):
    """One bounce with direct lighting of every path of `queue`, the light sample at a Lambertian hit being `sampler`'s (sample_light, or a
    function of its arguments and result keys) -> (the new state per INPUT slot, the fate of each -- lights_ref.bounce_lit's, or
    "light_counted" for a DIRECT path on a light's front face --, the additions u64 [npix, 3], per slot the light sample or None).
    With an empty list or no_direct: the part that no sampler changes."""
    if not isinstance(scene, Scene):
        scene = Scene(scene)
    n = len(queue["pixel"])
    was_direct = (queue["event"] & np.uint32(DIRECT)) != 0
    masked = {f: np.array(queue[f], copy=True) for f in pr.FIELDS}
    masked["event"] &= np.uint32(DIRECT ^ 0xFFFFFFFF)                             # masked off before any Philox use
    hits = [fast_hit(scene, queue["origin"][k].tolist(), queue["dir"][k].tolist(), t_min) for k in range(n)]
    counted = []
    for k in range(n):
        idx, _, p, _, _ = hits[k]
        if was_direct[k] and idx >= 0 and light.emission is not None and idx < len(light.emission) and lr.is_light(light.emission[idx]) \
                and light_front(scene, idx, queue["dir"][k].tolist(), p):
            counted.append(k)
            masked["pixel"][k] = OUTSIDE                                          # the previous hit's shadow ray counted this face: adds nothing
    new, fates, adds = lr.bounce_lit(scene, masked, seed, npix, light, t_min)
    for k in counted:
        assert fates[k] == "light"
        fates[k] = "light_counted"
    samples = [None] * n
    if len(lights) > 0 and not no_direct:
        lib = oracle.load()
        for k in range(n):
            if fates[k] != "lambertian":
                continue
            idx, _, p, nrm, _ = hits[k]
            assert int(scene.flat[idx]["kind"]) == wr.LAMBERTIAN
            pixel = int(queue["pixel"][k])
            s = sampler(scene, seed, light, lights, pixel, int(queue["sample"][k]), int(masked["event"][k]), p, nrm, new["throughput"][k].tolist(), t_min)
            samples[k] = s
            new["event"][k] |= np.uint32(DIRECT)
            if s["visible"] and pixel < npix:
                for c in range(3):
                    adds[pixel, c] = np.uint64((int(adds[pixel, c]) + int(lib.oracle_b_quantize(float(s["c"][c])))) & MASK64)
    return new, fates, adds, samples


def step_direct(scene, queue, seed, npix, light, lights, sampler, no_direct=False, t_min=1e-4):
    """rt_paths_step_nee_device with the sampler of direct->flags -> (the out queue, the additions u64 [npix, 3], the live count of
    `queue`, the shadow rays traced)."""
    new, fates, adds, samples = bounce_direct(scene, queue, seed, npix, light, lights, sampler, no_direct, t_min)
    return pr.compact(new, fates, adds) + (sum(1 for s in samples if s is not None and s["shadow"]),)


def render_direct(flat, ocam, width, height, spp, light, sampler, *, max_depth=50, seed=1, t_min=1e-4, sample_begin=0, batch=1 << 20):
    """rt_render_wavefront_nee and _nee_sampled: paths_ref.frame with step_direct, the list from the table, the LAST step of each batch
    with NO_DIRECT -> (fix u64 [H, W, 3], rays traced, shadow rays traced)."""
    scene, npix, lights = Scene(flat), width * height, light_list(light.emission)
    fix, rays, shadow = pr.frame(lambda first, n: pr.begin(ocam, width, height, seed, spp, sample_begin, first, n),
                                 lambda q, last: step_direct(scene, q, seed, npix, light, lights, sampler, last, t_min), npix, npix * spp, max_depth, batch)
    return fix.reshape(height, width, 3), rays, shadow


def bounce_nee(scene, queue, seed, npix, light, lights, no_direct=False, t_min=1e-4):
    """bounce_direct with the area sample."""
    return bounce_direct(scene, queue, seed, npix, light, lights, sample_light, no_direct, t_min)


def step_nee(scene, queue, seed, npix, light, lights, no_direct=False, t_min=1e-4):
    """step_direct with the area sample (direct->flags = 0)."""
    return step_direct(scene, queue, seed, npix, light, lights, sample_light, no_direct, t_min)


def render_nee(flat, ocam, width, height, spp, light, **frame):
    """rt_render_wavefront_nee: render_direct (whose keywords `frame` holds) with the area sample."""
    return render_direct(flat, ocam, width, height, spp, light, sample_light, **frame)


# ---- the hand-built NEE queue of the GPU tests: hard by construction, checked by tests/test_nee_host.py -------------------------------------

SEED, HAND_N, HAND_NPIX = lr.SEED, lr.HAND_N, lr.HAND_NPIX
# three more spheres over lights_ref.hand_queue()'s fourteen: sphere -> (centre, radius, kind, albedo, param, emission)
EXTRA = [
    ((-6.0, 9.0, 0.0), 1.0, wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, (3.0, 2.0, 1.0)),       # 14: a light straight above the Lambertian sphere 0
    ((-6.0, 5.5, 0.0), 0.4, wr.METAL, (0.9, 0.9, 0.9), 0.0, (0.0, 0.0, 0.0)),            # 15: an occluder between the two, above every ray's origin
    ((-4.0, 9.0, 2.0), 0.5, wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, (3.0e7, 1.0, 0.5)),     # 16: a light whose sample passes the clamp in x
]
# the list the step is handed: a light that contributes at each end, every light of the table, two entries that name no sphere
LIGHTS = (14, 5, 99, 9, 6, -1, 8, 7, 11, 12, 16)
# slot -> what it was rebuilt to do (test_nee_host.py checks each with the statement); every slot below 63
CASES = {1: "first_of_list", 19: "last_of_list", 25: "blocked", 31: "far_side", 37: "below_horizon", 43: "later_block", 49: "out_of_range",
         55: "clamp", 61: "first_try"}
DIRECT_SLOTS = {6: "front", 7: "inside", 2: "metal", 3: "glass", 17: "lambertian"}         # these carry the DIRECT bit on entry
ALL_WAVE, LAST_LANE_WAVE = range(320, 384), range(384, 448)                               # every lane a shadow ray; only lane 63


def _matches(what, s):
    if what == "first_of_list":
        return s["j"] == 0 and s["visible"]
    if what == "last_of_list":
        return s["j"] == len(LIGHTS) - 1 and s["visible"] and max(s["c"]) <= 65536.0
    if what == "blocked":
        return s["li"] == 14 and s["shadow"] and not s["visible"]
    if what == "far_side":
        return s["li"] == 14 and s["ns"] is not None and s["ns"] > 0.0 and s["nl"] <= 0.0
    if what == "below_horizon":
        return s["ns"] is not None and s["ns"] <= 0.0
    if what == "later_block":
        return s["tries"] >= 3 and s["visible"]
    if what == "out_of_range":
        return s["li"] in (99, -1)
    if what == "clamp":
        return s["li"] == 16 and s["visible"] and s["c"][0] > 65536.0
    if what == "first_try":
        return s["tries"] == 1 and s["visible"]
    if what == "shadow":
        return s["shadow"]
    raise KeyError(what)


@functools.lru_cache(None)
def hand_queue():
    """(flat, queue, light, lights): lights_ref.hand_queue()'s scene with EXTRA above it (no path of the original comes near: its rays
    start at y = 5 and below, or leave upwards around x = 0), its 513 paths with the slots of CASES, DIRECT_SLOTS and two waves of the
    second workgroup rebuilt, and the list LIGHTS.  Every rebuilt Lambertian path is the original's ray onto sphere 0 with the sample
    searched -- with the statement alone -- so that its light sample is the named case.  Read-only."""
    import rtiow_amd as rt
    base_flat, base_q, base_light = lr.hand_queue()
    flat = np.zeros(len(base_flat) + len(EXTRA), dtype=rt.SPHERE_DTYPE)
    flat[:len(base_flat)] = base_flat
    for k, (centre, radius, kind, albedo, param, _) in enumerate(EXTRA, start=len(base_flat)):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = centre, radius, albedo, param, kind
    emission = np.concatenate([base_light.emission, np.array([e for *_, e in EXTRA], dtype=np.float64)])
    light = lr.Light(base_light.sky_bottom, base_light.sky_top, emission)
    scene = Scene(flat)
    q = {f: np.array(base_q[f], copy=True) for f in pr.FIELDS}
    rng = np.random.default_rng(29)
    jit = lambda: rng.uniform(-0.2, 0.2)

    def lambertian(k, what):
        """Slot k: a ray down onto sphere 0 whose light sample is `what`, by search over samples."""
        q["origin"][k], q["dir"][k] = (-6.0 + jit(), 5.0, jit()), (0.1 * jit(), -1.0, 0.1 * jit())
        q["pixel"][k] = k % HAND_NPIX
        probe = {f: q[f][[k]].copy() for f in pr.FIELDS}
        for sample in range(4000):
            probe["sample"][0] = sample
            _, fates, _, samples = bounce_nee(scene, probe, SEED, HAND_NPIX, light, LIGHTS)
            assert fates[0] == "lambertian"
            if _matches(what, samples[0]):
                q["sample"][k] = sample
                return
        raise AssertionError(f"no sample below 4000 makes slot {k} the case {what}")

    for k, what in CASES.items():
        lambertian(k, what)
    for k in ALL_WAVE:
        lambertian(k, "shadow")
    lambertian(LAST_LANE_WAVE[-1], "shadow")
    for k in DIRECT_SLOTS:
        q["event"][k] |= np.uint32(DIRECT)
    for a in list(q.values()) + [emission]:
        a.setflags(write=False)
    return flat, q, light, LIGHTS


@functools.lru_cache(None)
def hand_step(count, no_direct=False, with_lights=True):
    """The statement's answer for the first `count` paths of hand_queue() (computed once per setting, read-only)."""
    flat, q, light, lights = hand_queue()
    out, adds, live, shadow = step_nee(flat, pr.prefix(q, count), SEED, HAND_NPIX, light, lights if with_lights else (), no_direct)
    for a in list(out.values()) + [adds]:
        a.setflags(write=False)
    return out, adds, live, shadow


# ---- the NEE book frame ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def book_frame(max_depth, batch=257):
    """The statement's NEE frame of lights_ref.book_case() at `max_depth` -> (fix, rays, shadow rays), read-only."""
    flat, light, _ = lr.book_case()
    fix, rays, shadow = render_nee(flat, oracle.book1_camera(lr.BW, lr.BH), lr.BW, lr.BH, lr.BSPP, light, max_depth=max_depth, seed=1, batch=batch)
    fix.setflags(write=False)
    return fix, rays, shadow


# ---- the small scene of the expectation and variance tests ---------------------------------------------------------------------------------

STAT_W, STAT_H, STAT_SPP, STAT_DEPTH = 16, 12, 64, 8
STAT_SEEDS = tuple(range(101, 117))
STAT_LIGHT = 1
STAT_EMISSION = (40.0, 32.0, 24.0)


def stat_scene():
    """(flat, light): a Lambertian ground, one small light above it, a Metal, a Dialectric and a Lambertian occluder between the light
    and the ground; a black sky, so that all a frame shows comes from the light.  The light hangs above the camera's field of view (26
    degrees above its axis, the field's half height is 20): pixels that see a light directly have the same variance under both estimators
    and would only mask the difference the variance test is about."""
    import rtiow_amd as rt
    spheres = [((0.0, -1000.0, 0.0), 1000.0, wr.LAMBERTIAN, (0.6, 0.6, 0.6), 0.0),
               ((0.0, 3.5, 0.0), 0.25, wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0),
               ((-1.5, 0.5, 0.0), 0.5, wr.METAL, (0.8, 0.8, 0.8), 0.0),
               ((1.5, 0.5, 0.0), 0.5, wr.DIALECTRIC, (1.0, 1.0, 1.0), 1.5),
               ((0.3, 1.4, 0.2), 0.35, wr.LAMBERTIAN, (0.7, 0.3, 0.3), 0.0)]
    flat = np.zeros(len(spheres), dtype=rt.SPHERE_DTYPE)
    for k, (centre, radius, kind, albedo, param) in enumerate(spheres):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = centre, radius, albedo, param, kind
    emission = np.zeros((len(spheres), 3))
    emission[STAT_LIGHT] = STAT_EMISSION
    return flat, lr.Light((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), emission)


def stat_camera():
    from rtiow_amd.scene import Camera
    return Camera((0.0, 2.0, 6.0), (0.0, 0.7, 0.0), (0.0, 1.0, 0.0), 40.0, STAT_W / STAT_H, 0.0, 6.0)


def stat_sample_bound():
    """The largest value a sample of the stat scene can add in one channel, by the statement's formula: a light hit adds throughput * e
    <= e (no albedo exceeds 1); a light sample adds weight * e * w with weight <= 1 and w = 4 r^2 n_lights (ns nl) / dd^2 <= 4 r^2 / gap^2,
    because ns <= |dv| and nl <= |dv| (n and u are unit vectors) and dd = |dv|^2 >= gap^2, the squared distance between the light's surface
    and the nearest surface of a Lambertian sphere that is no light."""
    flat, light = stat_scene()
    c, r = np.array(flat[STAT_LIGHT]["center"]), float(flat[STAT_LIGHT]["radius"])
    gaps = [float(np.linalg.norm(np.array(s["center"]) - c)) - float(s["radius"]) - r for k, s in enumerate(flat)
            if k != STAT_LIGHT and int(s["kind"]) == wr.LAMBERTIAN]
    assert min(gaps) > 0.0
    return max(STAT_EMISSION) * max(1.0, 4.0 * r * r / min(gaps) ** 2)


def stat_numbers(frames_nee, frames_lit):
    """From the 16 NEE and the 16 lit frames (u64 [H, W, 3], one per seed of STAT_SEEDS) -> (the mean of the per-seed differences of
    the frame-total energy, its standard error, the per-pixel variance over the seeds summed over the frame for NEE and for lit)."""
    nee = np.array([f.astype(np.float64) for f in frames_nee]) / 4294967296.0
    lit = np.array([f.astype(np.float64) for f in frames_lit]) / 4294967296.0
    diff = nee.sum(axis=(1, 2, 3)) - lit.sum(axis=(1, 2, 3))
    stderr = float(diff.std(ddof=1) / math.sqrt(len(diff)))
    return float(diff.mean()), stderr, float(nee.var(axis=0, ddof=1).sum()), float(lit.var(axis=0, ddof=1).sum())
