"""CPU statement of the lit path queue (include/rtiow_hip.h "lighting") -- a test helper.

Composed from tests/paths_ref.py (begin, bounce: what a path that scatters does, and the queue), tests/trace_ref.py (fast_hit: the closest
hit) and tests/wavefront_ref.py (the operation order of the sky term) and restating none of them: here is only what lighting adds -- the sky
between two colours, which sphere is a light, what a path that reaches one adds, and that it ends there.  A Light is (sky_bottom, sky_top,
emission): two colours and a float64 array [n_spheres, 3] or None.
"""
import collections
import functools
import os

import numpy as np

import oracle
import paths_ref as pr
import wavefront_ref as wr
from trace_ref import Scene, fast_hit

Light = collections.namedtuple("Light", "sky_bottom sky_top emission")
REFERENCE_SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
REFERENCE = Light(*REFERENCE_SKY, None)
MASK64 = (1 << 64) - 1
SURVIVES = pr.SURVIVES


def is_light(e):
    """A sphere whose entry is e: a NaN or a non-positive channel compares false."""
    return bool(e[0] > 0.0 or e[1] > 0.0 or e[2] > 0.0)


def sky_term(weight, d, bottom, top):
    """weight * sky(d) per channel: wavefront_ref.sky_sample's operations in its order, the two constants replaced by bottom and top."""
    with np.errstate(all="ignore"):
        w, d = [np.float64(x) for x in weight], [np.float64(x) for x in d]
        inv = np.float64(1.0) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        t = np.float64(0.5) * (d[1] * inv + np.float64(1.0))
        sky = [np.float64(bottom[c]) * (np.float64(1.0) - t) + np.float64(top[c]) * t for c in range(3)]
        return [w[c] * sky[c] for c in range(3)]


def _add(adds, pixel, v):
    lib = oracle.load()
    for c in range(3):
        adds[pixel, c] = np.uint64((int(adds[pixel, c]) + int(lib.oracle_b_quantize(float(v[c])))) & MASK64)


def bounce_lit(scene, queue, seed, npix, light, t_min=1e-4):
    """One lit bounce of every path of `queue` -> (the new state per INPUT slot, the fate of each -- paths_ref.FATES or "light" --, the
    additions u64 [npix, 3]).  A path that neither misses nor reaches a light is paths_ref.bounce's."""
    if not isinstance(scene, Scene):
        scene = Scene(scene)
    n = len(queue["pixel"])
    fates = [None] * n
    adds = np.zeros((npix, 3), dtype=np.uint64)
    rest = []
    for k in range(n):
        o, d, thr = queue["origin"][k].tolist(), queue["dir"][k].tolist(), queue["throughput"][k].tolist()
        pixel = int(queue["pixel"][k])
        idx = fast_hit(scene, o, d, t_min)[0]
        if idx < 0:
            if pixel < npix:
                _add(adds, pixel, sky_term(thr, d, light.sky_bottom, light.sky_top))
            fates[k] = "miss"
        elif light.emission is not None and idx < len(light.emission) and is_light(light.emission[idx]):
            if pixel < npix:
                with np.errstate(all="ignore"):
                    _add(adds, pixel, [np.float64(thr[c]) * np.float64(light.emission[idx][c]) for c in range(3)])     # one multiply per channel
            fates[k] = "light"
        else:
            rest.append(k)
    new = pr.empty(n)
    if rest:
        sub, sub_fates, sub_adds = pr.bounce(scene, {f: queue[f][rest] for f in pr.FIELDS}, seed, npix, t_min)
        assert not sub_adds.any() and "miss" not in sub_fates
        for f in pr.FIELDS:
            new[f][rest] = sub[f]
        for k, fate in zip(rest, sub_fates):
            fates[k] = fate
    return new, fates, adds


def step_lit(scene, queue, seed, npix, light, t_min=1e-4):
    """rt_paths_step_lit_device -> (the out queue, the additions u64 [npix, 3], the live count of `queue`)."""
    return pr.compact(*bounce_lit(scene, queue, seed, npix, light, t_min))


def render_lit(flat, ocam, width, height, spp, light, *, max_depth=50, seed=1, t_min=1e-4, sample_begin=0, batch=1 << 20):
    """rt_render_wavefront_lit: paths_ref.frame with the lit step -> (fix u64 [H, W, 3], rays traced)."""
    scene, npix = Scene(flat), width * height
    fix, rays, _ = pr.frame(lambda first, n: pr.begin(ocam, width, height, seed, spp, sample_begin, first, n),
                            lambda q, last: step_lit(scene, q, seed, npix, light, t_min), npix, npix * spp, max_depth, batch)
    return fix.reshape(height, width, 3), rays


# ---- the hand-built lit queue of the GPU tests: hard by construction, checked by tests/test_lights_host.py ---------------------------------

SEED, HAND_N, HAND_NPIX = pr.SEED, pr.HAND_N, pr.HAND_NPIX
NAN = float("nan")
BIG = (4.0, 3.2, 2.4)
# sphere -> (centre, kind, albedo, param, emission); 0 .. 4 are wavefront_ref.step_scene()'s, with an entry each that lights nothing
EXTRA = [
    ((-6.0, 1.0, 10.0), wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, BIG),                    # 5: a plain light
    ((-3.0, 1.0, 10.0), wr.DIALECTRIC, (1.0, 1.0, 1.0), 1.5, (0.25, 0.5, 2.0)),       # 6: a light of glass
    ((6.0, 1.0, 10.0), wr.METAL, (0.4, 0.5, 0.6), 1.0, (1.0, 1.0, 1.0)),              # 7: a light of fuzzy Metal, hit where it would absorb
    ((0.0, 1.0, 10.0), wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, (-2.0, 0.75, NAN)),       # 8: one negative, one positive, one NaN channel
    ((3.0, 1.0, 10.0), wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, (2.0e6, 1.0, 0.5)),       # 9: throughput * e above the clamp in x
    ((0.0, 1.0, 20.0), wr.LAMBERTIAN, (0.6, 0.6, 0.6), 0.0, (0.0, 0.0, 0.0)),         # 10: no light ...
    ((0.0, 1.0, 20.0), wr.LAMBERTIAN, (0.6, 0.6, 0.6), 0.0, (1.0, 2.0, 3.0)),         # 11: ... and the light in the same place, later: it wins
    ((6.0, 1.0, 20.0), wr.LAMBERTIAN, (0.6, 0.6, 0.6), 0.0, (1.0, 2.0, 3.0)),         # 12: a light ...
    ((6.0, 1.0, 20.0), wr.METAL, (0.9, 0.9, 0.2), 0.0, (0.0, 0.0, 0.0)),              # 13: ... and a mirror in the same place, later: it wins
]
BASE_EMISSION = [(-1.0, 0.0, -0.0), (0.0, 0.0, 0.0), (NAN, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, -3.0, NAN)]
HAND_SKY = ((0.3, 0.2, 0.1), (0.05, 0.1, 0.6))
# slot -> what it was rebuilt to do (test_lights_host.py checks each with the statement); slots 128 .. 191 all end on lights
SLOTS = {6: "front", 7: "inside", 8: "outside_frame", 9: "glass_light", 10: "metal_light", 11: "negative", 12: "clamp", 13: "tie_light",
         14: "tie_mirror", 63: "front"}


@functools.lru_cache(None)
def hand_queue():
    """(flat, queue, light): paths_ref.hand_queue()'s scene with nine more spheres behind it (z = 10 and 20: no path of the original
    comes near them), its 513 paths with the slots of SLOTS and the wave 128 .. 191 rebuilt, and an emission table.  Read-only."""
    import rtiow_amd as rt
    base_flat, base_q, _ = pr.hand_queue()
    flat = np.zeros(len(base_flat) + len(EXTRA), dtype=rt.SPHERE_DTYPE)
    flat[:len(base_flat)] = base_flat
    for k, (centre, kind, albedo, param, _) in enumerate(EXTRA, start=len(base_flat)):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = centre, 1.0, albedo, param, kind
    emission = np.array(BASE_EMISSION + [e for *_, e in EXTRA], dtype=np.float64)
    light = Light(*HAND_SKY, emission)
    q = {f: np.array(base_q[f], copy=True) for f in pr.FIELDS}
    rng = np.random.default_rng(23)
    jit = lambda: rng.uniform(-0.2, 0.2)
    down = lambda x, z: ((x + jit(), 5.0, z + jit()), (0.1 * jit(), -1.0, 0.1 * jit()))
    build = {
        "front": lambda: down(-6.0, 10.0),
        "inside": lambda: ((-3.0 + jit(), 1.0, 10.0 + jit()), (jit(), 1.0, jit())),     # from inside the glass light: its back face
        "outside_frame": lambda: down(-6.0, 10.0),
        "glass_light": lambda: down(-3.0, 10.0),
        "metal_light": lambda: ((4.5, 1.0 + 0.995, 10.0), (1.0, 0.0, 0.0)),              # paths_ref's grazing ray, at the Metal light
        "negative": lambda: down(0.0, 10.0),
        "clamp": lambda: down(3.0, 10.0),
        "tie_light": lambda: down(0.0, 20.0),
        "tie_mirror": lambda: down(6.0, 20.0),
    }
    for k, what in SLOTS.items():
        q["origin"][k], q["dir"][k] = build[what]()
    q["pixel"][8] = HAND_NPIX + 3
    q["pixel"][6], q["pixel"][63] = 17, 18                                               # (inside the frame whatever the draw was)
    for k in range(128, 192):
        q["origin"][k], q["dir"][k] = build[("front", "glass_light", "negative", "clamp", "tie_light")[k % 5]]()
    # the Metal light is hit where the unlit step absorbs: the pixel is searched with paths_ref alone
    scene = Scene(flat)
    probe = {f: q[f][[10]].copy() for f in pr.FIELDS}
    for pixel in range(1, 4000):
        probe["pixel"][0] = pixel % HAND_NPIX
        probe["sample"][0] = pixel // HAND_NPIX
        if pr.bounce(scene, probe, SEED, HAND_NPIX)[1][0] == "absorbed":
            q["pixel"][10], q["sample"][10] = probe["pixel"][0], probe["sample"][0]
            break
    else:
        raise AssertionError("no (pixel, sample) makes the grazing ray at the Metal light absorb")
    for a in list(q.values()) + [emission]:
        a.setflags(write=False)
    return flat, q, light


@functools.lru_cache(None)
def hand_step(count):
    """The statement's answer for the first `count` paths of hand_queue() (computed once per count, read-only)."""
    flat, q, light = hand_queue()
    out, adds, live = step_lit(flat, pr.prefix(q, count), SEED, HAND_NPIX, light)
    for a in list(out.values()) + [adds]:
        a.setflags(write=False)
    return out, adds, live


def dark_tables(n):
    """Emission settings that light nothing: none, all zero, only negative / NaN / -0 entries."""
    bad = np.zeros((n, 3))
    bad[::2] = (-1.0, NAN, -0.0)
    bad[1::3] = (NAN, NAN, NAN)
    bad[2::5, 1] = -np.inf
    return {"none": None, "zeros": np.zeros((n, 3)), "negative_nan": bad}


# ---- the lit book frame --------------------------------------------------------------------------------------------------------------------

BW, BH, BSPP = 32, 18, 4
DIM_SKY = ((0.02, 0.02, 0.05), (0.02, 0.02, 0.05))
SMALL_LIGHTS = ((8.0, 2.0, 1.0), (1.0, 6.0, 2.0), (1.0, 2.0, 9.0), (5.0, 5.0, 0.5), (0.5, 3.0, 3.0))


@functools.lru_cache(None)
def book_case():
    """(flat, light, first: the first-hit sphere of each of the frame's 32 x 18 x 4 camera rays, pixel-major).  The lights: the large
    Lambertian sphere and the five small spheres that most camera rays see first (ties: the lower index), chosen with the statement."""
    import rtiow_amd as rt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    flat = np.ascontiguousarray(np.load(os.path.join(root, "tests", "golden", "book1_scene_seed1.npy"), allow_pickle=False).astype(rt.SPHERE_DTYPE))
    scene = Scene(flat)
    q = pr.begin(oracle.book1_camera(BW, BH), BW, BH, 1, BSPP, 0, 0, BW * BH * BSPP)
    first = np.array([fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), 1e-4)[0] for k in range(len(q["pixel"]))])
    big = [k for k in range(len(flat)) if int(flat[k]["kind"]) == wr.LAMBERTIAN and float(flat[k]["radius"]) == 1.0]
    assert len(big) == 1
    small = [k for k in range(len(flat)) if float(flat[k]["radius"]) < 0.5]
    seen = sorted(small, key=lambda k: (-int((first == k).sum()), k))[:len(SMALL_LIGHTS)]
    emission = np.zeros((len(flat), 3))
    emission[big[0]] = BIG
    for k, e in zip(seen, SMALL_LIGHTS):
        emission[k] = e
    emission.setflags(write=False)
    first.setflags(write=False)
    return flat, Light(*DIM_SKY, emission), first


@functools.lru_cache(None)
def book_frame(max_depth, lit=True, batch=257):
    """The statement's lit book frame at `max_depth` (lit=False: the same dim sky without the lights) -> (fix, rays), read-only."""
    flat, light, _ = book_case()
    if not lit:
        light = light._replace(emission=None)
    fix, rays = render_lit(flat, oracle.book1_camera(BW, BH), BW, BH, BSPP, light, max_depth=max_depth, seed=1, batch=batch)
    fix.setflags(write=False)
    return fix, rays
