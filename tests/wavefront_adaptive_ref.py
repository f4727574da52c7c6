"""CPU statement of the wavefront frames over pixel lists and of the adaptive loop over them (include/rtiow_hip.h "wavefront frames over
pixel lists") -- a test helper.

Composed from tests/paths_ref.py (begin: which item a slot holds; step), tests/lights_ref.py (step_lit), tests/nee_ref.py, tests/cone_ref.py
and tests/weighted_ref.py (the three NEE steps) and the selection rule of tests/test_pixel_select_host.py (select_model), and restating none
of them: here is only the list -- which (pixel, sample) an item of a list is --, that the sums are frame-addressed, and the loop of
rt_render_adaptive over such passes.  A pass over a list is the dense statement pass with that sample_begin masked to the list: the
steps act on each path alone, so the paths of the listed pixels are all it takes.
"""
import numpy as np

import cone_ref as cr
import lights_ref as lr
import nee_ref as nr
import paths_ref as pr
import weighted_ref as wt
import wavefront_ref as wr
from trace_ref import Scene, canonical

AREA, CONE, WEIGHTED = 0, cr.CONE, wt.FLAGS              # rt_direct.flags: 0, 2, 10


def begin_pixels(ocam, width, height, seed, spp, sample_begin, first_item, n, pixels):
    """rt_paths_begin_pixels_device: slot k holds item first_item + k, list-major; the camera ray is the FULL frame's for that pixel."""
    q = pr.empty(n)
    for k in range(n):
        item = first_item + k
        pixel, sample = int(pixels[item // spp]), sample_begin + item % spp
        o, d, event, _ = wr.camera_path(ocam, width, height, seed, pixel, sample)
        q["pixel"][k], q["sample"][k], q["event"][k], q["origin"][k], q["dir"][k], q["throughput"][k] = pixel, sample, event, o, d, (1.0, 1.0, 1.0)
    q["origin"], q["dir"] = canonical(q["origin"]), canonical(q["dir"])
    return q


SAMPLERS = {AREA: nr.sample_light, CONE: cr.sample_light_cone, WEIGHTED: wt.sample_light_weighted}


def _step(scene, q, seed, npix, light, lights, flags, no_direct, t_min):
    """One step of the frame's kind -> (the out queue, the additions, the live count[, the shadow rays traced])."""
    if light is None:
        return pr.step(scene, q, seed, npix, t_min)
    if lights is None:
        return lr.step_lit(scene, q, seed, npix, light, t_min)
    return nr.step_direct(scene, q, seed, npix, light, lights, SAMPLERS[flags], no_direct, t_min)


def render_pixels(flat, ocam, width, height, spp, pixels=None, light=None, direct=False, flags=AREA, *, max_depth=50, seed=1, t_min=1e-4,
                  sample_begin=0, batch=1 << 20):
    """rt_render_wavefront_pixels without RT_FLAG_ACCUMULATE (with it: add the result to what was there) -> (fix u64 [H, W, 3]
    frame-addressed, rays traced, shadow rays traced).  light None: the unlit frame; direct: the lights of the table are sampled, flags how."""
    scene = flat if isinstance(flat, Scene) else Scene(flat)
    npix = width * height
    pixels = np.arange(npix, dtype=np.uint32) if pixels is None else np.asarray(pixels, dtype=np.uint32).reshape(-1)
    lights = nr.light_list(light.emission) if direct else None
    fix, rays, shadow = pr.frame(lambda first, n: begin_pixels(ocam, width, height, seed, spp, sample_begin, first, n, pixels),
                                 lambda q, last: _step(scene, q, seed, npix, light, lights, flags, last, t_min), npix, len(pixels) * spp, max_depth, batch)
    return fix.reshape(height, width, 3), rays, shadow


def render_adaptive(flat, ocam, width, height, cap, step, threshold, dark_floor, light=None, direct=False, flags=AREA, *, max_depth=50, seed=1,
                    t_min=1e-4, batch=1 << 20):
    """rt_render_wavefront_adaptive -> (fix, half, count, rays traced, shadow rays traced).  rt_render_adaptive's loop: round 1 every pixel,
    then select, render passes n / step (even: also into half) and n / step + 1 of the list, until it is empty or the cap is reached."""
    from test_pixel_select_host import select_model
    scene = Scene(flat)
    kw = dict(light=light, direct=direct, flags=flags, max_depth=max_depth, seed=seed, t_min=t_min, batch=batch)
    fix = np.zeros((height, width, 3), dtype=np.uint64)
    half = np.zeros((height, width, 3), dtype=np.uint64)
    count = np.zeros((height, width), dtype=np.uint32)
    rays = shadow = 0
    pixels, n = None, 0
    while True:
        for k in range(2):
            f, r, s = render_pixels(scene, ocam, width, height, step, pixels, sample_begin=n + k * step, **kw)
            fix += f
            if k == 0:
                half += f
            rays, shadow = rays + r, shadow + s
        if pixels is None:
            count += np.uint32(2 * step)
        else:
            count.reshape(-1)[pixels] += np.uint32(2 * step)
        n += 2 * step
        if n >= cap:
            break
        pixels = select_model(fix, half, count, n, threshold, dark_floor)
        if len(pixels) == 0:
            break
    return fix, half, count, rays, shadow


# ---- the adaptive NEE case of the GPU tests: the stat scene of nee_ref; hard by the statement alone (tests/test_wavefront_adaptive_host.py) ----

STAT = dict(width=nr.STAT_W, height=nr.STAT_H, max_depth=nr.STAT_DEPTH, seed=101, step=4, cap=32, threshold=0.2, dark_floor=0.01, batch=257)
_cache = {}


def stat_adaptive(flags=AREA, threshold=None):
    """The statement's adaptive frame of the stat scene with direct lighting (computed once per setting, read-only)."""
    import oracle
    threshold = STAT["threshold"] if threshold is None else threshold
    key = (flags, threshold)
    if key not in _cache:
        flat, light = nr.stat_scene()
        ocam = oracle.camera_from_host(nr.stat_camera())
        out = render_adaptive(flat, ocam, STAT["width"], STAT["height"], STAT["cap"], STAT["step"], threshold, STAT["dark_floor"], light, True, flags,
                              max_depth=STAT["max_depth"], seed=STAT["seed"], batch=STAT["batch"])
        for a in out[:3]:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]
