"""The ray-query kernel (rt_trace.hip) on the scenes and from the viewpoints of test_gpu_viewpoints.py: 6 layouts x
18 cameras, each case 192 rays = three waves --
  wave 0  the camera rays of 64 pixels strided over a 20 x 18 frame: one origin, spread directions;
  wave 1  rays from wave 0's reference hit points (t_min rejects the self-hit; a parent that missed starts at its point at t = 10) in
          seeded directions: what a wavefront integrator holds after one bounce, 64 rays going 64 ways;
  wave 2  origins uniform in the scene's bounding box, seeded directions, t_max cycling through its classes, four lanes degenerate --
closest hit and occlusion under both candidate schemes against tests/trace_ref.py, bit for bit: one upload and four launches a case.
tests/test_trace_host.py (no GPU) shows with the reference alone that the cases are hard."""
import functools
import math

import numpy as np
import pytest

import features_ref as fr
import trace_ref as tr
from test_gpu_features_viewpoints import case_seed
from test_gpu_viewpoints import CAMERAS, SCENES, flat_scene, layout, rt_cam

W, H = 20, 18
N_WAVE = 64

# Cases whose reference shows no hit, or no miss (at most 2 may be listed): none -- wave 2's rays with t_max <= 0 miss in every case and
# some of its downward rays hit the ground
ONE_SIDED = set()


@functools.lru_cache(None)
def scene_of(which):
    return tr.Scene(flat_scene(which))


def bounding_box(flat):
    """Of the spheres that are not a ground (|radius| < 100)."""
    small = np.abs(flat["radius"]) < 100.0
    c, r = flat["center"][small], np.abs(flat["radius"][small])
    return (c - r[:, None]).min(0), (c + r[:, None]).max(0)


@functools.lru_cache(None)
def case(scene, camera):
    """-> (origins [192,3], dirs [192,3], t_max [192], classes [192] -- the t_max class of every ray of wave 2, "" elsewhere --, the
    reference's answer), computed once and left unchanged (it depends on the spheres, not on the grid's layout)."""
    sc = scene_of(SCENES[scene][0])
    seed = case_seed(scene, camera)
    rng = np.random.default_rng(seed)
    ocam = fr.camera_from_rt(rt_cam(CAMERAS[camera](W, H)))
    # wave 0
    o0, d0 = np.zeros((N_WAVE, 3)), np.zeros((N_WAVE, 3))
    for k in range(N_WAVE):
        g = (k * W * H) // N_WAVE
        o, d = fr.camera_ray(ocam, W, H, seed, g % W, g // W, 0)
        o0[k], d0[k] = o[:], d[:]
    ref0 = tr.trace(sc, o0, d0)
    # wave 1
    o1 = np.where((ref0["index"] >= 0)[:, None], ref0["point"], o0 + d0 * 10.0)
    d1 = tr.unit_directions(rng, N_WAVE)
    # wave 2
    lo, hi = bounding_box(sc.flat)
    o2 = rng.uniform(lo, hi, (N_WAVE, 3))
    d2 = tr.unit_directions(rng, N_WAVE) * rng.choice([1.0, 1e-3, 1e3], N_WAVE)[:, None]      # (the reference never normalises)
    og, dg = tr.degenerate_rays()
    for lane in range(4):                                                       # four of the six kinds, rotating with the case
        kind = (seed + lane) % len(og)
        d2[60 + lane] = dg[kind]
        if kind == 4:                                                           # (the origin at 1e16; the others keep theirs in the box)
            o2[60 + lane] = og[kind]
    unclipped = tr.trace(sc, o2, d2)["t"]
    classes = [""] * (2 * N_WAVE) + [tr.T_MAX_CLASSES[k % len(tr.T_MAX_CLASSES)] for k in range(N_WAVE)]
    t2 = np.array([tr.t_max_of(classes[2 * N_WAVE + k], float(unclipped[k]), rng) for k in range(N_WAVE)])
    origins, dirs = np.concatenate([o0, o1, o2]), np.concatenate([d0, d1, d2])
    t_max = np.concatenate([np.full(2 * N_WAVE, math.inf), t2])
    want = tr.trace(sc, origins, dirs, t_max)
    for a in (origins, dirs, t_max):
        a.setflags(write=False)
    return origins, dirs, t_max, classes, want


@pytest.mark.gpu
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_trace_viewpoint_matches_reference(renderer, oracle_mod, monkeypatch, scene, camera):
    flat, _, _, _, _ = layout(monkeypatch, scene)
    origins, dirs, t_max, _, want = case(scene, camera)
    renderer.upload_scene(flat)                                         # RTIOW_GRID_DIM is read here
    for scheme in ("wave", "ray"):
        monkeypatch.setenv("RTIOW_TRACE_CANDIDATES", scheme)
        got = renderer.trace_rays(origins, dirs, t_max)
        tr.same(got, want)
        occ = renderer.occluded(origins, dirs, t_max)["occluded"]
        assert occ.dtype == np.uint8 and np.array_equal(occ, (want["index"] >= 0).astype(np.uint8)), (scheme, "occluded")
