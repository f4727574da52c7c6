"""The capped unit-sphere redraw on the device (rt_dense.hip): every render against Oracle B bit for bit on the sums, with
rays_traced and samples equal; the same launch again with RTIOW_DENSE_BODY=classic gives the identical frame; rt_last_dense_body says
which body ran while kernel_variant stays what the classic kernels report.

* the book scene and a large-grid scene at the smallest launch shapes that reach each of the four instantiations (small / large grid x
  blocks of 256 / 1 024), with the small work blocks (5 spp), the direct adds (3 spp) and a second pass (sample_begin + RT_FLAG_ACCUMULATE);
* a scene built to park: the camera inside one large Lambertian sphere of albedo near 1 (every ray hits, every path runs to max_depth), with a
  Metal sphere of fuzz 1 and a glass sphere in view -- about half a million scatters, ~5 % of which park, some two and three times in a row;
  a park that consumed depth, throughput or a ray count shows here, and glass lanes pass through passes in which their neighbours park;
* the same scene at max_depth 1, 2 and 3: a lane that parks on its last allowed bounce ends where the oracle's path ends."""
import os

import numpy as np
import pytest
import torch

import rtiow_amd as rt

pytestmark = pytest.mark.gpu


def _env(**kw):
    """Sets the given environment knobs (None: unset); returns what to restore."""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    return old


def _both_bodies(renderer, oracle_mod, flat, cam, w, h, spp, *, large=False, variant=None, **pkw):
    """One launch per body; both against Oracle B.  Returns the capped launch's stats."""
    renderer.upload_scene(flat)
    okw = {k: v for k, v in pkw.items() if k in ("sample_begin", "max_depth", "seed")}
    want_fix, want_sum, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), flat, oracle_mod.make_params(w, h, spp, nthreads=8, **okw))
    old = _env(RTIOW_LARGE_BLOCK_MIN_ITEMS=0 if large else None, RTIOW_DENSE_BODY="capped")
    try:
        sums, fix, st = renderer.render(cam, rt.make_params(w, h, spp, **pkw))
        body = renderer._lib.rt_last_dense_body(renderer._h)
        os.environ["RTIOW_DENSE_BODY"] = "classic"
        sums_c, fix_c, st_c = renderer.render(cam, rt.make_params(w, h, spp, **pkw))
        body_c = renderer._lib.rt_last_dense_body(renderer._h)
    finally:
        _env(**old)
    shipped = st["scan_mode"] == 5                              # (a context created under RTIOW_SCAN_MODE=1 has no capped body: classic both times)
    assert body == (1 if shipped else 0) and body_c == 0
    assert np.array_equal(fix, want_fix) and np.array_equal(sums, want_sum)
    assert st["rays_traced"] == ost["rays_traced"] and st["samples"] == w * h * spp
    assert np.array_equal(fix_c, fix) and np.array_equal(sums_c, sums)
    assert st_c["rays_traced"] == st["rays_traced"] and st_c["samples"] == st["samples"]
    assert st_c["kernel_variant"] == st["kernel_variant"] and st_c["direct_samples"] == st["direct_samples"]
    if variant is not None and shipped:
        assert st["kernel_variant"] == variant, st["kernel_variant"]
    return st


@pytest.mark.parametrize("w,h,spp,large,variant", [
    (24, 14, 72, True, 5),       # small grid, blocks of 1 024 (>= 69 spp): the headline's instantiation
    (32, 18, 20, False, 1),      # small grid, blocks of 256
    (32, 18, 5, False, 1),       # ... work blocks of 64
    (32, 18, 3, False, 1),       # ... every sample added to the frame buffer on its own
])
def test_book_scene_reaches_the_small_grid_kernels(renderer, oracle_mod, book1_flat, w, h, spp, large, variant):
    st = _both_bodies(renderer, oracle_mod, book1_flat, rt.book1_camera(w, h), w, h, spp, large=large, variant=variant)
    assert (st["direct_samples"] == st["samples"]) == (spp == 3)


@pytest.fixture(scope="module")
def large_grid_flat():
    return rt.random_scene(3, grid=(-27, 27)).flatten()


@pytest.mark.parametrize("spp,large,variant", [(147, True, 4), (20, False, 0)])
def test_large_grid_scene_reaches_the_large_grid_kernels(renderer, oracle_mod, large_grid_flat, spp, large, variant):
    _both_bodies(renderer, oracle_mod, large_grid_flat, rt.book1_camera(20, 12), 20, 12, spp, large=large, variant=variant)


def test_a_second_pass_accumulates_on_the_capped_body(renderer, oracle_mod, book1_flat):
    """72 + 72 samples per pixel in two launches on blocks of 1 024 (sample_begin, RT_FLAG_ACCUMULATE) = one Oracle-B render of 144."""
    w, h, spp = 24, 14, 72
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(w, h)
    d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    old = _env(RTIOW_LARGE_BLOCK_MIN_ITEMS=0, RTIOW_DENSE_BODY="capped")
    try:
        for k in range(2):
            renderer.render_device(cam, rt.make_params(w, h, spp, sample_begin=k * spp, flags=rt.RT_FLAG_ACCUMULATE), d_fix.data_ptr())
            assert renderer._lib.rt_last_dense_body(renderer._h) == (1 if renderer.last_stats()["scan_mode"] == 5 else 0)
        torch.cuda.synchronize()
        st = renderer.last_stats()
    finally:
        _env(**old)
    want, _, _ = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(w, h, 2 * spp, nthreads=8))
    _, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(w, h, spp, sample_begin=spp, nthreads=8))
    assert np.array_equal(d_fix.cpu().numpy().view(np.uint64), want)
    assert st["rays_traced"] == ost["rays_traced"] and st["samples"] == w * h * spp
    if st["scan_mode"] == 5:
        assert st["kernel_variant"] == 5


def test_without_the_knob_only_the_measured_winner_runs_capped(renderer, book1_flat, large_grid_flat):
    """RTIOW_DENSE_BODY unset: the small-grid kernel on blocks of 1 024 takes the capped body (profiles/capped_redraw_ab.txt), every other
    dense launch the classic one; RT_FLAG_UNIFORM53, RT_FLAG_DIAG_STATS and RT_FLAG_NO_FILTER have no capped body whatever the knob says."""
    old = _env(RTIOW_LARGE_BLOCK_MIN_ITEMS=0, RTIOW_DENSE_BODY=None)
    try:
        body = lambda: renderer._lib.rt_last_dense_body(renderer._h)
        renderer.upload_scene(book1_flat)
        _, _, st = renderer.render(rt.book1_camera(24, 14), rt.make_params(24, 14, 72), want_fix=False)
        shipped = st["scan_mode"] == 5
        assert body() == (1 if shipped else 0) and (st["kernel_variant"] == 5 or not shipped)
        _, _, st = renderer.render(rt.book1_camera(32, 18), rt.make_params(32, 18, 20), want_fix=False)
        assert body() == 0 and (st["kernel_variant"] == 1 or not shipped)
        os.environ["RTIOW_DENSE_BODY"] = "capped"
        for flags in (rt.RT_FLAG_UNIFORM53, rt.RT_FLAG_DIAG_STATS, rt.RT_FLAG_NO_FILTER):
            if shipped or flags == rt.RT_FLAG_NO_FILTER:
                renderer.render(rt.book1_camera(24, 14), rt.make_params(24, 14, 72, flags=flags), want_fix=False)
                assert body() == 0, flags
        os.environ.pop("RTIOW_DENSE_BODY")
        renderer.upload_scene(large_grid_flat)
        for spp in (147, 20):
            _, _, st = renderer.render(rt.book1_camera(20, 12), rt.make_params(20, 12, spp), want_fix=False)
            assert body() == 0 and (st["kernel_variant"] == (4 if spp == 147 else 0) or not shipped)
    finally:
        _env(**old)


def _shell_scene(metal=True, glass=True):
    """The camera sits at the origin of a Lambertian sphere of radius 50 and albedo 0.97: every ray hits, no path meets the sky."""
    world = rt.HittableList()
    world.push(rt.Sphere(rt.Point3(0.0, 0.0, 0.0), 50.0, rt.Lambertian(rt.Color(0.97, 0.95, 0.99))))
    if metal:
        world.push(rt.Sphere(rt.Point3(6.0, -2.0, -14.0), 5.0, rt.Metal(rt.Color(0.9, 0.9, 0.8), 1.0)))
    if glass:
        world.push(rt.Sphere(rt.Point3(-1.5, 0.5, -6.0), 2.0, rt.Dialectric(1.5)))
    return world.flatten()


def _shell_camera(w, h):
    return rt.Camera(rt.Point3(0.0, 0.0, 0.0), rt.Point3(0.0, 0.0, -1.0), rt.Vec3(0.0, 1.0, 0.0), 60.0, float(w) / float(h), 0.05, 6.0)


@pytest.mark.parametrize("spp,large", [(64, False), (150, True)])
def test_a_scene_built_to_park(renderer, oracle_mod, spp, large):
    """16 x 10 x 64 samples at depth 50: 512 000 rays if nothing is absorbed (the Metal of fuzz 1 absorbs a few), ~5.15 % of the
    Lambertian / Metal scatters park -- ~25 000 parks, some tens of triple parks -- next to the glass sphere's lanes.  150 spp: the
    same on blocks of 1 024 (a scene of three spheres has no tile grid: the large-grid kernels)."""
    w, h = 16, 10
    st = _both_bodies(renderer, oracle_mod, _shell_scene(), _shell_camera(w, h), w, h, spp, large=large, variant=4 if large else 0, seed=11)
    assert st["rays_traced"] > 40 * w * h * spp                 # the paths do run deep


@pytest.mark.parametrize("max_depth", [1, 2, 3])
def test_a_park_on_the_last_allowed_bounce(renderer, oracle_mod, max_depth):
    w, h, spp = 16, 10, 64
    st = _both_bodies(renderer, oracle_mod, _shell_scene(glass=False), _shell_camera(w, h), w, h, spp, max_depth=max_depth, seed=5)
    assert st["rays_traced"] <= max_depth * w * h * spp


def test_parks_inside_the_book_scene_on_the_small_grid_kernel(renderer, oracle_mod, book1_flat):
    """The book scene inside a Lambertian shell (appended: list order is part of the input): no path meets the sky, so every path of the
    small-grid kernel runs on through glass, metal and diffuse spheres until it is absorbed or out of depth."""
    flat = np.concatenate([book1_flat, _shell_scene(metal=False, glass=False)])
    flat[-1]["radius"] = 3000.0
    w, h, spp = 16, 10, 24
    st = _both_bodies(renderer, oracle_mod, flat, rt.book1_camera(w, h), w, h, spp, seed=3)
    assert st["rays_traced"] > 20 * w * h * spp
