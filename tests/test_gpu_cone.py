"""Direct lighting by solid angle on the GPU (RT_DIRECT_CONE: rt_paths_step_nee_device, rt_render_wavefront_nee_device,
rt_render_wavefront_nee_sampled) against tests/cone_ref.py, everything bit for bit: doubles as u64 patterns, the
32-bit words, the live counts, the u64 sums, both ray counts.  Against the area step every queue array is compared byte for byte: the
sampler changes only the sums and the shadow count.  Three frames have answers that need no statement, and two scenes are rendered with 16
seeds: the same expectation as the random walk and as area sampling, and, where the light is large and near, less variance than area
sampling -- which there has more than no direct lighting at all."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cone_ref as cr
import lights_ref as lr
import nee_ref as nr
import paths_ref as pr
import rtiow_amd as rt
import test_gpu_nee as tgn
from test_gpu_lights import lighting_of, same_bytes, u64
from test_gpu_paths import COUNTS, F64_FIELDS, U32_FIELDS, check_queue, device_queue, host, set_knob, torch_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, BSPP = lr.BW, lr.BH, lr.BSPP


# ---- rt_paths_step_nee_device with RT_DIRECT_CONE ----------------------------------------------------------------------------------------------

def run_step(renderer, q, capacity, npix, light, direct, *, sampling="cone", no_direct=False, seed=cr.SEED, rays0=5, shadow0=11, form="torch",
             side_stream=False):
    """One step of the numpy queue `q` -> (in, out, the sums u64 [npix, 3], d_rays, d_shadow_rays).  direct: True or a list of sphere
    indices.  form "device": Renderer.paths_step_device on raw structs and pointers; "torch": paths_step_torch."""
    torch, dev = torch_dev()
    A, B = device_queue(capacity, q), device_queue(capacity)
    fix = torch.zeros((npix, 3), dtype=torch.int64, device=dev)
    rays = torch.full((1,), rays0, dtype=torch.int64, device=dev)
    shadow = torch.full((1,), shadow0, dtype=torch.int64, device=dev)
    L = lighting_of(light, dev)
    if direct is not True:
        direct = torch.tensor(list(direct), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        if form == "torch":
            rt.paths_step_torch(renderer, seed, A, B, fix, rays, lighting=L, direct=direct, no_direct=no_direct, shadow_rays=shadow, sampling=sampling)
        else:
            renderer.paths_step_device(seed, A.struct(), B.struct(), fix.data_ptr(), npix, rays.data_ptr(), 1e-4, stream.cuda_stream, lighting=L,
                                       direct=direct, no_direct=no_direct, d_shadow_rays_ptr=shadow.data_ptr(), sampling=sampling)
    stream.synchronize()
    torch.cuda.synchronize()
    return A, B, u64(fix), int(rays.item()), int(shadow.item())


def check_step(renderer, count, capacity, what, **kw):
    flat, q, light, lights = cr.hand_queue()
    out, adds, live, shadow = cr.hand_step(count)
    A, B, fix, rays, got_shadow = run_step(renderer, pr.prefix(q, count), capacity, cr.HAND_NPIX, light, lights, **kw)
    check_queue(B, out, what)
    assert np.array_equal(fix, adds), what
    assert rays == 5 + live and got_shadow == 11 + shadow, (what, rays, got_shadow, shadow)
    got = host(A)
    assert int(got["count"][0]) == count                                        # *in->count is unchanged
    assert all((got[f][count:] == pr.SENTINEL_U32).all() for f in U32_FIELDS) and all((got[f][count:] == pr.SENTINEL_F64).all() for f in F64_FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["", "1"], ids=["grid", "one_block"])
@pytest.mark.parametrize("capacity", [513, 1024])
@pytest.mark.parametrize("count", COUNTS)
def test_cone_step_on_the_hand_queue(renderer, oracle_mod, monkeypatch, count, capacity, blocks):
    """A hit point inside a light, a sample below the horizon, disk tries accepted first and in a later block, both tangent frames, a blocked
    ray, a light's inner face behind t_min, a list entry that names no sphere, DIRECT paths on a light's two faces, a light at r / d = 1e-6;
    a wave whose 64 lanes all trace a shadow ray, waves where none does, one where only lane 63 does."""
    set_knob(monkeypatch, blocks)
    renderer.upload_scene(cr.hand_queue()[0])
    check_step(renderer, count, capacity, f"cone hand queue, {count} of {capacity}")


@pytest.mark.gpu
@pytest.mark.parametrize("form,side", [("device", True), ("torch", True), ("device", False)], ids=["device_side_stream", "torch_side_stream", "device"])
def test_cone_step_forms_and_streams(renderer, oracle_mod, form, side):
    renderer.upload_scene(cr.hand_queue()[0])
    check_step(renderer, cr.HAND_N, 513, f"{form} form, side stream {side}", form=form, side_stream=side)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}], ids=["no_grid", "grid_dim_9"])
def test_cone_step_under_the_scene_knobs(oracle_mod, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rt.Renderer(0) as r:
        r.upload_scene(cr.hand_queue()[0])                                       # RTIOW_NO_GRID / RTIOW_GRID_DIM are read here
        check_step(r, cr.HAND_N, 513, f"cone hand queue under {env}")


@pytest.mark.gpu
def test_cone_step_with_no_direct_against_the_statement(renderer, oracle_mod):
    """RT_STEP_NO_DIRECT on the hand queue, DIRECT bits and all: no light sample, no bit set, the front faces still not counted again."""
    flat, q, light, lights = cr.hand_queue()
    renderer.upload_scene(flat)
    out, adds, live, shadow = cr.hand_step(cr.HAND_N, no_direct=True)
    assert shadow == 0 and not (out["event"] & np.uint32(nr.DIRECT)).any()
    A, B, fix, rays, got_shadow = run_step(renderer, q, 600, cr.HAND_NPIX, light, lights, no_direct=True)
    check_queue(B, out, "NO_DIRECT")
    assert np.array_equal(fix, adds) and rays == 5 + live and got_shadow == 11


@pytest.mark.gpu
def test_flags_zero_on_the_cone_queue_is_the_area_statement(renderer, oracle_mod):
    """sampling="area" on this file's queue and scene: nee_ref's answer (cone_ref.hand_step with flags 0 is nee_ref.step_nee, test_cone_host.py)."""
    flat, q, light, lights = cr.hand_queue()
    renderer.upload_scene(flat)
    out, adds, live, shadow = cr.hand_step(cr.HAND_N, flags=0)
    A, B, fix, rays, got_shadow = run_step(renderer, q, 513, cr.HAND_NPIX, light, lights, sampling="area")
    check_queue(B, out, "area")
    assert np.array_equal(fix, adds) and rays == 5 + live and got_shadow == 11 + shadow


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hand", "book"])
def test_the_sampler_changes_what_is_added_never_where_paths_go(renderer, oracle_mod, which):
    """On the hand queue and on a book-scene queue from rt_paths_begin_device: every queue array -- `out`, `in` as the step leaves it,
    both scratch arrays -- and d_rays equal the area step's byte for byte; only the sums and the shadow count differ."""
    if which == "hand":
        flat, q, light, lights = cr.hand_queue()
        seed, npix, direct = cr.SEED, cr.HAND_NPIX, lights
        renderer.upload_scene(flat)
    else:
        flat, light, _ = lr.book_case()
        seed, npix, direct = 1, BW * BH, True
        renderer.upload_scene(flat)
        q = tgn.begun_book_queue(renderer)
    A0, B0, fix0, rays0, shadow0 = run_step(renderer, q, 600, npix, light, direct, seed=seed, sampling="area")
    A1, B1, fix1, rays1, shadow1 = run_step(renderer, q, 600, npix, light, direct, seed=seed)
    same_bytes(B1, B0, "out")
    same_bytes(A1, A0, "in")
    assert rays1 == rays0 == 5 + 513 and 0 < int(host(B1)["count"][0]) < 513
    assert (host(B1)["event"][:int(host(B1)["count"][0])] & np.uint32(nr.DIRECT)).any()
    print(f"{which}: shadow rays area {shadow0 - 11}, cone {shadow1 - 11}")
    assert not np.array_equal(fix1, fix0) and shadow1 != shadow0 and shadow1 > 11 and shadow0 > 11


# ---- the whole frame -----------------------------------------------------------------------------------------------------------------------

def device_frame(renderer, cam, p, L, direct=True, sampling="cone"):
    torch, dev = torch_dev()
    d_fix = torch.full((p.height, p.width, 3), -1, dtype=torch.int64, device=dev)
    d_rays = torch.full((1,), -1, dtype=torch.int64, device=dev)
    d_shadow = torch.full((1,), -1, dtype=torch.int64, device=dev)
    renderer.render_wavefront_device(cam, p, d_fix.data_ptr(), d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream, lighting=L, direct=direct,
                                     d_shadow_rays_ptr=d_shadow.data_ptr(), sampling=sampling)
    torch.cuda.synchronize()
    return u64(d_fix), int(d_rays.item()), int(d_shadow.item())


@pytest.mark.gpu
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_cone_frames_equal_the_statement(oracle_mod, monkeypatch, max_depth):
    """lights_ref.book_case() -- the book scene under a dim sky, lit by the large Lambertian sphere and five small ones -- with the lights
    sampled by solid angle: the new host form, the device form, and both again at another batch size.  rays_traced is the lit frame's."""
    torch, dev = torch_dev()
    flat, light, _ = lr.book_case()
    want, want_rays, want_shadow = cr.book_frame(max_depth)
    assert want_rays == lr.book_frame(max_depth)[1] and (want_shadow > 0) == (max_depth > 1)
    assert max_depth == 1 or (not np.array_equal(want, lr.book_frame(max_depth)[0]) and not np.array_equal(want, nr.book_frame(max_depth)[0]))
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    with rt.Renderer(0) as r:                                                    # (a context of its own: the first frame allocates its queues)
        r.upload_scene(flat)
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "257")
        fix, rays, st = r.render_wavefront(cam, p, lighting=lighting_of(light), direct=True, sampling="cone")
        assert np.array_equal(fix, want) and rays == want_rays and st == {"rays_traced": want_rays, "shadow_rays": want_shadow}, "host form"
        fix, rays, shadow = device_frame(r, cam, p, lighting_of(light, dev))
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form"
        lit_fix, lit_rays = r.render_wavefront(cam, p, lighting=lighting_of(light))
        assert lit_rays == rays
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "1000")
        fix, rays, st = r.render_wavefront(cam, p, lighting=lighting_of(light), direct=True, sampling="cone")
        assert np.array_equal(fix, want) and rays == want_rays and st["shadow_rays"] == want_shadow, "host form, another batch"
        fix, rays, shadow = device_frame(r, cam, p, lighting_of(light), direct=nr.light_list(light.emission))
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form, another batch, the list given"


def _sampled(renderer, cam, p, L, direct_flags):
    """rt_render_wavefront_nee_sampled as the C ABI has it -> (fix, rays, shadow rays)."""
    import ctypes as C
    from rtiow_amd import _ffi
    table = L.table(renderer.n_spheres)
    light = L.struct(table.ctypes.data, table.shape[0])
    fix = np.zeros((p.height, p.width, 3), dtype=np.uint64)
    rays, shadow = C.c_uint64(0), C.c_uint64(0)
    rc = cam.to_rt_camera()
    _ffi.check(_ffi.load().rt_render_wavefront_nee_sampled(renderer._h, C.byref(rc), C.byref(p), C.byref(light), direct_flags, fix.ctypes.data_as(C.c_void_p),
                                                           C.byref(rays), C.byref(shadow), None), "rt_render_wavefront_nee_sampled")
    return fix, int(rays.value), int(shadow.value)


@pytest.mark.gpu
def test_the_new_host_form_with_flags_zero_is_the_nee_frame(renderer, oracle_mod):
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=5, seed=3)
    L = lighting_of(light)
    want, want_rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True)
    fix, rays, shadow = _sampled(renderer, cam, p, L, 0)
    assert np.array_equal(fix, want) and fix.any() and rays == want_rays and shadow == st["shadow_rays"] > 0
    cone, cone_rays, cone_shadow = _sampled(renderer, cam, p, L, 2)
    assert cone_rays == rays and cone_shadow > shadow and not np.array_equal(cone, fix)
    via_python, _, st2 = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
    assert np.array_equal(via_python, cone) and st2["shadow_rays"] == cone_shadow


@pytest.mark.gpu
@pytest.mark.parametrize("sky", [((0, 0, 0), (0, 0, 0)), lr.HAND_SKY], ids=["black_sky", "hand_sky"])
def test_lights_inside_opaque_shells_leave_the_lit_frame(renderer, oracle_mod, sky):
    """Every light sits inside a Lambertian shell: no path and no shadow ray reaches one, so the cone frame is the lit frame bit for bit
    (under the black sky: black) although shadow rays are traced."""
    flat, emit = tgn.shell_scene()
    renderer.upload_scene(flat)
    w, h, spp = 33, 17, 3
    cam = rt.Camera((9.0, 3.0, 8.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0, w / h, 0.05, 10.0)
    p = rt.make_params(w, h, spp, max_depth=6, seed=7)
    L = rt.Lighting(sky[0], sky[1], emit)
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=L)
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
    assert np.array_equal(fix, lit) and rays == lit_rays and st["shadow_rays"] > 0
    assert fix.any() == (sky[0] != (0, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["none", "zeros"])
def test_a_frame_without_lights_is_the_lit_frame(renderer, oracle_mod, table):
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=50, seed=1)
    L = rt.Lighting(light.sky_bottom, light.sky_top, lr.dark_tables(len(flat))[table])
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=L)
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
    assert np.array_equal(fix, lit) and fix.any() and rays == lit_rays and st["shadow_rays"] == 0
    torch, dev = torch_dev()
    dark = lr.dark_tables(len(flat))["negative_nan"]                             # the device form validates no table: NaN and negative entries pass
    fix, rays, shadow = device_frame(renderer, cam, p, rt.Lighting(light.sky_bottom, light.sky_top, torch.from_numpy(np.array(dark)).to(dev)))
    assert np.array_equal(fix, lit) and rays == lit_rays and shadow == 0


@pytest.mark.gpu
def test_depth_one_is_the_lit_frame(renderer, oracle_mod):
    """max_depth = 1: the only step is the last one and runs with RT_STEP_NO_DIRECT."""
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=1, seed=1)
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=lighting_of(light))
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=lighting_of(light), direct=True, sampling="cone")
    assert np.array_equal(fix, lit) and fix.any() and rays == lit_rays == BW * BH * BSPP and st["shadow_rays"] == 0


# ---- the same expectation; less variance where the light is large and near ------------------------------------------------------------------

def _frames(flat, light, cam, w, h, spp, depth, seeds):
    """-> (frames cone, frames area, frames lit, shadow rays cone, shadow rays area), one frame per seed."""
    cone, area, lit, n_cone, n_area = [], [], [], 0, 0
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        L = lighting_of(light)
        for seed in seeds:
            p = rt.make_params(w, h, spp, max_depth=depth, seed=seed)
            fix, rays, st = r.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
            fix_area, rays_area, st_area = r.render_wavefront(cam, p, lighting=L, direct=True)
            fix_lit, rays_lit = r.render_wavefront(cam, p, lighting=L)
            assert rays == rays_area == rays_lit and st["shadow_rays"] > 0 and st_area["shadow_rays"] > 0
            cone.append(fix)
            area.append(fix_area)
            lit.append(fix_lit)
            n_cone += st["shadow_rays"]
            n_area += st_area["shadow_rays"]
    return cone, area, lit, n_cone, n_area


@functools.lru_cache(None)
def big_light_frames():
    flat, light = cr.big_light_scene()
    return _frames(flat, light, cr.big_light_camera(), cr.BIG_W, cr.BIG_H, cr.BIG_SPP, cr.BIG_DEPTH, cr.BIG_SEEDS)


@pytest.mark.gpu
def test_big_light_cone_and_lit_frames_have_the_same_expectation(oracle_mod):
    """A light of radius 1 resting on a Lambertian ground under a black sky, 16 x 12 pixels, 64 spp, depth 8, 16 fixed seeds.  Per seed the
    frame-total energy of cone minus lit: |mean| <= 5 standard errors of the 16 differences (the statement alone: 2.59 on these seeds,
    0.35 on 64 others)."""
    cone, area, lit, n_cone, n_area = big_light_frames()
    mean, stderr, var_cone, var_lit = nr.stat_numbers(cone, lit)
    print(f"energy cone - lit: mean {mean:.6g}, standard error {stderr:.6g}, |mean| / stderr {abs(mean) / stderr:.3f}; shadow rays area {n_area}, cone {n_cone}")
    assert stderr > 0.0 and all(f.any() for f in cone) and all(f.any() for f in lit)
    assert abs(mean) <= 5.0 * stderr


@pytest.mark.gpu
def test_big_light_cone_has_less_variance_than_area(oracle_mod):
    """On the same 16 seeds: the per-pixel variance over the seeds, summed over the frame, of cone sampling is strictly below area
    sampling's (the statement's ratio is 8.2; area sampling is there worse than the random walk, cone sampling better)."""
    cone, area, lit, _, _ = big_light_frames()
    _, _, var_cone, var_area = nr.stat_numbers(cone, area)
    var_lit = nr.stat_numbers(lit, lit)[2]
    print(f"variance lit {var_lit:.6g}, area {var_area:.6g}, cone {var_cone:.6g}, area / cone {var_area / var_cone:.3f}, lit / cone {var_lit / var_cone:.3f}")
    assert 0.0 < var_cone < var_area


@pytest.mark.gpu
def test_big_light_no_sample_can_reach_the_clamp(oracle_mod):
    """Every pixel sum is <= spp * depth * cone_sample_bound() on the 2^-32 grid (a path adds at most once per step, each time at most the
    bound, its throughput never above 1), far below what spp samples at the 2^16 clamp would give: the u64 sums are unbiased."""
    cone, _, _, _, _ = big_light_frames()
    bound = cr.cone_sample_bound()
    assert bound == 8.0 and bound * cr.BIG_DEPTH < 65536.0 / 1000.0
    limit = int(cr.BIG_SPP * cr.BIG_DEPTH * bound * 4294967296.0)
    assert all(int(f.max()) <= limit for f in cone)


@functools.lru_cache(None)
def stat_frames():
    flat, light = nr.stat_scene()
    return _frames(flat, light, nr.stat_camera(), nr.STAT_W, nr.STAT_H, nr.STAT_SPP, nr.STAT_DEPTH, nr.STAT_SEEDS)


@pytest.mark.gpu
def test_small_far_light_cone_and_area_frames_have_the_same_expectation(oracle_mod):
    """nee_ref.stat_scene(): a light of radius 0.25, far and out of view.  Per seed the frame-total energy of cone minus area: |mean| <= 5
    standard errors (the statement alone: 0.25).  The variances are printed, not asserted: the statement's ratio is only 1.08."""
    cone, area, lit, n_cone, n_area = stat_frames()
    mean, stderr, var_cone, var_area = nr.stat_numbers(cone, area)
    print(f"energy cone - area: mean {mean:.6g}, standard error {stderr:.6g}, |mean| / stderr {abs(mean) / stderr:.3f}")
    print(f"variance lit {nr.stat_numbers(lit, lit)[2]:.6g}, area {var_area:.6g}, cone {var_cone:.6g}, area / cone {var_area / var_cone:.3f}; "
          f"shadow rays area {n_area}, cone {n_cone}")
    assert stderr > 0.0 and all(f.any() for f in cone) and all(f.any() for f in area)
    assert abs(mean) <= 5.0 * stderr


# ---- the command line ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cpp_cli_direct_cone_writes_the_bytes_the_python_path_resolves(renderer, oracle_mod, tmp_path):
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    flat, light, _ = lr.book_case()
    big = int(np.argmax(np.all(light.emission == np.array(lr.BIG), axis=1)))
    small = next(k for k in range(len(flat)) if k != big and lr.is_light(light.emission[k]))
    scene_file, out = str(tmp_path / "scene.bin"), str(tmp_path / "night.ppm")
    rt.save_scene(scene_file, flat)
    w, h, spp = 64, 36, 5
    base = [exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--spp", str(spp), "--seed", "4", "--out", out]
    lit = ["--sky", "0,0,0:0,0,0", "--emit", f"{big}:4,3.2,2.4", "--emit", f"{small}:8,2,1"]
    run = subprocess.run(base + ["--wavefront", "--direct-cone"] + lit, check=True, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, RTIOW_WAVEFRONT_BATCH="4000"))
    renderer.upload_scene(flat)
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {big: (4, 3.2, 2.4), small: (8, 2, 1)})
    cam, p = rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=4)
    fix, _, st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
    want = renderer.resolve_rgba8(fix, spp, flip=True)[:, :, :3]
    assert np.array_equal(rt.read_ppm(out), want) and want.any()
    assert f"shadow rays: {st['shadow_rays']}" in run.stderr
    area_fix, _, _ = renderer.render_wavefront(cam, p, lighting=L, direct=True)
    assert not np.array_equal(renderer.resolve_rgba8(area_fix, spp, flip=True)[:, :, :3], want)
    for args in (["--direct-cone"] + lit, ["--wavefront", "--direct-cone"], ["--wavefront", "--direct-cone"] + lit[:2], ["--wavefront", "--direct", "--direct-cone"] + lit):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2, (args, bad.returncode, bad.stderr)
