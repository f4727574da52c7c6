"""The environment cube map in the lit path queue on the GPU (rt_paths_step_env_device, rt_render_wavefront_env*)
against tests/env_ref.py, everything bit for bit: doubles as u64 patterns, the 32-bit words, the live counts, the u64 sums, both ray
counts.  Where sampling changes only the sums, every queue array is compared with the unsampled step's byte for byte.  Two frames have
answers that need no statement, and one scene is rendered with 16 seeds both ways: the same expectation, less variance."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import env_ref as er
import lights_ref as lr
import paths_ref as pr
import rtiow_amd as rt
from test_gpu_lights import lighting_of, same_bytes, u64
from test_gpu_paths import COUNTS, F64_FIELDS, U32_FIELDS, check_queue, device_queue, host, set_knob, torch_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, BSPP = lr.BW, lr.BH, lr.BSPP


def environment_of(env, sampled=True):
    """(texels, cdf) of the statement -> rt.Environment whose device forms search exactly that table."""
    texels, cdf = env
    return rt.Environment(np.array(texels), sample=sampled and cdf is not None, sums=None if cdf is None else np.array(cdf))


# ---- rt_paths_step_env_device --------------------------------------------------------------------------------------------------------------

def run_env_step(renderer, q, capacity, npix, light, env, *, sampled=True, no_direct=False, seed=er.SEED, rays0=5, shadow0=11, form="torch",
                 side_stream=False):
    """One environment step of the numpy queue `q` -> (in, out, the sums u64 [npix, 3], d_rays, d_shadow_rays).  form "device":
    Renderer.paths_step_device on raw structs and pointers; "torch": paths_step_torch."""
    torch, dev = torch_dev()
    A, B = device_queue(capacity, q), device_queue(capacity)
    fix = torch.zeros((npix, 3), dtype=torch.int64, device=dev)
    rays = torch.full((1,), rays0, dtype=torch.int64, device=dev)
    shadow = torch.full((1,), shadow0, dtype=torch.int64, device=dev)
    L, E = lighting_of(light, dev), environment_of(env, sampled)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        if form == "torch":
            rt.paths_step_torch(renderer, seed, A, B, fix, rays, lighting=L, no_direct=no_direct, shadow_rays=shadow, environment=E)
        else:
            renderer.paths_step_device(seed, A.struct(), B.struct(), fix.data_ptr(), npix, rays.data_ptr(), 1e-4, stream.cuda_stream, lighting=L,
                                       no_direct=no_direct, d_shadow_rays_ptr=shadow.data_ptr(), environment=E)
    stream.synchronize()
    torch.cuda.synchronize()
    return A, B, u64(fix), int(rays.item()), int(shadow.item())


def check_env_step(renderer, count, capacity, what, size=8, sampled=True, no_direct=False, **kw):
    flat, q, light = er.hand_queue()
    out, adds, live, shadow = er.hand_step(count, size, sampled, no_direct)
    A, B, fix, rays, got_shadow = run_env_step(renderer, pr.prefix(q, count), capacity, er.HAND_NPIX, light, er.hand_env(size), sampled=sampled,
                                               no_direct=no_direct, **kw)
    check_queue(B, out, what)
    assert np.array_equal(fix, adds), what
    assert rays == 5 + live and got_shadow == 11 + shadow, (what, rays, got_shadow, shadow)
    got = host(A)
    assert int(got["count"][0]) == count                                        # *in->count is unchanged
    assert all((got[f][count:] == pr.SENTINEL_U32).all() for f in U32_FIELDS) and all((got[f][count:] == pr.SENTINEL_F64).all() for f in F64_FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [513, 1024])
@pytest.mark.parametrize("count", COUNTS)
def test_env_step_on_the_hand_queue(renderer, oracle_mod, count, capacity):
    """Misses with and without the bit, a sample below the horizon, an occluded and a visible shadow ray, the sun, a texel with a NaN
    channel, a light hit carrying the bit, a pixel outside the frame, a wave whose 64 lanes all trace a shadow ray, waves where none does."""
    renderer.upload_scene(er.hand_queue()[0])
    check_env_step(renderer, count, capacity, f"env hand queue, {count} of {capacity}")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["sampled", "no_table", "no_direct"])
@pytest.mark.parametrize("size", [1, 2, 8])
def test_env_step_sizes_and_switches(renderer, oracle_mod, monkeypatch, size, how):
    """Face edges 1, 2 and 8; with the table, without it, and with RT_STEP_NO_DIRECT -- in one workgroup, so that a wave makes several trips."""
    set_knob(monkeypatch, "1")
    renderer.upload_scene(er.hand_queue()[0])
    check_env_step(renderer, er.HAND_N, 513, f"size {size}, {how}", size=size, sampled=how != "no_table", no_direct=how == "no_direct")
    if how != "sampled":
        out, _, _, shadow = er.hand_step(er.HAND_N, size, how != "no_table", how == "no_direct")
        assert shadow == 0 and not (out["event"] & np.uint32(er.DIRECT)).any()     # nothing is sampled and no bit is set


@pytest.mark.gpu
@pytest.mark.parametrize("form,side", [("device", True), ("torch", True), ("device", False)], ids=["device_side_stream", "torch_side_stream", "device"])
def test_env_step_forms_and_streams(renderer, oracle_mod, form, side):
    renderer.upload_scene(er.hand_queue()[0])
    check_env_step(renderer, er.HAND_N, 513, f"{form} form, side stream {side}", form=form, side_stream=side)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}], ids=["no_grid", "grid_dim_9"])
def test_env_step_under_the_scene_knobs(oracle_mod, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rt.Renderer(0) as r:
        r.upload_scene(er.hand_queue()[0])                                       # RTIOW_NO_GRID / RTIOW_GRID_DIM are read here
        check_env_step(r, er.HAND_N, 513, f"env hand queue under {env}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["first", "last", "zero", "nan_table", "inf_table"])
def test_env_step_with_tables_that_sample_at_an_edge_or_not_at_all(renderer, oracle_mod, name):
    """Only the first texel positive, only the last; an all-zero, a NaN and an infinite table, where nothing is sampled and no bit is set."""
    flat, q, light = er.hand_queue()
    renderer.upload_scene(flat)
    env = er.special_envs(8)[name]
    out, adds, live, shadow = er.step_env(flat, q, er.SEED, er.HAND_NPIX, light, env, 8)
    # (the first texel lies on face +x below the horizon of every Lambertian hit here: it is chosen, the bit is set, no ray follows)
    assert bool((out["event"] & np.uint32(er.DIRECT)).any()) == (name in ("first", "last")) and (shadow > 0) == (name == "last")
    A, B, fix, rays, got_shadow = run_env_step(renderer, q, 600, er.HAND_NPIX, light, env)
    check_queue(B, out, name)
    assert np.array_equal(fix, adds) and rays == 5 + live and got_shadow == 11 + shadow


@pytest.mark.gpu
def test_sampling_changes_what_is_added_never_where_paths_go(renderer, oracle_mod):
    """With the table, on the hand queue: every queue array and d_rays after the step equal the unsampled step's except bit 31 of `event`,
    and the sums differ."""
    flat, q, light = er.hand_queue()
    renderer.upload_scene(flat)
    A0, B0, fix0, rays0, shadow0 = run_env_step(renderer, q, 600, er.HAND_NPIX, light, er.hand_env(8), sampled=False)
    A1, B1, fix1, rays1, shadow1 = run_env_step(renderer, q, 600, er.HAND_NPIX, light, er.hand_env(8))
    assert rays1 == rays0 and shadow0 == 11 and shadow1 > 11 + 64
    bit = np.int32(-(1 << 31))
    assert ((B1.event.cpu().numpy() ^ B0.event.cpu().numpy()) & ~bit == 0).all() and ((A1.event.cpu().numpy() ^ A0.event.cpu().numpy()) & ~bit == 0).all()
    m = int(host(B1)["count"][0])
    assert (host(B1)["event"][:m] & np.uint32(er.DIRECT)).any() and not (host(B0)["event"][:m] & np.uint32(er.DIRECT)).any()
    for X1, X0 in ((A1, A0), (B1, B0)):
        X1.event &= 0x7FFFFFFF
        X0.event &= 0x7FFFFFFF
        same_bytes(X1, X0, "every array but bit 31 of event")
    assert not np.array_equal(fix1, fix0)


@pytest.mark.gpu
def test_env_step_on_degenerate_directions(renderer, oracle_mod):
    """Directions with equal components, +-0, zero, infinite and NaN entries: whatever the closest-hit scan makes of them, the step equals
    the statement -- the lookup of those that miss included."""
    flat, _, light = er.hand_queue()
    renderer.upload_scene(flat)
    q, dirs = er.degenerate_queue()
    out, adds, live, shadow = er.step_env(flat, q, er.SEED, er.HAND_NPIX, light, er.hand_env(8), 8)
    missed = [k for k in range(len(dirs)) if adds[k].any()]
    assert len(missed) >= 8                                                      # (pixel k is path k's)
    A, B, fix, rays, got_shadow = run_env_step(renderer, q, 64, er.HAND_NPIX, light, er.hand_env(8))
    check_queue(B, out, "degenerate directions")
    assert np.array_equal(fix, adds) and rays == 5 + live and got_shadow == 11 + shadow


# ---- the whole frame -----------------------------------------------------------------------------------------------------------------------

def env_device_frame(renderer, cam, p, L, E):
    torch, dev = torch_dev()
    d_fix = torch.full((p.height, p.width, 3), -1, dtype=torch.int64, device=dev)
    d_rays = torch.full((1,), -1, dtype=torch.int64, device=dev)
    d_shadow = torch.full((1,), -1, dtype=torch.int64, device=dev)
    renderer.render_wavefront_device(cam, p, d_fix.data_ptr(), d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream, lighting=L,
                                     d_shadow_rays_ptr=d_shadow.data_ptr(), environment=E)
    torch.cuda.synchronize()
    return u64(d_fix), int(d_rays.item()), int(d_shadow.item())


@functools.lru_cache(None)
def book_environment():
    return rt.Environment.sun_sky(8, sun_dir=(0.3, 0.8, 0.6), sun_radiance=(40.0, 36.0, 30.0), cos_radius=0.99, bottom=(0.3, 0.3, 0.3),
                                  top=(0.1, 0.15, 0.3)).table()


@functools.lru_cache(None)
def book_frame(max_depth, sampled, batch=257):
    """The statement's frame of lights_ref.book_case() under book_environment() at `max_depth` -> (fix, rays, shadow rays), read-only."""
    import oracle
    flat, light, _ = lr.book_case()
    texels = book_environment()
    env = (texels, er.environment_cdf(texels, 8) if sampled else None)
    fix, rays, shadow = er.render_env(flat, oracle.book1_camera(BW, BH), BW, BH, BSPP, light, env, 8, max_depth=max_depth, seed=1, batch=batch)
    fix.setflags(write=False)
    return fix, rays, shadow


@pytest.mark.gpu
@pytest.mark.parametrize("sampled", [True, False], ids=["sampled", "looked_up"])
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_env_frames_equal_the_statement(oracle_mod, monkeypatch, max_depth, sampled):
    """lights_ref.book_case() -- the book scene, lit by the large Lambertian sphere and five small ones -- under a sun_sky map: the host
    form, the device form, and both again after the batch has been regrown."""
    torch, dev = torch_dev()
    flat, light, _ = lr.book_case()
    want, want_rays, want_shadow = book_frame(max_depth, sampled)
    assert want_rays == book_frame(max_depth, not sampled)[1] and (want_shadow > 0) == (sampled and max_depth > 1)
    assert (max_depth == 1) == np.array_equal(want, book_frame(max_depth, not sampled)[0])
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    E = rt.Environment(book_environment(), sample=sampled)
    with rt.Renderer(0) as r:                                                    # (a context of its own: the first frame allocates its queues)
        r.upload_scene(flat)
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "257")
        fix, rays, st = r.render_wavefront(cam, p, lighting=lighting_of(light), environment=E)
        assert np.array_equal(fix, want) and rays == want_rays and st == {"rays_traced": want_rays, "shadow_rays": want_shadow}, "host form"
        fix, rays, shadow = env_device_frame(r, cam, p, lighting_of(light, dev), E)
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form"
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "1000")
        fix, rays, st = r.render_wavefront(cam, p, lighting=lighting_of(light), environment=E)
        assert np.array_equal(fix, want) and rays == want_rays and st["shadow_rays"] == want_shadow, "regrown batch"
        fix, rays, shadow = env_device_frame(r, cam, p, lighting_of(light, dev), E)
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form, regrown batch"


@pytest.mark.gpu
def test_env_frame_honours_sample_begin(renderer, oracle_mod):
    import oracle
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    texels = book_environment()
    want, want_rays, want_shadow = er.render_env(flat, oracle.book1_camera(BW, BH), BW, BH, 2, light, (texels, er.environment_cdf(texels, 8)), 8,
                                                 max_depth=4, seed=5, sample_begin=3)
    p = rt.make_params(BW, BH, 2, max_depth=4, seed=5, sample_begin=3)
    fix, rays, st = renderer.render_wavefront(rt.book1_camera(BW, BH), p, lighting=lighting_of(light), environment=rt.Environment(texels))
    assert np.array_equal(fix, want) and rays == want_rays and st["shadow_rays"] == want_shadow


@pytest.mark.gpu
def test_a_black_environment_gives_the_black_sky_lit_frame(renderer, oracle_mod):
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=50, seed=1)
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=rt.Lighting((0, 0, 0), (0, 0, 0), np.array(light.emission)))
    for sample in (False, True):                                                 # (a black map's total is 0: nothing is sampled either way)
        fix, rays, st = renderer.render_wavefront(cam, p, lighting=lighting_of(light), environment=rt.Environment(np.zeros((6, 2, 2, 3)), sample=sample))
        assert np.array_equal(fix, lit) and lit.any() and rays == lit_rays and st["shadow_rays"] == 0


@pytest.mark.gpu
def test_a_constant_environment_seen_by_rays_that_all_miss(renderer, oracle_mod):
    flat = np.zeros(1, dtype=rt.SPHERE_DTYPE)
    flat[0]["center"], flat[0]["radius"], flat[0]["albedo"] = (13.0, 2.0, 30.0), 0.5, (0.5, 0.5, 0.5)
    renderer.upload_scene(flat)
    w, h, spp, c = 8, 6, 3, 0.25
    for sample in (False, True):
        fix, rays, st = renderer.render_wavefront(rt.book1_camera(w, h), rt.make_params(w, h, spp, max_depth=5, seed=3),
                                                  environment=rt.Environment(np.full((6, 4, 4, 3), c), sample=sample))
        assert (fix == spp * (1 << 30)).all() and rays == w * h * spp and st["shadow_rays"] == 0


# ---- the same expectation, less variance ---------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def stat_frames():
    """The stat scene with each of the 16 seeds, sampled and not -> (frames sampled, frames not), rendered once."""
    flat, light = er.stat_scene()
    cam = er.stat_camera()
    texels = er.stat_environment().table()
    sampled, plain = [], []
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        L = lighting_of(light)
        for seed in er.STAT_SEEDS:
            p = rt.make_params(er.STAT_W, er.STAT_H, er.STAT_SPP, max_depth=er.STAT_DEPTH, seed=seed)
            fix, rays, st = r.render_wavefront(cam, p, lighting=L, environment=rt.Environment(texels, sample=True))
            fix0, rays0, st0 = r.render_wavefront(cam, p, lighting=L, environment=rt.Environment(texels, sample=False))
            assert rays == rays0 and st["shadow_rays"] > 0 and st0["shadow_rays"] == 0
            sampled.append(fix)
            plain.append(fix0)
    return sampled, plain


@pytest.mark.gpu
def test_sampled_and_unsampled_frames_have_the_same_expectation(oracle_mod):
    """A Lambertian ground, a Metal, a Dialectric and an occluder under a sun_sky map whose sun is out of view, 16 x 12 pixels, 64 spp,
    depth 8, seeds 1..16.  Per seed the frame-total energy sampled minus unsampled: |mean| <= 4 standard errors of the 16 differences."""
    sampled, plain = stat_frames()
    mean, stderr, var_sampled, var_plain = er.stat_numbers(sampled, plain)
    print(f"energy sampled - unsampled: mean {mean:.6g}, standard error {stderr:.6g}, |mean| / stderr {abs(mean) / stderr:.3f}")
    assert stderr > 0.0 and all(f.any() for f in sampled) and all(f.any() for f in plain)
    assert abs(mean) <= 4.0 * stderr
    # ... and the numbers are the host test's, which computes them with the statement
    assert all(math.isclose(x, y, rel_tol=1e-9) for x, y in zip((mean, stderr, var_sampled, var_plain), er.STAT_EXPECTED))


@pytest.mark.gpu
def test_sampling_has_less_variance_than_the_random_walk(oracle_mod):
    """On the same 16 seeds: the per-pixel variance over the seeds, summed over the frame, sampled is strictly below unsampled (the ratio
    is in profiles/env.txt)."""
    sampled, plain = stat_frames()
    _, _, var_sampled, var_plain = er.stat_numbers(sampled, plain)
    print(f"variance unsampled {var_plain:.6g}, sampled {var_sampled:.6g}, unsampled / sampled {var_plain / var_sampled:.3f}")
    assert 0.0 < var_sampled < var_plain


# ---- context rules, the command line -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rejections_that_need_the_context(oracle_mod, book1_flat):
    """No scene (after the lighting and the environment checks); an emission table of another length; environment= with direct=."""
    torch, dev = torch_dev()
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, seed=1)
    E = rt.Environment(np.full((6, 2, 2, 3), 0.5))
    with rt.Renderer(0) as r:
        A, B = device_queue(64, count=7), device_queue(64)
        fix = torch.full((BH, BW, 3), 3, dtype=torch.int64, device=dev)
        shadow = torch.full((1,), 9, dtype=torch.int64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            rt.paths_step_torch(r, 1, A, B, fix, shadow_rays=shadow, environment=E)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_wavefront(cam, p, environment=E)
        r.upload_scene(book1_flat)
        wrong = torch.zeros((len(book1_flat) + 1, 3), dtype=torch.float64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_paths_step_env.*uploaded sphere count"):
            rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting(emission=wrong), shadow_rays=shadow, environment=E)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_render_wavefront_env.*uploaded sphere count"):
            r.render_wavefront_device(cam, p, fix.data_ptr(), lighting=rt.Lighting(emission=wrong), d_shadow_rays_ptr=shadow.data_ptr(), environment=E)
        with pytest.raises(ValueError, match="does not combine"):
            r.render_wavefront(cam, p, lighting=rt.Lighting(emission={0: (1, 1, 1)}), direct=True, environment=E)
        with pytest.raises(ValueError, match="does not combine"):
            rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting(emission={0: (1, 1, 1)}), direct=[0], environment=E)
        torch.cuda.synchronize()
        assert (fix == 3).all() and int(shadow.item()) == 9 and int(host(A)["count"][0]) == 7 and int(host(B)["count"][0]) == pr.SENTINEL_U32
        r.render(cam, p)
        before = r.last_stats()
        r.render_wavefront(cam, rt.make_params(BW, BH, 2, seed=9), environment=E)
        assert r.last_stats() == before                                          # no launch slot is taken


@pytest.mark.gpu
def test_another_scan_mode_refuses_every_env_form(oracle_mod, book1_flat):
    torch, dev = torch_dev()
    os.environ["RTIOW_SCAN_MODE"] = "1"
    try:
        r = rt.Renderer(0)                                                       # RTIOW_SCAN_MODE is read here
    finally:
        os.environ.pop("RTIOW_SCAN_MODE")
    try:
        r.upload_scene(book1_flat)
        E = rt.Environment(np.full((6, 2, 2, 3), 0.5))
        cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP)
        A, B = device_queue(64, count=7), device_queue(64)
        fix = torch.full((BH, BW, 3), 3, dtype=torch.int64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            rt.paths_step_torch(r, 1, A, B, fix, environment=E)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            r.render_wavefront_device(cam, p, fix.data_ptr(), environment=E)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            r.render_wavefront(cam, p, environment=E)
        torch.cuda.synchronize()
        assert (fix == 3).all() and int(host(A)["count"][0]) == 7 and int(host(B)["count"][0]) == pr.SENTINEL_U32
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [False, True], ids=["env", "env_sample"])
def test_cpp_cli_env_writes_the_bytes_the_python_path_resolves(renderer, oracle_mod, tmp_path, sample):
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    flat, light, _ = lr.book_case()
    big = int(np.argmax(np.all(light.emission == np.array(lr.BIG), axis=1)))
    scene_file, env_file, out = str(tmp_path / "scene.bin"), str(tmp_path / "env.bin"), str(tmp_path / "day.ppm")
    rt.save_scene(scene_file, flat)
    E = rt.Environment(book_environment(), sample=sample)
    E.save(env_file)
    w, h, spp = 64, 36, 5
    base = [exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--spp", str(spp), "--seed", "4", "--out", out]
    run = subprocess.run(base + ["--wavefront", "--env", env_file, "--emit", f"{big}:4,3.2,2.4"] + (["--env-sample"] if sample else []), check=True,
                         capture_output=True, text=True, timeout=120, env=dict(os.environ, RTIOW_WAVEFRONT_BATCH="4000"))
    renderer.upload_scene(flat)
    fix, _, st = renderer.render_wavefront(rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=4), lighting=rt.Lighting(emission={big: (4, 3.2, 2.4)}),
                                           environment=E)
    want = renderer.resolve_rgba8(fix, spp, flip=True)[:, :, :3]
    assert np.array_equal(rt.read_ppm(out), want) and want.any()
    assert (f"shadow rays: {st['shadow_rays']}" in run.stderr) == sample and (st["shadow_rays"] > 0) == sample
