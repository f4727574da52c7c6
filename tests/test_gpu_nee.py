"""Next-event estimation in the lit path queue on the GPU (rt_paths_step_nee_device, rt_render_wavefront_nee*) against
tests/nee_ref.py, everything bit for bit: doubles as u64 patterns, the 32-bit words, the live counts, the u64 sums, both ray counts.  Where
direct lighting changes nothing the NEE forms are compared with the lit ones byte for byte; where it changes only the sums, every queue
array is.  Three frames have answers that need no statement, and one scene is rendered with 16 seeds both ways: the same expectation,
less variance."""
import functools
import os
import subprocess

import numpy as np
import pytest

import lights_ref as lr
import nee_ref as nr
import paths_ref as pr
import rtiow_amd as rt
import wavefront_ref as wr
from test_gpu_lights import book_queue, device_frame, lighting_of, same_bytes, u64
from test_gpu_paths import COUNTS, F64_FIELDS, U32_FIELDS, bits, check_queue, device_queue, host, set_knob, torch_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, BSPP = lr.BW, lr.BH, lr.BSPP


# ---- rt_paths_step_nee_device --------------------------------------------------------------------------------------------------------------

def run_nee_step(renderer, q, capacity, npix, light, direct, *, no_direct=False, seed=nr.SEED, rays0=5, shadow0=11, form="torch", side_stream=False):
    """One step of the numpy queue `q` -> (in, out, the sums u64 [npix, 3], d_rays, d_shadow_rays).  direct: False (the lit step), True or
    a list of sphere indices.  form "device": Renderer.paths_step_device on raw structs and pointers; "torch": paths_step_torch."""
    torch, dev = torch_dev()
    A, B = device_queue(capacity, q), device_queue(capacity)
    fix = torch.zeros((npix, 3), dtype=torch.int64, device=dev)
    rays = torch.full((1,), rays0, dtype=torch.int64, device=dev)
    shadow = torch.full((1,), shadow0, dtype=torch.int64, device=dev)
    L = lighting_of(light, dev)
    if direct is not False and direct is not True:
        direct = torch.tensor(list(direct), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        if form == "torch":
            rt.paths_step_torch(renderer, seed, A, B, fix, rays, lighting=L, direct=direct, no_direct=no_direct,
                                shadow_rays=shadow if direct is not False else None)
        else:
            renderer.paths_step_device(seed, A.struct(), B.struct(), fix.data_ptr(), npix, rays.data_ptr(), 1e-4, stream.cuda_stream, lighting=L,
                                       direct=direct, no_direct=no_direct, d_shadow_rays_ptr=shadow.data_ptr() if direct is not False else 0)
    stream.synchronize()
    torch.cuda.synchronize()
    return A, B, u64(fix), int(rays.item()), int(shadow.item())


def check_nee_step(renderer, count, capacity, what, **kw):
    flat, q, light, lights = nr.hand_queue()
    out, adds, live, shadow = nr.hand_step(count)
    A, B, fix, rays, got_shadow = run_nee_step(renderer, pr.prefix(q, count), capacity, nr.HAND_NPIX, light, lights, **kw)
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
def test_nee_step_on_the_hand_queue(renderer, oracle_mod, monkeypatch, count, capacity, blocks):
    """Light samples at either end of the list, blocked by another sphere, on the light's far side, below the horizon, accepted first and in
    a later block, above the clamp, through a list entry that names no sphere; DIRECT paths on a light's two faces and through the three
    materials; a wave whose 64 lanes all trace a shadow ray, waves where none does, one where only lane 63 does."""
    set_knob(monkeypatch, blocks)
    renderer.upload_scene(nr.hand_queue()[0])
    check_nee_step(renderer, count, capacity, f"NEE hand queue, {count} of {capacity}")


@pytest.mark.gpu
@pytest.mark.parametrize("form,side", [("device", True), ("torch", True), ("device", False)], ids=["device_side_stream", "torch_side_stream", "device"])
def test_nee_step_forms_and_streams(renderer, oracle_mod, form, side):
    renderer.upload_scene(nr.hand_queue()[0])
    check_nee_step(renderer, nr.HAND_N, 513, f"{form} form, side stream {side}", form=form, side_stream=side)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}], ids=["no_grid", "grid_dim_9"])
def test_nee_step_under_the_scene_knobs(oracle_mod, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rt.Renderer(0) as r:
        r.upload_scene(nr.hand_queue()[0])                                       # RTIOW_NO_GRID / RTIOW_GRID_DIM are read here
        check_nee_step(r, nr.HAND_N, 513, f"NEE hand queue under {env}")


@pytest.mark.gpu
def test_nee_step_with_no_direct_against_the_statement(renderer, oracle_mod):
    """RT_STEP_NO_DIRECT on the hand queue, DIRECT bits and all: no light sample, no bit set, the front faces still not counted again."""
    flat, q, light, lights = nr.hand_queue()
    renderer.upload_scene(flat)
    out, adds, live, shadow = nr.hand_step(nr.HAND_N, no_direct=True)
    assert shadow == 0 and not (out["event"] & np.uint32(nr.DIRECT)).any()
    A, B, fix, rays, got_shadow = run_nee_step(renderer, q, 600, nr.HAND_NPIX, light, lights, no_direct=True)
    check_queue(B, out, "NO_DIRECT")
    assert np.array_equal(fix, adds) and rays == 5 + live and got_shadow == 11


def begun_book_queue(renderer):
    """The first 513 paths of the golden book frame as rt_paths_begin_device writes them, read back (the statement's: test_gpu_lights.py)."""
    torch, dev = torch_dev()
    Q = device_queue(513)
    rt.paths_begin_torch(renderer, rt.book1_camera(BW, BH), BW, BH, 1, BSPP, 0, 0, 513, Q)
    torch.cuda.synchronize()
    got = host(Q)
    q = {f: got[f].copy() for f in U32_FIELDS + F64_FIELDS}
    assert all(np.array_equal(bits(q[f]) if f in F64_FIELDS else q[f], bits(book_queue()[f]) if f in F64_FIELDS else book_queue()[f])
               for f in U32_FIELDS + F64_FIELDS)
    assert not (q["event"] & np.uint32(nr.DIRECT)).any()                         # rt_paths_begin_device never sets the bit
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["n_lights_0", "no_direct"])
@pytest.mark.parametrize("which", ["hand", "book"])
def test_nee_step_without_direct_lighting_is_the_lit_step(renderer, oracle_mod, which, how):
    """With n_lights == 0, or with RT_STEP_NO_DIRECT, on a queue without DIRECT bits: every output of rt_paths_step_nee_device -- `out`, `in`
    as the step leaves it, both scratch arrays, the sums, d_rays -- is rt_paths_step_lit_device's on the same input, byte for byte."""
    if which == "hand":
        flat, q, light, lights = nr.hand_queue()
        q = {f: np.array(q[f], copy=True) for f in pr.FIELDS}
        q["event"] &= np.uint32(0x7FFFFFFF)
        seed, npix = nr.SEED, nr.HAND_NPIX
        renderer.upload_scene(flat)
    else:
        flat, light, _ = lr.book_case()
        lights, seed, npix = nr.light_list(light.emission), 1, BW * BH
        renderer.upload_scene(flat)
        q = begun_book_queue(renderer)
    A0, B0, fix0, rays0, _ = run_nee_step(renderer, q, 600, npix, light, False, seed=seed)
    A1, B1, fix1, rays1, shadow = run_nee_step(renderer, q, 600, npix, light, () if how == "n_lights_0" else lights, no_direct=how == "no_direct", seed=seed)
    same_bytes(B1, B0, "out")
    same_bytes(A1, A0, "in")
    assert np.array_equal(fix1, fix0) and rays1 == rays0 == 5 + 513 and shadow == 11
    assert 0 < int(host(B0)["count"][0]) < 513


@pytest.mark.gpu
def test_nee_changes_what_is_added_never_where_paths_go(renderer, oracle_mod):
    """With lights, on the book-scene queue: every queue array and d_rays after the step equal the lit step's except bit 31 of `event`, and
    the sums differ."""
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    q = begun_book_queue(renderer)
    A0, B0, fix0, rays0, _ = run_nee_step(renderer, q, 600, BW * BH, light, False, seed=1)
    A1, B1, fix1, rays1, shadow = run_nee_step(renderer, q, 600, BW * BH, light, True, seed=1)
    assert rays1 == rays0 and shadow > 11
    bit = np.int32(-(1 << 31))
    assert ((B1.event.cpu().numpy() ^ B0.event.cpu().numpy()) & ~bit == 0).all() and ((A1.event.cpu().numpy() ^ A0.event.cpu().numpy()) & ~bit == 0).all()
    m = int(host(B1)["count"][0])
    assert (host(B1)["event"][:m] & np.uint32(nr.DIRECT)).any()
    for X1, X0 in ((A1, A0), (B1, B0)):
        X1.event &= 0x7FFFFFFF
        X0.event &= 0x7FFFFFFF
        same_bytes(X1, X0, "every array but bit 31 of event")
    assert not np.array_equal(fix1, fix0)


# ---- the whole frame -----------------------------------------------------------------------------------------------------------------------

def nee_device_frame(renderer, cam, p, L, direct=True):
    torch, dev = torch_dev()
    d_fix = torch.full((p.height, p.width, 3), -1, dtype=torch.int64, device=dev)
    d_rays = torch.full((1,), -1, dtype=torch.int64, device=dev)
    d_shadow = torch.full((1,), -1, dtype=torch.int64, device=dev)
    renderer.render_wavefront_device(cam, p, d_fix.data_ptr(), d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream, lighting=L, direct=direct,
                                     d_shadow_rays_ptr=d_shadow.data_ptr())
    torch.cuda.synchronize()
    return u64(d_fix), int(d_rays.item()), int(d_shadow.item())


@pytest.mark.gpu
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_nee_frames_equal_the_statement(oracle_mod, monkeypatch, max_depth):
    """lights_ref.book_case() -- the book scene under a dim sky, lit by the large Lambertian sphere and five small ones -- with direct
    lighting: the host form, the device form, and both again after the batch has been regrown.  rays_traced is the lit frame's."""
    torch, dev = torch_dev()
    flat, light, _ = lr.book_case()
    want, want_rays, want_shadow = nr.book_frame(max_depth)
    assert want_rays == lr.book_frame(max_depth)[1] and (want_shadow > 0) == (max_depth > 1)
    assert max_depth == 1 or not np.array_equal(want, lr.book_frame(max_depth)[0])
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    with rt.Renderer(0) as r:                                                    # (a context of its own: the first frame allocates its queues)
        r.upload_scene(flat)
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "257")
        fix, rays, st = r.render_wavefront(cam, p, lighting=lighting_of(light), direct=True)
        assert np.array_equal(fix, want) and rays == want_rays and st == {"rays_traced": want_rays, "shadow_rays": want_shadow}, "host form"
        fix, rays, shadow = nee_device_frame(r, cam, p, lighting_of(light, dev))
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form"
        lit_fix, lit_rays = r.render_wavefront(cam, p, lighting=lighting_of(light))
        assert lit_rays == rays
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "1000")
        fix, rays, st = r.render_wavefront(cam, p, lighting=lighting_of(light), direct=True)
        assert np.array_equal(fix, want) and rays == want_rays and st["shadow_rays"] == want_shadow, "regrown batch"
        fix, rays, shadow = nee_device_frame(r, cam, p, lighting_of(light), direct=nr.light_list(light.emission))
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form, regrown batch, the list given"


def shell_scene():
    """wavefront_ref.step_scene() on a Lambertian ground, and two lights each inside an opaque Lambertian shell."""
    flat = np.zeros(10, dtype=rt.SPHERE_DTYPE)
    flat[:5] = wr.step_scene()
    more = [((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5)), ((0.0, 1.0, 4.0), 0.3, (0.5, 0.5, 0.5)), ((0.0, 1.0, 4.0), 0.6, (0.8, 0.6, 0.4)),
            ((-3.0, 4.0, -2.0), 0.5, (0.5, 0.5, 0.5)), ((-3.0, 4.0, -2.0), 0.75, (0.3, 0.6, 0.9))]
    for k, (centre, radius, albedo) in enumerate(more, start=5):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["kind"] = centre, radius, albedo, wr.LAMBERTIAN
    return flat, {6: (5.0, 4.0, 3.0), 8: (1.0, 8.0, 2.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("sky", [((0, 0, 0), (0, 0, 0)), lr.HAND_SKY], ids=["black_sky", "hand_sky"])
def test_lights_inside_opaque_shells_leave_the_lit_frame(renderer, oracle_mod, sky):
    """Every light sits inside a Lambertian shell: no path and no shadow ray reaches one, so the NEE frame is the lit frame bit for bit
    (under the black sky: black) although shadow rays are traced."""
    flat, emit = shell_scene()
    renderer.upload_scene(flat)
    w, h, spp = 33, 17, 3
    cam = rt.Camera((9.0, 3.0, 8.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0, w / h, 0.05, 10.0)
    p = rt.make_params(w, h, spp, max_depth=6, seed=7)
    L = rt.Lighting(sky[0], sky[1], emit)
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=L)
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True)
    assert np.array_equal(fix, lit) and rays == lit_rays and st["shadow_rays"] > 0
    assert fix.any() == (sky[0] != (0, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["none", "zeros", "negative_nan"])
def test_a_frame_without_lights_is_the_lit_frame(renderer, oracle_mod, table):
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=50, seed=1)
    emission = lr.dark_tables(len(flat))[table]
    emission = None if emission is None else np.where(np.isfinite(emission) & (emission > 0), emission, 0.0)     # (what the host form accepts)
    L = rt.Lighting(light.sky_bottom, light.sky_top, emission)
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=L)
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True)
    assert np.array_equal(fix, lit) and fix.any() and rays == lit_rays and st["shadow_rays"] == 0
    torch, dev = torch_dev()
    dark = lr.dark_tables(len(flat))[table]                                      # the device form validates no table: NaN and negative entries pass
    Ld = rt.Lighting(light.sky_bottom, light.sky_top, None if dark is None else torch.from_numpy(np.array(dark)).to(dev))
    fix, rays, shadow = nee_device_frame(renderer, cam, p, Ld)
    assert np.array_equal(fix, lit) and rays == lit_rays and shadow == 0


@pytest.mark.gpu
def test_depth_one_is_the_lit_frame(renderer, oracle_mod):
    """max_depth = 1: the only step is the last one and runs with RT_STEP_NO_DIRECT."""
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=1, seed=1)
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=lighting_of(light))
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=lighting_of(light), direct=True)
    assert np.array_equal(fix, lit) and fix.any() and rays == lit_rays == BW * BH * BSPP and st["shadow_rays"] == 0


# ---- the same expectation, less variance ---------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def stat_frames():
    """The stat scene with each of the 16 seeds, NEE and lit -> (frames NEE, frames lit), rendered once."""
    flat, light = nr.stat_scene()
    cam = nr.stat_camera()
    nee, lit = [], []
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        L = lighting_of(light)
        for seed in nr.STAT_SEEDS:
            p = rt.make_params(nr.STAT_W, nr.STAT_H, nr.STAT_SPP, max_depth=nr.STAT_DEPTH, seed=seed)
            fix, rays, st = r.render_wavefront(cam, p, lighting=L, direct=True)
            fix_lit, rays_lit = r.render_wavefront(cam, p, lighting=L)
            assert rays == rays_lit and st["shadow_rays"] > 0
            nee.append(fix)
            lit.append(fix_lit)
    return nee, lit


@pytest.mark.gpu
def test_nee_and_lit_frames_have_the_same_expectation(oracle_mod):
    """A Lambertian ground, one small light, a Metal, a Dialectric and an occluder under a black sky, 16 x 12 pixels, 64 spp, depth 8, 16
    fixed seeds.  No sample can reach the 2^16 clamp (nee_ref.stat_sample_bound, from the statement's formula), so the u64 sums are
    unbiased for both estimators.  Per seed the frame-total energy of NEE minus lit: |mean| <= 5 standard errors of the 16 differences."""
    assert nr.stat_sample_bound() < 65536.0 / 1000.0
    nee, lit = stat_frames()
    mean, stderr, var_nee, var_lit = nr.stat_numbers(nee, lit)
    print(f"energy NEE - lit: mean {mean:.6g}, standard error {stderr:.6g}, |mean| / stderr {abs(mean) / stderr:.3f}")
    assert stderr > 0.0 and all(f.any() for f in nee) and all(f.any() for f in lit)
    assert abs(mean) <= 5.0 * stderr


@pytest.mark.gpu
def test_nee_has_less_variance_than_the_random_walk(oracle_mod):
    """On the same 16 seeds: the per-pixel variance over the seeds, summed over the frame, of NEE is strictly below lit's (the ratio is
    in profiles/nee.txt; the light subtends a small solid angle, so it is large)."""
    nee, lit = stat_frames()
    _, _, var_nee, var_lit = nr.stat_numbers(nee, lit)
    print(f"variance lit {var_lit:.6g}, NEE {var_nee:.6g}, lit / NEE {var_lit / var_nee:.3f}")
    assert 0.0 < var_nee < var_lit


# ---- context rules, the command line -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rejections_that_need_the_context(oracle_mod, book1_flat):
    """No scene (after the lighting and the direct checks); a table of another length; a list longer than the uploaded scene."""
    torch, dev = torch_dev()
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, seed=1)
    with rt.Renderer(0) as r:
        A, B = device_queue(64, count=7), device_queue(64)
        fix = torch.full((BH, BW, 3), 3, dtype=torch.int64, device=dev)
        shadow = torch.full((1,), 9, dtype=torch.int64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting(), direct=[0], shadow_rays=shadow)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_wavefront(cam, p, lighting=rt.Lighting(), direct=True)
        r.upload_scene(book1_flat)
        n = len(book1_flat)
        wrong = torch.zeros((n + 1, 3), dtype=torch.float64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*uploaded sphere count"):
            rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting(emission=wrong), direct=[0], shadow_rays=shadow)
        table = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        too_many = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        with pytest.raises(rt.RtiowHipError, match=rf"\(-1\).*rt_paths_step_nee.*n_lights \({n + 1}\) must be <= the uploaded sphere count \({n}\)"):
            rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting(emission=table), direct=too_many, shadow_rays=shadow)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_render_wavefront_nee.*n_lights"):
            r.render_wavefront_device(cam, p, fix.data_ptr(), lighting=rt.Lighting(emission=table), direct=too_many, d_shadow_rays_ptr=shadow.data_ptr())
        with pytest.raises(ValueError, match="needs a Lighting"):
            r.render_wavefront(cam, p, direct=True)
        torch.cuda.synchronize()
        assert (fix == 3).all() and int(shadow.item()) == 9 and int(host(A)["count"][0]) == 7 and int(host(B)["count"][0]) == pr.SENTINEL_U32
        r.render(cam, p)
        before = r.last_stats()
        r.render_wavefront(cam, rt.make_params(BW, BH, 2, seed=9), lighting=rt.Lighting(emission={0: (1, 1, 1)}), direct=True)
        assert r.last_stats() == before                                          # no launch slot is taken


@pytest.mark.gpu
def test_cpp_cli_direct_writes_the_bytes_the_python_path_resolves(renderer, oracle_mod, tmp_path):
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
    run = subprocess.run(base + ["--wavefront", "--direct"] + lit, check=True, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, RTIOW_WAVEFRONT_BATCH="4000"))
    renderer.upload_scene(flat)
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {big: (4, 3.2, 2.4), small: (8, 2, 1)})
    fix, _, st = renderer.render_wavefront(rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=4), lighting=L, direct=True)
    want = renderer.resolve_rgba8(fix, spp, flip=True)[:, :, :3]
    assert np.array_equal(rt.read_ppm(out), want) and want.any()
    assert f"shadow rays: {st['shadow_rays']}" in run.stderr
    lit_fix, _ = renderer.render_wavefront(rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=4), lighting=L)
    assert not np.array_equal(renderer.resolve_rgba8(lit_fix, spp, flip=True)[:, :, :3], want)
    for args in (["--direct"] + lit, ["--wavefront", "--direct"], ["--wavefront", "--direct"] + lit[:2]):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2, (args, bad.returncode, bad.stderr)
