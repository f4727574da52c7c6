"""Direct lighting with a weighted choice of the light on the GPU (RT_DIRECT_WEIGHTED | RT_DIRECT_CONE: rt_paths_step_nee_device,
rt_render_wavefront_nee_device, rt_render_wavefront_nee_sampled) against tests/weighted_ref.py, everything bit for
bit: doubles as u64 patterns, the 32-bit words, the live counts, the u64 sums, both ray counts.  Against the cone step every queue array
is compared byte for byte: the choice changes only the sums and the shadow count.  Frames with one light are the cone frames, frames
whose lights cannot be reached are the lit frames, and the eight-light scene is rendered with 16 seeds: the same expectation as the
random walk and as the uniform choice, at strictly less variance than the uniform choice."""
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
import test_gpu_cone as tgc
import test_gpu_nee as tgn
import weighted_ref as wt
from test_gpu_lights import lighting_of, same_bytes
from test_gpu_paths import COUNTS, F64_FIELDS, U32_FIELDS, check_queue, host, set_knob, torch_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, BSPP = lr.BW, lr.BH, lr.BSPP


# ---- rt_paths_step_nee_device with RT_DIRECT_WEIGHTED | RT_DIRECT_CONE ---------------------------------------------------------------------

def run_step(renderer, q, capacity, npix, light, direct, **kw):
    """test_gpu_cone.run_step with sampling="weighted" unless told otherwise."""
    kw.setdefault("sampling", "weighted")
    kw.setdefault("seed", wt.SEED)
    return tgc.run_step(renderer, q, capacity, npix, light, direct, **kw)


def check_step(renderer, count, capacity, what, lights=wt.LIGHTS, **kw):
    flat, q, light, _ = wt.hand_queue()
    out, adds, live, shadow = wt.hand_step(count, lights=lights)
    A, B, fix, rays, got_shadow = run_step(renderer, pr.prefix(q, count), capacity, wt.HAND_NPIX, light, lights, **kw)
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
def test_weighted_step_on_the_hand_queue(renderer, oracle_mod, monkeypatch, count, capacity, blocks):
    """A hit point inside one light while another is chosen, the first and the last positive entry of the list chosen, entries that name
    no sphere, no emitter and a light of NaN weight walked over, a sample below the horizon, a blocked ray, disk tries accepted first and
    in a later block, a light's inner face behind t_min, DIRECT paths on a light's two faces; a wave whose 64 lanes all trace a shadow
    ray, waves where none does, one where only lane 63 does (tests/test_weighted_host.py proves each with the statement)."""
    set_knob(monkeypatch, blocks)
    renderer.upload_scene(wt.hand_queue()[0])
    check_step(renderer, count, capacity, f"weighted hand queue, {count} of {capacity}")


@pytest.mark.gpu
def test_weighted_step_where_no_light_can_contribute(renderer, oracle_mod):
    """The list (no sphere, light 19, no emitter): slot 1's hit point lies inside light 19, so tot = 0 there -- no ray, the bit set --, and
    every other Lambertian hit chooses the one positive entry, in the middle of the list, and finds it below its horizon."""
    renderer.upload_scene(wt.hand_queue()[0])
    check_step(renderer, wt.HAND_N, 513, "the inner list", lights=wt.INNER_LIGHTS)
    check_step(renderer, 2, 513, "the inner list, slots 0 and 1", lights=wt.INNER_LIGHTS)


@pytest.mark.gpu
@pytest.mark.parametrize("form,side", [("device", True), ("torch", True), ("device", False)], ids=["device_side_stream", "torch_side_stream", "device"])
def test_weighted_step_forms_and_streams(renderer, oracle_mod, form, side):
    renderer.upload_scene(wt.hand_queue()[0])
    check_step(renderer, wt.HAND_N, 513, f"{form} form, side stream {side}", form=form, side_stream=side)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}], ids=["no_grid", "grid_dim_9"])
def test_weighted_step_under_the_scene_knobs(oracle_mod, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rt.Renderer(0) as r:
        r.upload_scene(wt.hand_queue()[0])                                       # RTIOW_NO_GRID / RTIOW_GRID_DIM are read here
        check_step(r, wt.HAND_N, 513, f"weighted hand queue under {env}")


@pytest.mark.gpu
def test_weighted_step_with_no_direct_against_the_statement(renderer, oracle_mod):
    """RT_STEP_NO_DIRECT on the hand queue, DIRECT bits and all: no light sample, no bit set, the front faces still not counted again."""
    flat, q, light, lights = wt.hand_queue()
    renderer.upload_scene(flat)
    out, adds, live, shadow = wt.hand_step(wt.HAND_N, no_direct=True)
    assert shadow == 0 and not (out["event"] & np.uint32(nr.DIRECT)).any()
    A, B, fix, rays, got_shadow = run_step(renderer, q, 600, wt.HAND_NPIX, light, lights, no_direct=True)
    check_queue(B, out, "NO_DIRECT")
    assert np.array_equal(fix, adds) and rays == 5 + live and got_shadow == 11


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hand", "book"])
def test_the_choice_changes_what_is_added_never_where_paths_go(renderer, oracle_mod, which):
    """On the hand queue and on a book-scene queue from rt_paths_begin_device: every queue array -- `out`, `in` as the step leaves it,
    both scratch arrays -- and d_rays equal the cone step's byte for byte; only the sums and the shadow count differ."""
    if which == "hand":
        flat, q, light, lights = wt.hand_queue()
        seed, npix, direct = wt.SEED, wt.HAND_NPIX, lights
        renderer.upload_scene(flat)
    else:
        flat, light, _ = lr.book_case()
        seed, npix, direct = 1, BW * BH, True
        renderer.upload_scene(flat)
        q = tgn.begun_book_queue(renderer)
    A0, B0, fix0, rays0, shadow0 = run_step(renderer, q, 600, npix, light, direct, seed=seed, sampling="cone")
    A1, B1, fix1, rays1, shadow1 = run_step(renderer, q, 600, npix, light, direct, seed=seed)
    same_bytes(B1, B0, "out")
    same_bytes(A1, A0, "in")
    assert rays1 == rays0 == 5 + 513 and 0 < int(host(B1)["count"][0]) < 513
    assert (host(B1)["event"][:int(host(B1)["count"][0])] & np.uint32(nr.DIRECT)).any()
    print(f"{which}: shadow rays cone {shadow0 - 11}, weighted {shadow1 - 11}")
    assert not np.array_equal(fix1, fix0) and shadow1 > 11 and shadow0 > 11
    assert which != "hand" or shadow1 > shadow0                                  # (no sample lost on an entry that can give nothing)


@pytest.mark.gpu
@pytest.mark.parametrize("one", [14, 20, 19])
def test_with_one_light_the_step_is_the_cone_step(renderer, oracle_mod, one):
    """A list of one valid light -- far, 5e-5 from a hit point, holding a hit point (and below every other one's horizon: no ray either way) --: tot / imp_j is exactly 1.0 and every output of the
    weighted step is the cone step's, byte for byte: the queues, the sums, d_rays, the shadow count."""
    flat, q, light, _ = wt.hand_queue()
    renderer.upload_scene(flat)
    A0, B0, fix0, rays0, shadow0 = run_step(renderer, q, 513, wt.HAND_NPIX, light, (one,), sampling="cone")
    A1, B1, fix1, rays1, shadow1 = run_step(renderer, q, 513, wt.HAND_NPIX, light, (one,))
    same_bytes(B1, B0, "out")
    same_bytes(A1, A0, "in")
    assert np.array_equal(fix1, fix0) and fix1.any() and rays1 == rays0 and shadow1 == shadow0 and (shadow1 > 11) == (one != 19)


# ---- the whole frame -----------------------------------------------------------------------------------------------------------------------

def device_frame(renderer, cam, p, L, direct=True, sampling="weighted"):
    return tgc.device_frame(renderer, cam, p, L, direct=direct, sampling=sampling)


@pytest.mark.gpu
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_weighted_frames_equal_the_statement(oracle_mod, monkeypatch, max_depth):
    """lights_ref.book_case() -- the book scene under a dim sky, lit by the large Lambertian sphere and five small ones -- with the light
    chosen by its contribution: the host form, the device form, and both again at another batch size.  rays_traced is the lit frame's."""
    torch, dev = torch_dev()
    flat, light, _ = lr.book_case()
    want, want_rays, want_shadow = wt.book_frame(max_depth)
    assert want_rays == lr.book_frame(max_depth)[1] and (want_shadow > 0) == (max_depth > 1)
    assert max_depth == 1 or (not np.array_equal(want, lr.book_frame(max_depth)[0]) and not np.array_equal(want, cr.book_frame(max_depth)[0]))
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    with rt.Renderer(0) as r:                                                    # (a context of its own: the first frame allocates its queues)
        r.upload_scene(flat)
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "257")
        fix, rays, st = r.render_wavefront(cam, p, lighting=lighting_of(light), direct=True, sampling="weighted")
        assert np.array_equal(fix, want) and rays == want_rays and st == {"rays_traced": want_rays, "shadow_rays": want_shadow}, "host form"
        fix, rays, shadow = device_frame(r, cam, p, lighting_of(light, dev))
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form"
        lit_fix, lit_rays = r.render_wavefront(cam, p, lighting=lighting_of(light))
        assert lit_rays == rays
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "1000")
        fix, rays, shadow = tgc._sampled(r, cam, p, lighting_of(light), 10)
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "the C entry point, another batch"
        fix, rays, shadow = device_frame(r, cam, p, lighting_of(light), direct=nr.light_list(light.emission))
        assert np.array_equal(fix, want) and rays == want_rays and shadow == want_shadow, "device form, another batch, the list given"


@pytest.mark.gpu
def test_with_one_light_the_frame_is_the_cone_frame(renderer, oracle_mod):
    """The book scene at night lit by its large sphere alone, and by one small sphere alone: host and device form, sums and both counts."""
    torch, dev = torch_dev()
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=6, seed=5)
    for s in nr.light_list(light.emission)[:2]:
        L = rt.Lighting((0, 0, 0), (0, 0, 0), {s: tuple(light.emission[s])})
        cone, cone_rays, cone_st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
        fix, rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="weighted")
        assert np.array_equal(fix, cone) and fix.any() and rays == cone_rays and st == cone_st and st["shadow_rays"] > 0, s
        table = torch.zeros((len(flat), 3), dtype=torch.float64, device=dev)
        table[s] = torch.tensor(tuple(light.emission[s]), dtype=torch.float64)
        fix, rays, shadow = device_frame(renderer, cam, p, rt.Lighting((0, 0, 0), (0, 0, 0), table))
        assert np.array_equal(fix, cone) and rays == cone_rays and shadow == cone_st["shadow_rays"], s


@pytest.mark.gpu
@pytest.mark.parametrize("sky", [((0, 0, 0), (0, 0, 0)), lr.HAND_SKY], ids=["black_sky", "hand_sky"])
def test_lights_inside_opaque_shells_leave_the_lit_frame(renderer, oracle_mod, sky):
    """Every light sits inside a Lambertian shell: no path and no shadow ray reaches one, so the weighted frame is the lit frame bit for
    bit (under the black sky: black) although shadow rays are traced."""
    flat, emit = tgn.shell_scene()
    renderer.upload_scene(flat)
    w, h, spp = 33, 17, 3
    cam = rt.Camera((9.0, 3.0, 8.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0, w / h, 0.05, 10.0)
    p = rt.make_params(w, h, spp, max_depth=6, seed=7)
    L = rt.Lighting(sky[0], sky[1], emit)
    lit, lit_rays = renderer.render_wavefront(cam, p, lighting=L)
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="weighted")
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
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="weighted")
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
    fix, rays, st = renderer.render_wavefront(cam, p, lighting=lighting_of(light), direct=True, sampling="weighted")
    assert np.array_equal(fix, lit) and fix.any() and rays == lit_rays == BW * BH * BSPP and st["shadow_rays"] == 0


# ---- the eight-light scene: the same expectation, less variance than the uniform choice ----------------------------------------------------

@functools.lru_cache(None)
def many_light_frames():
    """-> (frames weighted, cone, lit at depth 8, one per seed; the indirect pixels from the lit frames at depth 1; shadow rays weighted, cone)."""
    flat, light = wt.many_light_scene()
    cam = nr.stat_camera()
    weighted, cone, lit, first, n_weighted, n_cone = [], [], [], [], 0, 0
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        L = lighting_of(light)
        for seed in wt.MANY_SEEDS:
            p = rt.make_params(wt.MANY_W, wt.MANY_H, wt.MANY_SPP, max_depth=wt.MANY_DEPTH, seed=seed)
            fix, rays, st = r.render_wavefront(cam, p, lighting=L, direct=True, sampling="weighted")
            fix_cone, rays_cone, st_cone = r.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
            fix_lit, rays_lit = r.render_wavefront(cam, p, lighting=L)
            assert rays == rays_cone == rays_lit and st["shadow_rays"] > 0 and st_cone["shadow_rays"] > 0
            p1 = rt.make_params(wt.MANY_W, wt.MANY_H, wt.MANY_SPP, max_depth=1, seed=seed)
            first.append(r.render_wavefront(cam, p1, lighting=L)[0])
            weighted.append(fix)
            cone.append(fix_cone)
            lit.append(fix_lit)
            n_weighted += st["shadow_rays"]
            n_cone += st_cone["shadow_rays"]
    return weighted, cone, lit, wt.indirect_pixels(first), n_weighted, n_cone


@pytest.mark.gpu
@pytest.mark.parametrize("other", ["lit", "cone"])
def test_many_lights_weighted_has_the_expectation_of(oracle_mod, other):
    """Eight small lights on a Lambertian ground under a black sky, 16 x 12 pixels, 64 spp, depth 8, 16 fixed seeds.  Per seed the energy
    of weighted minus lit (minus cone), over the pixels that see no light directly and over the whole frame: |mean| <= 5 standard errors
    of the 16 differences (the statement alone, indirect pixels: 0.70 against lit, 1.95 against cone)."""
    weighted, cone, lit, mask, n_weighted, n_cone = many_light_frames()
    frames = lit if other == "lit" else cone
    assert all(f.any() for f in weighted) and all(f.any() for f in frames) and 100 < int(mask.sum()) < wt.MANY_W * wt.MANY_H
    for where, m in (("indirect pixels", mask), ("whole frame", np.ones_like(mask))):
        mean, stderr, _, _, _, _ = wt.many_numbers(weighted, frames, m)
        print(f"energy weighted - {other}, {where} ({int(m.sum())}): mean {mean:.6g}, standard error {stderr:.6g}, |mean| / stderr {abs(mean) / stderr:.3f}; "
              f"shadow rays cone {n_cone}, weighted {n_weighted}")
        assert stderr > 0.0 and abs(mean) <= 5.0 * stderr, where


@pytest.mark.gpu
def test_many_lights_weighted_has_less_variance_than_cone(oracle_mod):
    """On the same 16 seeds: the per-pixel variance over the seeds, summed over the pixels that see no light directly, of the weighted
    choice is strictly below the uniform choice's on the GPU's own cone frames (the statement alone: 5 294 against 19 964)."""
    weighted, cone, lit, mask, _, _ = many_light_frames()
    _, _, var_w, var_cone, all_w, all_cone = wt.many_numbers(weighted, cone, mask)
    _, _, _, var_lit, _, all_lit = wt.many_numbers(weighted, lit, mask)
    print(f"variance on {int(mask.sum())} indirect pixels: lit {var_lit:.6g}, cone {var_cone:.6g}, weighted {var_w:.6g}, cone / weighted {var_cone / var_w:.3f}; "
          f"whole frame: lit {all_lit:.6g}, cone {all_cone:.6g}, weighted {all_w:.6g}")
    assert 0.0 < var_w < var_cone


@pytest.mark.gpu
def test_many_lights_no_sample_can_reach_the_clamp(oracle_mod):
    """Every pixel sum is <= spp * depth * weighted_sample_bound() on the 2^-32 grid (a path adds at most once per step, each time at most
    the bound, its throughput never above 1), and no single sample reaches the 2^16 clamp: the u64 sums are unbiased."""
    weighted, _, _, _, _, _ = many_light_frames()
    bound = wt.weighted_sample_bound()
    assert bound == 432.0 < 65536.0
    limit = int(wt.MANY_SPP * wt.MANY_DEPTH * bound * 4294967296.0)
    assert all(int(f.max()) <= limit for f in weighted)


# ---- the command line ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cpp_cli_direct_weighted_writes_the_bytes_the_python_path_resolves(renderer, oracle_mod, tmp_path):
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
    run = subprocess.run(base + ["--wavefront", "--direct-weighted"] + lit, check=True, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, RTIOW_WAVEFRONT_BATCH="4000"))
    renderer.upload_scene(flat)
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {big: (4, 3.2, 2.4), small: (8, 2, 1)})
    cam, p = rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=4)
    fix, _, st = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="weighted")
    want = renderer.resolve_rgba8(fix, spp, flip=True)[:, :, :3]
    assert np.array_equal(rt.read_ppm(out), want) and want.any()
    assert f"shadow rays: {st['shadow_rays']}" in run.stderr
    cone_fix, _, _ = renderer.render_wavefront(cam, p, lighting=L, direct=True, sampling="cone")
    assert not np.array_equal(cone_fix, fix)
    for args in (["--direct-weighted"] + lit, ["--wavefront", "--direct-weighted"], ["--wavefront", "--direct-weighted"] + lit[:2],
                 ["--wavefront", "--direct", "--direct-weighted"] + lit, ["--wavefront", "--direct-cone", "--direct-weighted"] + lit):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2, (args, bad.returncode, bad.stderr)
