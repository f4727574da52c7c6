"""The lit path queue on the GPU (rt_paths_step_lit_device, rt_render_wavefront_lit*) against tests/lights_ref.py,
everything bit for bit: doubles as u64 patterns, the 32-bit words, the live counts, the u64 sums, the ray counts.  Where lighting changes
nothing the lit forms are compared with the unlit ones byte for byte: that is what catches a lit kernel that has drifted from the unlit
one.  Three frames have answers that need no statement at all, and one is integrated a second time from the separate path steps."""
import functools
import os
import subprocess

import numpy as np
import pytest

import lights_ref as lr
import paths_ref as pr
import rtiow_amd as rt
import wavefront_ref as wr
from test_gpu_paths import COUNTS, F64_FIELDS, U32_FIELDS, bits, check_queue, device_queue, host, set_knob, torch_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, BSPP = lr.BW, lr.BH, lr.BSPP


def lighting_of(light, dev=None):
    """lights_ref.Light -> rt.Lighting; dev: the emission as a tensor on that device (what the device forms take)."""
    emission = light.emission
    if emission is not None and dev is not None:
        import torch
        emission = torch.from_numpy(np.array(emission)).to(dev)
    return rt.Lighting(light.sky_bottom, light.sky_top, emission)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- rt_paths_step_lit_device --------------------------------------------------------------------------------------------------------------

def run_lit_step(renderer, q, capacity, npix, light, *, seed=lr.SEED, rays0=5, form="torch", side_stream=False):
    """One lit step of the numpy queue `q` -> (in, out, the sums u64 [npix, 3], d_rays).  form "device": Renderer.paths_step_device on raw
    structs and pointers; "torch": paths_step_torch."""
    torch, dev = torch_dev()
    A, B = device_queue(capacity, q), device_queue(capacity)
    fix = torch.zeros((npix, 3), dtype=torch.int64, device=dev)
    rays = torch.full((1,), rays0, dtype=torch.int64, device=dev)
    L = lighting_of(light, dev) if light is not None else None
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        if form == "torch":
            rt.paths_step_torch(renderer, seed, A, B, fix, rays, lighting=L)
        else:
            renderer.paths_step_device(seed, A.struct(), B.struct(), fix.data_ptr(), npix, rays.data_ptr(), 1e-4, stream.cuda_stream, lighting=L)
    stream.synchronize()
    torch.cuda.synchronize()
    return A, B, u64(fix), int(rays.item())


def check_lit_step(renderer, count, capacity, what, **kw):
    flat, q, light = lr.hand_queue()
    out, adds, live = lr.hand_step(count)
    A, B, fix, rays = run_lit_step(renderer, pr.prefix(q, count), capacity, lr.HAND_NPIX, light, **kw)
    check_queue(B, out, what)
    assert np.array_equal(fix, adds), what
    assert rays == 5 + live, (what, rays)
    got = host(A)
    assert int(got["count"][0]) == count                                        # *in->count is unchanged
    assert all((got[f][count:] == pr.SENTINEL_U32).all() for f in U32_FIELDS) and all((got[f][count:] == pr.SENTINEL_F64).all() for f in F64_FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["", "1"], ids=["grid", "one_block"])
@pytest.mark.parametrize("capacity", [513, 1024])
@pytest.mark.parametrize("count", COUNTS)
def test_lit_step_on_the_hand_queue(renderer, oracle_mod, monkeypatch, count, capacity, blocks):
    """Lights hit on either face, of every material, outside the frame, above the clamp, with negative and NaN channels, tied with a
    sphere that is none; entries that light nothing; a wave that ends on lights whole and one where none does; the hand sky."""
    set_knob(monkeypatch, blocks)
    renderer.upload_scene(lr.hand_queue()[0])
    check_lit_step(renderer, count, capacity, f"lit hand queue, {count} of {capacity}")


@pytest.mark.gpu
@pytest.mark.parametrize("form,side", [("device", True), ("torch", True), ("device", False)], ids=["device_side_stream", "torch_side_stream", "device"])
def test_lit_step_forms_and_streams(renderer, oracle_mod, form, side):
    renderer.upload_scene(lr.hand_queue()[0])
    check_lit_step(renderer, lr.HAND_N, 513, f"{form} form, side stream {side}", form=form, side_stream=side)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}], ids=["no_grid", "grid_dim_9"])
def test_lit_step_under_the_scene_knobs(oracle_mod, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rt.Renderer(0) as r:
        r.upload_scene(lr.hand_queue()[0])                                       # RTIOW_NO_GRID / RTIOW_GRID_DIM are read here
        check_lit_step(r, lr.HAND_N, 513, f"lit hand queue under {env}")


def same_bytes(a, b, what):
    """Two device queues after a step: every array whole (sentinels, intermediate values and scratch included), byte for byte."""
    for f in rt.PathQueue.FIELDS:
        x, y = getattr(a, f).cpu().numpy(), getattr(b, f).cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, f)


@functools.lru_cache(None)
def book_queue():
    """The first 513 items of the golden book frame, from the statement (what rt_paths_begin_device writes: test_gpu_paths.py)."""
    import oracle
    q = pr.begin(oracle.book1_camera(BW, BH), BW, BH, 1, BSPP, 0, 0, 513)
    for a in q.values():
        a.setflags(write=False)
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["none", "zeros", "negative_nan"])
@pytest.mark.parametrize("which", ["hand", "book"])
def test_lit_step_without_lights_is_the_unlit_step(renderer, oracle_mod, book1_flat, which, table):
    """The reference's sky and a table that lights nothing: every output of rt_paths_step_lit_device -- `out`, `in` as the step leaves it,
    both scratch arrays, the sums, d_rays -- is rt_paths_step_device's on the same input, byte for byte."""
    torch, dev = torch_dev()
    if which == "hand":
        flat, q, _ = lr.hand_queue()
        seed, npix = lr.SEED, lr.HAND_NPIX
        renderer.upload_scene(flat)
    else:
        flat, seed, npix = book1_flat, 1, BW * BH
        renderer.upload_scene(flat)
        Q = device_queue(513)                                                    # the queue rt_paths_begin_device makes, read back
        rt.paths_begin_torch(renderer, rt.book1_camera(BW, BH), BW, BH, 1, BSPP, 0, 0, 513, Q)
        torch.cuda.synchronize()
        got = host(Q)
        q = {f: got[f].copy() for f in U32_FIELDS + F64_FIELDS}
        assert all(np.array_equal(bits(q[f]) if f in F64_FIELDS else q[f], bits(book_queue()[f]) if f in F64_FIELDS else book_queue()[f])
                   for f in U32_FIELDS + F64_FIELDS)
    light = lr.Light(*lr.REFERENCE_SKY, lr.dark_tables(len(flat))[table])
    A0, B0, fix0, rays0 = run_lit_step(renderer, q, 600, npix, None, seed=seed)
    A1, B1, fix1, rays1 = run_lit_step(renderer, q, 600, npix, light, seed=seed)
    same_bytes(B1, B0, "out")
    same_bytes(A1, A0, "in")
    assert np.array_equal(fix1, fix0) and (fix0.any() or which == "book") and rays1 == rays0 == 5 + 513       # (the book frame's first 513 paths all hit the ground)
    assert 0 < int(host(B0)["count"][0]) < 513


# ---- the whole frame -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["257", ""], ids=["nine_batches", "one_batch"])
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_frame_under_the_reference_lighting_equals_the_megakernel(renderer, oracle_mod, book1_flat, monkeypatch, max_depth, batch):
    """rt_render_wavefront_lit with Lighting()'s defaults on the golden frame: Renderer.render's u64 sums bit for bit, and its rays."""
    if batch:
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", batch)
    else:
        monkeypatch.delenv("RTIOW_WAVEFRONT_BATCH", raising=False)
    renderer.upload_scene(book1_flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    _, dense, st = renderer.render(cam, p)
    fix, rays = renderer.render_wavefront(cam, p, lighting=rt.Lighting())
    assert np.array_equal(fix, dense) and dense.any()
    assert rays == st["rays_traced"]
    zeros, zrays = renderer.render_wavefront(cam, p, lighting=rt.Lighting(emission=np.zeros((len(book1_flat), 3))))
    assert np.array_equal(zeros, dense) and zrays == rays


def device_frame(renderer, cam, p, L):
    torch, dev = torch_dev()
    d_fix = torch.full((p.height, p.width, 3), -1, dtype=torch.int64, device=dev)
    d_rays = torch.full((1,), -1, dtype=torch.int64, device=dev)
    renderer.render_wavefront_device(cam, p, d_fix.data_ptr(), d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream, lighting=L)
    torch.cuda.synchronize()
    return u64(d_fix), int(d_rays.item())


@pytest.mark.gpu
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_lit_frames_equal_the_statement(oracle_mod, monkeypatch, max_depth):
    """The book scene under a dim sky, lit by the large Lambertian sphere and five small ones (lights_ref.book_case: pixels lit directly
    and pixels lit only indirectly): the host form, the device form, and the host form again after the batch has been regrown."""
    torch, dev = torch_dev()
    flat, light, _ = lr.book_case()
    want, want_rays = lr.book_frame(max_depth)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    with rt.Renderer(0) as r:                                                    # (a context of its own: the first frame allocates its queues)
        r.upload_scene(flat)
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "257")
        fix, rays = r.render_wavefront(cam, p, lighting=lighting_of(light))
        assert np.array_equal(fix, want) and rays == want_rays, "host form"
        fix, rays = device_frame(r, cam, p, lighting_of(light, dev))
        assert np.array_equal(fix, want) and rays == want_rays, "device form"
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "1000")
        fix, rays = r.render_wavefront(cam, p, lighting=rt.Lighting(light.sky_bottom, light.sky_top,
                                                                    {k: tuple(e) for k, e in enumerate(light.emission) if lr.is_light(e)}))
        assert np.array_equal(fix, want) and rays == want_rays, "regrown batch, emission as a dict"
        fix, rays = device_frame(r, cam, p, lighting_of(light))                 # (a numpy table: Lighting puts it on the device)
        assert np.array_equal(fix, want) and rays == want_rays, "device form, regrown batch"


Q = lambda x: int(np.floor(np.float64(x) * 4294967296.0))                       # quantize of an exactly representable value below the clamp


@pytest.mark.gpu
def test_black_sky_without_lights_is_black(renderer, oracle_mod, book1_flat):
    renderer.upload_scene(book1_flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=50, seed=1)
    _, _, st = renderer.render(cam, p)
    fix, rays = renderer.render_wavefront(cam, p, lighting=rt.Lighting((0, 0, 0), (0, 0, 0)))
    assert not fix.any() and rays == st["rays_traced"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
def test_a_light_around_the_camera_is_all_a_frame_shows(renderer, oracle_mod, form):
    """Black sky; the camera sits inside sphere 5, far above the five others, which radiates (0.25, 0.5, 2.0) -- its back face, as every
    camera ray meets it: each channel sum is exactly spp * quantize(e_c), and one ray per sample was traced, whatever the depth."""
    torch, dev = torch_dev()
    flat = np.zeros(6, dtype=rt.SPHERE_DTYPE)
    flat[:5] = wr.step_scene()
    flat[5]["center"], flat[5]["radius"], flat[5]["albedo"], flat[5]["kind"] = (0.0, 100.0, 0.0), 5.0, (0.5, 0.5, 0.5), wr.LAMBERTIAN
    renderer.upload_scene(flat)
    w, h, spp = 33, 17, 3
    cam = rt.Camera((0.5, 100.0, 1.0), (0.0, 100.5, -1.0), (0.0, 1.0, 0.0), 70.0, w / h, 0.2, 2.0)
    p = rt.make_params(w, h, spp, max_depth=50, seed=11)
    e = (0.25, 0.5, 2.0)
    if form == "host":
        fix, rays = renderer.render_wavefront(cam, p, lighting=rt.Lighting((0, 0, 0), (0, 0, 0), {5: e}))
    else:
        fix, rays = device_frame(renderer, cam, p, rt.Lighting((0, 0, 0), (0, 0, 0), {5: e}))
    assert rays == w * h * spp
    for c in range(3):
        assert (fix[:, :, c] == spp * Q(e[c])).all(), c


@pytest.mark.gpu
def test_a_constant_sky_seen_from_above_is_that_colour(renderer, oracle_mod):
    """The camera above wavefront_ref.step_scene() looks up: no sphere is hit.  With t in (0.5, 1], 1 - t is exact and (1 - t) + t == 1, so
    for a colour c of powers of two c (1 - t) + c t == c exactly: every sum is spp * quantize(c)."""
    renderer.upload_scene(wr.step_scene())
    w, h, spp = 31, 19, 5
    cam = rt.Camera((0.0, 10.0, 0.0), (0.0, 20.0, 0.0), (0.0, 0.0, 1.0), 60.0, w / h, 0.1, 10.0)
    c = (0.5, 0.25, 2.0)
    fix, rays = renderer.render_wavefront(cam, rt.make_params(w, h, spp, max_depth=7, seed=3), lighting=rt.Lighting(c, c))
    assert rays == w * h * spp
    for k in range(3):
        assert (fix[:, :, k] == spp * Q(c[k])).all(), k


@pytest.mark.gpu
def test_a_second_statement_from_the_path_steps(renderer, oracle_mod, monkeypatch):
    """The lit book frame under the REFERENCE's sky, integrated again on the device from the separate steps: trace_rays_torch, then
    accumulate_torch with sky_dir for the misses, accumulate_torch with weight = throughput * e for the light hits, scatter_torch for
    the rest.  rt_render_wavefront_lit_device gives the same sums and the same ray count."""
    torch, dev = torch_dev()
    flat, light, _ = lr.book_case()
    renderer.upload_scene(flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=50, seed=1)
    E = torch.from_numpy(np.array(light.emission)).to(dev)
    is_light = (E > 0).any(dim=1)
    fix = torch.zeros((BH, BW, 3), dtype=torch.int64, device=dev)
    item = torch.arange(0, BW * BH * BSPP, dtype=torch.int64, device=dev)
    pixel, sample = torch.div(item, BSPP, rounding_mode="floor").to(torch.int32), (item % BSPP).to(torch.int32)
    cr = rt.camera_rays_torch(renderer, cam, BW, BH, 1, pixel, sample)
    origin, dirs, event = cr["origin"], cr["dir"], cr["event"]
    thr = torch.ones((pixel.shape[0], 3), dtype=torch.float64, device=dev)
    rays = lit_paths = 0
    for _ in range(50):
        if pixel.shape[0] == 0:
            break
        rays += int(pixel.shape[0])
        hit = rt.trace_rays_torch(renderer, origin, dirs, t_min=1e-4, want=("point", "normal", "front_face"))
        index = hit["index"]
        rt.accumulate_torch(renderer, fix, pixel, thr, sky_dir=dirs, select=(index < 0).to(torch.uint8))
        on_light = (index >= 0) & is_light[index.clamp(min=0).long()]
        lit_paths += int(on_light.sum())
        rt.accumulate_torch(renderer, fix, pixel, (thr * E[index.clamp(min=0).long()]).contiguous(), sky_dir=None, select=on_light.to(torch.uint8))
        index = torch.where(on_light, torch.full_like(index, -1), index)        # a path on a light ends: no scatter, no draw
        sc = rt.scatter_torch(renderer, 1, dirs, index, hit["point"], hit["normal"], hit["front_face"], pixel, sample, event)
        keep = torch.nonzero(sc["status"] == rt._ffi.RT_SCATTER_SCATTERED).squeeze(1)
        thr = thr[keep] * sc["attenuation"][keep]
        pixel, sample, event, origin, dirs = pixel[keep], sample[keep], event[keep], sc["out_origin"][keep], sc["out_dir"][keep]
    torch.cuda.synchronize()
    assert lit_paths > 100
    monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "700")
    got, got_rays = device_frame(renderer, cam, p, rt.Lighting(emission=E))
    assert np.array_equal(got, u64(fix)) and got_rays == rays


# ---- context rules, the command line -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rejections_that_need_the_context(oracle_mod, book1_flat):
    """A table of another length than the uploaded scene; no scene at all (after the lighting checks)."""
    torch, dev = torch_dev()
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, seed=1)
    with rt.Renderer(0) as r:
        A, B = device_queue(64, count=7), device_queue(64)
        fix = torch.full((BH, BW, 3), 3, dtype=torch.int64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting())
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_wavefront(cam, p, lighting=rt.Lighting())
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*sky_top\[0\]"):
            r.render_wavefront(cam, p, lighting=rt.Lighting(sky_top=(-1, 0, 0)))
        r.upload_scene(book1_flat)
        n = len(book1_flat)
        for rows in (n - 1, n + 1):
            wrong = torch.zeros((rows, 3), dtype=torch.float64, device=dev)
            with pytest.raises(rt.RtiowHipError, match=rf"\(-1\).*n_emission \({rows}\) must be the uploaded sphere count \({n}\)"):
                rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting(emission=wrong))
            with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*uploaded sphere count"):
                r.render_wavefront_device(cam, p, fix.data_ptr(), lighting=rt.Lighting(emission=wrong))
            with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*uploaded sphere count"):
                r.render_wavefront(cam, p, lighting=rt.Lighting(emission=np.zeros((rows, 3))))
        torch.cuda.synchronize()
        assert (fix == 3).all() and int(host(A)["count"][0]) == 7 and int(host(B)["count"][0]) == pr.SENTINEL_U32
        r.render(cam, p)
        before = r.last_stats()
        r.render_wavefront(cam, rt.make_params(BW, BH, 2, seed=9), lighting=rt.Lighting())
        assert r.last_stats() == before                                          # no launch slot is taken


@pytest.mark.gpu
def test_another_scan_mode_refuses_every_lit_form(oracle_mod, book1_flat):
    torch, dev = torch_dev()
    os.environ["RTIOW_SCAN_MODE"] = "1"
    try:
        r = rt.Renderer(0)                                                       # RTIOW_SCAN_MODE is read here
    finally:
        os.environ.pop("RTIOW_SCAN_MODE")
    try:
        r.upload_scene(book1_flat)
        cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP)
        A, B = device_queue(64, count=7), device_queue(64)
        fix = torch.full((BH, BW, 3), 3, dtype=torch.int64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            rt.paths_step_torch(r, 1, A, B, fix, lighting=rt.Lighting())
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            r.render_wavefront_device(cam, p, fix.data_ptr(), lighting=rt.Lighting())
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            r.render_wavefront(cam, p, lighting=rt.Lighting())
        torch.cuda.synchronize()
        assert (fix == 3).all() and int(host(A)["count"][0]) == 7 and int(host(B)["count"][0]) == pr.SENTINEL_U32
    finally:
        r.close()


@pytest.mark.gpu
def test_cpp_cli_writes_the_bytes_the_python_path_resolves(renderer, oracle_mod, tmp_path):
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
    lit = ["--sky", "0,0,0:0.01,0.02,0.04", "--emit", f"{big}:4,3.2,2.4", "--emit", f"{small}:8,2,1"]
    subprocess.run(base + ["--wavefront"] + lit, check=True, timeout=120, env=dict(os.environ, RTIOW_WAVEFRONT_BATCH="4000"))
    renderer.upload_scene(flat)
    L = rt.Lighting((0, 0, 0), (0.01, 0.02, 0.04), {big: (4, 3.2, 2.4), small: (8, 2, 1)})
    fix, _ = renderer.render_wavefront(rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=4), lighting=L)
    want = renderer.resolve_rgba8(fix, spp, flip=True)[:, :, :3]
    assert np.array_equal(rt.read_ppm(out), want) and want.any()
    for args in (lit, lit[:2], lit[2:4]):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2 and "--wavefront" in bad.stderr
    bad = subprocess.run(base + ["--wavefront", "--emit", f"{len(flat)}:1,1,1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "spheres" in bad.stderr
