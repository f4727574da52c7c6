"""Wavefront frames over pixel lists, accumulated and adaptively sampled, on the GPU (rt_paths_begin_pixels_device,
rt_render_wavefront_pixels*, rt_render_wavefront_adaptive), everything bit for bit: the begin over a list against
tests/wavefront_adaptive_ref.py, the list frames against the dense frames the library already renders (a list render, a resumed render and
a dense render of the same samples are the same integers), the adaptive loop against Renderer.render_adaptive where the frame is unlit and
against the statement where it is lit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import nee_ref as nr
import paths_ref as pr
import rtiow_amd as rt
import wavefront_adaptive_ref as ar
import wavefront_ref as wr
from test_gpu_lights import lighting_of, u64
from test_gpu_paths import S32, check_queue, device_queue, set_knob, torch_dev
from test_wavefront_adaptive_host import BOOK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW, BH, BSPP = 32, 18, 4                                   # the golden book frame
S = ar.STAT
SW, SH = S["width"], S["height"]


def set_batch(monkeypatch, batch):
    if batch:
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", batch)
    else:
        monkeypatch.delenv("RTIOW_WAVEFRONT_BATCH", raising=False)


# ---- rt_paths_begin_pixels_device ----------------------------------------------------------------------------------------------------------

BEGIN = dict(spp=4, sample_begin=3, first_item=5)            # a first item that is no multiple of spp, samples from 3 on
NPIX = wr.CW * wr.CH
# ascending, descending, a duplicate (twice, once next to itself), entries at and past width * height: 66 entries, 264 items >= 5 + 257
BEGIN_LIST = np.array(list(range(3, 23)) + [NPIX, 7, 7, 0xFFFFFFF0] + list(range(NPIX - 1, NPIX - 21, -1)) + [7, NPIX + 9] + list(range(40, 60)),
                      dtype=np.uint32)


@functools.lru_cache(None)
def begin_reference():
    import oracle
    cam = wr.camera_cases()[0]                                # a wide lens: the lens draws matter
    assert len(BEGIN_LIST) * BEGIN["spp"] >= BEGIN["first_item"] + 257
    q = ar.begin_pixels(oracle.camera_from_host(cam), wr.CW, wr.CH, pr.SEED, BEGIN["spp"], BEGIN["sample_begin"], BEGIN["first_item"], 257, BEGIN_LIST)
    assert (q["pixel"] >= NPIX).sum() >= 8 and (np.diff(q["pixel"].astype(np.int64)) < 0).any()
    for a in q.values():
        a.setflags(write=False)
    return cam, q


def device_list(pixels):
    torch, dev = torch_dev()
    return torch.from_numpy(np.ascontiguousarray(pixels, dtype=np.uint32).view(np.int32).copy()).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["", "1"], ids=["grid", "one_block"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_begin_over_a_list_equals_the_statement(renderer, oracle_mod, monkeypatch, n, blocks):
    torch, dev = torch_dev()
    set_knob(monkeypatch, blocks)
    cam, want = begin_reference()
    Q, d_list = device_queue(300), device_list(BEGIN_LIST)
    renderer.paths_begin_pixels_device(cam, wr.CW, wr.CH, pr.SEED, BEGIN["spp"], BEGIN["sample_begin"], BEGIN["first_item"], n, d_list.data_ptr(),
                                       len(BEGIN_LIST), Q.struct())
    torch.cuda.synchronize()
    check_queue(Q, pr.prefix(want, n), f"begin over a list, n={n}")          # *count == n; the slots past n keep their bytes
    assert (Q.scratch.cpu().numpy() == S32).all()


@pytest.mark.gpu
def test_begin_over_a_list_torch_on_a_side_stream(renderer, oracle_mod):
    torch, dev = torch_dev()
    cam, want = begin_reference()
    Q, d_list = device_queue(257), device_list(BEGIN_LIST)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        rt.paths_begin_pixels_torch(renderer, cam, wr.CW, wr.CH, pr.SEED, BEGIN["spp"], BEGIN["sample_begin"], BEGIN["first_item"], 257, d_list, Q)
    side.synchronize()
    check_queue(Q, want, "begin over a list on a side stream")


@pytest.mark.gpu
def test_begin_over_the_identity_list_is_the_frames_begin(renderer, oracle_mod):
    torch, dev = torch_dev()
    cam = wr.camera_cases()[0]
    A, B = device_queue(257), device_queue(257)
    d_list = device_list(np.arange(NPIX, dtype=np.uint32))
    renderer.paths_begin_device(cam, wr.CW, wr.CH, pr.SEED, 4, 3, 5, 257, A.struct())
    renderer.paths_begin_pixels_device(cam, wr.CW, wr.CH, pr.SEED, 4, 3, 5, 257, d_list.data_ptr(), NPIX, B.struct())
    torch.cuda.synchronize()
    for f in rt.PathQueue.FIELDS:
        assert torch.equal(getattr(A, f), getattr(B, f)), f


# ---- the list frame, unlit, under the reference's sky ----------------------------------------------------------------------------------------

def book_list():
    """Half the golden frame's pixels, in no order."""
    return np.random.default_rng(5).permutation(BW * BH)[:BW * BH // 2].astype(np.uint32)


@functools.lru_cache(None)
def book_list_statement(max_depth):
    import oracle
    flat = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "book1_scene_seed1.npy"), allow_pickle=False).astype(rt.SPHERE_DTYPE))
    fix, rays, _ = ar.render_pixels(flat, oracle.book1_camera(BW, BH), BW, BH, BSPP, book_list(), max_depth=max_depth, seed=1, batch=257)
    fix.setflags(write=False)
    return fix, rays


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["257", ""], ids=["batches_of_257", "one_batch"])
@pytest.mark.parametrize("max_depth", [50, 1])
def test_unlit_list_frame_on_the_golden_book_frame(renderer, oracle_mod, book1_flat, monkeypatch, max_depth, batch):
    set_batch(monkeypatch, batch)
    renderer.upload_scene(book1_flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    pixels = book_list()
    listed = np.zeros(BW * BH, dtype=bool)
    listed[pixels] = True
    listed = listed.reshape(BH, BW)
    _, dense, st = renderer.render(cam, p)
    fix, stats = renderer.render_wavefront_pixels(cam, p, pixels)
    assert np.array_equal(fix[listed], dense[listed]) and dense[listed].any(), "listed pixels are Renderer.render's"
    assert not fix[~listed].any() and dense[~listed].any(), "unlisted pixels are zero"
    compact, _ = renderer.render_pixels(cam, p, pixels)
    scattered = np.zeros((BH * BW, 3), dtype=np.uint64)
    scattered[pixels] = compact
    assert np.array_equal(fix.reshape(-1, 3), scattered), "Renderer.render_pixels' compact result, scattered"
    want, want_rays = book_list_statement(max_depth)
    assert np.array_equal(fix, want) and stats["rays_traced"] == want_rays and stats["shadow_rays"] == 0
    assert max_depth != 1 or want_rays == len(pixels) * BSPP
    # a NULL list is the dense frame
    whole, whole_stats = renderer.render_wavefront_pixels(cam, p)
    wf, wf_rays = renderer.render_wavefront(cam, p)
    assert np.array_equal(whole, wf) and np.array_equal(whole, dense) and whole_stats["rays_traced"] == wf_rays == st["rays_traced"]
    # an empty list does nothing but the zeroing
    none, none_stats = renderer.render_wavefront_pixels(cam, p, np.zeros(0, dtype=np.uint32))
    assert not none.any() and none_stats["rays_traced"] == 0


# ---- the list frame with lights ------------------------------------------------------------------------------------------------------------

MODES = {"lit": dict(direct=False, sampling="area"), "nee": dict(direct=True, sampling="area"), "weighted": dict(direct=True, sampling="weighted")}


def dense_stat_frame(r, p, mode):
    out = r.render_wavefront(nr.stat_camera(), p, lighting=lighting_of(nr.stat_scene()[1]), **MODES[mode])
    return out[0], out[1], (out[2]["shadow_rays"] if len(out) > 2 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_list_frame_with_lights_on_the_stat_scene(renderer, oracle_mod, monkeypatch, mode):
    """Every other pixel listed; the listed pixels are the dense frame's.  Then the device form with an entry outside the frame (adds nothing,
    faults nothing) and a duplicate (doubles its pixel)."""
    torch, dev = torch_dev()
    set_batch(monkeypatch, "257")
    flat, light = nr.stat_scene()
    renderer.upload_scene(flat)
    # (4 samples per pixel; the random walk alone finds the small light so rarely that its frame is black below 16: nee_ref.STAT_SPP there)
    cam, p = nr.stat_camera(), rt.make_params(SW, SH, nr.STAT_SPP if mode == "lit" else 4, max_depth=S["max_depth"], seed=S["seed"])
    dense, dense_rays, dense_shadow = dense_stat_frame(renderer, p, mode)
    pixels = np.arange(0, SW * SH, 2, dtype=np.uint32)
    listed = np.zeros(SW * SH, dtype=bool)
    listed[pixels] = True
    listed = listed.reshape(SH, SW)
    fix, stats = renderer.render_wavefront_pixels(cam, p, pixels, lighting=lighting_of(light), **MODES[mode])
    assert np.array_equal(fix[listed], dense[listed]) and not fix[~listed].any() and dense[listed].any() and dense[~listed].any()
    assert 0 < stats["rays_traced"] < dense_rays and (stats["shadow_rays"] > 0) == (mode != "lit") and stats["shadow_rays"] <= dense_shadow
    # the device form: entries outside the frame and a duplicate
    dup = int(pixels[np.flatnonzero(fix.reshape(-1, 3)[pixels].any(axis=1))[0]])   # a listed pixel that is not black
    more = np.concatenate([pixels[:50], np.array([SW * SH, 0xFFFFFFF0, dup], dtype=np.uint32), pixels[50:], np.array([SW * SH + 3], dtype=np.uint32)])
    d_list = device_list(more)
    d_fix = torch.full((SH, SW, 3), -1, dtype=torch.int64, device=dev)
    d_rays = torch.full((1,), -1, dtype=torch.int64, device=dev)
    d_shadow = torch.full((1,), -1, dtype=torch.int64, device=dev)
    direct = MODES[mode]["direct"] or False
    renderer.render_wavefront_pixels_device(cam, p, d_list.data_ptr(), len(more), d_fix.data_ptr(), d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream,
                                            lighting=lighting_of(light, dev), direct=direct, d_shadow_rays_ptr=d_shadow.data_ptr(), sampling=MODES[mode]["sampling"])
    torch.cuda.synchronize()
    got = u64(d_fix)
    want = fix.copy().reshape(-1, 3)
    want[dup] += want[dup]                                                        # (u64: wraps as the device's adds do)
    assert np.array_equal(got.reshape(-1, 3), want) and want[dup].any()
    assert int(d_rays.item()) > stats["rays_traced"] and int(d_shadow.item()) >= stats["shadow_rays"]      # the outside paths are traced, and add nothing


@pytest.mark.gpu
def test_accumulate_resumes_a_frame(renderer, oracle_mod, monkeypatch):
    """Two calls of 2 spp at sample_begin 0 and 2, the second with the flag, are one dense NEE frame of 4 spp in sums, rays and shadow rays;
    without the flag the second call's frame is its own pass alone."""
    torch, dev = torch_dev()
    set_batch(monkeypatch, "257")
    flat, light = nr.stat_scene()
    renderer.upload_scene(flat)
    cam, L = nr.stat_camera(), lighting_of(light)
    kw = dict(max_depth=S["max_depth"], seed=S["seed"])
    dense, dense_rays, dense_shadow = dense_stat_frame(renderer, rt.make_params(SW, SH, 4, **kw), "nee")
    second, second_rays, second_shadow = dense_stat_frame(renderer, rt.make_params(SW, SH, 2, sample_begin=2, **kw), "nee")
    a, sa = renderer.render_wavefront_pixels(cam, rt.make_params(SW, SH, 2, **kw), lighting=L, direct=True)
    before = a.copy()
    b, sb = renderer.render_wavefront_pixels(cam, rt.make_params(SW, SH, 2, sample_begin=2, **kw), lighting=L, direct=True, into=a)
    assert np.array_equal(a, before)                                              # `into` is read, not written
    assert np.array_equal(b, dense) and sa["rays_traced"] + sb["rays_traced"] == dense_rays and sa["shadow_rays"] + sb["shadow_rays"] == dense_shadow
    alone, s_alone = renderer.render_wavefront_pixels(cam, rt.make_params(SW, SH, 2, sample_begin=2, **kw), lighting=L, direct=True)
    assert np.array_equal(alone, second) and np.array_equal(a + alone, dense) and (s_alone["rays_traced"], s_alone["shadow_rays"]) == (second_rays, second_shadow)
    # the device form: the three buffers are added to with the flag, zeroed without it
    d_fix = torch.from_numpy(a.view(np.int64).copy()).to(dev)
    d_rays = torch.full((1,), sa["rays_traced"], dtype=torch.int64, device=dev)
    d_shadow = torch.full((1,), sa["shadow_rays"], dtype=torch.int64, device=dev)
    p = rt.make_params(SW, SH, 2, sample_begin=2, flags=rt.RT_FLAG_ACCUMULATE, **kw)
    stream = torch.cuda.current_stream().cuda_stream
    renderer.render_wavefront_pixels_device(cam, p, 0, SW * SH, d_fix.data_ptr(), d_rays.data_ptr(), stream, lighting=lighting_of(light, dev), direct=True,
                                            d_shadow_rays_ptr=d_shadow.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(u64(d_fix), dense) and int(d_rays.item()) == dense_rays and int(d_shadow.item()) == dense_shadow
    p.flags = 0
    renderer.render_wavefront_pixels_device(cam, p, 0, SW * SH, d_fix.data_ptr(), d_rays.data_ptr(), stream, lighting=lighting_of(light, dev), direct=True,
                                            d_shadow_rays_ptr=d_shadow.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(u64(d_fix), second) and int(d_rays.item()) == second_rays and int(d_shadow.item()) == second_shadow


# ---- the adaptive loop -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_adaptive_unlit_equals_render_adaptive(renderer, oracle_mod, book1_flat, monkeypatch):
    """The book scene with the parameters tests/test_wavefront_adaptive_host.py fixed with the model: fix, half and count are
    Renderer.render_adaptive's bit for bit."""
    set_batch(monkeypatch, "")
    B = BOOK
    renderer.upload_scene(book1_flat)
    cam, p = rt.book1_camera(B["width"], B["height"]), rt.make_params(B["width"], B["height"], B["cap"], seed=B["seed"])
    a = rt.make_adaptive(B["step"], B["threshold"], B["dark_floor"])
    want_fix, want_half, want_count, want_st = renderer.render_adaptive(cam, p, a)
    fix, half, count, st = renderer.render_wavefront_adaptive(cam, p, a)
    assert len(np.unique(want_count)) >= 3
    assert np.array_equal(count, want_count) and np.array_equal(fix, want_fix) and np.array_equal(half, want_half)
    assert st["samples"] == int(count.sum(dtype=np.uint64)) == want_st["samples"] and st["rays"] == want_st["rays_traced"]
    assert st["shadow_rays"] == 0 and st["kernel_ms"] > 0
    # under the reference's lighting, stated, the same frame; and without the half buffer
    fix2, none, count2, st2 = renderer.render_wavefront_adaptive(cam, p, a, lighting=rt.Lighting(), want_half=False)
    assert none is None and np.array_equal(fix2, want_fix) and np.array_equal(count2, want_count) and st2["rays"] == st["rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("sampling,flags", [("area", ar.AREA), ("weighted", ar.WEIGHTED)])
def test_adaptive_nee_equals_the_statement(renderer, oracle_mod, monkeypatch, sampling, flags):
    """The stat scene (16 x 12, depth 8, seed 101, step 4, cap 32, threshold 0.2, floor 0.01, batches of 257): fix, half, count, rays and
    shadow rays are the statement's; area sampling, and once with cone sampling and the weighted choice."""
    set_batch(monkeypatch, str(S["batch"]))
    flat, light = nr.stat_scene()
    renderer.upload_scene(flat)
    want_fix, want_half, want_count, want_rays, want_shadow = ar.stat_adaptive(flags)
    assert len(np.unique(want_count)) >= 3
    p = rt.make_params(SW, SH, S["cap"], max_depth=S["max_depth"], seed=S["seed"])
    a = rt.make_adaptive(S["step"], S["threshold"], S["dark_floor"])
    fix, half, count, st = renderer.render_wavefront_adaptive(nr.stat_camera(), p, a, lighting=lighting_of(light), direct=True, sampling=sampling)
    assert np.array_equal(count, want_count), (np.unique(count, return_counts=True), np.unique(want_count, return_counts=True))
    assert np.array_equal(fix, want_fix) and np.array_equal(half, want_half)
    assert (st["rays"], st["shadow_rays"], st["samples"]) == (want_rays, want_shadow, int(want_count.sum(dtype=np.uint64)))


@pytest.mark.gpu
def test_adaptive_at_the_two_ends(renderer, oracle_mod, monkeypatch):
    set_batch(monkeypatch, str(S["batch"]))
    flat, light = nr.stat_scene()
    renderer.upload_scene(flat)
    cam, L = nr.stat_camera(), lighting_of(light)
    kw = dict(max_depth=S["max_depth"], seed=S["seed"])
    step, cap = S["step"], S["cap"]
    p = rt.make_params(SW, SH, cap, **kw)
    # a threshold so large that round 1 ends it
    fix, half, count, st = renderer.render_wavefront_adaptive(cam, p, rt.make_adaptive(step, 1e9, S["dark_floor"]), lighting=L, direct=True)
    two, two_rays, two_shadow = dense_stat_frame(renderer, rt.make_params(SW, SH, 2 * step, **kw), "nee")
    one, _, _ = dense_stat_frame(renderer, rt.make_params(SW, SH, step, **kw), "nee")
    assert (count == 2 * step).all() and np.array_equal(fix, two) and np.array_equal(half, one)
    assert (st["rays"], st["shadow_rays"], st["samples"]) == (two_rays, two_shadow, SW * SH * 2 * step)
    # threshold 0: every pixel whose halves differ at all goes on to the cap, and there fix is the dense NEE frame at spp = cap
    fix, half, count, st = renderer.render_wavefront_adaptive(cam, p, rt.make_adaptive(step, 0.0, S["dark_floor"]), lighting=L, direct=True)
    dense, dense_rays, dense_shadow = dense_stat_frame(renderer, p, "nee")
    at_cap = count == cap
    assert at_cap.any() and np.array_equal(fix[at_cap], dense[at_cap]) and dense[at_cap].any()
    # a pixel that stopped early did so because its halves agreed (under this black sky: a pixel no sample lights)
    early = ~at_cap
    assert (2 * half[early].astype(np.int64) == fix[early].astype(np.int64)).all() or not early.any()
    if at_cap.all():
        assert (st["rays"], st["shadow_rays"]) == (dense_rays, dense_shadow)
    even = sum(dense_stat_frame(renderer, rt.make_params(SW, SH, step, sample_begin=k * step, **kw), "nee")[0] for k in range(0, cap // step, 2))
    assert np.array_equal(half[at_cap], even[at_cap])                            # `half` never sees an odd pass


# ---- the rest --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rejections_that_need_the_context(oracle_mod, book1_flat, monkeypatch):
    torch, dev = torch_dev()
    cam = rt.book1_camera(BW, BH)
    p, a = rt.make_params(BW, BH, 8, seed=1), rt.make_adaptive(4, 0.05)
    with rt.Renderer(0) as r:
        d_fix = torch.full((BH, BW, 3), 3, dtype=torch.int64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_wavefront_pixels(cam, p, [0, 1])
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_wavefront_adaptive(cam, p, a, lighting=rt.Lighting(), direct=True)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_wavefront_pixels_device(cam, p, 0, BW * BH, d_fix.data_ptr())
        r.upload_scene(book1_flat)
        n = len(book1_flat)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_render_wavefront_adaptive.*spp \* max_depth must be <= 32767"):
            r.render_wavefront_adaptive(cam, rt.make_params(BW, BH, 32, max_depth=1024), a, lighting=rt.Lighting(emission={0: (1, 1, 1)}), direct=True)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_render_wavefront_adaptive.*uploaded sphere count"):
            r.render_wavefront_adaptive(cam, p, a, lighting=rt.Lighting(emission=np.zeros((n + 1, 3))))
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_render_wavefront_pixels.*uploaded sphere count"):
            r.render_wavefront_pixels(cam, p, [0], lighting=rt.Lighting(emission=np.zeros((n + 1, 3))), direct=True)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_render_wavefront_pixels.*lies outside the frame"):
            r.render_wavefront_pixels(cam, p, [0, BW * BH])
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*when the list is NULL"):
            r.render_wavefront_pixels_device(cam, p, 0, 5, d_fix.data_ptr())
        too_many = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        table = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*rt_render_wavefront_pixels.*n_lights"):
            r.render_wavefront_pixels_device(cam, p, 0, BW * BH, d_fix.data_ptr(), lighting=rt.Lighting(emission=table), direct=too_many)
        with pytest.raises(ValueError, match="needs a Lighting"):
            r.render_wavefront_adaptive(cam, p, a, direct=True)
        torch.cuda.synchronize()
        assert (d_fix == 3).all()
        r.render(cam, p)
        before = r.last_stats()
        r.render_wavefront_adaptive(cam, p, a)
        r.render_wavefront_pixels(cam, p, [5, 6])
        assert r.last_stats() == before                                          # no launch slot is taken
    monkeypatch.setenv("RTIOW_SCAN_MODE", "1")
    with rt.Renderer(0) as r:
        r.upload_scene(book1_flat)
        for call in (lambda: r.render_wavefront_pixels(cam, p, [0]), lambda: r.render_wavefront_adaptive(cam, p, a)):
            with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*scan mode 5"):
                call()


@pytest.mark.gpu
def test_cpp_cli_wavefront_adaptive_writes_the_bytes_the_python_path_resolves(renderer, oracle_mod, tmp_path):
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    import lights_ref as lr
    flat, light, _ = lr.book_case()
    big = int(np.argmax(np.all(light.emission == np.array(lr.BIG), axis=1)))
    scene_file, out = str(tmp_path / "scene.bin"), str(tmp_path / "night.ppm")
    rt.save_scene(scene_file, flat)
    w, h, cap, step = 64, 36, 32, 4
    base = [exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--spp", str(cap), "--seed", "4", "--out", out]
    lit = ["--sky", "0,0,0:0,0,0", "--emit", f"{big}:4,3.2,2.4"]
    run = subprocess.run(base + ["--wavefront", "--direct", "--adaptive", "0.05", "--step", str(step)] + lit, check=True, capture_output=True, text=True,
                         timeout=120, env=dict(os.environ, RTIOW_WAVEFRONT_BATCH="4000"))
    renderer.upload_scene(flat)
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {big: (4, 3.2, 2.4)})
    fix, _, count, st = renderer.render_wavefront_adaptive(rt.book1_camera(w, h), rt.make_params(w, h, cap, seed=4), rt.make_adaptive(step, 0.05, 0.01),
                                                           lighting=L, direct=True, want_half=False)
    want = renderer.resolve_rgba8_counts(fix, count, flip=True)[:, :, :3]
    assert np.array_equal(rt.read_ppm(out), want) and want.any() and len(np.unique(count)) >= 2
    assert f"shadow rays: {st['shadow_rays']}" in run.stderr
    assert f"adaptive threshold 0.05 step {step}: {st['samples'] / (w * h):.1f} samples per pixel (min {count.min()}, max {count.max()})," in run.stdout
    assert f"{st['rays']} rays" in run.stdout
    for args in (["--wavefront", "--adaptive", "0.05", "--denoise"], ["--wavefront", "--adaptive", "0.05", "--direct"]):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2, (args, bad.returncode, bad.stderr)
