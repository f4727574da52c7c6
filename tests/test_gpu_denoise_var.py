"""The variance-guided denoiser on the GPU (rt_denoise_var, rt_denoise_var_device): both forms of the level kernel
against the library's CPU statement (rt_denoise_var_host, which tests/test_denoise_var_host.py holds to the numpy statement of the
contract), bit for bit; real adaptive frames, unlit and lit; the two accumulated passes the command line makes `half` from; what a denoise
leaves alone; a side stream; the command line; and the quality of the result on the book scene at night."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as vr
import nee_ref as nr
import rtiow_amd as rt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 1 x 1; 5 x 3 is narrower than the 5 x 5 kernel; 37 x 19: a partial tile; 70 x 45 with 5 levels: s = 16 spans a 16 x 16 tile, so the halo
# crosses tiles
SIZES = [(1, 1), (5, 3), (37, 19), (70, 45)]
# levels 6-8 (hole steps 32, 64, 128) at 150 x 9: sub-lattices one to three pixels wide, nri = min(s, width) = 128 < width while
# nrj = 9 < s, and the taps at +-128 of the columns 0..21 and 128..149 land inside the frame.  The variance shrinks from level to level
# and the colour stop with it: at the default width the eighth level returns its input on this frame, so wrong taps would not show.  At 64
# standard deviations every one of these levels moves pixels -- asserted on the CPU statement below.
DEEP = (150, 9)
WIDE_COLOR = 64.0
KNOB = "RTIOW_DENOISE_LEVEL_KERNEL"


def differing(got, want):
    return f"{int((got != want).any(axis=-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


@pytest.fixture(scope="module")
def cases():
    out = {}
    for w, h in SIZES + [DEEP]:
        case = vr.synthetic_case(w, h)
        for a in (case[0], case[1], case[2], case[4]):
            a.setflags(write=False)
        out[(w, h)] = case
    return out


@pytest.fixture(scope="module")
def host_results(cases):
    """rt_denoise_var_host of (size, levels, demodulate, with count, sigma_color), computed once and shared by the three kernel choices."""
    memo = {}

    def get(size, levels, demodulate, with_count, sigma_color=vr.SIGMA_COLOR):
        key = (size, levels, demodulate, with_count, sigma_color)
        if key not in memo:
            fix, half, count, spp, feat, feat_spp = cases[size]
            want = rt.denoise_var_host(fix, half, spp, feat, feat_spp, rt.make_denoise_var(levels, sigma_color, demodulate=demodulate),
                                       count=count if with_count else None)
            want.setflags(write=False)
            memo[key] = want
        return memo[key]
    return get


@pytest.fixture(params=[None, "gather", "tile"], ids=["shipped", "gather", "tile"])
def level_kernel(request):
    """The diagnostic knob is read per call."""
    if request.param is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = request.param
    yield request.param
    os.environ.pop(KNOB, None)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_buffers_form_equals_host(renderer, cases, host_results, level_kernel, size):
    fix, half, count, spp, feat, feat_spp = cases[size]
    for levels in (1, 2, 3, 4, 5):
        for demodulate in (True, False):
            for with_count in (False, True):
                got, ms = renderer.denoise_var(fix, half, spp, feat, feat_spp, rt.make_denoise_var(levels, demodulate=demodulate),
                                               count=count if with_count else None)
                want = host_results(size, levels, demodulate, with_count)
                assert np.array_equal(got, want), (levels, demodulate, with_count, differing(got, want))
                assert ms > 0.0                                          # the kernels' time, from the call's own events
    got, _ = renderer.denoise_var(fix, half, spp, feat, feat_spp, rt.make_denoise_var(4, 0.5), count=count)          # another width
    assert np.array_equal(got, host_results(size, 4, True, True, 0.5)), differing(got, host_results(size, 4, True, True, 0.5))


def test_buffers_form_equals_host_at_levels_six_to_eight(renderer, cases, host_results, level_kernel):
    fix, half, count, spp, feat, feat_spp = cases[DEEP]
    for sigma_color in (vr.SIGMA_COLOR, WIDE_COLOR):
        for levels in (6, 7, 8):
            for demodulate in (True, False):
                for with_count in (False, True):
                    got, _ = renderer.denoise_var(fix, half, spp, feat, feat_spp, rt.make_denoise_var(levels, sigma_color, demodulate=demodulate),
                                                  count=count if with_count else None)
                    want = host_results(DEEP, levels, demodulate, with_count, sigma_color)
                    assert np.array_equal(got, want), (sigma_color, levels, demodulate, with_count, differing(got, want))
    for levels in (6, 7, 8):                                            # with the wide colour term none of these levels is idle
        assert (host_results(DEEP, levels, True, False, WIDE_COLOR) != host_results(DEEP, levels - 1, True, False, WIDE_COLOR)).any(), levels


def device_form(renderer, cases, host_results, size, options, stream=None, sigma_color=vr.SIGMA_COLOR):
    """The device form under guard words: the workspace is sized by rt_denoise_var_workspace_bytes, and the words behind it and behind the
    output are intact afterwards; the inputs are left as they were."""
    import torch
    fix, half, count, spp, feat, feat_spp = cases[size]
    w, h = size
    dev = torch.device("cuda", 0)
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t).copy()).to(dev)
    d_fix, d_half, d_feat, d_count = up(fix, np.int64), up(half, np.int64), up(feat, np.int64), up(count, np.int32)
    words = rt.Renderer.denoise_var_workspace_bytes(w, h) // 8
    assert words == w * h * 19
    guard = 64
    d_work = torch.full((words + guard,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    d_out = torch.full((h * w * 3 + guard,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    handle = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    for levels, demodulate, with_count in options:
        renderer.denoise_var_device(d_fix.data_ptr(), d_half.data_ptr(), spp, d_feat.data_ptr(), feat_spp, w, h,
                                    rt.make_denoise_var(levels, sigma_color, demodulate=demodulate), d_work.data_ptr(), d_out.data_ptr(),
                                    d_count_ptr=d_count.data_ptr() if with_count else 0, stream=handle)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        got = d_out[:h * w * 3].cpu().numpy().view(np.uint64).reshape(h, w, 3)
        want = host_results(size, levels, demodulate, with_count, sigma_color)
        assert np.array_equal(got, want), (levels, demodulate, with_count, differing(got, want))
    assert (d_work[words:] == 0x5A5A5A5A).all().item() and (d_out[h * w * 3:] == 0x5A5A5A5A).all().item()
    back = lambda t: t.cpu().numpy().view(np.uint64)
    assert np.array_equal(back(d_fix), fix) and np.array_equal(back(d_half), half) and np.array_equal(back(d_feat), feat)


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 19), (70, 45)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_form_equals_host_and_stays_inside_its_buffers(renderer, cases, host_results, level_kernel, size):
    device_form(renderer, cases, host_results, size, ((5, True, True), (4, False, False), (1, True, False)))


def test_device_form_with_eight_levels_on_a_wide_frame(renderer, cases, host_results, level_kernel):
    device_form(renderer, cases, host_results, DEEP, ((8, True, True), (6, False, False)))
    device_form(renderer, cases, host_results, DEEP, ((8, True, True),), sigma_color=WIDE_COLOR)


def test_device_form_on_a_side_stream(renderer, cases, host_results):
    import torch
    device_form(renderer, cases, host_results, (70, 45), ((5, True, True), (2, False, False)), stream=torch.cuda.Stream(device=torch.device("cuda", 0)))


def test_an_adaptive_frame_with_its_half_and_count(renderer, book1_flat, level_kernel):
    """A real unlit adaptive result: fix, half and count of render_adaptive."""
    w, h = 64, 36
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    fix, half, count, _ = renderer.render_adaptive(cam, rt.make_params(w, h, 32), rt.make_adaptive(4, 0.05))
    assert count.min() >= 8 and len(np.unique(count)) > 1 and (count % 2 == 0).all()
    feat, _, _ = renderer.render_features(cam, rt.make_params(w, h, 8), want_ids=False)
    dn = rt.make_denoise_var()
    got, _ = renderer.denoise_var(fix, half, 0, feat, 8, dn, count=count)                       # (spp is ignored with a count buffer)
    want = rt.denoise_var_host(fix, half, 0, feat, 8, dn, count=count)
    assert np.array_equal(got, want), differing(got, want)
    assert np.array_equal(want, vr.denoise_var(fix, half, 0, feat, 8, count=count))
    assert (got != rt.denoise_var_host(fix, half, 32, feat, 8, dn)).any()                        # the counts matter
    assert (got != rt.denoise_var_host(fix, fix >> np.uint64(1), 0, feat, 8, dn, count=count)).any()      # ... and so does the half buffer


def test_a_lit_adaptive_frame_of_the_path_queue(renderer, level_kernel):
    """render_wavefront_adaptive on nee_ref's stat scene (16 x 12, depth 8), direct lighting: fix, half and count as they come."""
    flat, light = nr.stat_scene()
    renderer.upload_scene(flat)
    w, h = nr.STAT_W, nr.STAT_H
    cam = nr.stat_camera()
    L = rt.Lighting((0, 0, 0), (0, 0, 0), light.emission)
    fix, half, count, _ = renderer.render_wavefront_adaptive(cam, rt.make_params(w, h, 32, max_depth=nr.STAT_DEPTH, seed=101), rt.make_adaptive(4, 0.2, 0.01),
                                                             lighting=L, direct=True)
    assert len(np.unique(count)) >= 2 and fix.any() and half.any()
    feat, _, _ = renderer.render_features(cam, rt.make_params(w, h, 4), want_ids=False)
    for dn in (rt.make_denoise_var(), rt.make_denoise_var(3, 1.0, demodulate=False)):
        got, _ = renderer.denoise_var(fix, half, 0, feat, 4, dn, count=count)
        want = rt.denoise_var_host(fix, half, 0, feat, 4, dn, count=count)
        assert np.array_equal(got, want), differing(got, want)
    assert np.array_equal(want, vr.denoise_var(fix, half, 0, feat, 4, levels=3, sigma_color=1.0, demodulate=False, count=count))


def test_two_accumulated_passes_are_one_pass(renderer):
    """The command line's way to make `half`: pass 1 (spp / 2 samples) is kept, pass 2 renders the samples from spp / 2 on into it.  The
    sums are those of one pass of spp samples."""
    flat, light = nr.stat_scene()
    renderer.upload_scene(flat)
    w, h = nr.STAT_W, nr.STAT_H
    cam = nr.stat_camera()
    L = rt.Lighting((0, 0, 0), (0, 0, 0), light.emission)
    kw = dict(max_depth=nr.STAT_DEPTH, seed=101)
    one, s1 = renderer.render_wavefront_pixels(cam, rt.make_params(w, h, 8, **kw), lighting=L, direct=True, sampling="weighted")
    half, sa = renderer.render_wavefront_pixels(cam, rt.make_params(w, h, 4, **kw), lighting=L, direct=True, sampling="weighted")
    fix, sb = renderer.render_wavefront_pixels(cam, rt.make_params(w, h, 4, sample_begin=4, **kw), lighting=L, direct=True, sampling="weighted", into=half)
    assert np.array_equal(fix, one) and one.any() and (fix != half).any()
    assert sa["rays_traced"] + sb["rays_traced"] == s1["rays_traced"]


def test_a_denoise_leaves_the_render_path_alone(renderer, oracle_mod, book1_flat, cases):
    """No launch slot, no report in rt_last_stats; a rejected call writes nothing; the dense render issued right after is Oracle B's."""
    import torch
    w, h, spp = 96, 54, 4                                               # the smoke frame
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    renderer.render(cam, rt.make_params(w, h, 1))
    before = renderer.last_stats()
    fix, half, count, s_spp, feat, feat_spp = cases[(37, 19)]
    renderer.denoise_var(fix, half, s_spp, feat, feat_spp)
    assert renderer.last_stats() == before
    dev = torch.device("cuda", 0)
    d_in = torch.zeros(37 * 19 * 8, dtype=torch.int64, device=dev)
    d_work = torch.full((37 * 19 * 19,), 0x5A5A, dtype=torch.int64, device=dev)
    d_out = torch.full((37 * 19 * 3,), 0x5A5A, dtype=torch.int64, device=dev)
    with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*levels must be"):
        renderer.denoise_var_device(d_in.data_ptr(), d_in.data_ptr(), 2, d_in.data_ptr(), 1, 37, 19, rt.make_denoise_var(9), d_work.data_ptr(), d_out.data_ptr())
    with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*half"):
        renderer.denoise_var_device(d_in.data_ptr(), 0, 2, d_in.data_ptr(), 1, 37, 19, rt.make_denoise_var(), d_work.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    assert (d_work == 0x5A5A).all().item() and (d_out == 0x5A5A).all().item() and renderer.last_stats() == before
    _, got_fix, st = renderer.render(cam, rt.make_params(w, h, spp, seed=1))
    want_fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(w, h, spp, seed=1))
    assert np.array_equal(got_fix, want_fix) and st["rays_traced"] == ost["rays_traced"] and st["samples"] == w * h * spp
    # a context without a scene denoises too
    with rt.Renderer(0) as r:
        got, _ = r.denoise_var(fix, half, s_spp, feat, feat_spp)
    assert np.array_equal(got, rt.denoise_var_host(fix, half, s_spp, feat, feat_spp))


def test_cli_images_are_the_python_paths(renderer, book1_flat, tmp_path):
    w, h, spp, fspp = 48, 27, 8, 6
    exe = os.path.join(ROOT, "host", "rtiow_render")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    feat, _, _ = renderer.render_features(cam, rt.make_params(w, h, fspp), want_ids=False)
    big = int(np.argmax(book1_flat["radius"][1:])) + 1                   # a large sphere of the scene's list (not the ground)
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {big: (4, 3.2, 2.4)})
    lit = ["--wavefront", "--sky", "0,0,0:0,0,0", "--emit", f"{big}:4,3.2,2.4", "--direct-weighted"]
    base = [exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--feature-spp", str(fspp), "--denoise-variance"]

    def rgba_of(fix, half, dn, spp, count=None):
        clean, _ = renderer.denoise_var(fix, half, spp, feat, fspp, dn, count=count)
        return renderer.resolve_rgba8(clean, 1, flip=True)

    # the lit frame of the path queue as two accumulated passes, with options of its own
    out = str(tmp_path / "lit.png")
    run = subprocess.run([*base, *lit, "--spp", str(spp), "--out", out, "--denoise-levels", "3", "--sigma-color", "2.5", "--sigma-normal", "0.75",
                          "--sigma-depth", "0.1"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "denoised by variance: 3 levels" in run.stdout, run.stderr
    half, _ = renderer.render_wavefront_pixels(cam, rt.make_params(w, h, spp // 2), lighting=L, direct=True, sampling="weighted")
    fix, _ = renderer.render_wavefront_pixels(cam, rt.make_params(w, h, spp // 2, sample_begin=spp // 2), lighting=L, direct=True, sampling="weighted", into=half)
    want = rgba_of(fix, half, rt.make_denoise_var(3, 2.5, 0.75, 0.1), spp)
    assert np.array_equal(rt.read_png(out), want) and want[..., :3].any()
    assert not np.array_equal(rt.read_png(out), renderer.resolve_rgba8(fix, spp, flip=True))
    # the dense frame, adaptive: the loop's own half and count go in; the default width
    out = str(tmp_path / "adaptive.png")
    run = subprocess.run([*base, "--spp", "16", "--adaptive", "0.05", "--step", "4", "--out", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    afix, ahalf, count, _ = renderer.render_adaptive(cam, rt.make_params(w, h, 16), rt.make_adaptive(4, 0.05))
    assert np.array_equal(rt.read_png(out), rgba_of(afix, ahalf, rt.make_denoise_var(), 16, count=count))
    # the dense frame as two passes, and the lit adaptive frame of the path queue
    out = str(tmp_path / "dense.png")
    run = subprocess.run([*base, "--spp", str(spp), "--out", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    _, dhalf, _ = renderer.render(cam, rt.make_params(w, h, spp // 2))
    _, dfix, _ = renderer.render(cam, rt.make_params(w, h, spp))
    assert np.array_equal(rt.read_png(out), rgba_of(dfix, dhalf, rt.make_denoise_var(), spp))
    out = str(tmp_path / "lit_adaptive.png")
    run = subprocess.run([*base, *lit, "--spp", "16", "--adaptive", "0.05", "--step", "4", "--out", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lfix, lhalf, lcount, _ = renderer.render_wavefront_adaptive(cam, rt.make_params(w, h, 16), rt.make_adaptive(4, 0.05, 0.01), lighting=L, direct=True,
                                                                sampling="weighted")
    assert np.array_equal(rt.read_png(out), rgba_of(lfix, lhalf, rt.make_denoise_var(), 16, count=lcount))


def test_quality_on_the_book_scene_at_night(renderer):
    """Frame (b) of DESIGN.md section 25: random_scene(1), book1_camera(240, 135), a black sky, the sphere at index 528 radiating
    (4, 3.2, 2.4), weighted direct lighting, depth 16: 16 spp (seed 1) as two passes of 8, the guides at 8 spp, against a 1024-spp frame of
    seed 7.  RMSE over all channels of the clipped linear means.  The condition: the variance-guided frame is better than the noisy one.
    The three figures are also the numpy statement's on the same sums, digit for digit.  The sweep of DESIGN.md section 25 put the filter
    below rt_denoise on both of its frames at the shipped width (daylight 0.599 against 0.610 of the noisy RMSE, this frame 0.933 against
    0.968), so the ratio to rt_denoise's figure is asserted below 1 here as well.  Measured: noisy 0.01900, rt_denoise 0.01840,
    rt_denoise_var 0.01773."""
    w, h = 240, 135
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(flat)
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {528: (4, 3.2, 2.4)})
    kw = dict(lighting=L, direct=True, sampling="weighted")
    half, _ = renderer.render_wavefront_pixels(cam, rt.make_params(w, h, 8, seed=1, max_depth=16), **kw)
    fix, _ = renderer.render_wavefront_pixels(cam, rt.make_params(w, h, 8, seed=1, max_depth=16, sample_begin=8), into=half, **kw)
    ref_fix = renderer.render_wavefront(cam, rt.make_params(w, h, 1024, seed=7, max_depth=16), **kw)[0]
    feat, _, _ = renderer.render_features(cam, rt.make_params(w, h, 8, seed=1), want_ids=False)
    ref = dr.mean_of(ref_fix, 1024)
    by_variance, _ = renderer.denoise_var(fix, half, 16, feat, 8, rt.make_denoise_var())
    absolute, _ = renderer.denoise(fix, 16, feat, 8, rt.make_denoise())
    gpu = [dr.rmse(dr.mean_of(fix, 16), ref), dr.rmse(dr.mean_of(absolute, 1), ref), dr.rmse(dr.mean_of(by_variance, 1), ref)]
    stated = [gpu[0], dr.rmse(dr.mean_of(dr.denoise(fix, 16, feat, 8), 1), ref), dr.rmse(dr.mean_of(vr.denoise_var(fix, half, 16, feat, 8), 1), ref)]
    print(f"night frame 240x135x16: noisy {gpu[0]:.5f} rt_denoise {gpu[1]:.5f} rt_denoise_var {gpu[2]:.5f}; ratio to noisy {gpu[2] / gpu[0]:.4f}, "
          f"to rt_denoise {gpu[2] / gpu[1]:.4f}")
    assert gpu[2] < gpu[0]
    assert gpu[2] < gpu[1]
    assert [repr(x) for x in gpu] == [repr(x) for x in stated]
