"""The denoiser on the GPU (rt_denoise, rt_denoise_device): both forms of the level kernel against the
library's CPU statement (rt_denoise_host, which tests/test_denoise_host.py holds to the numpy statement of the contract), bit for bit;
what a denoise leaves alone; the CLI; and the quality of the result on the book scene."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import rtiow_amd as rt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (37, 19), (70, 45)]        # 70 x 45 with 5 levels: s = 16 is wider than a 16 x 16 tile, ragged tile edges; 5 x 3 is narrower than the kernel
# levels 6-8 (hole steps 32, 64, 128): the tile kernel's sub-lattices are 1-3 pixels wide and most of a workgroup's lanes idle.  150 x 9 at
# s = 128: residues 0..21 hold two pixels and the rest one, nri = min(s, width) = 128 < width while nrj = 9 < s, and the taps at +-128 of
# the columns 0..21 and 128..149 land inside the frame; at 70 x 45 nri = 64 < 70 < 128: both branches of the minimum
DEEP_SIZES = [(70, 45), (150, 9)]
# The colour width halves with every level: at the default 0.35 no tap of a level past the fifth carries weight on these frames (each such
# level returns its input, by the numpy statement too), so wrong taps would not show.  At 45 ~ 0.35 * 2^7 every level that has a tap
# inside the frame moves pixels -- asserted on the CPU statement below.
WIDE_COLOR = 45.0
KNOB = "RTIOW_DENOISE_LEVEL_KERNEL"


def differing(got, want):
    return f"{int((got != want).any(axis=-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


@pytest.fixture(scope="module")
def cases():
    out = {}
    for w, h in SIZES + [(150, 9)]:
        case = dr.synthetic_case(w, h)
        for a in (case[0], case[1], case[3]):
            a.setflags(write=False)
        out[(w, h)] = case
    return out


@pytest.fixture(scope="module")
def host_results(cases):
    """rt_denoise_host of (size, levels, demodulate, with count), computed once and shared by the three kernel choices."""
    memo = {}

    def get(size, levels, demodulate, with_count, sigma_color=0.35):
        key = (size, levels, demodulate, with_count, sigma_color)
        if key not in memo:
            fix, count, spp, feat, feat_spp = cases[size]
            want = rt.denoise_host(fix, spp, feat, feat_spp, rt.make_denoise(levels, sigma_color, demodulate=demodulate), count=count if with_count else None)
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
    fix, count, spp, feat, feat_spp = cases[size]
    for levels in (1, 2, 3, 4, 5):
        for demodulate in (True, False):
            for with_count in (False, True):
                got, ms = renderer.denoise(fix, spp, feat, feat_spp, rt.make_denoise(levels, demodulate=demodulate), count=count if with_count else None)
                want = host_results(size, levels, demodulate, with_count)
                assert np.array_equal(got, want), (levels, demodulate, with_count, differing(got, want))
                assert ms > 0.0                                          # the kernels' time, from the call's own events


@pytest.mark.parametrize("size", DEEP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_buffers_form_equals_host_at_levels_six_to_eight(renderer, cases, host_results, level_kernel, size):
    fix, count, spp, feat, feat_spp = cases[size]
    for sigma_color in (0.35, WIDE_COLOR):
        for levels in (6, 7, 8):
            for demodulate in (True, False):
                for with_count in (False, True):
                    got, _ = renderer.denoise(fix, spp, feat, feat_spp, rt.make_denoise(levels, sigma_color, demodulate=demodulate),
                                              count=count if with_count else None)
                    want = host_results(size, levels, demodulate, with_count, sigma_color)
                    assert np.array_equal(got, want), (sigma_color, levels, demodulate, with_count, differing(got, want))
    # with the wide colour term each of these levels moves the frame (70 x 45 has no tap at +-128 inside it: its eighth level is idle)
    for levels in (6, 7, 8) if size == (150, 9) else (6, 7):
        assert (host_results(size, levels, True, False, WIDE_COLOR) != host_results(size, levels - 1, True, False, WIDE_COLOR)).any(), levels


def device_form(renderer, cases, host_results, size, options, sigma_color=0.35):
    import torch
    fix, count, spp, feat, feat_spp = cases[size]
    w, h = size
    dev = torch.device("cuda", 0)
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t).copy()).to(dev)
    d_fix, d_feat, d_count = up(fix, np.int64), up(feat, np.int64), up(count, np.int32)
    words = rt.Renderer.denoise_workspace_bytes(w, h) // 8
    assert words == w * h * 16
    guard = 64
    d_work = torch.full((words + guard,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    d_out = torch.full((h * w * 3 + guard,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for levels, demodulate, with_count in options:
        renderer.denoise_device(d_fix.data_ptr(), spp, d_feat.data_ptr(), feat_spp, w, h, rt.make_denoise(levels, sigma_color, demodulate=demodulate),
                                d_work.data_ptr(), d_out.data_ptr(), d_count_ptr=d_count.data_ptr() if with_count else 0, stream=stream)
        torch.cuda.synchronize()
        got = d_out[:h * w * 3].cpu().numpy().view(np.uint64).reshape(h, w, 3)
        want = host_results(size, levels, demodulate, with_count, sigma_color)
        assert np.array_equal(got, want), (levels, demodulate, with_count, differing(got, want))
    assert (d_work[words:] == 0x5A5A5A5A).all().item() and (d_out[h * w * 3:] == 0x5A5A5A5A).all().item()
    assert np.array_equal(d_fix.cpu().numpy().view(np.uint64), fix) and np.array_equal(d_feat.cpu().numpy().view(np.uint64), feat)


@pytest.mark.parametrize("size", [(5, 3), (70, 45)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_form_equals_host_and_stays_inside_its_buffers(renderer, cases, host_results, level_kernel, size):
    device_form(renderer, cases, host_results, size, ((5, True, True), (4, False, False), (1, True, False)))


def test_device_form_with_eight_levels_on_a_wide_frame(renderer, cases, host_results, level_kernel):
    device_form(renderer, cases, host_results, (150, 9), ((8, True, True),))
    device_form(renderer, cases, host_results, (150, 9), ((8, True, True),), sigma_color=WIDE_COLOR)


def test_adaptive_frame_with_its_count_buffer(renderer, book1_flat, level_kernel):
    w, h = 64, 36
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    fix, _, count, _ = renderer.render_adaptive(cam, rt.make_params(w, h, 32), rt.make_adaptive(4, 0.05), want_half=False)
    assert count.min() >= 8 and len(np.unique(count)) > 1               # pixels stopped at different numbers of samples
    feat, _, _ = renderer.render_features(cam, rt.make_params(w, h, 8), want_ids=False)
    dn = rt.make_denoise()
    got, _ = renderer.denoise(fix, 0, feat, 8, dn, count=count)         # (spp is ignored with a count buffer)
    want = rt.denoise_host(fix, 0, feat, 8, dn, count=count)
    assert np.array_equal(got, want), differing(got, want)
    assert np.array_equal(want, dr.denoise(fix, 0, feat, 8, count=count))
    assert (got != rt.denoise_host(fix, 32, feat, 8, dn)).any()          # the counts matter


def test_a_denoise_leaves_the_render_path_alone(renderer, oracle_mod, book1_flat, cases):
    """No launch slot, no report in rt_last_stats; a rejected call writes nothing; the dense render issued right after is Oracle B's."""
    import torch
    w, h, spp = 96, 54, 4                                               # the smoke frame
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    renderer.render(cam, rt.make_params(w, h, 1))
    before = renderer.last_stats()
    fix, count, s_spp, feat, feat_spp = cases[(37, 19)]
    renderer.denoise(fix, s_spp, feat, feat_spp)
    assert renderer.last_stats() == before
    dev = torch.device("cuda", 0)
    d_in = torch.zeros(37 * 19 * 8, dtype=torch.int64, device=dev)
    d_work = torch.full((37 * 19 * 16,), 0x5A5A, dtype=torch.int64, device=dev)
    d_out = torch.full((37 * 19 * 3,), 0x5A5A, dtype=torch.int64, device=dev)
    with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*levels must be"):
        renderer.denoise_device(d_in.data_ptr(), 1, d_in.data_ptr(), 1, 37, 19, rt.make_denoise(9), d_work.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    assert (d_work == 0x5A5A).all().item() and (d_out == 0x5A5A).all().item() and renderer.last_stats() == before
    _, got_fix, st = renderer.render(cam, rt.make_params(w, h, spp, seed=1))
    want_fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(w, h, spp, seed=1))
    assert np.array_equal(got_fix, want_fix) and st["rays_traced"] == ost["rays_traced"] and st["samples"] == w * h * spp
    # a context without a scene denoises too
    with rt.Renderer(0) as r:
        got, _ = r.denoise(fix, s_spp, feat, feat_spp)
    assert np.array_equal(got, rt.denoise_host(fix, s_spp, feat, feat_spp))


def test_cli_denoise_png_is_the_python_paths(renderer, book1_flat, tmp_path):
    w, h, spp, fspp = 48, 27, 4, 6
    exe = os.path.join(ROOT, "host", "rtiow_render")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    feat, _, _ = renderer.render_features(cam, rt.make_params(w, h, fspp), want_ids=False)

    def rgba_of(fix, dn, count=None):
        """The Python path's bytes: the image the PNG must hold (the CLI's encoder stores, Python's deflates: the files differ)."""
        clean, _ = renderer.denoise(fix, spp, feat, fspp, dn, count=count)
        return renderer.resolve_rgba8(clean, 1, flip=True)

    base = [exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--feature-spp", str(fspp), "--denoise"]
    # a dense frame with options of its own
    out = str(tmp_path / "dense.png")
    run = subprocess.run([*base, "--spp", str(spp), "--out", out, "--denoise-levels", "3", "--sigma-color", "0.5", "--sigma-normal", "0.75",
                          "--sigma-depth", "0.1"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "denoised: 3 levels" in run.stdout, run.stderr
    _, fix, _ = renderer.render(cam, rt.make_params(w, h, spp))
    assert np.array_equal(rt.read_png(out), rgba_of(fix, rt.make_denoise(3, 0.5, 0.75, 0.1)))
    assert not np.array_equal(rt.read_png(out), renderer.resolve_rgba8(fix, spp, flip=True))
    # an adaptive frame: the count buffer goes in
    out = str(tmp_path / "adaptive.png")
    run = subprocess.run([*base, "--spp", "16", "--adaptive", "0.05", "--step", "4", "--out", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    afix, _, count, _ = renderer.render_adaptive(cam, rt.make_params(w, h, 16), rt.make_adaptive(4, 0.05), want_half=False)
    assert np.array_equal(rt.read_png(out), rgba_of(afix, rt.make_denoise(), count=count))
    for extra in (["--uniform53"], ["--devices", "0"], ["--orbit", "2"], ["--passes", "2"], ["--two-calls"]):
        bad = subprocess.run([exe, "--denoise", *extra], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "goes with none of" in bad.stderr, extra


def test_quality_on_the_book_scene(renderer):
    """Book scene random_scene(1), book1_camera(240, 135), depth 50: 8 spp (seed 1) filtered with the guides at 8 spp (seed 1) against a
    1024-spp reference (seed 7); 4 levels, sigmas 0.35 / 1.0 / 0.2, demodulated.  RMSE over all channels of the clipped linear means.
    Measured with the numpy statement of the contract on Oracle-B sums: noisy 0.03894, denoised 0.02376 (ratio 0.610); the filter is
    deterministic, so the bound's margin is for nothing but a different reading of the contract.  A filter that ignores the colour
    term makes the frame WORSE than the noisy one (0.045-0.062 with sigma_color = 1e6)."""
    w, h = 240, 135
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(flat)
    _, fix, _ = renderer.render(cam, rt.make_params(w, h, 8, seed=1, max_depth=50))
    feat, _, _ = renderer.render_features(cam, rt.make_params(w, h, 8, seed=1), want_ids=False)
    _, ref_fix, _ = renderer.render(cam, rt.make_params(w, h, 1024, seed=7, max_depth=50))
    clean, _ = renderer.denoise(fix, 8, feat, 8, rt.make_denoise(4, 0.35, 1.0, 0.2, True))
    ref = dr.mean_of(ref_fix, 1024)
    noisy, denoised = dr.rmse(dr.mean_of(fix, 8), ref), dr.rmse(dr.mean_of(clean, 1), ref)
    geometry_only, _ = renderer.denoise(fix, 8, feat, 8, rt.make_denoise(4, 1e6, 1.0, 0.2, True))
    print(f"denoise quality 240x135: noisy {noisy:.5f} denoised {denoised:.5f} ratio {denoised / noisy:.4f}; "
          f"geometry-only weights {dr.rmse(dr.mean_of(geometry_only, 1), ref):.5f}")
    assert denoised < 0.75 * noisy
