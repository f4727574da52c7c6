"""Temporal accumulation with second moments and the variance-guided denoiser fed by its variance, on the GPU (rt_temporal_var,
rt_denoise_var_given and their device forms): every device form against the library's CPU statements (which
tests/test_temporal_var_host.py holds to the numpy statement of the contract), bit for bit -- the doubles compared as u64 --; guard words
behind every output and the workspace; what a call leaves alone; Renderer.render_sequence_var and the CLI against the composition made
by hand; and the quality of the result on the night scene."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as vr
import rtiow_amd as rt
import temporal_ref as tr
import temporal_var_ref as tv
from rtiow_amd import _ffi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 2 x 2: one lane pair of one wave; 5 x 3: narrower than a tile; 37 x 19 and 70 x 45: ragged on both sides, several workgroups
PAIRS = ["identical", "subpixel_pan", "wide_pan", "facing_away", "roll_90", "fov", "nan_prev", "lens_radius", "orbit_step"]
THREE_OPTIONS = (tr.OPTION_SETS[0], tr.OPTION_SETS[3], tr.OPTION_SETS[1])
FILTER_SIZES = [(1, 1), (5, 3), (37, 19), (70, 45)]
KNOB = "RTIOW_DENOISE_LEVEL_KERNEL"
GUARD = 0x5A5A5A5A


def same(got, want):
    return (got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(tv.bits(got[2]), tv.bits(want[2])) and np.array_equal(tv.bits(got[3]), tv.bits(want[3])))


def differing(got, want):
    return (f"{int((got[0] != want[0]).any(axis=-1).sum())} sums, {int((got[1] != want[1]).sum())} lengths, "
            f"{int((tv.bits(got[2]) != tv.bits(want[2])).any(axis=-1).sum())} moments and "
            f"{int((tv.bits(got[3]) != tv.bits(want[3])).any(axis=-1).sum())} variances of {got[1].size} pixels differ")


@pytest.fixture(scope="module")
def cases():
    out = {}
    for w, h in tr.SIZES:
        frame, hist = tr.synthetic_frame(w, h, 3), tr.synthetic_history(w, h, 3)
        hist = hist + (tv.synthetic_m2(hist[0], 3),)
        for a in (frame[0], frame[1], frame[3], hist[0], hist[1], hist[2], hist[4]):
            a.setflags(write=False)
        out[(w, h)] = (frame, hist)
    return out


@pytest.fixture(scope="module")
def filter_cases():
    """size -> (fix, var for spp, var for the counts, count, spp, feat, feat_spp) and the host statement's results, computed once"""
    out = {}
    for w, h in FILTER_SIZES + [(150, 9)]:
        fix, _, count, spp, feat, feat_spp = vr.synthetic_case(w, h)
        out[(w, h)] = (fix, tv.synthetic_var(fix, None, spp, 5), tv.synthetic_var(fix, count, spp, 6), count, spp, feat, feat_spp)
        for a in out[(w, h)][:4] + (feat,):
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def filter_host(filter_cases):
    memo = {}

    def get(size, levels, demodulate, with_count):
        key = (size, levels, demodulate, with_count)
        if key not in memo:
            fix, var_spp, var_count, count, spp, feat, feat_spp = filter_cases[size]
            memo[key] = rt.denoise_var_given_host(fix, var_count if with_count else var_spp, spp, feat, feat_spp,
                                                  rt.make_denoise_var(levels, demodulate=demodulate), count=count if with_count else None)
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


def upload(a, view):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).to(torch.device("cuda", 0))


@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_temporal_var_buffers_form_equals_host(renderer, cases, size):
    w, h = size
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp, pm2) = cases[size]
    pairs = tr.camera_pairs(w, h)
    for pair in PAIRS:
        cur, prev = pairs[pair]
        hist = (pfix, plen, pfeat, pspp, prev, pm2)
        for options in THREE_OPTIONS:
            for cnt in (None, count):
                for history in (hist, None):
                    tp = tr.make_options(**options)
                    got = renderer.temporal_var(fix, spp, feat, feat_spp, cur, history, tp, count=cnt)
                    want = rt.temporal_var_host(fix, spp, feat, feat_spp, cur, history, tp, count=cnt)
                    assert same(got, want), (pair, options, cnt is not None, history is not None, differing(got, want))
                    assert got[4] > 0.0                                  # the kernel's time, from the call's own events
    assert (want[1] == 1).all()


@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_temporal_var_device_form_equals_host_and_stays_inside_its_buffers(renderer, cases, size):
    import torch
    w, h = size
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp, pm2) = cases[size]
    dev = torch.device("cuda", 0)
    d_fix, d_feat, d_count = upload(fix, np.int64), upload(feat, np.int64), upload(count, np.int32)
    d_pfix, d_plen, d_pfeat, d_pm2 = upload(pfix, np.int64), upload(plen, np.int32), upload(pfeat, np.int64), upload(pm2, np.int64)
    guard, n = 64, h * w
    d_out = torch.full((n * 3 + guard,), GUARD, dtype=torch.int64, device=dev)
    d_len = torch.full((n + guard,), GUARD, dtype=torch.int32, device=dev)
    d_m2 = torch.full((n * 3 + guard,), GUARD, dtype=torch.int64, device=dev)
    d_var = torch.full((n * 3 + guard,), GUARD, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    pairs = tr.camera_pairs(w, h)
    for pair in PAIRS:
        cur, prev = pairs[pair]
        for options, with_count, with_history in ((tr.OPTION_SETS[0], False, True), (tr.OPTION_SETS[3], True, True), (tr.OPTION_SETS[1], True, False)):
            tp = tr.make_options(**options)
            history = (d_pfix.data_ptr(), d_plen.data_ptr(), d_pfeat.data_ptr(), pspp, prev, d_pm2.data_ptr()) if with_history else None
            renderer.temporal_var_device(d_fix.data_ptr(), spp, d_feat.data_ptr(), feat_spp, cur, w, h, tp, d_out.data_ptr(), d_len.data_ptr(),
                                         d_m2.data_ptr(), d_var.data_ptr(), history=history, d_count_ptr=d_count.data_ptr() if with_count else 0,
                                         stream=stream)
            torch.cuda.synchronize()
            f64 = lambda t: t[:n * 3].cpu().numpy().view(np.float64).reshape(h, w, 3)
            got = (d_out[:n * 3].cpu().numpy().view(np.uint64).reshape(h, w, 3), d_len[:n].cpu().numpy().view(np.uint32).reshape(h, w), f64(d_m2), f64(d_var))
            want = rt.temporal_var_host(fix, spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev, pm2) if with_history else None, tp,
                                        count=count if with_count else None)
            assert same(got, want), (pair, options, with_count, with_history, differing(got, want))
    assert (d_out[n * 3:] == GUARD).all().item() and (d_len[n:] == GUARD).all().item()
    assert (d_m2[n * 3:] == GUARD).all().item() and (d_var[n * 3:] == GUARD).all().item()
    for d, a in ((d_fix, fix), (d_feat, feat), (d_pfix, pfix), (d_pfeat, pfeat)):
        assert np.array_equal(d.cpu().numpy().view(np.uint64), a)
    assert np.array_equal(d_pm2.cpu().numpy().view(np.uint64).reshape(h, w, 3), tv.bits(pm2))
    assert np.array_equal(d_plen.cpu().numpy().view(np.uint32), plen) and np.array_equal(d_count.cpu().numpy().view(np.uint32), count)


def test_a_chain_of_three_frames_with_ping_pong_buffers_on_one_stream(renderer):
    """No host wait between the calls: the side stream orders them; the filter follows the last on the same stream."""
    import torch
    w, h = 70, 45
    n = w * h
    cams = rt.orbit_cameras(180, w, h)[:3]
    frames = [tr.synthetic_frame(w, h, 40 + k) for k in range(3)]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    d_fix = [upload(f[0], np.int64) for f in frames]
    d_feat = [upload(f[3], np.int64) for f in frames]
    zeros = lambda count, t=torch.int64: [torch.zeros(count, dtype=t, device=dev) for _ in range(2)]
    d_out, d_len, d_m2, d_var = zeros(n * 3), zeros(n, torch.int32), zeros(n * 3), zeros(n * 3)
    d_work = torch.zeros(rt.Renderer.denoise_var_workspace_bytes(w, h) // 8, dtype=torch.int64, device=dev)
    d_shown = torch.zeros(n * 3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    tp, dn = rt.make_temporal(), rt.make_denoise_var()
    for k in range(3):
        wr, rd = k & 1, 1 - (k & 1)
        history = (d_out[rd].data_ptr(), d_len[rd].data_ptr(), d_feat[k - 1].data_ptr(), frames[k - 1][4], cams[k - 1], d_m2[rd].data_ptr()) if k else None
        renderer.temporal_var_device(d_fix[k].data_ptr(), frames[k][2], d_feat[k].data_ptr(), frames[k][4], cams[k], w, h, tp, d_out[wr].data_ptr(),
                                     d_len[wr].data_ptr(), d_m2[wr].data_ptr(), d_var[wr].data_ptr(), history=history, stream=stream.cuda_stream)
    renderer.denoise_var_given_device(d_out[0].data_ptr(), d_var[0].data_ptr(), 1, d_feat[2].data_ptr(), frames[2][4], w, h, dn, d_work.data_ptr(),
                                      d_shown.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    history = None
    for k in range(3):
        fix, _, spp, feat, feat_spp = frames[k]
        want = rt.temporal_var_host(fix, spp, feat, feat_spp, cams[k], history, tp)
        history = (want[0], want[1], feat, feat_spp, cams[k], want[2])
    f64 = lambda t: t.cpu().numpy().view(np.float64).reshape(h, w, 3)
    got = (d_out[0].cpu().numpy().view(np.uint64).reshape(h, w, 3), d_len[0].cpu().numpy().view(np.uint32).reshape(h, w), f64(d_m2[0]), f64(d_var[0]))
    assert same(got, want), differing(got, want)
    assert (want[1] == 3).any() and (want[1] == 1).any()
    assert np.array_equal(d_shown.cpu().numpy().view(np.uint64).reshape(h, w, 3), rt.denoise_var_given_host(want[0], want[3], 1, feat, feat_spp, dn))


@pytest.mark.parametrize("size", FILTER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_buffers_form_equals_host(renderer, filter_cases, filter_host, level_kernel, size):
    fix, var_spp, var_count, count, spp, feat, feat_spp = filter_cases[size]
    for levels in (1, 2, 3, 4, 5, 8):
        for demodulate in (True, False):
            for with_count in (False, True):
                got, ms = renderer.denoise_var_given(fix, var_count if with_count else var_spp, spp, feat, feat_spp,
                                                     rt.make_denoise_var(levels, demodulate=demodulate), count=count if with_count else None)
                want = filter_host(size, levels, demodulate, with_count)
                assert np.array_equal(got, want), (levels, demodulate, with_count, int((got != want).any(axis=-1).sum()))
                assert ms > 0.0


def filter_device_form(renderer, filter_cases, filter_host, size, options):
    """The device form under guard words: the workspace is rt_denoise_var_workspace_bytes, and the words behind it and behind the output
    are intact afterwards; the inputs are left as they were."""
    import torch
    fix, var_spp, var_count, count, spp, feat, feat_spp = filter_cases[size]
    w, h = size
    dev = torch.device("cuda", 0)
    d_fix, d_feat, d_count = upload(fix, np.int64), upload(feat, np.int64), upload(count, np.int32)
    d_var = {False: upload(var_spp, np.int64), True: upload(var_count, np.int64)}
    words = rt.Renderer.denoise_var_workspace_bytes(w, h) // 8
    guard = 64
    d_work = torch.full((words + guard,), GUARD, dtype=torch.int64, device=dev)
    d_out = torch.full((h * w * 3 + guard,), GUARD, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for levels, demodulate, with_count in options:
        renderer.denoise_var_given_device(d_fix.data_ptr(), d_var[with_count].data_ptr(), spp, d_feat.data_ptr(), feat_spp, w, h,
                                          rt.make_denoise_var(levels, demodulate=demodulate), d_work.data_ptr(), d_out.data_ptr(),
                                          d_count_ptr=d_count.data_ptr() if with_count else 0, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_out[:h * w * 3].cpu().numpy().view(np.uint64).reshape(h, w, 3)
        want = filter_host(size, levels, demodulate, with_count)
        assert np.array_equal(got, want), (levels, demodulate, with_count, int((got != want).any(axis=-1).sum()))
    assert (d_work[words:] == GUARD).all().item() and (d_out[h * w * 3:] == GUARD).all().item()
    back = lambda t: t.cpu().numpy().view(np.uint64)
    assert np.array_equal(back(d_fix), fix) and np.array_equal(back(d_feat), feat)
    assert np.array_equal(back(d_var[False]).reshape(h, w, 3), tv.bits(var_spp)) and np.array_equal(back(d_var[True]).reshape(h, w, 3), tv.bits(var_count))


@pytest.mark.parametrize("size", FILTER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_device_form_equals_host_and_stays_inside_its_buffers(renderer, filter_cases, filter_host, level_kernel, size):
    filter_device_form(renderer, filter_cases, filter_host, size, ((5, True, True), (4, False, False), (1, True, False)))


def test_filter_device_form_with_six_levels_on_a_wide_frame(renderer, filter_cases, filter_host, level_kernel):
    filter_device_form(renderer, filter_cases, filter_host, (150, 9), ((6, True, True), (6, False, False)))


def test_a_call_leaves_the_render_path_alone(renderer, oracle_mod, book1_flat, cases):
    """No launch slot, no report in rt_last_stats; the dense render issued right after is Oracle B's; a context without a scene works."""
    w, h, spp = 96, 54, 4                                               # the smoke frame
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    renderer.render(cam, rt.make_params(w, h, 1))
    before = renderer.last_stats()
    (fix, count, s_spp, feat, feat_spp), (pfix, plen, pfeat, pspp, pm2) = cases[(37, 19)]
    cur, prev = tr.camera_pairs(37, 19)["subpixel_pan"]
    hist = (pfix, plen, pfeat, pspp, prev, pm2)
    acc, _, _, var, _ = renderer.temporal_var(fix, s_spp, feat, feat_spp, cur, hist)
    renderer.denoise_var_given(acc, var, 1, feat, feat_spp)
    assert renderer.last_stats() == before
    _, got_fix, st = renderer.render(cam, rt.make_params(w, h, spp, seed=1))
    want_fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(w, h, spp, seed=1))
    assert np.array_equal(got_fix, want_fix) and st["rays_traced"] == ost["rays_traced"] and st["samples"] == w * h * spp
    assert renderer.last_stats()["samples"] == w * h * spp               # rt_last_stats reports the render
    with rt.Renderer(0) as r:
        got = r.temporal_var(fix, s_spp, feat, feat_spp, cur, hist)
        shown, _ = r.denoise_var_given(got[0], got[3], 1, feat, feat_spp)
    assert same(got, rt.temporal_var_host(fix, s_spp, feat, feat_spp, cur, hist))
    assert np.array_equal(shown, rt.denoise_var_given_host(got[0], got[3], 1, feat, feat_spp))


def by_hand(renderer, cams, params, stride, feature_spp, tp, dn, lighting=None, **how):
    fixes = renderer.render_frames(cams, params, stride)[0] if lighting is None else None
    out, history = [], None
    for f, cam in enumerate(cams):
        begin = params.sample_begin + f * stride
        if lighting is None:
            fix = fixes[f]
        else:
            fix = renderer.render_wavefront(cam, rt.make_params(params.width, params.height, params.spp, sample_begin=begin, max_depth=params.max_depth,
                                                                seed=params.seed), lighting=lighting, **how)[0]
        feat, _, _ = renderer.render_features(cam, rt.make_params(params.width, params.height, feature_spp, sample_begin=begin, seed=params.seed), want_ids=False)
        acc, length, m2, var, _ = renderer.temporal_var(fix, params.spp, feat, feature_spp, cam, history, tp)
        history = (acc, length, feat, feature_spp, cam, m2)
        out.append(renderer.resolve_rgba8(renderer.denoise_var_given(acc, var, 1, feat, feature_spp, dn)[0], 1, flip=True))
    return np.stack(out), length, var, acc


def test_render_sequence_var_is_the_composition_made_by_hand(renderer, book1_flat):
    w, h, spp, fspp = 48, 27, 4, 6
    renderer.upload_scene(book1_flat)
    cams = rt.orbit_cameras(120, w, h)[:4]
    big = int(np.argmax(book1_flat["radius"][1:])) + 1
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {big: (4, 3.2, 2.4)})
    from rtiow_amd import render
    default = rt.make_denoise_var(sigma_color=render.TEMPORAL_VAR_SIGMA_COLOR)
    for params, tp, dn, lighting, how in ((rt.make_params(w, h, spp, sample_begin=3, seed=5), None, None, None, {}),
                                          (rt.make_params(w, h, spp, sample_begin=3, seed=5), rt.make_temporal(0.2, 0.6, 0.2, True, 0.75),
                                           rt.make_denoise_var(2, 2.5), None, {}),
                                          (rt.make_params(w, h, spp, seed=2, max_depth=8), None, None, L, dict(direct=True, sampling="weighted"))):
        got, lengths, var = renderer.render_sequence_var(cams, params, spp, fspp, temporal=tp, denoise=dn, lighting=lighting, **how)
        want, want_len, want_var, acc = by_hand(renderer, cams, params, spp, fspp, tp if tp is not None else rt.make_temporal(),
                                                dn if dn is not None else default, lighting, **how)
        assert got.shape == (4, h, w, 4) and got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(lengths, want_len)
        assert np.array_equal(tv.bits(var), tv.bits(want_var)) and (lengths == 4).any() and (var > 0.0).any()
        assert not np.array_equal(got[3], renderer.resolve_rgba8(acc, 1, flip=True))         # the filter moved the accumulated frame


def test_cli_sequence_frames_are_the_python_paths(renderer, book1_flat, tmp_path):
    w, h, spp, fspp = 48, 27, 5, 5                                      # (an odd spp: the sequence needs no half sums)
    exe = os.path.join(ROOT, "host", "rtiow_render")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    renderer.upload_scene(book1_flat)
    cams = rt.orbit_cameras(3, w, h)
    big = int(np.argmax(book1_flat["radius"][1:])) + 1
    L = rt.Lighting((0, 0, 0), (0, 0, 0), {big: (4, 3.2, 2.4)})
    lit = ["--wavefront", "--sky", "0,0,0:0,0,0", "--emit", f"{big}:4,3.2,2.4", "--direct-weighted", "--depth", "8"]
    base = [exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--spp", str(spp), "--feature-spp", str(fspp), "--orbit", "3", "--temporal",
            "--denoise-variance"]
    for name, extra, params, tp, dn, kw in (
            ("plain", [], rt.make_params(w, h, spp), None, None, {}),
            ("options", ["--alpha-min", "0.25", "--temporal-clamp", "0.5", "--denoise-levels", "2", "--sigma-color", "2.5"], rt.make_params(w, h, spp),
             rt.make_temporal(0.25, 0.5, 0.1, True, 0.5), rt.make_denoise_var(2, 2.5), {}),
            ("lit", lit, rt.make_params(w, h, spp, max_depth=8), None, None, dict(lighting=L, direct=True, sampling="weighted"))):
        prefix = str(tmp_path / name)
        run = subprocess.run([*base, *extra, "--out", prefix + ".png"], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "second moments carried" in run.stdout, run.stderr
        want, _, _ = renderer.render_sequence_var(cams, params, spp, fspp, temporal=tp, denoise=dn, **kw)
        for f in range(3):
            assert np.array_equal(rt.read_png(f"{prefix}_{f:04d}.png"), want[f]), (name, f)
    bad = subprocess.run([exe, "--denoise-variance", "--orbit", "2", "--spp", "8"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "goes with none of" in bad.stderr


# what tools/temporal_var_sweep.py measured with the host statements (profiles/temporal_var_sweep.txt): the filtered sequence's RMSE over
# the accumulated frame's at the shipped sigma_color, 0.01944 / 0.02063
MEASURED_RATIO = 0.9423


def test_quality_on_the_night_sequence(renderer):
    """Section 25's night scene -- random_scene(1), a black sky, sphere 528 radiating (4, 3.2, 2.4), weighted direct lighting, depth 16 --
    on section 16's geometry: 96 x 54, the first 6 cameras of orbit_cameras(180); every frame 8 spp with sample_stride 8 (seed 1), guides at
    8 spp; the last frame against a 1024-spp render of its camera (seed 7).  RMSE over all channels of the clipped linear means.  Four
    figures: noisy; accumulated only (rt_temporal_var's out_fix); accumulated then rt_denoise_var_given at the shipped default; the last
    frame alone through rt_denoise_var, rendered as 2 x 4.  The GPU's four equal the numpy statements' on the same sums, repr for repr.
    The filtered sequence's ratio to "accumulated only" is asserted at most the ratio tools/temporal_var_sweep.py measured with the host
    statement plus 0.10 (section 16's margin).  The measurement puts that ratio below 1 and the sequence below the single-frame figure, so
    both inequalities are asserted too.
    Measured (sigma_color 1.5, the swept value with the lowest final-frame RMSE): noisy 0.02545, accumulated 0.02063 (0.811 of noisy),
    accumulated + rt_denoise_var_given 0.01944 (0.9423 of accumulated, 0.764 of noisy), single frame rt_denoise_var 0.01986 (0.780 of
    noisy); 94 % of the last frame's hit pixels have history, 76 % at length >= 4."""
    w, h, spp, frames = 96, 54, 8, 6
    flat = rt.random_scene(1).flatten()
    cams = rt.orbit_cameras(180, w, h)[:frames]
    renderer.upload_scene(flat)
    kw = dict(lighting=rt.Lighting((0, 0, 0), (0, 0, 0), {528: (4, 3.2, 2.4)}), direct=True, sampling="weighted")
    fixes = [renderer.render_wavefront(cams[f], rt.make_params(w, h, spp, sample_begin=f * spp, seed=1, max_depth=16), **kw)[0] for f in range(frames)]
    feats = [renderer.render_features(cams[f], rt.make_params(w, h, spp, sample_begin=f * spp, seed=1), want_ids=False)[0] for f in range(frames)]
    begin = (frames - 1) * spp
    half = renderer.render_wavefront_pixels(cams[-1], rt.make_params(w, h, spp // 2, sample_begin=begin, seed=1, max_depth=16), **kw)[0]
    both = renderer.render_wavefront_pixels(cams[-1], rt.make_params(w, h, spp // 2, sample_begin=begin + spp // 2, seed=1, max_depth=16),
                                            into=half.copy(), **kw)[0]
    assert np.array_equal(both, fixes[-1])
    ref = dr.mean_of(renderer.render_wavefront(cams[-1], rt.make_params(w, h, 1024, seed=7, max_depth=16), **kw)[0], 1024)
    from rtiow_amd import render
    dn = rt.make_denoise_var(sigma_color=render.TEMPORAL_VAR_SIGMA_COLOR)
    history = None
    for f in range(frames):
        acc, length, m2, var, _ = renderer.temporal_var(fixes[f], spp, feats[f], spp, cams[f], history)
        history = (acc, length, feats[f], spp, cams[f], m2)
    shown, _ = renderer.denoise_var_given(acc, var, 1, feats[-1], spp, dn)
    single, _ = renderer.denoise_var(fixes[-1], half, spp, feats[-1], spp, rt.make_denoise_var())
    gpu = [dr.rmse(dr.mean_of(fixes[-1], spp), ref), dr.rmse(dr.mean_of(acc, 1), ref), dr.rmse(dr.mean_of(shown, 1), ref), dr.rmse(dr.mean_of(single, 1), ref)]
    s_acc, s_len, s_m2, s_var = tv.chain([(fixes[f], spp, feats[f], spp, cams[f]) for f in range(frames)])[-1]
    s_shown = tv.denoise_var_given(s_acc, s_var, 1, feats[-1], spp, sigma_color=render.TEMPORAL_VAR_SIGMA_COLOR)
    stated = [gpu[0], dr.rmse(dr.mean_of(s_acc, 1), ref), dr.rmse(dr.mean_of(s_shown, 1), ref),
              dr.rmse(dr.mean_of(vr.denoise_var(fixes[-1], half, spp, feats[-1], spp), 1), ref)]
    print(f"night sequence 96x54, 6 frames of 8 spp: noisy {gpu[0]:.5f} accumulated {gpu[1]:.5f} accumulated + rt_denoise_var_given {gpu[2]:.5f} "
          f"single frame rt_denoise_var {gpu[3]:.5f}; filtered / accumulated {gpu[2] / gpu[1]:.4f}, filtered / single {gpu[2] / gpu[3]:.4f}")
    assert [repr(x) for x in gpu] == [repr(x) for x in stated]
    assert np.array_equal(length, s_len) and np.array_equal(tv.bits(var), tv.bits(s_var))
    assert gpu[2] / gpu[1] <= MEASURED_RATIO + 0.10
    assert gpu[2] < gpu[1] and gpu[2] < gpu[3]
