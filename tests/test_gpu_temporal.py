"""Temporal accumulation on the GPU (rt_temporal, rt_temporal_device): both device forms against the library's CPU
statement (rt_temporal_host, which tests/test_temporal_host.py holds to the numpy statement of the contract), bit for bit; what a call
leaves alone; Renderer.render_sequence and the CLI against the composition made by hand; and the quality of the result on the book scene."""
import os
import subprocess

import numpy as np
import pytest

import features_ref as fr
import rtiow_amd as rt
import temporal_ref as tr
from rtiow_amd import _ffi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 2 x 2: one lane pair of one wave; 5 x 3: narrower than a tile; 37 x 19 and 70 x 45: ragged on both sides, several workgroups
PAIRS = ["identical", "subpixel_pan", "wide_pan", "facing_away", "roll_90", "fov", "nan_prev", "lens_radius", "orbit_step"]
GUARD = 0x5A5A5A5A


def differing(got, want):
    return f"{int((got[0] != want[0]).any(axis=-1).sum())} sums and {int((got[1] != want[1]).sum())} lengths of {got[1].size} pixels differ"


def same(got, want):
    return got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def cases():
    out = {}
    for w, h in tr.SIZES:
        frame, hist = tr.synthetic_frame(w, h, 3), tr.synthetic_history(w, h, 3)
        for a in (frame[0], frame[1], frame[3], hist[0], hist[1], hist[2]):
            a.setflags(write=False)
        out[(w, h)] = (frame, hist)
    return out


@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_buffers_form_equals_host(renderer, cases, size):
    w, h = size
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp) = cases[size]
    pairs = tr.camera_pairs(w, h)
    for pair in PAIRS:
        cur, prev = pairs[pair]
        hist = (pfix, plen, pfeat, pspp, prev)
        for options in tr.OPTION_SETS:
            for cnt in (None, count):
                tp = tr.make_options(**options)
                got = renderer.temporal(fix, spp, feat, feat_spp, cur, hist, tp, count=cnt)
                want = rt.temporal_host(fix, spp, feat, feat_spp, cur, hist, tp, count=cnt)
                assert same(got, want), (pair, options, cnt is not None, differing(got, want))
                assert got[2] > 0.0                                      # the kernel's time, from the call's own events
    got = renderer.temporal(fix, spp, feat, feat_spp, cur, None)
    assert same(got, rt.temporal_host(fix, spp, feat, feat_spp, cur, None)) and (got[1] == 1).all()


def upload(a, view):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).to(torch.device("cuda", 0))


@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_form_equals_host_and_stays_inside_its_buffers(renderer, cases, size):
    import torch
    w, h = size
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp) = cases[size]
    dev = torch.device("cuda", 0)
    d_fix, d_feat, d_count = upload(fix, np.int64), upload(feat, np.int64), upload(count, np.int32)
    d_pfix, d_plen, d_pfeat = upload(pfix, np.int64), upload(plen, np.int32), upload(pfeat, np.int64)
    guard = 64
    d_out = torch.full((h * w * 3 + guard,), GUARD, dtype=torch.int64, device=dev)
    d_len = torch.full((h * w + guard,), GUARD, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    pairs = tr.camera_pairs(w, h)
    for pair in PAIRS:
        cur, prev = pairs[pair]
        for options, with_count, with_history in ((tr.OPTION_SETS[0], False, True), (tr.OPTION_SETS[3], True, True), (tr.OPTION_SETS[1], True, False)):
            tp = tr.make_options(**options)
            history = (d_pfix.data_ptr(), d_plen.data_ptr(), d_pfeat.data_ptr(), pspp, prev) if with_history else None
            renderer.temporal_device(d_fix.data_ptr(), spp, d_feat.data_ptr(), feat_spp, cur, w, h, tp, d_out.data_ptr(), d_len.data_ptr(), history=history,
                                     d_count_ptr=d_count.data_ptr() if with_count else 0, stream=stream)
            torch.cuda.synchronize()
            got = (d_out[:h * w * 3].cpu().numpy().view(np.uint64).reshape(h, w, 3), d_len[:h * w].cpu().numpy().view(np.uint32).reshape(h, w))
            want = rt.temporal_host(fix, spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev) if with_history else None, tp,
                                    count=count if with_count else None)
            assert same(got, want), (pair, options, with_count, with_history, differing(got, want))
    assert (d_out[h * w * 3:] == GUARD).all().item() and (d_len[h * w:] == GUARD).all().item()
    for d, a in ((d_fix, fix), (d_feat, feat), (d_pfix, pfix), (d_pfeat, pfeat)):
        assert np.array_equal(d.cpu().numpy().view(np.uint64), a)
    assert np.array_equal(d_plen.cpu().numpy().view(np.uint32), plen) and np.array_equal(d_count.cpu().numpy().view(np.uint32), count)


def test_a_chain_of_three_frames_with_ping_pong_buffers_on_one_stream(renderer):
    import torch
    w, h = 70, 45
    cams = rt.orbit_cameras(180, w, h)[:3]
    frames = [tr.synthetic_frame(w, h, 40 + k) for k in range(3)]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    d_fix = [upload(f[0], np.int64) for f in frames]
    d_feat = [upload(f[3], np.int64) for f in frames]
    d_out = [torch.zeros(h * w * 3, dtype=torch.int64, device=dev) for _ in range(2)]
    d_len = [torch.zeros(h * w, dtype=torch.int32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    tp = rt.make_temporal()
    for k in range(3):                                                  # no host wait between the calls: the stream orders them
        wr, rd = k & 1, 1 - (k & 1)
        history = (d_out[rd].data_ptr(), d_len[rd].data_ptr(), d_feat[k - 1].data_ptr(), frames[k - 1][4], cams[k - 1]) if k else None
        renderer.temporal_device(d_fix[k].data_ptr(), frames[k][2], d_feat[k].data_ptr(), frames[k][4], cams[k], w, h, tp, d_out[wr].data_ptr(),
                                 d_len[wr].data_ptr(), history=history, stream=stream.cuda_stream)
    stream.synchronize()
    history = None
    for k in range(3):
        fix, _, spp, feat, feat_spp = frames[k]
        want = rt.temporal_host(fix, spp, feat, feat_spp, cams[k], history, tp)
        history = (want[0], want[1], feat, feat_spp, cams[k])
    got = (d_out[0].cpu().numpy().view(np.uint64).reshape(h, w, 3), d_len[0].cpu().numpy().view(np.uint32).reshape(h, w))
    assert same(got, want), differing(got, want)
    assert (want[1] == 3).any() and (want[1] == 1).any()


def test_a_call_leaves_the_render_path_alone(renderer, oracle_mod, book1_flat, cases):
    """No launch slot, no report in rt_last_stats; the dense render issued right after is Oracle B's; a context without a scene accumulates."""
    w, h, spp = 96, 54, 4                                               # the smoke frame
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    renderer.render(cam, rt.make_params(w, h, 1))
    before = renderer.last_stats()
    (fix, count, s_spp, feat, feat_spp), (pfix, plen, pfeat, pspp) = cases[(37, 19)]
    cur, prev = tr.camera_pairs(37, 19)["subpixel_pan"]
    renderer.temporal(fix, s_spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev))
    assert renderer.last_stats() == before
    _, got_fix, st = renderer.render(cam, rt.make_params(w, h, spp, seed=1))
    want_fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(w, h, spp, seed=1))
    assert np.array_equal(got_fix, want_fix) and st["rays_traced"] == ost["rays_traced"] and st["samples"] == w * h * spp
    assert renderer.last_stats()["samples"] == w * h * spp               # rt_last_stats reports the render
    with rt.Renderer(0) as r:
        got = r.temporal(fix, s_spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev))
    assert same(got, rt.temporal_host(fix, s_spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev)))


@pytest.mark.parametrize("form", ["device", "buffers"])
def test_rejections_through_the_device_forms_touch_nothing(renderer, form):
    """Every rejection with a live context: RT_ERR_INVALID_ARGUMENT, the reason, and the outputs untouched."""
    import torch
    lib = _ffi.load()
    arrays = tr.rejection_arrays()
    if form == "device":
        held = {k: upload(a, np.int64 if a.dtype == np.uint64 else np.int32) for k, a in arrays.items()}
        bufs = {k: t.data_ptr() for k, t in held.items()}
        torch.cuda.synchronize()
    else:
        bufs = {k: a.ctypes.data for k, a in arrays.items()}
    for kw, msg in tr.BAD:
        rc = tr.call_form(lib, form, kw, bufs, ctx=renderer._h, stream=None)
        assert rc == -1 and msg in lib.rt_last_error().decode(), (kw, lib.rt_last_error().decode())
    if form == "device":
        torch.cuda.synchronize()
        assert (held["out"] == 0xABCD).all().item() and (held["olen"] == 0xABCD).all().item()
    else:
        assert (arrays["out"] == 0xABCD).all() and (arrays["olen"] == 0xABCD).all()
    assert tr.call_form(lib, form, {}, bufs, ctx=renderer._h, stream=None) == 0          # ... and the same arguments, whole, are accepted
    if form == "device":
        torch.cuda.synchronize()
        assert (held["olen"] == 1).all().item()                         # (no pixel of these feature sums has a hit)
    else:
        assert (arrays["olen"] == 1).all()


def by_hand(renderer, cams, params, stride, feature_spp, tp, dn):
    fixes, _ = renderer.render_frames(cams, params, stride)
    out, history = [], None
    for f, cam in enumerate(cams):
        fp = rt.make_params(params.width, params.height, feature_spp, sample_begin=params.sample_begin + f * stride, seed=params.seed)
        feat, _, _ = renderer.render_features(cam, fp, want_ids=False)
        acc, length, _ = renderer.temporal(fixes[f], params.spp, feat, feature_spp, cam, history, tp)
        history = (acc, length, feat, feature_spp, cam)
        shown = renderer.denoise(acc, 1, feat, feature_spp, dn)[0] if dn is not None else acc
        out.append(renderer.resolve_rgba8(shown, 1, flip=True))
    return np.stack(out), length, fixes


def test_render_sequence_is_the_composition_made_by_hand(renderer, book1_flat):
    w, h, spp, fspp = 48, 27, 4, 6
    renderer.upload_scene(book1_flat)
    cams = rt.orbit_cameras(120, w, h)[:4]
    params = rt.make_params(w, h, spp, sample_begin=3, seed=5)
    for tp, dn in ((None, None), (rt.make_temporal(0.2, 0.6, 0.2, True, 0.75), rt.make_denoise(2))):
        got, lengths = renderer.render_sequence(cams, params, spp, fspp, temporal=tp, denoise=dn)
        want, want_len, fixes = by_hand(renderer, cams, params, spp, fspp, tp if tp is not None else rt.make_temporal(), dn)
        assert got.shape == (4, h, w, 4) and got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(lengths, want_len)
        assert (lengths == 4).any()
        assert not np.array_equal(got[3], renderer.resolve_rgba8(fixes[3], spp, flip=True))


def test_cli_temporal_frames_are_the_python_paths(renderer, book1_flat, tmp_path):
    w, h, spp, fspp = 48, 27, 4, 5
    exe = os.path.join(ROOT, "host", "rtiow_render")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    renderer.upload_scene(book1_flat)
    cams = rt.orbit_cameras(3, w, h)
    base = [exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--spp", str(spp), "--feature-spp", str(fspp), "--orbit", "3", "--temporal"]
    for name, extra, tp, dn in (("plain", [], rt.make_temporal(), None),
                                ("options", ["--alpha-min", "0.25", "--temporal-sigma-normal", "0.75", "--temporal-sigma-depth", "0.2", "--temporal-clamp", "0.5",
                                             "--denoise", "--denoise-levels", "2"], rt.make_temporal(0.25, 0.75, 0.2, True, 0.5), rt.make_denoise(2)),
                                ("no_clamp", ["--temporal-clamp", "-1"], rt.make_temporal(clamp=False), None)):
        prefix = str(tmp_path / name)
        run = subprocess.run([*base, *extra, "--out", prefix + ".png"], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "temporal: alpha_min" in run.stdout, run.stderr
        want, _ = renderer.render_sequence(cams, rt.make_params(w, h, spp), spp, fspp, temporal=tp, denoise=dn)
        for f in range(3):
            assert np.array_equal(rt.read_png(f"{prefix}_{f:04d}.png"), want[f]), (name, f)
    for extra in (["--temporal"], ["--temporal", "--orbit", "2", "--uniform53"], ["--temporal", "--orbit", "2", "--devices", "0"],
                  ["--temporal", "--orbit", "2", "--passes", "2"], ["--temporal", "--orbit", "2", "--adaptive", "0.1"], ["--temporal", "--orbit", "2", "--two-calls"],
                  ["--denoise", "--orbit", "2"]):
        bad = subprocess.run([exe, *extra], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "goes with none of" in bad.stderr, extra


def test_quality_on_the_book_scene(renderer):
    """Book scene random_scene(1) at 96 x 54, the first 6 cameras of orbit_cameras(180) (2 degrees per step), depth 50, 4 spp per frame with
    sample_stride 4 (seed 1), guides at 4 spp with each frame's sample_begin, default options; the last frame against a 512-spp render of
    its camera (seed 7).  RMSE over all channels of the clipped linear means.  Measured with the numpy statement of the contract on
    Oracle-B sums (tools/temporal_sweep.py --oracle): noisy 0.05675, accumulated 0.04113, ratio 0.725; the bound is that ratio + 0.10.
    Hit pixels that found valid history, per step: 93 94 93 93 93 %; at least 85 % are asked for."""
    w, h, spp, frames = 96, 54, 4, 6
    flat = rt.random_scene(1).flatten()
    cams = rt.orbit_cameras(180, w, h)[:frames]
    renderer.upload_scene(flat)
    fixes, _ = renderer.render_frames(cams, rt.make_params(w, h, spp, seed=1, max_depth=50), spp)
    feats = [renderer.render_features(cams[f], rt.make_params(w, h, spp, sample_begin=f * spp, seed=1), want_ids=False)[0] for f in range(frames)]
    _, ref_fix, _ = renderer.render(cams[-1], rt.make_params(w, h, 512, seed=7, max_depth=50))
    history, shares = None, []
    for f in range(frames):
        acc, length, _ = renderer.temporal(fixes[f], spp, feats[f], spp, cams[f], history)
        history = (acc, length, feats[f], spp, cams[f])
        if f:
            hit = feats[f][..., 7] != 0
            shares.append(float((length[hit] >= 2).mean()))
    stated = tr.chain([(fixes[f], spp, feats[f], spp, cams[f]) for f in range(frames)])[-1]
    ref = fr.fix_to_f64(ref_fix) / 512.0
    noisy = tr.rmse(fr.fix_to_f64(fixes[-1]) / float(spp), ref)
    accumulated, accumulated_stated = tr.rmse(fr.fix_to_f64(acc), ref), tr.rmse(fr.fix_to_f64(stated[0]), ref)
    print(f"temporal quality 96x54, 6 frames, 2 degrees per step: noisy {noisy:.5f} accumulated {accumulated:.5f} ratio {accumulated / noisy:.4f}; "
          f"hit pixels with history per step {' '.join(f'{100 * s:.1f}%' for s in shares)}")
    assert accumulated / noisy == accumulated_stated / noisy and np.array_equal(length, stated[1])
    assert accumulated / noisy < 0.825
    assert len(shares) == 5 and min(shares) >= 0.85
