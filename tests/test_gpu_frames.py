"""Frame batches (rt_render_frames / rt_render_frames_device / rt_render_frames_rgba8): n_frames cameras in ONE launch.
The contract: frame f of a batch equals, bit for bit, the dense render of cams[f] with sample_begin + f * sample_stride --
so every frame is compared with its own Oracle-B render (array_equal, no tolerances), on the small-grid kernel (the book
scene) and on the general one (10 001 spheres), with direct adds (1, 4 spp), blocks of 64-192 (8 spp) and blocks of 256
(24, 100 spp), at a frame size whose pixel-samples are a multiple of neither 64 nor 256 (frame boundaries fall inside
would-be work blocks)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rtiow_amd as rt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPPS = (1, 4, 8, 24, 100)


def _nine_cameras(w, h):
    asp = float(w) / float(h)
    return rt.orbit_cameras(6, w, h) + [
        rt.book1_camera(w, h),
        rt.Camera((-12, 0.3, 0.1), (12, 0.3, 0), (0, 1, 0), 40, asp, 0.05, 8),       # ground level along +x
        rt.Camera((0, 1, 0), (4, 1, 0), (0, 1, 0), 60, asp, 0.0, 1),                # inside the large glass sphere
    ]


def _oracle_frame(oracle_mod, cam, flat, w, h, spp, begin, seed):
    fix, _, st = oracle_mod.render_b(oracle_mod.camera_from_host(cam), flat, oracle_mod.make_params(w, h, spp, sample_begin=begin, seed=seed))
    return fix, st["rays_traced"]


def _oracle_prefixes(oracle_mod, cam, flat, w, h, begin, seed, spps):
    """Oracle-B sums and ray counts of the samples [begin, begin + spp) for every spp of `spps` (ascending), from additive passes."""
    out, acc, rays, lo = {}, np.zeros((h, w, 3), dtype=np.uint64), 0, 0
    for spp in spps:
        f, r = _oracle_frame(oracle_mod, cam, flat, w, h, spp - lo, begin + lo, seed)
        acc, rays, lo = acc + f, rays + r, spp
        out[spp] = (acc.copy(), rays)
    return out


def _check_batch(renderer, cams, w, h, spp, begin, stride, seed, want, want_bit0):
    """want[f] = (oracle fix, oracle rays) of frame f."""
    fix, st = renderer.render_frames(cams, rt.make_params(w, h, spp, sample_begin=begin, seed=seed), sample_stride=stride)
    assert fix.shape == (len(cams), h, w, 3)
    for f in range(len(cams)):
        assert np.array_equal(fix[f], want[f][0]), (spp, stride, f)
    assert st["samples"] == len(cams) * w * h * spp, (spp, stride)
    assert st["rays_traced"] == sum(r for _, r in want), (spp, stride)
    assert st["kernel_variant"] & 16 and (st["kernel_variant"] & 1) == want_bit0 and st["scan_mode"] == 5
    if spp < 5:
        assert st["direct_samples"] == st["samples"]
    return fix


def test_every_frame_equals_its_oracle_render_on_the_book_scene(renderer, oracle_mod, book1_flat):
    w, h, seed, begin = 97, 55, 7, 5
    assert (w * h) % 64 and all((w * h * s) % 64 for s in SPPS if s % 64)
    renderer.upload_scene(book1_flat)
    cams = _nine_cameras(w, h)
    assert len(cams) == 9
    # stride 0: every frame the samples [begin, begin + spp); stride 1000: frame f the samples [begin + 1000 f, ...): prefixes of one run each
    for stride in (0, 1000):
        pre = [_oracle_prefixes(oracle_mod, c, book1_flat, w, h, begin + f * stride, seed, SPPS) for f, c in enumerate(cams)]
        for spp in SPPS:
            _check_batch(renderer, cams, w, h, spp, begin, stride, seed, [pre[f][spp] for f in range(len(cams))], 1)
    # stride spp: the frames' sample ranges follow one another
    for spp in SPPS:
        want = [_oracle_frame(oracle_mod, c, book1_flat, w, h, spp, begin + f * spp, seed) for f, c in enumerate(cams)]
        _check_batch(renderer, cams, w, h, spp, begin, spp, seed, want, 1)


def test_every_frame_equals_its_oracle_render_on_the_general_kernel(renderer, oracle_mod):
    flat = rt.random_scene(1, grid=(-50, 49)).flatten()
    assert len(flat) == 10001
    w, h, seed = 96, 54, 2
    renderer.upload_scene(flat)
    cams = rt.orbit_cameras(4, w, h)
    for spp in (4, 24, 40):
        want = [_oracle_frame(oracle_mod, c, flat, w, h, spp, f * spp, seed) for f, c in enumerate(cams)]
        _check_batch(renderer, cams, w, h, spp, 0, spp, seed, want, 0)


def test_degenerate_batches(renderer, oracle_mod, book1_flat):
    w, h, seed, spp = 97, 55, 3, 24
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(w, h)
    p = rt.make_params(w, h, spp, seed=seed)
    _, dense, dst = renderer.render(cam, p)
    one, st = renderer.render_frames([cam], p)                                        # n_frames = 1 is rt_render's fix
    assert np.array_equal(one[0], dense) and st["rays_traced"] == dst["rays_traced"]
    F = 5
    same, _ = renderer.render_frames([cam] * F, p, sample_stride=0)                   # one camera F times, the same random numbers
    for f in range(F):
        assert np.array_equal(same[f], dense)
    split, st = renderer.render_frames([cam] * F, p, sample_stride=spp)               # ... and consecutive sample ranges: F * spp samples in all
    want, rays = _oracle_frame(oracle_mod, cam, book1_flat, w, h, F * spp, 0, seed)
    assert np.array_equal(split.sum(axis=0, dtype=np.uint64), want) and st["rays_traced"] == rays
    assert not np.array_equal(split[0], split[1])


def test_progressive_overlapped_passes_and_a_dense_launch_in_flight(renderer, oracle_mod, book1_flat):
    w, h, seed, F = 97, 55, 9, 5
    renderer.upload_scene(book1_flat)
    cams = rt.orbit_cameras(F, w, h)
    want = [_oracle_frame(oracle_mod, c, book1_flat, w, h, 41, 1000 * f, seed)[0] for f, c in enumerate(cams)]
    d_cams = torch.from_numpy(rt.cameras_to_array(cams)).cuda()
    d_fix = torch.zeros((F, h, w, 3), dtype=torch.int64, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    # passes [0, 30) and [30, 41) of the batch, accumulated into one zeroed buffer from two streams
    for k, (spp, begin) in enumerate(((30, 0), (11, 30))):
        p = rt.make_params(w, h, spp, sample_begin=begin, seed=seed, flags=rt.RT_FLAG_ACCUMULATE | rt.RT_FLAG_OVERLAPPED)
        renderer.render_frames_device(d_cams.data_ptr(), F, 1000, p, d_fix.data_ptr(), streams[k].cuda_stream)
    torch.cuda.synchronize()
    assert renderer.last_stats()["samples"] == F * w * h * 11
    got = d_fix.cpu().numpy().view(np.uint64)
    for f in range(F):
        assert np.array_equal(got[f], want[f]), f
    # a batch launch and a plain rt_render_device launch of another camera in flight together: each its own oracle frames
    other = rt.Camera((-12, 0.3, 0.1), (12, 0.3, 0), (0, 1, 0), 40, float(w) / float(h), 0.05, 8)
    want_other = _oracle_frame(oracle_mod, other, book1_flat, w, h, 41, 0, seed)[0]
    d_one = torch.full((h, w, 3), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_fix.fill_(0x5A5A5A5A)
    torch.cuda.synchronize()
    renderer.render_frames_device(d_cams.data_ptr(), F, 1000, rt.make_params(w, h, 41, seed=seed), d_fix.data_ptr(), streams[0].cuda_stream)
    renderer.render_device(other, rt.make_params(w, h, 41, seed=seed), d_one.data_ptr(), streams[1].cuda_stream)
    torch.cuda.synchronize()
    got = d_fix.cpu().numpy().view(np.uint64)
    for f in range(F):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(d_one.cpu().numpy().view(np.uint64), want_other)


@pytest.mark.parametrize("flip", [0, 1])
def test_one_call_to_bytes(renderer, oracle_mod, book1_flat, flip):
    w, h, seed, spp, stride = 97, 55, 4, 8, 8
    renderer.upload_scene(book1_flat)
    cams = _nine_cameras(w, h)[3:8]
    rgba, st = renderer.render_frames_rgba8(cams, rt.make_params(w, h, spp, seed=seed), sample_stride=stride, flip=bool(flip))
    assert rgba.shape == (len(cams), h, w, 4) and st["samples"] == len(cams) * w * h * spp
    for f, c in enumerate(cams):
        want, _ = _oracle_frame(oracle_mod, c, book1_flat, w, h, spp, f * stride, seed)
        assert np.array_equal(rgba[f], oracle_mod.resolve_b(want, spp, flip=bool(flip))), f
        single, _ = renderer.render_rgba8(c, rt.make_params(w, h, spp, sample_begin=f * stride, seed=seed), flip=bool(flip))
        assert np.array_equal(rgba[f], single), f


def test_a_rejected_call_touches_nothing_and_an_empty_batch_does_nothing(renderer, book1_flat):
    w, h, F = 64, 36, 3
    renderer.upload_scene(book1_flat)
    cams = rt.orbit_cameras(F, w, h)
    renderer.render_frames(cams, rt.make_params(w, h, 6))
    before = renderer.last_stats()
    d_cams = torch.from_numpy(rt.cameras_to_array(cams)).cuda()
    d_fix = torch.full((F, h, w, 3), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def call(n_frames=F, stride=0, cams_ptr=None, fix_ptr=None, r=renderer, **kw):
        spp = kw.pop("spp", 6)
        r.render_frames_device(d_cams.data_ptr() if cams_ptr is None else cams_ptr, n_frames, stride, rt.make_params(w, h, spp, **kw),
                               d_fix.data_ptr() if fix_ptr is None else fix_ptr, stream)

    rejected = [
        (dict(flags=rt.RT_FLAG_UNIFORM53), "RT_FLAG_UNIFORM53"), (dict(flags=rt.RT_FLAG_DIAG_STATS), "RT_FLAG_DIAG_STATS"),
        (dict(flags=rt.RT_FLAG_NO_FILTER), "RT_FLAG_NO_FILTER"), (dict(flags=0x20), "unknown flags"), (dict(shard_count=2), "shard_count"),
        (dict(n_frames=-1), "n_frames"), (dict(stride=-1), "sample_stride"),
        (dict(n_frames=2 ** 31 // (w * h) + 1), "at most 2^31"),
        (dict(stride=2 ** 30, sample_begin=10), "sample indices"), (dict(n_frames=1, sample_begin=2 ** 31 - 6), "spp/sample_begin"),
        (dict(n_frames=300000, spp=1000), "work blocks"),
        (dict(cams_ptr=0), "NULL"), (dict(fix_ptr=0), "NULL"),
    ]
    for kw, msg in rejected:
        with pytest.raises(rt.RtiowHipError, match=re.escape(msg)):
            call(**kw)
    with pytest.raises(rt.RtiowHipError, match="spp >= 1"):                          # to_rgba divides by the sample count
        renderer.render_frames_rgba8(cams, rt.make_params(w, h, 0))
    fresh = rt.Renderer(0)                                                          # no scene yet
    try:
        with pytest.raises(rt.RtiowHipError, match="rt_upload_scene"):
            call(r=fresh)
    finally:
        fresh.close()
    os.environ["RTIOW_SCAN_MODE"] = "1"                                             # a context of the VALU cross-check mode
    try:
        valu = rt.Renderer(0)
    finally:
        os.environ.pop("RTIOW_SCAN_MODE")
    try:
        valu.upload_scene(book1_flat)
        with pytest.raises(rt.RtiowHipError, match="scan mode 5"):
            call(r=valu)
    finally:
        valu.close()
    call(n_frames=0)                                                                # an empty batch: nothing happens
    empty, st = renderer.render_frames([], rt.make_params(w, h, 6))
    assert empty.shape == (0, h, w, 3) and st is None
    torch.cuda.synchronize()
    assert (d_fix.cpu().numpy() == 0x5A5A5A5A).all()
    after = renderer.last_stats()
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in before.items() if k != "kernel_ms"}
    call(max_depth=0)                                                               # black frames without a launch
    torch.cuda.synchronize()
    assert (d_fix.cpu().numpy() == 0).all()
    st = renderer.last_stats()
    assert st["samples"] == F * w * h * 6 and st["rays_traced"] == 0


def test_cli_writes_the_batch_as_numbered_pngs(renderer, book1_flat, tmp_path):
    w, h, spp, seed = 97, 55, 8, 5
    cams = _nine_cameras(w, h)[4:8]
    cam_file, scene_file = str(tmp_path / "cams.bin"), str(tmp_path / "scene.bin")
    rt.save_cameras(cam_file, cams)
    rt.save_scene(scene_file, book1_flat)
    renderer.upload_scene(book1_flat)
    exe = os.path.join(ROOT, "host", "rtiow_render")
    for stride_args, stride in (([], spp), (["--sample-stride", "0"], 0)):
        prefix = str(tmp_path / f"turn{stride}")
        run = subprocess.run([exe, "--scene", scene_file, "--cameras", cam_file, "--width", str(w), "--height", str(h), "--spp", str(spp),
                              "--seed", str(seed), "--out", prefix, *stride_args], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        want, _ = renderer.render_frames_rgba8(cams, rt.make_params(w, h, spp, seed=seed), sample_stride=stride, flip=True)
        for f in range(len(cams)):
            got = rt.read_png(f"{prefix}_{f:04d}.png")
            assert np.array_equal(np.asarray(got).reshape(h, w, 4), want[f]), (stride, f)
    for bad in (["--passes", "2"], ["--adaptive", "0.05"], ["--uniform53"], ["--two-calls"], ["--devices", "0"]):
        run = subprocess.run([exe, "--cameras", cam_file, *bad], capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "go with none of" in run.stderr, bad
