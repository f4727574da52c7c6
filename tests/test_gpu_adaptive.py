"""Adaptive sampling on the GPU: the device selection equals the host's (same list, same order), rt_render_adaptive equals the
loop run in numpy on Oracle-B passes (render = take pass k at the active pixels) in count, fix and half, and the resolve with
per-pixel counts equals oracle.resolve_b taken per count.  All bit-exact."""
import os

import numpy as np
import pytest

import rtiow_amd as rt
from test_pixel_select_host import oracle_state, select_model

pytestmark = pytest.mark.gpu

W, H, STEP, CAP, THRESHOLD, FLOOR, SEED = 160, 90, 8, 256, 0.05, 0.01, 1


@pytest.fixture(scope="module")
def oracle_passes(oracle_mod, book1_flat):
    """The CAP / STEP dense Oracle-B passes of the frame: pass k = samples [k STEP, (k + 1) STEP)."""
    cam = oracle_mod.camera_from_host(rt.book1_camera(W, H))
    return [oracle_mod.render_b(cam, book1_flat, oracle_mod.make_params(W, H, STEP, sample_begin=k * STEP, seed=SEED))[0]
            for k in range(CAP // STEP)]


def adaptive_model(passes, step, cap, threshold, floor):
    h, w, _ = passes[0].shape
    fix = passes[0] + passes[1]
    half = passes[0].copy()
    count = np.full((h, w), 2 * step, dtype=np.uint32)
    active_per_round = []
    n = 2 * step
    while n < cap:
        lst = select_model(fix, half, count, n, threshold, floor)
        if len(lst) == 0:
            break
        active_per_round.append(len(lst))
        m = np.zeros(h * w, dtype=bool)
        m[lst] = True
        m = m.reshape(h, w)
        k = n // step
        fix[m] += passes[k][m] + passes[k + 1][m]
        half[m] += passes[k][m]
        count[m] += 2 * step
        n += 2 * step
    return fix, half, count, active_per_round


def test_device_selection_equals_the_host_selection(renderer, oracle_mod, book1_flat, oracle_passes):
    states = []
    fix, half = oracle_passes[0] + oracle_passes[1], oracle_passes[0].copy()
    states.append((fix, half, np.full((H, W), 2 * STEP, dtype=np.uint32), 2 * STEP, STEP, THRESHOLD))
    mf, mh, mc, _ = adaptive_model(oracle_passes[:8], STEP, 8 * STEP, THRESHOLD, FLOOR)               # a state with pixels that have left
    states.append((mf, mh, mc, 8 * STEP, STEP, THRESHOLD))
    f, hf, c = oracle_state(oracle_mod, book1_flat, 97, 61, 4, 2)                                      # (a width that is no multiple of anything)
    c[::5, ::3] = 4
    states.append((f, hf, c, 8, 4, 0.1))
    z = np.zeros((7, 9, 3), dtype=np.uint64)
    zz = np.full((7, 9, 3), 1 << 31, dtype=np.uint64)
    zh = zz >> np.uint64(1)
    zh[0, 0] = 0
    zh[6, 8] = 0
    states.append((zz, zh, np.full((7, 9), 16, dtype=np.uint32), 16, 8, 0.05))                          # corners
    states.append((z, z, np.full((7, 9), 16, dtype=np.uint32), 16, 8, 0.0))                             # all black: nothing
    for fix, half, count, n, step, thr in states:
        a = rt.make_adaptive(step, thr, FLOOR)
        host = rt.select_pixels_host(fix, half, count, n, a)
        dev = renderer.select_pixels(fix, half, count, n, a)
        assert np.array_equal(dev, host) and np.array_equal(host, select_model(fix, half, count, n, thr, FLOOR))
    assert len(rt.select_pixels_host(*states[0][:4], rt.make_adaptive(STEP, THRESHOLD, FLOOR))) > 1000


def test_device_selection_on_a_1200x675_state(renderer, book1_flat):
    w, h, step = 1200, 675, 4
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(w, h)
    _, p0, _ = renderer.render(cam, rt.make_params(w, h, step, seed=2))
    _, p1, _ = renderer.render(cam, rt.make_params(w, h, step, sample_begin=step, seed=2))
    fix, half, count = p0 + p1, p0, np.full((h, w), 2 * step, dtype=np.uint32)
    count[100:140, 300:500] = 4 * step
    for thr in (0.05, 0.3):
        a = rt.make_adaptive(step, thr, FLOOR)
        host = rt.select_pixels_host(fix, half, count, 2 * step, a)
        assert np.array_equal(renderer.select_pixels(fix, half, count, 2 * step, a), host)
        assert 1000 < len(host) < w * h - 8000
        assert np.array_equal(renderer.select_pixels(fix, half, count, 2 * step, a), host)             # the same list on every run


def test_render_adaptive_equals_the_model_on_oracle_passes(renderer, book1_flat, oracle_passes):
    mf, mh, mc, rounds = adaptive_model(oracle_passes, STEP, CAP, THRESHOLD, FLOOR)
    counts = np.unique(mc)
    share_min, share_cap = (mc == 2 * STEP).mean(), (mc == CAP).mean()
    print(f"model: mean {mc.mean():.1f} spp, {100 * share_min:.1f} % at {2 * STEP}, {100 * share_cap:.1f} % at {CAP}, "
          f"{len(counts)} distinct counts, active per round {rounds[:8]}")
    assert share_min >= 0.10 and share_cap >= 0.10 and len(counts) >= 8                                # (the model's result: no vacuous pass)
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(W, H)
    fix, half, count, st = renderer.render_adaptive(cam, rt.make_params(W, H, CAP, seed=SEED), rt.make_adaptive(STEP, THRESHOLD, FLOOR))
    assert np.array_equal(count, mc)
    assert np.array_equal(fix, mf)
    assert np.array_equal(half, mh)
    assert st["samples"] == int(mc.sum(dtype=np.uint64)) and st["rays_traced"] > st["samples"] and st["kernel_ms"] > 0
    fix2, none, count2, _ = renderer.render_adaptive(cam, rt.make_params(W, H, CAP, seed=SEED), rt.make_adaptive(STEP, THRESHOLD, FLOOR), want_half=False)
    assert none is None and np.array_equal(fix2, mf) and np.array_equal(count2, mc)


def test_render_adaptive_at_the_two_ends(renderer, oracle_mod, book1_flat, oracle_passes):
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(W, H)
    # a threshold so large that round 1 ends it
    fix, half, count, st = renderer.render_adaptive(cam, rt.make_params(W, H, CAP, seed=SEED), rt.make_adaptive(STEP, 1e9, FLOOR))
    assert (count == 2 * STEP).all() and np.array_equal(fix, oracle_passes[0] + oracle_passes[1]) and np.array_equal(half, oracle_passes[0])
    assert st["samples"] == W * H * 2 * STEP
    # threshold 0: every pixel whose halves differ at all goes on; on this scene that is every pixel, up to the cap
    cap = 64
    fix, half, count, st = renderer.render_adaptive(cam, rt.make_params(W, H, cap, seed=SEED), rt.make_adaptive(STEP, 0.0, FLOOR))
    assert (count == cap).all() and st["samples"] == W * H * cap
    _, dense, _ = renderer.render(cam, rt.make_params(W, H, cap, seed=SEED))
    assert np.array_equal(fix, dense) and np.array_equal(fix, sum(oracle_passes[:cap // STEP]))
    assert np.array_equal(half, sum(oracle_passes[0:cap // STEP:2]))


def test_resolve_with_per_pixel_counts(renderer, oracle_mod, oracle_passes):
    mf, _, mc, _ = adaptive_model(oracle_passes, STEP, CAP, THRESHOLD, FLOOR)
    for flip in (True, False):
        got = renderer.resolve_rgba8_counts(mf, mc, flip=flip)
        cc = mc[::-1] if flip else mc
        for c in np.unique(mc):
            want = oracle_mod.resolve_b(mf, int(c), flip=flip)
            assert np.array_equal(got[cc == c], want[cc == c]), c
    const = np.full((H, W), 40, dtype=np.uint32)
    fix40 = sum(oracle_passes[:5])
    assert np.array_equal(renderer.resolve_rgba8_counts(fix40, const), renderer.resolve_rgba8(fix40, 40))
    assert np.array_equal(renderer.resolve_rgba8_counts(fix40, const), oracle_mod.resolve_b(fix40, 40))


def test_cpp_cli_adaptive_writes_the_resolve_with_counts(renderer, tmp_path):
    """host/rtiow_render --adaptive: rt_render_adaptive + rt_resolve_rgba8_counts from the compiled host; the file holds the bytes the
    Python binding gets for the same scene, and the summary line reports the samples per pixel."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.skip("host CLI not built")
    out = str(tmp_path / "adaptive.ppm")
    run = subprocess.run([exe, "--width", str(W), "--height", str(H), "--spp", "64", "--seed", "4", "--adaptive", "0.05", "--step", "8", "--out", out],
                         check=True, timeout=300, capture_output=True, text=True)
    renderer.upload_scene(rt.random_scene(1).flatten())
    fix, _, count, st = renderer.render_adaptive(rt.book1_camera(W, H), rt.make_params(W, H, 64, seed=4), rt.make_adaptive(8, 0.05, 0.01), want_half=False)
    want = renderer.resolve_rgba8_counts(fix, count, flip=True)
    assert rt.read_ppm(out).tobytes() == want[..., :3].tobytes()
    assert f"{count.mean():.1f} samples per pixel (min {count.min()}, max {count.max()})" in run.stdout and f"{st['rays_traced']} rays" in run.stdout
