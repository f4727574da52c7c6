"""Wavefront path steps on the GPU (rt_camera_rays*, rt_scatter*, rt_accumulate*, render_wavefront_torch) against
tests/wavefront_ref.py, everything bit for bit: doubles as u64 patterns (so that NaN compares and -0.0 differs from 0.0), the status
bytes, the advanced events, the u64 sums.  The whole frame: the wavefront integrator against the megakernel."""
import numpy as np
import pytest

import rtiow_amd as rt
import wavefront_ref as wr

SIZES = (1, 63, 64, 65, 257)            # a lone path, a wave less one, a full wave, a wave and one, a workgroup and one (the stride trip under the knob)
KNOB = "RTIOW_SHADE_GRID_BLOCKS"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, names):
    for name in names:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = bits(g) != bits(w) if w.dtype == np.float64 else g.view(w.dtype) != w
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: {g[bad][:3]} != {w[bad][:3]}"


def set_knob(monkeypatch, blocks):
    if blocks:
        monkeypatch.setenv(KNOB, blocks)
    else:
        monkeypatch.delenv(KNOB, raising=False)


def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def to_dev(a):
    """numpy -> a tensor on cuda:0; the unsigned 32-bit arrays travel as int32 holding the same bits."""
    torch, dev = torch_dev()
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def side_stream():
    torch, dev = torch_dev()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    return s


# ---- rt_camera_rays ----------------------------------------------------------------------------------------------------------------------

CAMERA_OUT = ("origin", "dir", "event")


def camera_want(sel):
    cam, pixel, sample, want = wr.camera_cases()
    return cam, pixel[sel], sample[sel], {k: want[k][sel] for k in CAMERA_OUT}


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, "1"])
def test_camera_rays_host_form(renderer, oracle_mod, monkeypatch, blocks):
    set_knob(monkeypatch, blocks)
    for n in SIZES:
        cam, pixel, sample, want = camera_want(slice(0, n))
        got = renderer.camera_rays(cam, wr.CW, wr.CH, wr.SEED, pixel, sample)
        assert got["event"].dtype == np.uint32 and got["kernel_ms"] > 0.0
        same(got, want, CAMERA_OUT)
    perm = np.random.default_rng(3).permutation(wr.N_CASES)                     # the same path gives the same bytes wherever it stands
    cam, pixel, sample, want = camera_want(perm)
    same(renderer.camera_rays(cam, wr.CW, wr.CH, wr.SEED, pixel, sample), want, CAMERA_OUT)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, "1"])
def test_camera_rays_device_and_torch_forms(renderer, oracle_mod, monkeypatch, blocks):
    """The torch form on a NON-default stream, and the device form on raw pointers into sentinel-filled buffers one path longer than the
    batch: nothing past the batch's end is written."""
    torch, dev = torch_dev()
    set_knob(monkeypatch, blocks)
    for n in SIZES:
        cam, pixel, sample, want = camera_want(slice(0, n))
        P, S = to_dev(pixel), to_dev(sample)
        stream = side_stream()
        with torch.cuda.stream(stream):
            got = rt.camera_rays_torch(renderer, cam, wr.CW, wr.CH, wr.SEED, P, S)
        stream.synchronize()
        assert got["event"].dtype == torch.int32 and got["origin"].shape == (n, 3)
        same({k: v.cpu().numpy() for k, v in got.items()}, want, CAMERA_OUT)
        O = torch.full((n + 1, 3), wr.F64_SENTINEL, dtype=torch.float64, device=dev)
        D = torch.full((n + 1, 3), wr.F64_SENTINEL, dtype=torch.float64, device=dev)
        E = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        renderer.camera_rays_device(cam, wr.CW, wr.CH, wr.SEED, n, P.data_ptr(), S.data_ptr(), O.data_ptr(), D.data_ptr(), E.data_ptr())
        torch.cuda.synchronize()
        same({"origin": O[:n].cpu().numpy(), "dir": D[:n].cpu().numpy(), "event": E[:n].cpu().numpy()}, want, CAMERA_OUT)
        assert (O[n] == wr.F64_SENTINEL).all().item() and (D[n] == wr.F64_SENTINEL).all().item() and E[n].item() == 0x5A5A5A5A
    with pytest.raises(ValueError):
        rt.camera_rays_torch(renderer, cam, wr.CW, wr.CH, wr.SEED, P.long(), S)
    with pytest.raises(ValueError, match="renderer's device"):
        rt.camera_rays_torch(renderer, cam, wr.CW, wr.CH, wr.SEED, P.cpu(), S.cpu())


@pytest.mark.gpu
def test_camera_rays_are_the_render_kernels(renderer, oracle_mod):
    """The book camera at 37 x 19, sample 0, seed 1: the rays tests/features_ref.py states for the feature kernel."""
    import features_ref as fr
    w, h = 37, 19
    cam = rt.book1_camera(w, h)
    ocam = fr.camera_from_rt(cam.to_rt_camera())
    pixel = np.arange(w * h, dtype=np.uint32)
    got = renderer.camera_rays(cam, w, h, 1, pixel, np.zeros(w * h, dtype=np.uint32))
    for g in (0, 36, 300, 702):
        o, d = fr.camera_ray(ocam, w, h, 1, g % w, g // w, 0)
        assert got["origin"][g].tolist() == list(o) and got["dir"][g].tolist() == list(d)


# ---- rt_scatter ----------------------------------------------------------------------------------------------------------------------------

SCATTER_OUT = ("out_origin", "out_dir", "attenuation", "status", "event")
SCATTER_IN = ("dirs", "index", "point", "normal", "front_face", "pixel", "sample", "event")


def scatter_want(sel):
    flat, inp, want = wr.scatter_cases()
    return flat, {k: inp[k][sel] for k in SCATTER_IN}, {k: want[k][sel] for k in SCATTER_OUT}


def prefilled(n):
    return {k: np.full((n, 3), wr.F64_SENTINEL) for k in ("out_origin", "out_dir", "attenuation")}


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, "1"])
def test_scatter_host_form(renderer, oracle_mod, monkeypatch, blocks):
    """Outputs prefilled with the sentinel: what the contract says is not written (everything of a MISS or a BAD_INDEX but the status,
    the ray of an absorbed path) still holds it -- the reference writes into the same prefilled arrays."""
    set_knob(monkeypatch, blocks)
    flat = wr.step_scene()
    renderer.upload_scene(flat)
    for n in SIZES:
        _, inp, want = scatter_want(slice(0, n))
        got = renderer.scatter(wr.SEED, out=prefilled(n), **inp)
        assert got["status"].dtype == np.uint8 and got["event"].dtype == np.uint32 and got["kernel_ms"] > 0.0
        same(got, want, SCATTER_OUT)
    perm = np.random.default_rng(4).permutation(wr.N_CASES)
    _, inp, want = scatter_want(perm)
    same(renderer.scatter(wr.SEED, out=prefilled(wr.N_CASES), **inp), want, SCATTER_OUT)
    # the caller's event array is an input of the Python wrapper: the advanced values come back as a copy
    assert np.array_equal(inp["event"], wr.scatter_cases()[1]["event"][perm])


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, "1"])
def test_scatter_device_and_torch_forms(renderer, oracle_mod, monkeypatch, blocks):
    """scatter_torch on a NON-default stream into sentinel-filled tensors (status included); event is advanced in place."""
    torch, dev = torch_dev()
    set_knob(monkeypatch, blocks)
    renderer.upload_scene(wr.step_scene())
    for n in SIZES:
        _, inp, want = scatter_want(slice(0, n))
        T = {k: to_dev(v) for k, v in inp.items()}
        out = {k: torch.full((n, 3), wr.F64_SENTINEL, dtype=torch.float64, device=dev) for k in ("out_origin", "out_dir", "attenuation")}
        out["status"] = torch.full((n,), wr.U8_SENTINEL, dtype=torch.uint8, device=dev)
        stream = side_stream()
        with torch.cuda.stream(stream):
            got = rt.scatter_torch(renderer, wr.SEED, out=out, **T)
        stream.synchronize()
        assert got["out_dir"] is out["out_dir"] and got["status"].dtype == torch.uint8
        res = {k: v.cpu().numpy() for k, v in got.items()}
        res["event"] = T["event"].cpu().numpy()
        same(res, want, SCATTER_OUT)
        assert (res["status"] != wr.U8_SENTINEL).all()                          # the status is always written
        fresh = rt.scatter_torch(renderer, wr.SEED, **{k: to_dev(v) for k, v in inp.items()})     # outputs allocated by the wrapper
        ok = want["status"] == wr.SCATTERED
        assert np.array_equal(fresh["status"].cpu().numpy(), want["status"])
        assert np.array_equal(bits(fresh["out_dir"].cpu().numpy()[ok]), bits(want["out_dir"][ok]))
    with pytest.raises(ValueError):
        rt.scatter_torch(renderer, wr.SEED, **{**T, "front_face": T["front_face"].int()})


@pytest.mark.gpu
def test_scatter_in_place(renderer, oracle_mod):
    """out_dir = dir, host form and device form: the separate-buffer result, and the direction of a path that did not scatter is kept."""
    torch, dev = torch_dev()
    renderer.upload_scene(wr.step_scene())
    _, inp, want = scatter_want(slice(0, wr.N_CASES))
    scattered = want["status"] == wr.SCATTERED
    expect = np.where(scattered[:, None], want["out_dir"], inp["dirs"])
    dirs = np.array(inp["dirs"])
    got = renderer.scatter(wr.SEED, out={**prefilled(wr.N_CASES), "out_dir": dirs}, **{**inp, "dirs": dirs})
    assert got["out_dir"] is dirs and np.array_equal(bits(dirs), bits(expect))
    same(got, want, ("out_origin", "attenuation", "status", "event"))
    # the device form on raw pointers, default stream
    n = wr.N_CASES
    T = {k: to_dev(v) for k, v in inp.items()}
    org = torch.full((n, 3), wr.F64_SENTINEL, dtype=torch.float64, device=dev)
    att = torch.full((n, 3), wr.F64_SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((n,), wr.U8_SENTINEL, dtype=torch.uint8, device=dev)
    renderer.scatter_device(wr.SEED, n, T["dirs"].data_ptr(), T["index"].data_ptr(), T["point"].data_ptr(), T["normal"].data_ptr(),
                            T["front_face"].data_ptr(), T["pixel"].data_ptr(), T["sample"].data_ptr(), T["event"].data_ptr(), org.data_ptr(),
                            T["dirs"].data_ptr(), att.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(T["dirs"].cpu().numpy()), bits(expect))
    same({"out_origin": org.cpu().numpy(), "attenuation": att.cpu().numpy(), "status": status.cpu().numpy(), "event": T["event"].cpu().numpy()},
         want, ("out_origin", "attenuation", "status", "event"))


@pytest.mark.gpu
def test_scatter_needs_a_scene_and_takes_no_launch_slot(oracle_mod):
    """RT_ERR_NO_SCENE from rt_scatter before an upload; the other two steps need no scene; rt_last_stats still reports the render."""
    _, inp, want = scatter_want(slice(0, 65))
    cam, pixel, sample, cwant = camera_want(slice(0, 65))
    with rt.Renderer(0) as r:
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\).*rt_upload_scene has not been called"):
            r.scatter(wr.SEED, **inp)
        same(r.camera_rays(cam, wr.CW, wr.CH, wr.SEED, pixel, sample), cwant, CAMERA_OUT)
        fix = np.zeros((4, 3), dtype=np.uint64)
        r.accumulate(fix, np.array([1, 1, 9], dtype=np.uint32), np.array([[0.5, 0.25, 1.0]] * 3))
        assert fix[1].tolist() == [1 << 32, 1 << 31, 1 << 33] and not fix[[0, 2, 3]].any()
        r.upload_scene(wr.step_scene())
        _, _, st = r.render(rt.book1_camera(16, 9), rt.make_params(16, 9, 2, seed=3))
        same(r.scatter(wr.SEED, out=prefilled(65), **inp), want, SCATTER_OUT)
        after = r.last_stats()
        assert after["rays_traced"] == st["rays_traced"] and after["samples"] == st["samples"] == 16 * 9 * 2
        # n == 0 succeeds and touches nothing
        empty = r.scatter(wr.SEED, **{k: v[:0] for k, v in inp.items()})
        assert empty["status"].shape == (0,) and r.camera_rays(cam, wr.CW, wr.CH, wr.SEED, pixel[:0], sample[:0])["event"].shape == (0,)
        assert r.accumulate(fix, pixel[:0], np.zeros((0, 3))) == 0.0
        with pytest.raises(rt.RtiowHipError, match="RT_FLAG_UNIFORM53"):
            r.scatter(wr.SEED, flags=rt.RT_FLAG_UNIFORM53, **inp)


# ---- rt_accumulate -------------------------------------------------------------------------------------------------------------------------

NPIX = 37


def accumulate_case(n):
    """n samples into a frame of 37 pixels: pixel numbers up to 44 (some past the end), so every pixel is hit several times; weights with
    NaN, negatives, infinities, values above RT_SAMPLE_CLAMP and exactly at it; sky directions of every length, zero and NaN among them;
    select bytes 0, 1 and other non-zero values; sums that start non-zero."""
    rng = np.random.default_rng(50 + n)
    pixel = rng.integers(0, NPIX + 8, n).astype(np.uint32)
    weight = rng.uniform(0.0, 2.0, (n, 3))
    special = [np.nan, -0.5, np.inf, -np.inf, 65536.0, 65537.5, 1e300, 0.0, -0.0, 2.0 ** -33, 1.0 - 2.0 ** -53]
    for k, v in enumerate(special[:n]):
        weight[k, k % 3] = v
    sky = rng.normal(size=(n, 3)) * rng.choice([1.0, 1e-5, 1e7], n)[:, None]
    if n > 40:
        sky[35], sky[36, 1], sky[37] = 0.0, np.nan, (0.0, -3.0, 0.0)
        pixel[38], pixel[39] = 2 ** 32 - 1, NPIX
    select = rng.choice([0, 1, 1, 2, 255], n).astype(np.uint8)
    fix0 = rng.integers(0, 1 << 60, (NPIX, 3), dtype=np.uint64)
    return pixel, weight, sky, select, fix0


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, "1"])
def test_accumulate(renderer, oracle_mod, monkeypatch, blocks):
    """Host form and torch form on a NON-default stream, with and without sky_dir, with and without select, against the reference."""
    torch, dev = torch_dev()
    set_knob(monkeypatch, blocks)
    for n in SIZES:
        pixel, weight, sky, select, fix0 = accumulate_case(n)
        for use_sky in (False, True):
            for use_sel in (False, True):
                sd, sl = sky if use_sky else None, select if use_sel else None
                want = wr.accumulate(fix0, pixel, weight, sd, sl)
                fix = np.array(fix0)
                assert renderer.accumulate(fix, pixel, weight, sd, sl) > 0.0
                assert np.array_equal(fix, want), (n, use_sky, use_sel)
                F = to_dev(fix0.view(np.int64))
                stream = side_stream()
                with torch.cuda.stream(stream):
                    rt.accumulate_torch(renderer, F, to_dev(pixel), to_dev(weight), to_dev(sd) if use_sky else None, to_dev(sl) if use_sel else None)
                stream.synchronize()
                assert np.array_equal(F.cpu().numpy().view(np.uint64), want), (n, use_sky, use_sel)
    assert (want != fix0).any()


@pytest.mark.gpu
def test_accumulate_rules(renderer, oracle_mod):
    """Duplicates of one pixel inside a batch sum exactly; NaN and negative weights add 0; a weight above RT_SAMPLE_CLAMP adds 2^48;
    select == 0 and pixel >= npix add nothing; the sky straight up is (0.5, 0.7, 1.0), straight down white."""
    q = lambda x: int(oracle_mod.load().oracle_b_quantize(float(x)))
    n = 200
    fix = np.zeros((3, 3), dtype=np.uint64)
    w = np.tile([0.3, 0.1, 0.7], (n, 1))
    renderer.accumulate(fix, np.full(n, 1, dtype=np.uint32), w)
    assert fix[1].tolist() == [n * q(0.3), n * q(0.1), n * q(0.7)] and not fix[[0, 2]].any()
    fix[:] = 0
    renderer.accumulate(fix, np.array([0, 0, 0, 2, 3, 2 ** 32 - 1], dtype=np.uint32),
                        np.array([[np.nan, -1.0, 1e9], [np.inf, -np.inf, 65536.0], [-0.0, 0.0, 2.0 ** -32], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]),
                        select=np.array([1, 7, 1, 0, 1, 1], dtype=np.uint8))
    assert fix[0].tolist() == [1 << 48, 0, (1 << 48) + (1 << 48) + 1] and not fix[1:].any()
    fix[:] = 0
    renderer.accumulate(fix, np.array([0, 1], dtype=np.uint32), np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]]),
                        sky_dir=np.array([[0.0, 5.0, 0.0], [0.0, -0.25, 0.0]]))
    assert fix[0].tolist() == [q(0.5), q(0.7), q(1.0)] and fix[1].tolist() == [q(2.0)] * 3


@pytest.mark.gpu
def test_two_accumulate_calls_on_two_streams_equal_one(renderer, oracle_mod):
    torch, dev = torch_dev()
    pixel, weight, sky, select, fix0 = accumulate_case(257)
    want = wr.accumulate(fix0, pixel, weight, sky, select)
    F = to_dev(fix0.view(np.int64))
    P, Wt, S, L = to_dev(pixel), to_dev(weight), to_dev(sky), to_dev(select)
    halves = [(slice(0, 100), side_stream()), (slice(100, 257), side_stream())]
    for sel, stream in halves:
        with torch.cuda.stream(stream):
            rt.accumulate_torch(renderer, F, P[sel].contiguous(), Wt[sel].contiguous(), S[sel].contiguous(), L[sel].contiguous())
    for _, stream in halves:
        stream.synchronize()
    assert np.array_equal(F.cpu().numpy().view(np.uint64), want)
    with pytest.raises(ValueError):
        rt.accumulate_torch(renderer, F.int(), P, Wt)


# ---- the whole frame -----------------------------------------------------------------------------------------------------------------------

W, H, SPP = 32, 18, 4


def frame_pair(renderer, book1_flat, max_depth):
    torch, dev = torch_dev()
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(W, H)
    p = rt.make_params(W, H, SPP, max_depth=max_depth, seed=1)
    _, dense, st = renderer.render(cam, p)
    fix, rays = rt.render_wavefront_torch(renderer, cam, p, batch=500)         # five batches, the last ragged
    torch.cuda.synchronize()
    assert fix.dtype == torch.int64 and tuple(fix.shape) == (H, W, 3)
    return fix.cpu().numpy().view(np.uint64), rays, dense, st


@pytest.mark.gpu
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_wavefront_frame_equals_the_megakernel(renderer, oracle_mod, book1_flat, max_depth):
    """render_wavefront_torch on the book scene, 32 x 18 x 4 spp: Renderer.render's u64 sums bit for bit, and rt_stats.rays_traced."""
    wave, rays, dense, st = frame_pair(renderer, book1_flat, max_depth)
    assert np.array_equal(wave, dense)
    assert rays == st["rays_traced"] and dense.any()
    if max_depth == 1:
        assert rays == W * H * SPP


@pytest.mark.gpu
def test_wavefront_frame_under_the_wave_candidate_scheme(renderer, oracle_mod, book1_flat, monkeypatch):
    monkeypatch.setenv("RTIOW_TRACE_CANDIDATES", "wave")
    wave, rays, dense, st = frame_pair(renderer, book1_flat, 50)
    assert np.array_equal(wave, dense) and rays == st["rays_traced"]


@pytest.mark.gpu
def test_wavefront_frame_resolves_to_the_dense_bytes(renderer, oracle_mod, book1_flat, golden_small):
    """rt_resolve_rgba8 on the wavefront's buffer = the bytes of the dense render; and the sums are Oracle B's (the committed golden)."""
    wave, rays, dense, st = frame_pair(renderer, book1_flat, 50)
    rgba, _ = renderer.render_rgba8(rt.book1_camera(W, H), rt.make_params(W, H, SPP, max_depth=50, seed=1), flip=True)
    assert np.array_equal(renderer.resolve_rgba8(wave, SPP, flip=True), rgba)
    want, _, ost = oracle_mod.render_b(oracle_mod.book1_camera(W, H), book1_flat, oracle_mod.make_params(W, H, SPP, max_depth=50, seed=1))
    assert np.array_equal(wave, want) and rays == ost["rays_traced"]
    with pytest.raises(ValueError):
        rt.render_wavefront_torch(renderer, rt.book1_camera(W, H), rt.make_params(W, H, SPP, flags=rt.RT_FLAG_UNIFORM53))
