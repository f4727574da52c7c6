"""The device path queue on the GPU (rt_paths_begin_device, rt_paths_step_device, rt_render_wavefront*) against
tests/paths_ref.py, everything bit for bit: doubles as u64 patterns, the 32-bit words, the live counts, the u64 sums, the ray counts.
What a call must not write is prefilled with a sentinel and compared afterwards.  The whole frame: against the megakernel, the torch
reference integrator and the committed golden."""
import functools
import os
import subprocess

import numpy as np
import pytest

import paths_ref as pr
import rtiow_amd as rt
import wavefront_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "RTIOW_PATHS_GRID_BLOCKS"
U32_FIELDS, F64_FIELDS = ("pixel", "sample", "event"), ("origin", "dir", "throughput")
S32 = int(np.array(pr.SENTINEL_U32, dtype=np.uint32).view(np.int32))
COUNTS = (0, 1, 63, 64, 65, 256, 257, 513)      # nothing, a lone path, a wave less one, a wave, a wave and one, a workgroup, one more, two and one


def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def set_knob(monkeypatch, blocks):
    if blocks:
        monkeypatch.setenv(KNOB, blocks)
    else:
        monkeypatch.delenv(KNOB, raising=False)


def device_queue(capacity, q=None, count=None, alloc=None):
    """A PathQueue of `capacity` slots (its tensors `alloc` slots long), every word a sentinel; then the paths of the numpy queue `q` in
    slots [0, len) and the count word (default: len)."""
    torch, dev = torch_dev()
    Q = rt.PathQueue(alloc or capacity, dev)
    Q.capacity = capacity
    for f in U32_FIELDS + ("scratch", "count"):
        getattr(Q, f).fill_(S32)
    for f in F64_FIELDS:
        getattr(Q, f).fill_(pr.SENTINEL_F64)
    n = 0
    if q is not None:
        n = len(q["pixel"])
        for f in U32_FIELDS:
            getattr(Q, f)[:n] = torch.from_numpy(np.array(q[f]).view(np.int32)).to(dev)
        for f in F64_FIELDS:
            getattr(Q, f)[:n] = torch.from_numpy(np.array(q[f])).to(dev)
    if q is not None or count is not None:
        Q.count.fill_(int(np.array(n if count is None else count, dtype=np.uint32).view(np.int32)))
    return Q


def host(Q):
    """The queue's arrays as numpy, u32 / f64, whole."""
    out = {f: getattr(Q, f).cpu().numpy().view(np.uint32) for f in U32_FIELDS + ("count",)}
    out.update({f: getattr(Q, f).cpu().numpy() for f in F64_FIELDS})
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_queue(Q, want, what):
    """Slots [0, m) hold `want` bit for bit, the count word is m, and every slot at or past m still holds the sentinel."""
    got, m = host(Q), len(want["pixel"])
    assert int(got["count"][0]) == m, (what, int(got["count"][0]), m)
    for f in U32_FIELDS:
        assert np.array_equal(got[f][:m], want[f]), (what, f)
        assert (got[f][m:] == pr.SENTINEL_U32).all(), (what, f, "past the count")
    for f in F64_FIELDS:
        bad = bits(got[f][:m]) != bits(want[f])
        assert not bad.any(), f"{what} {f}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"
        assert (got[f][m:] == pr.SENTINEL_F64).all(), (what, f, "past the count")


# ---- rt_paths_begin_device -----------------------------------------------------------------------------------------------------------------

BEGIN = dict(spp=4, sample_begin=3, first_item=5)            # a first item inside a pixel, samples from 3 on


@functools.lru_cache(None)
def begin_reference():
    import oracle
    cam = wr.camera_cases()[0]                                # a wide lens: the lens draws matter
    q = pr.begin(oracle.camera_from_host(cam), wr.CW, wr.CH, pr.SEED, BEGIN["spp"], BEGIN["sample_begin"], BEGIN["first_item"], 257)
    for a in q.values():
        a.setflags(write=False)
    return cam, q


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["", "1"], ids=["grid", "one_block"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_begin_equals_the_reference(renderer, oracle_mod, monkeypatch, n, blocks):
    torch, dev = torch_dev()
    set_knob(monkeypatch, blocks)
    cam, want = begin_reference()
    Q = device_queue(300)
    renderer.paths_begin_device(cam, wr.CW, wr.CH, pr.SEED, BEGIN["spp"], BEGIN["sample_begin"], BEGIN["first_item"], n, Q.struct())
    torch.cuda.synchronize()
    check_queue(Q, pr.prefix(want, n), f"begin n={n}")
    assert (Q.scratch.cpu().numpy() == S32).all()


@pytest.mark.gpu
def test_begin_torch_on_a_side_stream(renderer, oracle_mod):
    torch, dev = torch_dev()
    cam, want = begin_reference()
    Q = device_queue(257)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        rt.paths_begin_torch(renderer, cam, wr.CW, wr.CH, pr.SEED, BEGIN["spp"], BEGIN["sample_begin"], BEGIN["first_item"], 257, Q)
    side.synchronize()
    check_queue(Q, want, "begin on a side stream")


# ---- rt_paths_step_device ------------------------------------------------------------------------------------------------------------------

def run_step(renderer, q, capacity, npix, *, count=None, alloc=None, rays0=5):
    """One step of the numpy queue `q` from a queue of `capacity` slots into another -> (in, out, the sums u64 [npix, 3], d_rays)."""
    torch, dev = torch_dev()
    A, B = device_queue(capacity, q, count=count, alloc=alloc), device_queue(capacity, alloc=alloc)
    fix = torch.zeros((npix, 3), dtype=torch.int64, device=dev)
    rays = torch.full((1,), rays0, dtype=torch.int64, device=dev)
    rt.paths_step_torch(renderer, pr.SEED, A, B, fix, rays)
    torch.cuda.synchronize()
    return A, B, fix.cpu().numpy().view(np.uint64), int(rays.item())


def check_step(renderer, q, want, capacity, npix, what, **kw):
    out, adds, live = want
    A, B, fix, rays = run_step(renderer, q, capacity, npix, **kw)
    check_queue(B, out, what)
    assert np.array_equal(fix, adds), what
    assert rays == 5 + live, (what, rays)
    return A, B


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["", "1"], ids=["grid", "one_block"])
@pytest.mark.parametrize("capacity", [513, 1024])
@pytest.mark.parametrize("count", COUNTS)
def test_step_on_the_hand_queue(renderer, oracle_mod, monkeypatch, count, capacity, blocks):
    """Every fate, full and empty waves, an empty workgroup: the survivors in order, the sky terms, the counts."""
    set_knob(monkeypatch, blocks)
    flat, q, _ = pr.hand_queue()
    renderer.upload_scene(flat)
    A, _ = check_step(renderer, pr.prefix(q, count), pr.hand_step(count), capacity, pr.HAND_NPIX, f"hand queue, {count} of {capacity}")
    got = host(A)
    assert int(got["count"][0]) == count                                        # *in->count is unchanged
    assert all((got[f][count:] == pr.SENTINEL_U32).all() for f in U32_FIELDS) and all((got[f][count:] == pr.SENTINEL_F64).all() for f in F64_FIELDS)


BW, BH, BSPP = 32, 18, 4


@functools.lru_cache(None)
def book_reference():
    """The first 513 items of the golden book frame and the reference's first and second bounce of them."""
    import oracle
    flat = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "book1_scene_seed1.npy"), allow_pickle=False).astype(rt.SPHERE_DTYPE))
    q0 = pr.begin(oracle.book1_camera(BW, BH), BW, BH, 1, BSPP, 0, 0, 513)
    one = {n: pr.step(flat, pr.prefix(q0, n), 1, BW * BH) for n in (257, 513)}
    two = pr.step(flat, one[513][0], 1, BW * BH)
    return flat, q0, one, two


def book_step(renderer, n, capacity=513):
    torch, dev = torch_dev()
    flat, q0, one, _ = book_reference()
    out, adds, live = one[n]
    A, B = device_queue(capacity, pr.prefix(q0, n)), device_queue(capacity)
    fix = torch.zeros((BH, BW, 3), dtype=torch.int64, device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    rt.paths_step_torch(renderer, 1, A, B, fix, rays)
    torch.cuda.synchronize()
    check_queue(B, out, f"book queue, {n}")
    assert np.array_equal(fix.cpu().numpy().view(np.uint64).reshape(-1, 3), adds) and int(rays.item()) == live


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["", "1"], ids=["grid", "one_block"])
@pytest.mark.parametrize("n", [257, 513])
def test_step_on_book_scene_queues(renderer, oracle_mod, monkeypatch, n, blocks):
    set_knob(monkeypatch, blocks)
    renderer.upload_scene(book_reference()[0])
    book_step(renderer, n)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}], ids=["no_grid", "grid_dim_9"])
def test_step_under_the_scene_knobs(oracle_mod, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rt.Renderer(0) as r:
        r.upload_scene(book_reference()[0])                                     # RTIOW_NO_GRID / RTIOW_GRID_DIM are read here
        book_step(r, 513)
        flat, q, _ = pr.hand_queue()
        r.upload_scene(flat)
        check_step(r, q, pr.hand_step(pr.HAND_N), 513, pr.HAND_NPIX, f"hand queue under {env}")


@pytest.mark.gpu
def test_a_count_above_the_capacity_is_read_as_the_capacity(renderer, oracle_mod):
    """*count = capacity + 5 over arrays twice as long, sentinel-filled past the capacity: the step is that of `capacity` paths, and no
    word past the capacity changes -- in `in`, which is rewritten in place, or in `out`."""
    flat, q, _ = pr.hand_queue()
    renderer.upload_scene(flat)
    cap = 100
    A, B = check_step(renderer, pr.prefix(q, cap), pr.hand_step(cap), cap, pr.HAND_NPIX, "clamped count", count=cap + 5, alloc=2 * cap)
    got = host(A)
    assert int(got["count"][0]) == cap + 5
    assert all((got[f][cap:] == pr.SENTINEL_U32).all() for f in U32_FIELDS) and all((got[f][cap:] == pr.SENTINEL_F64).all() for f in F64_FIELDS)
    words = int(rt._ffi.load().rt_path_scratch_words(cap))
    assert (A.scratch.cpu().numpy()[words:] == S32).all() and (B.scratch.cpu().numpy() == S32).all()


@pytest.mark.gpu
def test_two_chained_steps_equal_the_reference_loop(renderer, oracle_mod):
    """begin, then two steps A -> B -> A through the torch forms in a Python loop, with no host wait between them."""
    torch, dev = torch_dev()
    flat, q0, one, two = book_reference()
    renderer.upload_scene(flat)
    cam = rt.book1_camera(BW, BH)
    Q = [device_queue(513), device_queue(513)]
    fix = torch.zeros((BH, BW, 3), dtype=torch.int64, device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    rt.paths_begin_torch(renderer, cam, BW, BH, 1, BSPP, 0, 0, 513, Q[0])
    for k in range(2):
        rt.paths_step_torch(renderer, 1, Q[k & 1], Q[(k + 1) & 1], fix, rays)
    torch.cuda.synchronize()
    out, adds, live = two
    got, m = host(Q[0]), len(out["pixel"])
    assert int(got["count"][0]) == m and 0 < m < len(one[513][0]["pixel"])
    for f in U32_FIELDS:
        assert np.array_equal(got[f][:m], out[f]), f
    for f in F64_FIELDS:
        assert np.array_equal(bits(got[f][:m]), bits(out[f])), f
    want_fix = (one[513][1] + adds).reshape(BH, BW, 3)
    assert np.array_equal(fix.cpu().numpy().view(np.uint64), want_fix) and int(rays.item()) == 513 + live


# ---- the whole frame -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["257", ""], ids=["nine_batches", "one_batch"])
@pytest.mark.parametrize("max_depth", [50, 1, 3])
def test_frame_equals_the_megakernel(renderer, oracle_mod, book1_flat, monkeypatch, max_depth, batch):
    """Renderer.render_wavefront on the book scene, 32 x 18 x 4 spp: Renderer.render's u64 sums bit for bit, and rt_stats.rays_traced."""
    if batch:
        monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", batch)
    else:
        monkeypatch.delenv("RTIOW_WAVEFRONT_BATCH", raising=False)
    renderer.upload_scene(book1_flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=max_depth, seed=1)
    _, dense, st = renderer.render(cam, p)
    fix, rays = renderer.render_wavefront(cam, p)
    assert np.array_equal(fix, dense) and dense.any()
    assert rays == st["rays_traced"]
    if max_depth == 1:
        assert rays == BW * BH * BSPP


@pytest.mark.gpu
def test_frame_equals_the_torch_integrator_and_the_golden(renderer, oracle_mod, book1_flat, golden_small, monkeypatch):
    torch, dev = torch_dev()
    monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "500")
    renderer.upload_scene(book1_flat)
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=50, seed=1)
    fix, rays = renderer.render_wavefront(cam, p)
    ref, ref_rays = rt.render_wavefront_torch(renderer, cam, p, batch=500)
    torch.cuda.synchronize()
    assert np.array_equal(fix, ref.cpu().numpy().view(np.uint64)) and rays == ref_rays
    assert np.array_equal(fix, golden_small["fix"]) and rays == int(golden_small["rays_b"])
    assert np.array_equal(renderer.resolve_rgba8(fix, BSPP, flip=True), golden_small["rgba"])
    # the device form on torch's stream: the same sums, and the count in a device word
    d_fix = torch.full((BH, BW, 3), -1, dtype=torch.int64, device=dev)
    d_rays = torch.full((1,), -1, dtype=torch.int64, device=dev)
    renderer.render_wavefront_device(cam, p, d_fix.data_ptr(), d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_fix.cpu().numpy().view(np.uint64), fix) and int(d_rays.item()) == rays


@pytest.mark.gpu
def test_frames_of_one_context_with_a_growing_batch(oracle_mod, book1_flat, monkeypatch):
    """The context's queues are allocated by the first frame and regrown by the second, whose batch is larger; both frames are right."""
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, max_depth=50, seed=7, sample_begin=2)
    with rt.Renderer(0) as r:
        r.upload_scene(book1_flat)
        _, dense, st = r.render(cam, p)
        for batch in ("257", "1000", "300"):
            monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", batch)
            fix, rays = r.render_wavefront(cam, p)
            assert np.array_equal(fix, dense) and rays == st["rays_traced"], batch


@pytest.mark.gpu
def test_frame_of_a_hand_scene(renderer, oracle_mod, monkeypatch):
    """wavefront_ref.step_scene(): five spheres, every material, no ground -- most paths end in the sky at once."""
    monkeypatch.setenv("RTIOW_WAVEFRONT_BATCH", "333")
    renderer.upload_scene(wr.step_scene())
    cam = rt.Camera((0.0, 2.0, 14.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 40.0, 37 / 19, 0.1, 14.0)
    p = rt.make_params(37, 19, 3, max_depth=12, seed=pr.SEED)
    _, dense, st = renderer.render(cam, p)
    fix, rays = renderer.render_wavefront(cam, p)
    assert np.array_equal(fix, dense) and rays == st["rays_traced"] and rays > 37 * 19 * 3


@pytest.mark.gpu
def test_cpp_cli_wavefront_writes_the_default_runs_bytes(tmp_path):
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    one, two = str(tmp_path / "dense.ppm"), str(tmp_path / "wavefront.ppm")
    base = [exe, "--width", "64", "--height", "36", "--spp", "5", "--seed", "4"]
    subprocess.run(base + ["--out", one], check=True, timeout=120)
    subprocess.run(base + ["--out", two, "--wavefront"], check=True, timeout=120, env=dict(os.environ, RTIOW_WAVEFRONT_BATCH="4000"))
    assert open(one, "rb").read() == open(two, "rb").read()
    bad = subprocess.run(base + ["--out", two, "--wavefront", "--uniform53"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--wavefront" in bad.stderr


# ---- context rules -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_another_scan_mode_refuses_every_form(oracle_mod, book1_flat):
    """A context created under RTIOW_SCAN_MODE=1 has no tube tables: every form fails with RT_ERR_INVALID_ARGUMENT and touches nothing."""
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
            rt.paths_begin_torch(r, cam, BW, BH, 1, BSPP, 0, 0, 64, A)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            rt.paths_step_torch(r, 1, A, B, fix)
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            r.render_wavefront_device(cam, p, fix.data_ptr())
        with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
            r.render_wavefront(cam, p)
        torch.cuda.synchronize()
        assert (fix == 3).all()
        for Q, count in ((A, 7), (B, pr.SENTINEL_U32)):
            got = host(Q)
            assert int(got["count"][0]) == count
            assert all((got[f] == pr.SENTINEL_U32).all() for f in U32_FIELDS) and all((got[f] == pr.SENTINEL_F64).all() for f in F64_FIELDS)
    finally:
        r.close()


@pytest.mark.gpu
def test_no_launch_slot_is_taken_and_no_scene_is_an_error(oracle_mod, book1_flat):
    torch, dev = torch_dev()
    cam, p = rt.book1_camera(BW, BH), rt.make_params(BW, BH, BSPP, seed=1)
    with rt.Renderer(0) as r:
        A, B = device_queue(64), device_queue(64)
        fix = torch.zeros((BH, BW, 3), dtype=torch.int64, device=dev)
        rt.paths_begin_torch(r, cam, BW, BH, 1, BSPP, 0, 0, 64, A)                # the camera step needs no scene
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            rt.paths_step_torch(r, 1, A, B, fix)
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_wavefront(cam, p)
        r.upload_scene(book1_flat)
        r.render(cam, p)
        before = r.last_stats()
        rt.paths_step_torch(r, 1, A, B, fix)
        r.render_wavefront(cam, rt.make_params(BW, BH, 2, seed=9))
        torch.cuda.synchronize()
        assert r.last_stats() == before
