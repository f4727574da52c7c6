"""First-hit feature buffers on the GPU (rt_render_features*, rt_features_to_f32*): all eight words and the ids,
bit for bit, against the CPU reference of tests/features_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import features_ref as fr
import rtiow_amd as rt
from features_ref import same
from rtiow_amd import _ffi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOK = dict(w=37, h=19, spp=3, begin=5)         # neither side a multiple of 8; the book camera's aperture makes lens retries run on into B_1


@pytest.fixture(scope="module")
def book_ref(oracle_mod, book1_flat):
    """The reference's book frame (37 x 19, samples 5..7), computed once and left unchanged."""
    cam = rt.book1_camera(BOOK["w"], BOOK["h"])
    feat, ids = fr.render_features(oracle_mod.camera_from_host(cam), book1_flat, BOOK["w"], BOOK["h"], BOOK["spp"], sample_begin=BOOK["begin"])
    feat.setflags(write=False); ids.setflags(write=False)
    return cam, feat, ids


def book_params(**kw):
    return rt.make_params(BOOK["w"], BOOK["h"], BOOK["spp"], sample_begin=BOOK["begin"], **kw)


def test_book_scene_odd_frame(renderer, book1_flat, book_ref):
    cam, feat, ids = book_ref
    renderer.upload_scene(book1_flat)
    got = renderer.render_features(cam, book_params())
    same(got, (feat, ids))
    assert got[2] > 0.0                                                 # the kernel's time, from the call's own events
    assert 0 < int(feat[..., 7].sum()) < BOOK["w"] * BOOK["h"] * BOOK["spp"]        # hits and misses both occur
    # max_depth, tile_rows and RT_FLAG_OVERLAPPED change nothing; without ids the sums are the same
    alt = renderer.render_features(cam, book_params(max_depth=1, tile_rows=3, flags=rt.RT_FLAG_OVERLAPPED), want_ids=False)
    assert alt[1] is None and np.array_equal(alt[0], feat)


@pytest.mark.parametrize("env", [{"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}], ids=["no_grid", "grid_dim_9"])
def test_book_scene_other_tile_layouts(book1_flat, book_ref, env):
    """The same frame from a table without a grid (every tile scanned) and from a 9 x 9 grid (the wave's rectangle of cell tiles)."""
    cam, feat, ids = book_ref
    os.environ.update(env)
    try:
        r = rt.Renderer(0)
        r.upload_scene(book1_flat)                                      # RTIOW_NO_GRID / RTIOW_GRID_DIM are read here
        got = r.render_features(cam, book_params())
        r.close()
    finally:
        for k in env:
            os.environ.pop(k)
    same(got, (feat, ids))


def test_three_thousand_spheres_large_grid(renderer, oracle_mod):
    """~3 000 spheres: the large grid, many tiles outside a wave's footprint."""
    flat = rt.random_scene(1, grid=(-27, 27)).flatten()
    assert 2900 < len(flat) < 3100
    w, h, spp = 40, 24, 2
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(flat)
    same(renderer.render_features(cam, rt.make_params(w, h, spp)), fr.render_features(oracle_mod.camera_from_host(cam), flat, w, h, spp))


def test_small_scene_without_a_grid(renderer, oracle_mod):
    flat = rt.random_scene(1, grid=(-3, 3)).flatten()
    w, h, spp = 16, 9, 1
    (grid_dim, _), _, _ = rt.tile_layout_host(flat)
    assert grid_dim == 0
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(flat)
    same(renderer.render_features(cam, rt.make_params(w, h, spp)), fr.render_features(oracle_mod.camera_from_host(cam), flat, w, h, spp))


@pytest.mark.parametrize("name", ["one_sphere", "inside", "coincident", "glass", "negative_radius"])
def test_hand_scenes(renderer, oracle_mod, name):
    flat, cam = fr.hand_scenes()[name]
    renderer.upload_scene(flat)
    got = renderer.render_features(cam, rt.make_params(16, 16, 1))
    same(got, fr.render_features(oracle_mod.camera_from_host(cam), flat, 16, 16, 1))
    assert got[0][..., 7].any()
    if name == "coincident":
        assert set(np.unique(got[1]).tolist()) == {-1, 1}               # the later sphere wins on equal t
    if name == "glass":
        assert (got[0][got[1] == 0][:, 0:3] == np.uint64(1 << 32)).all()


def degenerate_camera(kind):
    """Cameras whose rays leave the filter's analysed range.  "zero": lower_left_corner = origin and a viewport of size 0, every
    direction is the zero vector (root = 0/0 = NaN for every sphere); "tiny": a viewport of size 1e-170, |d|^2 underflows to 0 while d
    does not (roots of -inf, +inf or NaN); "nan": a NaN in the viewport; "mixed": rays aimed at the scene's centre with
    |d|^2 <= 1e-20 for the first few columns only, so one wave holds rays of both kinds."""
    c = _ffi.rt_camera()
    c.origin = (C.c_double * 3)(13.0, 2.0, 3.0)
    c.u = (C.c_double * 3)(0.0, 0.0, 1.0)
    c.v = (C.c_double * 3)(0.0, 1.0, 0.0)
    c.lens_radius = 0.0
    if kind == "mixed":
        c.lower_left_corner = (C.c_double * 3)(13.0 - 13e-12, 2.0 - 2e-12, 3.0 - 3e-12)
        c.horizontal = (C.c_double * 3)(-13e-10, -2e-10, -3e-10)
        c.vertical = (C.c_double * 3)(0.0, 0.0, 0.0)
        return c
    scale = {"zero": 0.0, "tiny": 1e-170, "nan": 1.0}[kind]
    c.lower_left_corner = (C.c_double * 3)(13.0, 2.0, 3.0)
    c.horizontal = (C.c_double * 3)(scale * -0.3, float("nan") if kind == "nan" else 0.0, scale * 1.0)
    c.vertical = (C.c_double * 3)(scale * -0.1, scale * 1.0, scale * -0.05)
    return c


@pytest.mark.parametrize("kind", ["zero", "tiny", "nan", "mixed"])
def test_degenerate_directions_take_the_list_as_written(renderer, kind):
    """sphere.rs:29-33 accepts a NaN root and mod.rs:63-64 then takes every later sphere with a root >= t_min: such rays go through
    the whole list in list order, and their hit record (NaN normal -> 0, NaN depth -> 0, the LAST accepted sphere's albedo) is the
    reference's."""
    flat = rt.random_scene(1, grid=(-4, 4)).flatten()                   # ~80 small spheres + ground + the three big ones
    w, h, spp = 24, 14, 2
    cam = degenerate_camera(kind)
    renderer.upload_scene(flat)
    got = renderer.render_features(cam, rt.make_params(w, h, spp))
    want = fr.render_features(fr.camera_from_rt(cam), flat, w, h, spp)
    same(got, want)
    if kind == "zero":                                                  # every scan ends on the last sphere, through NaN roots
        assert (got[1] == len(flat) - 1).all() and (got[0][..., 7] == spp).all() and not got[0][..., 3:7].any()
    if kind == "mixed":                                                 # column 0 is outside the analysed range (|d|^2 <= 1e-20 in f32), column 23 inside
        a2 = lambda i: sum(np.float32(x) ** 2 for x in fr.camera_ray(fr.camera_from_rt(cam), w, h, 1, i, 0, 0)[1])
        assert a2(0) <= 1e-20 < a2(w - 1) and got[0][..., 7].all()


def test_context_states_that_refuse_a_feature_launch(book1_flat):
    """RT_ERR_NO_SCENE (-4) before an upload; RT_ERR_INVALID_ARGUMENT (-1) on a context created under RTIOW_SCAN_MODE=1, with or
    without a scene: nothing is written either way."""
    import torch
    w, h = 16, 9
    cam, p = rt.book1_camera(w, h), rt.make_params(w, h, 1)
    d_feat = torch.full((h, w, 8), 0x5A5A, dtype=torch.int64, device="cuda:0")
    with rt.Renderer(0) as r:
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\).*rt_upload_scene has not been called"):
            r.render_features_device(cam, p, d_feat.data_ptr())
        with pytest.raises(rt.RtiowHipError, match=r"\(-4\)"):
            r.render_features(cam, p)
    os.environ["RTIOW_SCAN_MODE"] = "1"
    try:
        r = rt.Renderer(0)                                               # RTIOW_SCAN_MODE is read here
    finally:
        os.environ.pop("RTIOW_SCAN_MODE")
    with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
        r.render_features_device(cam, p, d_feat.data_ptr())
    r.upload_scene(book1_flat)
    with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
        r.render_features_device(cam, p, d_feat.data_ptr())
    with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
        r.render_features(cam, p)
    r.close()
    torch.cuda.synchronize()
    assert (d_feat == 0x5A5A).all().item()


def test_accumulate_passes_equal_one_call(renderer, book1_flat):
    """2 + 3 samples (sample_begin 0 and 2, the second pass adding, without ids) == one call of 5; the ids are the first sample's."""
    import torch
    w, h = 37, 19
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    one, ids_one, _ = renderer.render_features(cam, rt.make_params(w, h, 5))
    first, ids_first, _ = renderer.render_features(cam, rt.make_params(w, h, 1))
    d_feat = torch.full((h, w, 8), 12345, dtype=torch.int64, device="cuda:0")          # (the first pass must overwrite it)
    d_ids = torch.full((h, w), -7, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    renderer.render_features_device(cam, rt.make_params(w, h, 2), d_feat.data_ptr(), d_ids.data_ptr(), stream)
    renderer.render_features_device(cam, rt.make_params(w, h, 3, sample_begin=2, flags=rt.RT_FLAG_ACCUMULATE), d_feat.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_feat.cpu().numpy().view(np.uint64), one)
    assert np.array_equal(d_ids.cpu().numpy(), ids_one) and np.array_equal(ids_one, ids_first)
    assert np.array_equal(first[..., 7] == 1, ids_first >= 0)


def test_features_to_f32_is_the_numpy_statement(renderer, book_ref):
    q, spp = fr.synthetic_sums()
    assert np.array_equal(renderer.features_to_f32(q, spp).view(np.uint32), fr.features_to_f32(q, spp).view(np.uint32))
    _, feat, _ = book_ref
    f = renderer.features_to_f32(feat, BOOK["spp"])
    assert np.array_equal(f.view(np.uint32), fr.features_to_f32(feat, BOOK["spp"]).view(np.uint32))
    hit = feat[..., 7] == BOOK["spp"]                                   # fully covered pixels: a unit normal's mean is at most 1 long
    assert hit.any() and (np.linalg.norm(f[hit][:, 3:6], axis=-1) < 1.0 + 1e-6).all() and (f[..., 7] <= 1.0).all()


def test_features_to_f32_beyond_one_grid(renderer):
    """rt_features_to_f32_device caps its grid at 8192 x 256 = 2 097 152 lanes and strides beyond: 2048 x 1026 pixels (a 3840 x 2160 frame
    has four times as many) take a second trip for the last 4 096, and the hand-made pixels of synthetic_sums() sit on the last twelve."""
    hand, spp = fr.synthetic_sums()
    w, h, Q1 = 2048, 1026, 1 << 32
    assert w * h > 8192 * 256 + hand.shape[0] * hand.shape[1]
    rng = np.random.default_rng(2048)
    q = np.zeros((h, w, 8), dtype=np.uint64)
    q[..., 0:3] = rng.integers(0, 3 * Q1, size=(h, w, 3), dtype=np.uint64)
    q[..., 3:6] = rng.integers(-3 * Q1, 3 * Q1, size=(h, w, 3), dtype=np.int64).view(np.uint64)
    q[..., 7] = rng.integers(0, 4, size=(h, w), dtype=np.uint64)
    q[..., 6] = rng.integers(0, 1 << 40, size=(h, w), dtype=np.uint64) * q[..., 7]
    q.reshape(-1, 8)[-12:] = hand.reshape(12, 8)
    got, want = renderer.features_to_f32(q, spp), fr.features_to_f32(q, spp)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want.reshape(-1, 8)[8192 * 256:].any() and np.array_equal(want.reshape(-1, 8)[-12:], fr.features_to_f32(hand, spp).reshape(12, 8))


def test_rejected_call_touches_nothing_and_dense_render_is_unchanged(renderer, oracle_mod, book1_flat):
    import torch
    w, h, spp = 96, 54, 4                                               # the smoke frame
    cam = rt.book1_camera(w, h)
    renderer.upload_scene(book1_flat)
    renderer.render(cam, rt.make_params(w, h, 1))
    before = renderer.last_stats()
    d_feat = torch.full((h, w, 8), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
    d_ids = torch.full((h, w), -7, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(rt.RtiowHipError, match="RT_FLAG_UNIFORM53"):
        renderer.render_features_device(cam, rt.make_params(w, h, spp, flags=rt.RT_FLAG_UNIFORM53), d_feat.data_ptr(), d_ids.data_ptr(), stream)
    torch.cuda.synchronize()
    assert (d_feat == 0x5A5A5A5A).all().item() and (d_ids == -7).all().item()
    assert renderer.last_stats() == before
    # a feature launch takes no launch slot and rt_last_stats does not report on it ...
    renderer.render_features_device(cam, rt.make_params(w, h, spp), d_feat.data_ptr(), d_ids.data_ptr(), stream)
    assert renderer.last_stats() == before
    # ... and the dense render issued right after it on the same context is still Oracle B's
    _, fix, st = renderer.render(cam, rt.make_params(w, h, spp, seed=1))
    want_fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(w, h, spp, seed=1))
    assert np.array_equal(fix, want_fix) and st["rays_traced"] == ost["rays_traced"]
    torch.cuda.synchronize()


def test_cli_writes_the_f32_array_as_npy(renderer, oracle_mod, book1_flat, tmp_path):
    w, h, spp = 32, 18, 2
    exe = os.path.join(ROOT, "host", "rtiow_render")
    scene_file, npy, img = str(tmp_path / "scene.bin"), str(tmp_path / "features.npy"), str(tmp_path / "image.ppm")
    rt.save_scene(scene_file, book1_flat)
    run = subprocess.run([exe, "--scene", scene_file, "--width", str(w), "--height", str(h), "--spp", str(spp), "--out", img, "--features", npy],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert os.path.getsize(npy) == 128 + h * w * 8 * 4
    got = np.load(npy, allow_pickle=False)
    assert got.dtype == np.dtype("<f4") and got.shape == (h, w, 8)
    cam = rt.book1_camera(w, h)
    want_sums, _ = fr.render_features(oracle_mod.camera_from_host(cam), book1_flat, w, h, spp)
    assert np.array_equal(got.view(np.uint32), fr.features_to_f32(want_sums, spp).view(np.uint32))
    renderer.upload_scene(book1_flat)
    assert np.array_equal(got.view(np.uint32), renderer.features_to_f32(want_sums, spp).view(np.uint32))
    for extra in (["--uniform53"], ["--adaptive", "0.05"], ["--devices", "0"], ["--orbit", "2"]):
        bad = subprocess.run([exe, "--features", npy, *extra], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "goes with none of" in bad.stderr, extra
