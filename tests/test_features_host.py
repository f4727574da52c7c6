"""First-hit feature buffers without a GPU: the reference (tests/features_ref.py) against hand scenes with analytic answers, the
context-free validation of the four entry points, and the rule of rt_features_to_f32 restated in numpy on synthetic sums (the GPU
test compares the device with that statement)."""
import ctypes as C
import math

import numpy as np
import pytest

import features_ref as fr
import rtiow_amd as rt
from rtiow_amd import _ffi

Q1 = 1 << 32        # the quantum's reciprocal: 1.0 on the 2^-32 grid


def central_ray(ocam):
    """The pinhole ray through the middle of the viewport (u = v = 0.5: no jitter, no lens)."""
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    fr.oracle.load().oracle_get_ray(C.byref(ocam), 0.5, 0.5, 0.0, 0.0, o, d)
    return o, d


def hit_of(flat, ocam):
    o, d = central_ray(ocam)
    idx, t, _, n, _ = fr.fast_hit(fr.Scene(flat), o, d, 1e-4)
    return idx, t, n


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    return {name: (flat, cam, oracle_mod.camera_from_host(cam)) for name, (flat, cam) in fr.hand_scenes().items()}


@pytest.fixture(scope="module")
def frames(scenes):
    """The reference's 16 x 16 x 1 frame of every hand scene, computed once."""
    return {name: fr.render_features(ocam, flat, 16, 16, 1) for name, (flat, _, ocam) in scenes.items()}


def test_quantize_is_the_oracles(oracle_mod):
    lib = oracle_mod.load()
    for x in (0.0, -0.0, 1.0, 0.5, 1e-12, 0.7 * 0.3, 4.000000000000001, 65535.99999, 65536.0, 1e9, math.inf, -1.0, math.nan, 2.0 ** -33):
        assert fr.quantize(x) == int(lib.oracle_b_quantize(x)), x
    assert fr.qs(1.0) == Q1 and fr.qs(-1.0) == (1 << 64) - Q1 and fr.qs(math.nan) == 0
    assert fr.qs(-(2.0 ** -33)) == (1 << 64) - 1 and fr.qs(2.0 ** -33) == 0                # floor, not truncation
    assert fr.qs(-1e9) == (1 << 64) - (65536 << 32) and fr.qs(math.inf) == 65536 << 32


def test_one_sphere_centre(scenes, frames):
    """A unit sphere 5 in front of a pinhole with focus distance 1: the central ray (length 1) hits at t = 4, normal (0, 0, 1)."""
    flat, _, ocam = scenes["one_sphere"]
    idx, t, n = hit_of(flat, ocam)
    assert idx == 0 and t == 4.0 and n == (0.0, 0.0, 1.0)
    feat, ids = frames["one_sphere"]
    # the four pixels around the centre: their rays cross the image plane (half height tan 20 deg = 0.364) within 0.1 x 0.728 of the
    # axis in x and y, i.e. d = (x, y, -1) with x^2 + y^2 <= 0.0106: t = (5 - sqrt(25 - 24 |d|^2)) / |d|^2 lies in [4, 4.094], n_z = 5 - t
    for j, i in ((7, 7), (7, 8), (8, 7), (8, 8)):
        assert ids[j, i] == 0 and feat[j, i, 7] == 1
        assert [int(x) for x in feat[j, i, 0:3]] == [Q1 // 4, Q1 // 2, 3 * Q1 // 4]
        assert 4.0 <= int(feat[j, i, 6]) / Q1 < 4.094
        assert 0.906 < int(feat[j, i, 5]) / Q1 <= 1.0                                       # towards the camera
    # the corners look past the sphere: nothing is added, the id is -1
    for j, i in ((0, 0), (0, 15), (15, 0), (15, 15)):
        assert ids[j, i] == -1 and not feat[j, i].any()
    assert 0 < int(feat[..., 7].sum()) < 256


def test_camera_inside_a_sphere(scenes, frames):
    """From (0, 0, 1) inside a sphere of radius 4 about the origin, looking down -z: t = 5, and the normal is flipped against
    the ray -- it points AT the camera."""
    flat, _, ocam = scenes["inside"]
    idx, t, n = hit_of(flat, ocam)
    assert idx == 0 and t == 5.0 and n == (0.0, 0.0, 1.0)
    feat, ids = frames["inside"]
    assert (ids == 0).all() and (feat[..., 7] == 1).all()                                   # every ray hits: alpha 1
    assert (feat[..., 5].view(np.int64) > 0).all()                                          # n_z > 0 everywhere


def test_coincident_spheres_the_later_one_wins(scenes, frames):
    flat, _, ocam = scenes["coincident"]
    idx, t, _ = hit_of(flat, ocam)
    assert idx == 1 and t == 4.0
    feat, ids = frames["coincident"]
    hit = feat[..., 7] == 1
    assert hit.any() and (ids[hit] == 1).all() and (ids[~hit] == -1).all()
    assert (feat[hit][:, 0:3] == np.array([3 * Q1 // 4, Q1 // 2, Q1 // 4], dtype=np.uint64)).all()
    # the same geometry as the single sphere: normals and depths agree word for word
    assert np.array_equal(feat[..., 3:8], frames["one_sphere"][0][..., 3:8])


def test_dialectric_albedo_is_one_by_kind(scenes, frames):
    flat, _, _ = scenes["glass"]
    assert tuple(flat[0]["albedo"]) == (0.3, 0.6, 0.9)                                      # the field is filled, and not read
    feat, ids = frames["glass"]
    hit = ids == 0
    assert hit.any() and (feat[hit][:, 0:3] == np.uint64(Q1)).all()


def test_negative_radius_flips_the_outward_normal(scenes, frames):
    """sphere.rs:37 divides by the (negative) radius: the outward normal points inwards, front_face is false, and
    HitRecord::new flips it back -- the same words as the positive radius."""
    flat, _, ocam = scenes["negative_radius"]
    idx, t, n = hit_of(flat, ocam)
    assert idx == 0 and t == 4.0 and n == (0.0, 0.0, 1.0)
    assert np.array_equal(frames["negative_radius"][0], frames["one_sphere"][0])


def test_lens_retries_run_on_into_later_blocks():
    """The book camera's pixels: about one sample in five redraws its lens point, some of them into block 1 and beyond."""
    blocks = [fr.camera_sample(37, 19, 1, i, 7, s)[4] for i in range(37) for s in range(5, 8)]
    assert min(blocks) == 1 and max(blocks) >= 2


# ---- the C ABI without a context --------------------------------------------------------------------------------------------------

def _err(lib):
    return lib.rt_last_error().decode()


def test_the_four_symbols_resolve():
    lib = _ffi.load()
    for name in ("rt_render_features_device", "rt_render_features", "rt_features_to_f32_device", "rt_features_to_f32"):
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert _ffi.RT_FEATURE_WORDS == 8 == rt.RT_FEATURE_WORDS


@pytest.mark.parametrize("kw,nullbuf,msg", [
    (dict(flags=_ffi.RT_FLAG_UNIFORM53), False, "RT_FLAG_UNIFORM53"),
    (dict(flags=_ffi.RT_FLAG_DIAG_STATS), False, "RT_FLAG_DIAG_STATS"),
    (dict(flags=_ffi.RT_FLAG_NO_FILTER), False, "RT_FLAG_NO_FILTER"),
    (dict(flags=0x40), False, "unknown flags"),
    (dict(shard_count=2), False, "shard_count must be 1"),
    (dict(spp=0), False, "spp >= 1"),
    (dict(), True, "feature buffer is NULL"),
    (dict(), False, "ctx is NULL"),
])
@pytest.mark.parametrize("host_form", [False, True])
def test_context_free_validation(kw, nullbuf, msg, host_form):
    """Every reason comes before the context is looked at: a caller without a device gets the precise message."""
    lib = _ffi.load()
    cam = rt.book1_camera(16, 9).to_rt_camera()
    p = rt.make_params(16, 9, kw.get("spp", 2), **{k: v for k, v in kw.items() if k != "spp"})
    buf = np.full(16 * 9 * 8, 0xABCD, dtype=np.uint64)
    ptr = None if nullbuf else buf.ctypes.data_as(C.c_void_p)
    if host_form:
        rc = lib.rt_render_features(None, C.byref(cam), C.byref(p), ptr, None, None)
    else:
        rc = lib.rt_render_features_device(None, C.byref(cam), C.byref(p), ptr, None, None)
    assert rc == -1 and msg in _err(lib), _err(lib)
    assert (buf == 0xABCD).all()


def test_to_f32_validation_without_a_context():
    lib = _ffi.load()
    buf = np.zeros(8, dtype=np.uint64)
    out = np.zeros(8, dtype=np.float32)
    b, o = buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args, msg in (((b, 0, 1, 1, o), "bad width/rows/spp"), ((b, 1, 1, 0, o), "bad width/rows/spp"), ((b, 1, -1, 1, o), "bad width/rows/spp"),
                      ((None, 1, 1, 1, o), "a buffer is NULL"), ((b, 1, 1, 1, None), "a buffer is NULL"), ((b, 1, 1, 1, o), "ctx is NULL")):
        assert lib.rt_features_to_f32(None, *args) == -1 and msg in _err(lib), (args, _err(lib))
        assert lib.rt_features_to_f32_device(None, *args, None) == -1 and msg in _err(lib), (args, _err(lib))


# ---- the rule of rt_features_to_f32 -----------------------------------------------------------------------------------------------

def test_to_f32_rule_in_numpy():
    q, spp = fr.synthetic_sums()
    f = fr.features_to_f32(q, spp)
    assert f.dtype == np.float32 and f.shape == q.shape
    assert not f[0, 0].any()                                                                # no sample hit: all zero, depth included
    assert f[0, 1].tolist() == [np.float32(0.5 / 3), np.float32(0.25 / 3), np.float32(1 / 3), np.float32(-1 / 3),
                                np.float32((Q1 // 3) / Q1 / 3), np.float32(-(2.0 ** -32) / 3), np.float32(5 + 12345 / Q1), np.float32(1 / 3)]
    assert f[0, 2].tolist()[0:4] == [1.0, np.float32((3 * Q1 - 1) / Q1 / 3), np.float32(2.0 ** -32 / 3), -1.0]
    assert f[0, 2, 6] == 65536.0 and f[0, 2, 7] == 1.0                                      # the mean over the HITTING samples
    assert f[0, 3, 4] == np.float32(-(2 + 2.0 ** -32) / 3) and f[0, 3, 5] == np.float32((2 + 2.0 ** -32) / 3)
    assert f[0, 3, 6] == np.float32(((1 << 55) + 12345678901) / Q1 / 2)
    zero = q[..., 7] == 0
    assert (f[zero][:, 6] == 0).all() and np.isfinite(f).all()
