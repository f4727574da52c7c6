"""The denoiser without a GPU (rt_denoise_host): the library's CPU statement against the numpy statement of
the contract (tests/denoise_ref.py), bit for bit; the context-free validation of the four entry points; and rt_denoise_core.hpp alone
under ASan + UBSan in a stand-alone program."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import features_ref as fr
import rtiow_amd as rt
from rtiow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (37, 19), (70, 45)]


def differing(got, want):
    return f"{int((got != want).any(axis=-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


@pytest.fixture(scope="module")
def cases():
    """The synthetic frames, built once and left unchanged."""
    out = {}
    for w, h in SIZES:
        case = dr.synthetic_case(w, h)
        for a in (case[0], case[1], case[3]):
            a.setflags(write=False)
        out[(w, h)] = case
    return out


def test_the_abi_surface():
    lib = _ffi.load()
    for name in ("rt_denoise_workspace_bytes", "rt_denoise_device", "rt_denoise", "rt_denoise_host"):
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert C.sizeof(_ffi.rt_denoise) == 32 and _ffi.rt_denoise.sigma_color.offset == 8
    d = rt.make_denoise()
    assert (d.levels, d.flags, d.sigma_color, d.sigma_normal, d.sigma_depth) == (4, _ffi.RT_DENOISE_DEMODULATE, 0.35, 1.0, 0.2)
    assert rt.make_denoise(demodulate=False).flags == 0
    assert rt.Renderer.denoise_workspace_bytes(37, 19) == 37 * 19 * 16 * 8
    n = C.c_int64(-7)
    for w, h in ((0, 4), (4, 0), (65536, 32769)):
        assert lib.rt_denoise_workspace_bytes(w, h, C.byref(n)) == -1 and n.value == -7
    assert lib.rt_denoise_workspace_bytes(4, 4, None) == -1
    assert lib.rt_denoise_workspace_bytes(65536, 32768, C.byref(n)) == 0 and n.value == (1 << 31) * 128


def test_the_synthetic_frames_exercise_the_contract(cases):
    fix, count, spp, feat, feat_spp = cases[(37, 19)]
    assert (feat[..., 7] == 0).any() and (feat[..., 7] == feat_spp).any()                       # pixels with zero hits, and covered ones
    assert (feat[..., 3:6].view(np.int64) < 0).any() and int(fix.max()) > 1 << 53 and int(feat[..., 6].max()) > 1 << 53
    assert len(np.unique(count)) > 10 and count.min() >= 1
    # the edge-stops take values inside (0, 1): the filter moves the frame, and neither the colour nor the geometry term is idle
    c, m, n, z = dr.prepare(fix, None, spp, feat, feat_spp, True)
    assert (m == dr.ALBEDO_FLOOR).any() and (m > 1.0).any()
    base = dr.denoise(fix, spp, feat, feat_spp)
    assert (base != dr.quantize(c * m)).any()
    assert (dr.denoise(fix, spp, feat, feat_spp, sigma_color=1e6) != base).any()
    assert (dr.denoise(fix, spp, feat, feat_spp, sigma_normal=1e6, sigma_depth=1e6) != base).any()
    # a constant frame with constant guides is a fixed point of every level (all weights equal the kernel's)
    flat_fix = np.full((9, 11, 3), 3 * dr.Q1 // 4, dtype=np.uint64)
    flat_feat = np.zeros((9, 11, 8), dtype=np.uint64)
    assert np.array_equal(dr.denoise(flat_fix, 1, flat_feat, 1, levels=5, demodulate=False), flat_fix)


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_numpy_on_synthetic_frames(cases, size, levels):
    """1-5 levels: from 70 x 45 down, 4 s exceeds the frame on both sides; demodulate on and off; spp and a count buffer."""
    fix, count, spp, feat, feat_spp = cases[size]
    for demodulate in (True, False):
        for cnt in (None, count):
            dn = rt.make_denoise(levels, 0.35, 1.0, 0.2, demodulate)
            got = rt.denoise_host(fix, spp, feat, feat_spp, dn, count=cnt)
            want = dr.denoise(fix, spp, feat, feat_spp, levels=levels, demodulate=demodulate, count=cnt)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (demodulate, cnt is not None, differing(got, want))


def test_host_equals_numpy_with_other_sigmas_and_eight_levels(cases):
    fix, count, spp, feat, feat_spp = cases[(37, 19)]
    for levels, sc, sn, sd in ((8, 0.35, 1.0, 0.2), (3, 1e6, 0.1, 5.0), (2, 0.01, 1e-3, 1e-3), (4, 3.0, 2.0, 1e6)):
        got = rt.denoise_host(fix, spp, feat, feat_spp, rt.make_denoise(levels, sc, sn, sd, True), count=count)
        want = dr.denoise(fix, spp, feat, feat_spp, levels=levels, sigma_color=sc, sigma_normal=sn, sigma_depth=sd, count=count)
        assert np.array_equal(got, want), (levels, sc, sn, sd, differing(got, want))


@pytest.mark.parametrize("levels", [6, 7, 8])
def test_host_equals_numpy_at_levels_six_to_eight_on_a_wide_frame(levels):
    """150 x 9, hole steps 32, 64 and 128: the taps at +-128 of the columns 0..21 and 128..149 are inside the frame, every vertical tap
    but the centre row's is outside it.  What the GPU's levels 6-8 are held to (tests/test_gpu_denoise.py) is pinned here at that size.
    The colour width halves per level: at the default 0.35 these levels return their input on this frame, so the same is asked at
    45 ~ 0.35 * 2^7, where each of them moves pixels."""
    fix, count, spp, feat, feat_spp = dr.synthetic_case(150, 9)
    for sigma_color in (0.35, 45.0):
        for demodulate in (True, False):
            for cnt in (None, count):
                got = rt.denoise_host(fix, spp, feat, feat_spp, rt.make_denoise(levels, sigma_color, 1.0, 0.2, demodulate), count=cnt)
                want = dr.denoise(fix, spp, feat, feat_spp, levels=levels, sigma_color=sigma_color, demodulate=demodulate, count=cnt)
                assert np.array_equal(got, want), (sigma_color, demodulate, cnt is not None, differing(got, want))
    assert (want != dr.denoise(fix, spp, feat, feat_spp, levels=levels - 1, sigma_color=45.0, demodulate=False, count=count)).any()


def test_host_equals_numpy_on_an_oracle_render(oracle_mod, book1_flat):
    """Oracle B's sums and the reference's feature sums of the book scene, 37 x 19 x 4 spp."""
    w, h, spp = 37, 19, 4
    cam = rt.book1_camera(w, h)
    ocam = oracle_mod.camera_from_host(cam)
    fix, _, _ = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, seed=1))
    feat, _ = fr.render_features(ocam, book1_flat, w, h, spp)
    for levels in (1, 4):
        got = rt.denoise_host(fix, spp, feat, spp, rt.make_denoise(levels))
        want = dr.denoise(fix, spp, feat, spp, levels=levels)
        assert np.array_equal(got, want), differing(got, want)
    assert (got != fix).any()


BAD = [
    (dict(dn=None), "dn is NULL"), (dict(fix=None), "a buffer is NULL"), (dict(feat=None), "a buffer is NULL"), (dict(out=None), "a buffer is NULL"),
    (dict(levels=0), "levels must be 1..8"), (dict(levels=9), "levels must be 1..8"), (dict(flags=2), "unknown flags"), (dict(flags=0x80000001), "unknown flags"),
    (dict(sigma_color=0.0), "sigma"), (dict(sigma_normal=-1.0), "sigma"), (dict(sigma_depth=math.inf), "sigma"), (dict(sigma_color=math.nan), "sigma"),
    (dict(width=0), "bad width/height"), (dict(height=-3), "bad width/height"), (dict(width=65536, height=32769), "<= 2^31"),
    (dict(spp=0), "spp >= 1 without a count"), (dict(feat_spp=0), "feat_spp >= 1"),
]


@pytest.mark.parametrize("form", ["host", "device", "buffers"])
@pytest.mark.parametrize("kw,msg", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD])
def test_rejections_touch_nothing(kw, msg, form):
    """Every rejection, from every form, without a context: RT_ERR_INVALID_ARGUMENT, the reason, and out_fix untouched."""
    lib = _ffi.load()
    w, h = 4, 3
    fix = np.full((h, w, 3), 1 << 32, dtype=np.uint64)
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    out = np.full((h, w, 3), 0xABCD, dtype=np.uint64)
    work = np.zeros(h * w * 16, dtype=np.float64)
    dn = rt.make_denoise()
    for k in ("levels", "flags", "sigma_color", "sigma_normal", "sigma_depth"):
        if k in kw:
            setattr(dn, k, kw[k])
    ptr = lambda name, a: None if name in kw else a.ctypes.data_as(C.c_void_p)
    dnp = None if "dn" in kw else C.byref(dn)
    common = (kw.get("spp", 8), ptr("feat", feat), kw.get("feat_spp", 8), kw.get("width", w), kw.get("height", h), dnp)
    if form == "host":
        rc = lib.rt_denoise_host(ptr("fix", fix), None, *common, ptr("out", out))
    elif form == "buffers":
        rc = lib.rt_denoise(None, ptr("fix", fix), None, *common, ptr("out", out), None)
    else:
        rc = lib.rt_denoise_device(None, ptr("fix", fix), None, *common, work.ctypes.data_as(C.c_void_p), ptr("out", out), None)
    assert rc == -1 and msg in lib.rt_last_error().decode(), lib.rt_last_error().decode()
    assert (out == 0xABCD).all()


def test_the_forms_with_a_context_name_what_is_missing():
    lib = _ffi.load()
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    dn = rt.make_denoise()
    assert lib.rt_denoise_device(None, p, None, 1, p, 1, 1, 1, C.byref(dn), None, p, None) == -1 and "workspace is NULL" in lib.rt_last_error().decode()
    assert lib.rt_denoise_device(None, p, None, 1, p, 1, 1, 1, C.byref(dn), p, p, None) == -1 and "ctx is NULL" in lib.rt_last_error().decode()
    assert lib.rt_denoise(None, p, None, 1, p, 1, 1, 1, C.byref(dn), p, None) == -1 and "ctx is NULL" in lib.rt_last_error().decode()
    # a count buffer stands in for spp
    cnt = np.ones(1, dtype=np.uint32)
    out = np.zeros(3, dtype=np.uint64)
    assert lib.rt_denoise_host(p, cnt.ctypes.data_as(C.c_void_p), 0, p, 1, 1, 1, C.byref(dn), out.ctypes.data_as(C.c_void_p)) == 0


def test_core_header_alone_under_asan_and_ubsan(cases, tmp_path):
    """tests/denoise_san_main.cpp includes rt_denoise_core.hpp and nothing else of the library; the sanitizers watch it filter the 1 x 1,
    5 x 3 and 37 x 19 frames (buffers of exactly the size the filter may touch), and its checksum is numpy's."""
    assert shutil.which("g++")
    src = open(os.path.join(ROOT, "rtiow_amd", "csrc", "rt_denoise_core.hpp")).read()
    assert "#include <hip" not in src and src.count("#include") == 1
    exe = str(tmp_path / "denoise_san_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "denoise_san_main.cpp")], check=True, timeout=300)
    for (w, h), levels, demodulate, with_count in (((1, 1), 3, True, False), ((5, 3), 5, True, True), ((37, 19), 5, False, True), ((37, 19), 4, True, False)):
        fix, count, spp, feat, feat_spp = cases[(w, h)]
        path = str(tmp_path / f"case_{w}x{h}_{levels}.bin")
        with open(path, "wb") as f:
            f.write(np.array([w, h, spp, feat_spp, levels, int(demodulate), int(with_count)], dtype="<i8").tobytes())
            f.write(np.array([0.35, 1.0, 0.2], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(fix, dtype="<u8").tobytes())
            if with_count:
                f.write(np.ascontiguousarray(count, dtype="<u4").tobytes())
            f.write(np.ascontiguousarray(feat, dtype="<u8").tobytes())
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and not run.stderr, run.stderr
        want = dr.denoise(fix, spp, feat, feat_spp, levels=levels, demodulate=demodulate, count=count if with_count else None)
        assert int(run.stdout.strip(), 16) == dr.checksum(want), (w, h, levels)
