"""Adaptive sampling without a GPU: rt_select_pixels_host (the library's own CPU statement of the selection rule of
include/rtiow_hip.h) against a numpy statement of the same rule written here; the argument validation of the pixel-list and
adaptive entry points; and the proof that the pixel-list kernel variant left the existing kernels' machine code alone
(tools/isa_fingerprint.py against the parent commit's output, profiles/isa_fingerprint_before_pixel_lists.txt)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rtiow_amd as rt
from rtiow_amd import _ffi
from isa_pins import fingerprint_lines as _fingerprint_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def select_model(fix, half, count, n, threshold, dark_floor):
    """The rule as the header states it: integers for d_c, float64 for the rest in the written order, dilation by padding."""
    fix = np.asarray(fix, dtype=np.uint64)
    half = np.asarray(half, dtype=np.uint64)
    h, w = count.shape
    t = (2 * half.astype(np.int64) - fix.astype(np.int64))          # |2 half - fix| <= fix < 2^63
    d = np.abs(t).astype(np.uint64)
    D = (d[..., 0].astype(np.float64) + d[..., 1].astype(np.float64)) + d[..., 2].astype(np.float64)
    S = (fix[..., 0].astype(np.float64) + fix[..., 1].astype(np.float64)) + fix[..., 2].astype(np.float64)
    sc = np.float64(1.0) / (np.float64(n) * np.float64(4294967296.0))
    err = (D * sc) / np.sqrt(np.maximum(S * sc, np.float64(dark_floor)))
    cand = count == n
    noisy = cand & ~(err <= threshold)
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = noisy
    near = np.zeros((h, w), dtype=bool)
    for dj in range(3):
        for di in range(3):
            near |= pad[dj:dj + h, di:di + w]
    return np.flatnonzero((cand & near).reshape(-1)).astype(np.uint32)


def oracle_state(oracle_mod, flat, w, h, step, passes, seed=1):
    """fix / half / count after `passes` (even) dense passes of `step` samples, assembled from Oracle-B passes."""
    cam = oracle_mod.camera_from_host(rt.book1_camera(w, h))
    fix = np.zeros((h, w, 3), dtype=np.uint64)
    half = np.zeros((h, w, 3), dtype=np.uint64)
    for k in range(passes):
        f, _, _ = oracle_mod.render_b(cam, flat, oracle_mod.make_params(w, h, step, sample_begin=k * step, seed=seed))
        fix += f
        if k % 2 == 0:
            half += f
    return fix, half, np.full((h, w), passes * step, dtype=np.uint32)


@pytest.mark.parametrize("w,h,step,passes,threshold", [(64, 36, 4, 2, 0.05), (48, 27, 8, 4, 0.02), (40, 30, 2, 2, 0.2), (33, 17, 4, 2, 0.0)])
def test_host_selection_equals_the_numpy_rule_on_oracle_states(oracle_mod, book1_flat, w, h, step, passes, threshold):
    fix, half, count = oracle_state(oracle_mod, book1_flat, w, h, step, passes)
    n = passes * step
    # some pixels have already left the active set: they are no candidates and make no neighbour active
    count[::5, ::3] = n - 2 * step if n > 2 * step else n + 2
    want = select_model(fix, half, count, n, threshold, 0.01)
    got = rt.select_pixels_host(fix, half, count, n, rt.make_adaptive(step, threshold, 0.01))
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    if threshold > 0:
        assert 0 < len(want) < w * h                                     # (not a vacuous comparison)
    else:
        assert len(want) == int((count == n).sum()) or len(want) > 0


def _state(w, h, n, value=1 << 30):
    """every pixel converged: both halves equal (fix = 2 half)"""
    half = np.full((h, w, 3), value, dtype=np.uint64)
    return 2 * half, half, np.full((h, w), n, dtype=np.uint32)


@pytest.mark.parametrize("j,i,size", [(0, 0, 4), (0, 8, 4), (6, 0, 4), (6, 8, 4), (0, 4, 6), (3, 0, 6), (3, 4, 9)])
def test_one_noisy_pixel_activates_its_clipped_neighbourhood(j, i, size):
    w, h, n = 9, 7, 16
    fix, half, count = _state(w, h, n)
    half[j, i] = 0                                                       # all of the pixel's light in the odd passes: err is large
    a = rt.make_adaptive(8, 0.05, 0.01)
    got = rt.select_pixels_host(fix, half, count, n, a)
    assert np.array_equal(got, select_model(fix, half, count, n, 0.05, 0.01))
    assert len(got) == size
    jj, ii = np.divmod(got.astype(np.int64), w)
    assert (np.abs(jj - j) <= 1).all() and (np.abs(ii - i) <= 1).all() and (np.diff(got.astype(np.int64)) > 0).all()


def test_error_equal_to_the_threshold_is_not_noisy():
    """err = (D sc) / sqrt(max(S sc, floor)) with D = 3 * 2^32 * n * 2^-4, S = 3 * 2^32 * n: D sc = 3/16, S sc = 3 -> err = 0.1875 / sqrt(3)."""
    w, h, n = 5, 4, 16
    fix = np.full((h, w, 3), n << 32, dtype=np.uint64)
    half = np.full((h, w, 3), (n << 31) + (n << 27), dtype=np.uint64)   # 2 half - fix = n * 2^28 = fix / 16
    count = np.full((h, w), n, dtype=np.uint32)
    err = np.float64(0.1875) / np.sqrt(np.float64(3.0))
    assert len(rt.select_pixels_host(fix, half, count, n, rt.make_adaptive(8, float(err), 0.01))) == 0
    assert len(rt.select_pixels_host(fix, half, count, n, rt.make_adaptive(8, float(np.nextafter(err, 0.0)), 0.01))) == w * h
    assert np.array_equal(select_model(fix, half, count, n, float(np.nextafter(err, 0.0)), 0.01), np.arange(w * h))


def test_black_pixels_are_decided_by_the_floor_not_by_a_nan():
    w, h, n = 6, 5, 8
    z = np.zeros((h, w, 3), dtype=np.uint64)
    count = np.full((h, w), n, dtype=np.uint32)
    assert len(rt.select_pixels_host(z, z, count, n, rt.make_adaptive(4, 0.0, 1e-300))) == 0     # err = 0 / sqrt(floor) = 0 <= 0
    assert len(select_model(z, z, count, n, 0.0, 1e-300)) == 0


def test_pixels_with_another_count_are_never_selected_and_activate_nobody():
    w, h, n = 8, 6, 32
    fix, half, count = _state(w, h, n)
    half[2, 3] = 0
    half[4, 6] = 0
    count[2, 3] = 16                                                     # noisy by its sums, but it left the active set at 16 samples
    got = rt.select_pixels_host(fix, half, count, n, rt.make_adaptive(8, 0.05, 0.01))
    assert np.array_equal(got, select_model(fix, half, count, n, 0.05, 0.01))
    assert 2 * w + 3 not in got and len(got) == 9                        # only (4, 6)'s 3 x 3, all of it inside the frame
    count[3, 6] = 48                                                     # a neighbour that is no candidate is not selected either
    got = rt.select_pixels_host(fix, half, count, n, rt.make_adaptive(8, 0.05, 0.01))
    assert 3 * w + 6 not in got and np.array_equal(got, select_model(fix, half, count, n, 0.05, 0.01))


def test_sums_near_two_to_the_62():
    """n = 16 382 saturated samples of 2^48: sums of 2^62 - 2^49, differences up to the whole sum -- still exact in i64."""
    w, h, n = 7, 5, 16382
    rng = np.random.default_rng(7)
    top = np.uint64(n) << np.uint64(48)
    fix = np.full((h, w, 3), top, dtype=np.uint64) - rng.integers(0, 1 << 20, size=(h, w, 3)).astype(np.uint64)
    half = (fix >> np.uint64(1)) + rng.integers(-(1 << 40), 1 << 40, size=(h, w, 3)).astype(np.int64).astype(np.uint64)
    half[0, 0] = 0
    half[4, 6] = fix[4, 6]
    count = np.full((h, w), n, dtype=np.uint32)
    for thr in (1e-7, 1e-3, 10.0, 200.0):
        want = select_model(fix, half, count, n, thr, 0.01)
        assert np.array_equal(rt.select_pixels_host(fix, half, count, n, rt.make_adaptive(1, thr, 0.01)), want)
    assert 0 < len(select_model(fix, half, count, n, 10.0, 0.01)) < w * h


# ---- argument validation ------------------------------------------------------------------------------------------------

def _select_rc(a, n=16, w=4, h=4, null=None):
    lib = _ffi.load()
    fix = np.zeros((max(h, 1), max(w, 1), 3), dtype=np.uint64)
    count = np.zeros((max(h, 1), max(w, 1)), dtype=np.uint32)
    out = np.zeros(max(h, 1) * max(w, 1), dtype=np.uint32)
    m = C.c_int64(-7)
    args = [fix.ctypes.data_as(C.c_void_p), fix.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p), w, h, n,
            C.byref(a) if a is not None else None, out.ctypes.data_as(C.c_void_p), C.byref(m)]
    if null is not None:
        args[null] = None
    rc = lib.rt_select_pixels_host(*args)
    return rc, lib.rt_last_error().decode(), m.value


@pytest.mark.parametrize("kw,msg", [(dict(step=0), "step"), (dict(step=-3), "step"), (dict(threshold=-1e-9), "threshold"),
                                    (dict(threshold=float("nan")), "threshold"), (dict(dark_floor=0.0), "dark_floor"),
                                    (dict(dark_floor=-1.0), "dark_floor"), (dict(dark_floor=float("nan")), "dark_floor")])
def test_select_rejects_bad_adaptive_settings(kw, msg):
    base = dict(step=8, threshold=0.05, dark_floor=0.01)
    base.update(kw)
    rc, err, m = _select_rc(rt.make_adaptive(**base))
    assert rc == -1 and msg in err and m == -7


def test_select_rejects_null_buffers_and_bad_sizes():
    a = rt.make_adaptive(8, 0.05)
    assert _select_rc(a)[0] == 0
    for k in (0, 1, 2, 6, 7, 8):
        rc, err, _ = _select_rc(a, null=k)
        assert rc == -1 and err
    assert _select_rc(a, n=0)[0] == -1 and _select_rc(a, n=15)[0] == -1 and _select_rc(a, n=32768)[0] == -1
    assert _select_rc(a, w=0)[0] == -1 and _select_rc(a, h=-1)[0] == -1
    lib = _ffi.load()
    assert lib.rt_select_pixels_device(None, None, None, None, 4, 4, 16, C.byref(a), None, None, None) == -1


def _cam():
    return rt.book1_camera(16, 9).to_rt_camera()


@pytest.mark.parametrize("kw,a_kw,msg", [
    (dict(spp=24), {}, "multiple of 2 * step"), (dict(spp=8), {}, "multiple of 2 * step"), (dict(spp=0), {}, "multiple of 2 * step"),
    (dict(spp=32768), {}, "<= 32766"), (dict(spp=32, sample_begin=16), {}, "sample_begin"),
    (dict(spp=32), dict(step=0), "step"), (dict(spp=32), dict(threshold=-1.0), "threshold"), (dict(spp=32), dict(threshold=float("nan")), "threshold"),
    (dict(spp=32), dict(dark_floor=0.0), "dark_floor"),
    (dict(spp=32, flags=rt.RT_FLAG_UNIFORM53), {}, "RT_FLAG_UNIFORM53"), (dict(spp=32, flags=rt.RT_FLAG_DIAG_STATS), {}, "RT_FLAG_DIAG_STATS"),
    (dict(spp=32, flags=rt.RT_FLAG_NO_FILTER), {}, "RT_FLAG_NO_FILTER"), (dict(spp=32, shard_count=2), {}, "shard_count"),
    (dict(spp=32, flags=0x40), {}, "unknown flags"), (dict(spp=32, width=1), {}, "width and height"),
])
def test_render_adaptive_validates_before_it_needs_a_device(kw, a_kw, msg):
    """The checks that need no context come first: a NULL context is only reported once the arguments are sound."""
    lib = _ffi.load()
    base = dict(width=16, height=9, spp=32)
    base.update(kw)
    p = rt.make_params(base.pop("width"), base.pop("height"), base.pop("spp"), **base)
    ad = dict(step=8, threshold=0.05, dark_floor=0.01)
    ad.update(a_kw)
    a = rt.make_adaptive(**ad)
    cam = _cam()
    rc = lib.rt_render_adaptive(None, C.byref(cam), C.byref(p), C.byref(a), None, None, None, None)
    assert rc == -1 and msg in lib.rt_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(flags=rt.RT_FLAG_UNIFORM53), "RT_FLAG_UNIFORM53"), (dict(flags=rt.RT_FLAG_DIAG_STATS), "RT_FLAG_DIAG_STATS"),
    (dict(flags=rt.RT_FLAG_NO_FILTER), "RT_FLAG_NO_FILTER"), (dict(shard_count=3), "shard_count"), (dict(flags=0x20), "unknown flags"),
    (dict(t_min=0.0), "t_min"),
])
def test_render_pixels_validates_before_it_needs_a_device(kw, msg):
    lib = _ffi.load()
    p = rt.make_params(16, 9, 4, **kw)
    cam = _cam()
    px = np.arange(4, dtype=np.uint32)
    out = np.full((4, 3), 77, dtype=np.uint64)
    for fn, extra in ((lib.rt_render_pixels_device, (None,)), (lib.rt_render_pixels, (None,))):
        rc = fn(None, C.byref(cam), C.byref(p), px.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p), *extra)
        assert rc == -1 and msg in lib.rt_last_error().decode()
    assert (out == 77).all()


def test_null_arguments_of_the_new_entries_are_errors_not_crashes():
    lib = _ffi.load()
    p = rt.make_params(16, 9, 32)
    a = rt.make_adaptive(8, 0.05)
    cam = _cam()
    assert lib.rt_render_pixels_device(None, None, None, None, 0, None, None) == -1
    assert lib.rt_render_pixels(None, None, None, None, 0, None, None) == -1
    assert lib.rt_render_pixels(None, C.byref(cam), C.byref(p), None, -1, None, None) == -1 and "n_pixels" in lib.rt_last_error().decode()
    assert lib.rt_render_pixels(None, C.byref(cam), C.byref(p), None, 4, None, None) == -1 and "NULL" in lib.rt_last_error().decode()
    assert lib.rt_render_adaptive(None, None, None, None, None, None, None, None) == -1
    assert lib.rt_render_adaptive(None, C.byref(cam), C.byref(p), None, None, None, None, None) == -1
    assert lib.rt_render_adaptive(None, C.byref(cam), C.byref(p), C.byref(a), None, None, None, None) == -1 and "NULL" in lib.rt_last_error().decode()
    assert lib.rt_resolve_rgba8_counts(None, None, None, 4, 4, 1, None) == -1
    assert lib.rt_resolve_rgba8_counts_device(None, None, None, 4, 4, 1, None, None) == -1
    assert C.sizeof(_ffi.rt_adaptive) == 24 and _ffi.rt_adaptive.threshold.offset == 8
    assert lib.rt_abi_version() == 5 and _ffi.RT_FLAG_KNOWN == 0x1f


# ---- the existing kernels' machine code --------------------------------------------------------------------------------

def test_existing_kernels_keep_their_machine_code():
    """Every kernel that exists on the parent commit has the instruction counts and the opcode-sequence hash the PARENT's
    tools/isa_fingerprint.py printed (the committed file was produced from a checkout of the parent): no instantiation is
    allowed to differ.  The pixel-list variant adds instantiations (ITEMS = -256) and the per-pixel-count resolve; it changes none."""
    before = _fingerprint_lines(open(os.path.join(ROOT, "profiles", "isa_fingerprint_before_pixel_lists.txt")).read())
    assert len(before) == 15 and before["void rt::render_kernel<5, false, true, false, 256>"].endswith("ops-sha=b7a4e26be357")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    now = _fingerprint_lines(run.stdout)
    for name, want in before.items():
        assert now.get(name) == want, f"{name}: {now.get(name)} != {want}"
    added = sorted(set(now) - set(before))
    assert added == ["rt::resolve_rgba8_counts_kernel", "void rt::render_kernel<5, false, false, false, -256>",
                     "void rt::render_kernel<5, false, true, false, -256>"], added
