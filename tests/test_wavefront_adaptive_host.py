"""Wavefront frames over pixel lists and the adaptive loop over them without a GPU (include/rtiow_hip.h "wavefront frames over pixel
lists"): every new rejection from the loaded library without a context, outputs untouched, in the documented order
behind the existing ones; the header, ctypes and Rust function lists; the CLI's exit codes; that the adaptive cases the GPU tests use are
hard, by the statement and the model alone; and what the compiler says of the two new kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nee_ref as nr
import rtiow_amd as rt
import wavefront_adaptive_ref as ar
from rtiow_amd import _ffi
from test_gpu_adaptive import adaptive_model
from test_lights_host import FIX, RAYS, TABLE, Queue, lighting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_paths_begin_pixels_device", "rt_render_wavefront_pixels_device", "rt_render_wavefront_pixels", "rt_render_wavefront_adaptive")
SHADOW = np.full(8, 0x5A, dtype=np.uint8)
HALF = np.full(6 * 3 * 8, 0x5A, dtype=np.uint8)
COUNT = np.full(64 * 4, 0x5A, dtype=np.uint8)
PIXELS = np.array([0, 5, 63, 5], dtype=np.uint32)
LIGHTS = np.array([0, 2], dtype=np.int32)
INF = float("inf")
# the unlit adaptive case of the GPU tests: the book scene; chosen with the model on Oracle-B passes (test_the_unlit_case_is_hard)
BOOK = dict(width=48, height=27, step=4, cap=32, threshold=0.05, dark_floor=0.01, seed=1)


def _err(lib):
    return lib.rt_last_error().decode()


def _snapshot():
    return tuple(a.copy() for a in (FIX, RAYS, SHADOW, HALF, COUNT, PIXELS, TABLE, LIGHTS))


def _untouched(before):
    return all(np.array_equal(a, b) for a, b in zip((FIX, RAYS, SHADOW, HALF, COUNT, PIXELS, TABLE, LIGHTS), before))


def _params(**kw):
    p = rt.make_params(8, 8, kw.pop("spp", 2))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _begin(q, *, pixels=PIXELS, n_pixels=4, n=3, first_item=5, spp=2, width=8, height=8, flags=0, cam=True):
    camera = rt.book1_camera(8, 8).to_rt_camera()
    return _ffi.load().rt_paths_begin_pixels_device(None, C.byref(camera) if cam else None, width, height, 1, flags, spp, 0, first_item, n,
                                                    pixels.ctypes.data if pixels is not None else None, n_pixels, C.byref(q.q) if q else None, None)


def _direct(flags=0, n_lights=2, lights=LIGHTS):
    return _ffi.rt_direct(lights.ctypes.data if lights is not None else None, n_lights, flags)


def _frame(form, light=None, direct=None, *, pixels=PIXELS, n_pixels=4, direct_flags=0, fix=True, params=True, **kw):
    """direct: for the device form an rt_direct or None, for the host form a bool."""
    lib = _ffi.load()
    camera, p = rt.book1_camera(8, 8).to_rt_camera(), _params(**kw)
    pp, f = C.byref(p) if params else None, FIX.ctypes.data if fix else None
    ll = C.byref(light) if light is not None else None
    px = pixels.ctypes.data if pixels is not None else None
    if form == "device":
        return lib.rt_render_wavefront_pixels_device(None, C.byref(camera), pp, ll, C.byref(direct) if direct is not None else None, px, n_pixels, f,
                                                     RAYS.ctypes.data, SHADOW.ctypes.data, None)
    return lib.rt_render_wavefront_pixels(None, C.byref(camera), pp, ll, int(bool(direct)), direct_flags, px, n_pixels, f,
                                          RAYS.ctypes.data_as(C.POINTER(C.c_uint64)), SHADOW.ctypes.data_as(C.POINTER(C.c_uint64)), None)


def _adaptive(light=None, direct=False, *, direct_flags=0, a=None, fix=True, count=True, **kw):
    lib = _ffi.load()
    camera = rt.book1_camera(8, 8).to_rt_camera()
    kw.setdefault("spp", 32)
    p = _params(**kw)
    a = rt.make_adaptive(4, 0.05) if a is None else a
    return lib.rt_render_wavefront_adaptive(None, C.byref(camera), C.byref(p), C.byref(a), C.byref(light) if light is not None else None, int(direct),
                                            direct_flags, FIX.ctypes.data if fix else None, HALF.ctypes.data, COUNT.ctypes.data if count else None,
                                            RAYS.ctypes.data_as(C.POINTER(C.c_uint64)), SHADOW.ctypes.data_as(C.POINTER(C.c_uint64)), None)


# ---- the lists ---------------------------------------------------------------------------------------------------------------------------

def test_the_symbols_resolve_and_the_three_lists_agree():
    lib = _ffi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ENTRY_POINTS:
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
        assert re.search(rf"\bint {name}\(", src) and f"pub fn {name}(" in rs
    assert lib.rt_abi_version() == 5 and "#define RTIOW_HIP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", src)      # the change only adds
    header = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"#ifdef RTIOW_CROSSCHECK_MODES.*?#endif", "", src, flags=re.S))))
    assert sorted(re.findall(r"pub fn (rt_\w+)\(", rs)) == header
    assert set(header) <= {n for n, _, _ in _ffi.SYMBOLS}
    # the argument counts of the header and of ctypes
    for name in ENTRY_POINTS:
        args = re.search(rf"\bint {name}\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(dict((n, a) for n, _, a in _ffi.SYMBOLS)[name]), name
    for f in (rt.paths_begin_pixels_torch, rt.Renderer.paths_begin_pixels_device, rt.Renderer.render_wavefront_pixels,
              rt.Renderer.render_wavefront_pixels_device, rt.Renderer.render_wavefront_adaptive):
        assert callable(f)


# ---- rt_paths_begin_pixels_device ----------------------------------------------------------------------------------------------------------

BEGIN_CASES = [
    (dict(cam=False), "cam is NULL"),
    (dict(n=5), "n must be in [0, capacity"),
    (dict(width=1), "width and height must be >= 2"),
    (dict(spp=0), "spp must be >= 1"),
    (dict(first_item=-1), "must lie in [0, n_pixels * spp)"),
    (dict(first_item=6), "must lie in [0, n_pixels * spp)"),                      # 6 + 3 > 4 * 2
    (dict(n_pixels=1, first_item=0), "must lie in [0, n_pixels * spp)"),
    (dict(flags=8), "RT_FLAG_UNIFORM53"),
    (dict(flags=1), "unknown flags 0x1"),
    (dict(pixels=None, n=0, first_item=0), "n_pixels must be 0 when the list is NULL"),
    (dict(n_pixels=-1, n=0, first_item=0), "n_pixels must be in [0, 2^31 - 1]"),
    (dict(n_pixels=1 << 31, n=0, first_item=0), "n_pixels must be in [0, 2^31 - 1]"),
    (dict(), "ctx is NULL"),
    (dict(n=0, first_item=8), "ctx is NULL"),                                       # first_item + n == n_pixels * spp
    (dict(pixels=None, n_pixels=0, n=0, first_item=0), "ctx is NULL"),
]


@pytest.mark.parametrize("kw,msg", BEGIN_CASES, ids=[f"{m}-{i}" for i, (_, m) in enumerate(BEGIN_CASES)])
def test_begin_rejections_need_no_context(kw, msg):
    lib = _ffi.load()
    q, before = Queue(), _snapshot()
    assert _begin(q, **kw) == -1
    assert msg in _err(lib) and ("rt_paths_begin_pixels" in _err(lib) or msg == "ctx is NULL"), _err(lib)
    assert q.untouched() and _untouched(before)


def test_begin_order_of_the_checks():
    """rt_paths_begin_device's checks in their order, the items against n_pixels * spp; then the list; then the context."""
    lib = _ffi.load()
    assert _begin(None, cam=False, width=1, spp=0, first_item=-1, flags=8, pixels=None) == -1 and "cam is NULL" in _err(lib)
    assert _begin(None, width=1, spp=0, first_item=-1, flags=8, pixels=None) == -1 and "queue is NULL" in _err(lib)
    assert _begin(Queue(), n=9, width=1, spp=0, first_item=-1, flags=8, pixels=None) == -1 and "n must be in" in _err(lib)
    assert _begin(Queue(), width=1, spp=0, first_item=-1, flags=8, pixels=None) == -1 and "width and height" in _err(lib)
    assert _begin(Queue(), spp=0, first_item=-1, flags=8, pixels=None) == -1 and "spp must be" in _err(lib)
    assert _begin(Queue(), first_item=-1, flags=8, pixels=None) == -1 and "n_pixels * spp" in _err(lib)
    assert _begin(Queue(), flags=8, pixels=None) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
    assert _begin(Queue(), pixels=None, n_pixels=-4, n=0, first_item=0) == -1 and "when the list is NULL" in _err(lib)
    assert _begin(Queue(), n_pixels=-4, n=0, first_item=0) == -1 and "[0, 2^31 - 1]" in _err(lib)
    assert _begin(Queue()) == -1 and _err(lib) == "ctx is NULL"


# ---- the frame forms -----------------------------------------------------------------------------------------------------------------------

def test_frame_rejections_need_no_context_and_come_in_order():
    lib = _ffi.load()
    before = _snapshot()
    lit, table = lighting(), lighting(emission=TABLE, n_emission=4)
    bad_table = np.full((4, 3), -1.0)
    for form in ("device", "host"):
        d_bad, d_ok = (_direct(flags=1, n_lights=-1), _direct()) if form == "device" else (True, True)
        assert _frame(form, params=False) == -1 and "params is NULL" in _err(lib)
        assert _frame(form, fix=False, flags=2) == -1 and "fix is NULL" in _err(lib)
        assert _frame(form, flags=8, shard_count=2) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
        assert _frame(form, flags=9, shard_count=2) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
        for flags in (2, 4, 3, 0x10, 0x16):
            assert _frame(form, flags=flags, shard_count=2) == -1 and f"unknown flags 0x{flags:x}" in _err(lib) and "RT_FLAG_ACCUMULATE" in _err(lib)
        assert _frame(form, flags=1, shard_count=2, t_min=INF) == -1 and "shard_count must be 1" in _err(lib)
        assert _frame(form, flags=1, t_min=INF, pixels=None) == -1 and "t_min must be" in _err(lib)
        # direct without light; the lighting checks; the direct checks; the list; the context
        assert _frame(form, None, d_bad, pixels=None, direct_flags=1) == -1 and "light is NULL" in _err(lib)
        assert _frame(form, lighting(flags=4), d_bad, pixels=None, direct_flags=1) == -1 and "light->flags" in _err(lib)
        assert _frame(form, lighting(emission=bad_table, n_emission=-1), d_bad, pixels=None, direct_flags=1) == -1 and "n_emission must be >= 0" in _err(lib)
        assert _frame(form, lit, d_bad, pixels=None, direct_flags=1) == -1 and "direct->flags 0x1" in _err(lib)
        assert _frame(form, lit, d_ok, pixels=None, direct_flags=8) == -1 and ("direct->flags 0x8" in _err(lib)) == (form == "host")
        assert _frame(form, lit, d_ok, pixels=None, n_pixels=4) == -1 and "n_pixels must be width * height = 64 when the list is NULL" in _err(lib)
        assert _frame(form, lit, d_ok, pixels=None, n_pixels=0) == -1 and "when the list is NULL" in _err(lib)
        assert _frame(form, lit, d_ok, n_pixels=-1) == -1 and "n_pixels must be in [0, 2^31 - 1]" in _err(lib)
        assert _frame(form, lit, d_ok, n_pixels=1 << 31) == -1 and "n_pixels must be in [0, 2^31 - 1]" in _err(lib)
        for flags in (0, 1):
            assert _frame(form, flags=flags) == -1 and _err(lib) == "ctx is NULL"
            assert _frame(form, lit, flags=flags, pixels=None, n_pixels=64) == -1 and _err(lib) == "ctx is NULL"
            assert _frame(form, table, d_ok, flags=flags, direct_flags=10, n_pixels=0) == -1 and _err(lib) == "ctx is NULL"
    assert _frame("device", lit, _direct(n_lights=-1)) == -1 and "n_lights must be >= 0" in _err(lib)
    assert _frame("device", lit, _direct(lights=None)) == -1 and "n_lights must be 0" in _err(lib)
    # the host form can see its table and its list
    assert _frame("host", lighting(emission=bad_table, n_emission=4), True) == -1 and "light->emission[0][0]" in _err(lib)
    assert _frame("host", None, False, direct_flags=2) == -1 and "direct_flags must be 0 without direct lighting" in _err(lib)
    outside = np.array([0, 63, 64, 1], dtype=np.uint32)
    assert _frame("host", lit, False, pixels=outside) == -1 and "pixels[2] = 64 lies outside the frame of 64 pixels" in _err(lib)
    assert _frame("host", lit, False, pixels=outside, n_pixels=2) == -1 and _err(lib) == "ctx is NULL"
    assert _frame("device", lit, None, pixels=outside) == -1 and _err(lib) == "ctx is NULL"          # a device list cannot be looked at
    assert _untouched(before)


# ---- rt_render_wavefront_adaptive ----------------------------------------------------------------------------------------------------------

def test_adaptive_rejections_need_no_context_and_come_in_order():
    lib = _ffi.load()
    before = _snapshot()
    lit, table = lighting(), lighting(emission=TABLE, n_emission=4)
    assert _adaptive(fix=False) == -1 and "out_fix is NULL" in _err(lib)
    assert _adaptive(count=False) == -1 and "out_count is NULL" in _err(lib)
    assert _adaptive(width=1, sample_begin=4) == -1 and "width" in _err(lib)
    assert _adaptive(a=rt.make_adaptive(0, 0.05), sample_begin=4) == -1 and "step" in _err(lib)
    assert _adaptive(a=rt.make_adaptive(4, -1.0), sample_begin=4) == -1 and "threshold" in _err(lib)
    assert _adaptive(a=rt.make_adaptive(4, 0.05, 0.0), sample_begin=4) == -1 and "dark_floor" in _err(lib)
    # rt_render_adaptive's three, in its order, before the frame's
    assert _adaptive(sample_begin=4, spp=12, flags=1) == -1 and "sample_begin must be 0" in _err(lib) and "rt_render_wavefront_adaptive" in _err(lib)
    for spp in (4, 12, 36):
        assert _adaptive(spp=spp, flags=1) == -1 and "multiple of 2 * step = 8" in _err(lib)
    assert _adaptive(spp=32768, flags=1) == -1 and "<= 32766" in _err(lib)
    assert _adaptive(None, False, direct_flags=2, flags=1) == -1 and "direct_flags must be 0 without direct lighting" in _err(lib)
    # the frame's: no flag at all here, ACCUMULATE included -- the loop numbers and zeroes its own passes
    for flags, word in ((1, "unknown flags 0x1"), (8, "RT_FLAG_UNIFORM53"), (0x10, "unknown flags 0x10")):
        assert _adaptive(flags=flags, shard_count=2) == -1 and word in _err(lib)
    assert _adaptive(shard_count=2, t_min=INF) == -1 and "shard_count must be 1" in _err(lib)
    assert _adaptive(t_min=INF) == -1 and "t_min must be" in _err(lib)
    # the lighting and the direct checks in their established order; then the one of its own; then the context
    assert _adaptive(None, True, direct_flags=1, max_depth=5000) == -1 and "light is NULL" in _err(lib)
    assert _adaptive(lighting(sky_top=(0, -1, 0)), True, direct_flags=1, max_depth=5000) == -1 and "sky_top[1]" in _err(lib)
    assert _adaptive(lighting(emission=np.full((4, 3), -1.0), n_emission=4), True, direct_flags=1, max_depth=5000) == -1 and "light->emission[0][0]" in _err(lib)
    assert _adaptive(table, True, direct_flags=1, max_depth=5000) == -1 and "direct->flags 0x1" in _err(lib)
    assert _adaptive(table, True, direct_flags=8, max_depth=5000) == -1 and "direct->flags 0x8" in _err(lib)
    for direct_flags in (0, 2, 10):
        assert _adaptive(table, True, direct_flags=direct_flags, spp=32, max_depth=1024) == -1
        assert "spp * max_depth must be <= 32767 (is 32768)" in _err(lib) and "2^63" in _err(lib)
        assert _adaptive(table, True, direct_flags=direct_flags, spp=16, max_depth=2047) == -1 and _err(lib) == "ctx is NULL"      # 32752
    assert _adaptive(table, True, spp=32, max_depth=1023) == -1 and _err(lib) == "ctx is NULL"                                 # 32736
    assert _adaptive(table, True, spp=8, max_depth=4096) == -1 and "(is 32768)" in _err(lib)
    # without direct lighting a sample adds one term: the bound is rt_render_adaptive's spp <= 32766 alone
    assert _adaptive(table, False, spp=32, max_depth=5000) == -1 and _err(lib) == "ctx is NULL"
    assert _adaptive(None, False, spp=32760, max_depth=5000) == -1 and _err(lib) == "ctx is NULL"
    assert _untouched(before)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------

def test_the_cli_takes_adaptive_with_wavefront_and_keeps_its_other_exclusions(tmp_path, book1_flat):
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert "rt_render_wavefront_adaptive(" in src and "rt_resolve_rgba8_counts(" in src
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    base = [exe, "--scene", scene_file, "--width", "8", "--height", "8", "--spp", "16", "--out", str(tmp_path / "o.ppm")]
    adaptive = ["--wavefront", "--adaptive", "0.05", "--step", "4"]
    # (every one is refused while the arguments are read: no device is asked for)
    for args, word in ((adaptive + ["--denoise"], "--denoise"), (adaptive + ["--passes", "2"], "--passes"), (adaptive + ["--two-calls"], "--two-calls"),
                       (adaptive + ["--uniform53"], "--uniform53"), (adaptive + ["--devices", "0"], "--devices"), (adaptive + ["--direct"], "--emit"),
                       (adaptive + ["--features", str(tmp_path / "f.npy")], "--features"), (adaptive + ["--orbit", "2"], "--wavefront"),
                       (["--adaptive", "0.05", "--emit", "0:1,1,1"], "--wavefront"), (["--adaptive", "0.05", "--direct", "--emit", "0:1,1,1"], "--wavefront")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.returncode, bad.stderr)
    # accepted by the argument checks: what fails now is the device (here there is none) or nothing at all; never the exit code of a refusal
    ok = subprocess.run(base + adaptive + ["--sky", "0,0,0:0,0,0", "--emit", "0:4,3.2,2.4", "--direct-weighted"], capture_output=True, text=True, timeout=120)
    assert ok.returncode in (0, 1) and "goes with none of" not in ok.stderr, (ok.returncode, ok.stderr)


# ---- the cases of the GPU tests are hard -----------------------------------------------------------------------------------------------------

def test_the_nee_case_is_hard(oracle_mod):
    """The stat scene of nee_ref (16 x 12, depth 8, seed 101, area sampling, step 4, cap 32, threshold 0.2, floor 0.01, batches of 257), by the
    statement alone: the final counts are 8 / 16 / 24 / 32 samples on 78 / 32 / 41 / 41 pixels -- every value a pixel can stop at occurs."""
    S = ar.STAT
    assert (S["width"], S["height"], S["max_depth"], S["seed"], S["step"], S["cap"], S["threshold"], S["dark_floor"], S["batch"]) == \
        (16, 12, 8, 101, 4, 32, 0.2, 0.01, 257)
    fix, half, count, rays, shadow = ar.stat_adaptive()
    values, pixels = np.unique(count, return_counts=True)
    print("counts", values.tolist(), "on", pixels.tolist(), "pixels; rays", rays, "shadow rays", shadow)
    assert values.tolist() == [8, 16, 24, 32] and pixels.tolist() == [78, 32, 41, 41]
    assert shadow > 0 and rays > int(count.sum()) and fix.any() and half.any()
    assert S["cap"] * S["max_depth"] <= 32767
    # `half` holds the even passes: at a pixel that stopped after round 1 it is pass 0 alone, a dense pass of the same statement
    flat, light = nr.stat_scene()
    import oracle
    first = nr.render_nee(flat, oracle.camera_from_host(nr.stat_camera()), 16, 12, 4, light, max_depth=8, seed=101, batch=257)[0]
    assert np.array_equal(half[count == 8], first[count == 8]) and not np.array_equal(half[count == 32], first[count == 32])
    # a list pass is the dense pass masked to the list
    listed = np.flatnonzero((count > 8).reshape(-1)).astype(np.uint32)
    dense = nr.render_nee(flat, oracle.camera_from_host(nr.stat_camera()), 16, 12, 4, light, max_depth=8, seed=101, sample_begin=8, batch=257)[0]
    sparse = ar.render_pixels(flat, oracle.camera_from_host(nr.stat_camera()), 16, 12, 4, listed, light, True, max_depth=8, seed=101, sample_begin=8, batch=257)[0]
    mask = (count > 8)
    assert np.array_equal(sparse[mask], dense[mask]) and not sparse[~mask].any() and dense[~mask].any()


def test_the_unlit_case_is_hard(oracle_mod, book1_flat):
    """The book scene at 48 x 27, step 4, cap 32, threshold 0.05, floor 0.01, seed 1: on Oracle-B passes the model's counts take at least
    three distinct values (the parameters the issue names give that; none had to be changed)."""
    B = BOOK
    cam = oracle_mod.camera_from_host(rt.book1_camera(B["width"], B["height"]))
    passes = [oracle_mod.render_b(cam, book1_flat, oracle_mod.make_params(B["width"], B["height"], B["step"], sample_begin=k * B["step"], seed=B["seed"]))[0]
              for k in range(B["cap"] // B["step"])]
    _, _, count, rounds = adaptive_model(passes, B["step"], B["cap"], B["threshold"], B["dark_floor"])
    values, pixels = np.unique(count, return_counts=True)
    print("counts", values.tolist(), "on", pixels.tolist(), "pixels; active per round", rounds)
    assert len(values) >= 3 and values.min() == 2 * B["step"] and values.max() == B["cap"]


# ---- the kernels, without a GPU ------------------------------------------------------------------------------------------------------------

def test_the_path_kernels_keep_their_machine_code_and_the_two_new_ones_are_pinned():
    """tools/isa_fingerprint.py --paths --weighted --pixels: the pinned lines of the lights, NEE, cone and weighted files exactly, and the two
    new lines of profiles/isa_fingerprint_wavefront_pixels.txt behind path_begin_kernel's."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--paths", "--weighted", "--pixels"], capture_output=True,
                         text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [ln for ln in run.stdout.splitlines() if re.match(r"rt::(path_|pass_|bounce|queue_)", ln)]
    pinned = lambda name: [ln for ln in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if ln.startswith("rt::")]
    new = pinned("isa_fingerprint_wavefront_pixels.txt")
    assert len(new) == 2 and "path_begin_pixels_kernel" in new[0] and "pass_add_listed_kernel" in new[1]
    before = pinned("isa_fingerprint_lights.txt") + pinned("isa_fingerprint_nee.txt") + pinned("isa_fingerprint_cone.txt") + pinned("isa_fingerprint_weighted.txt")
    assert len(before) == 8
    assert sorted(ln for ln in got if ln not in new) == sorted(before)
    assert got[1:3] == new and "rt::path_begin_kernel " in got[0]
    plain = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--paths"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert plain.returncode == 0 and "path_begin_pixels_kernel" not in plain.stdout and "pass_add_listed_kernel" not in plain.stdout


def test_the_new_kernels_use_no_scratch_memory_and_spill_no_vector_register():
    """The compiler's own resource remarks for wavefront/rt_paths.hip, read the way the lights tests read them."""
    import tempfile
    csrc = os.path.join(ROOT, "rtiow_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                              "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-c", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "paths.o"), os.path.join(csrc, "wavefront", "rt_paths.hip")],
                             capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    cur, rows = None, {}
    for line in (run.stderr + run.stdout).splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = m.group(2)
    for kind in ("path_begin_pixels_kernel", "pass_add_listed_kernel"):
        found = [r for name, r in rows.items() if f"{kind}E" in name]
        assert len(found) == 1, kind
        r = found[0]
        print(kind, "VGPRs", r["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "SGPR spills", r["SGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, (kind, r)
