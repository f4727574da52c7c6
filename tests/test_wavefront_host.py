"""Wavefront path steps without a GPU (include/rtiow_hip.h "wavefront path steps"): the reference loop of
tests/wavefront_ref.py against Oracle B over a whole frame (which pins the restatement and the event arithmetic), the context-free
validation of the six entry points, the struct layouts against the header, and that the step inputs the GPU tests use are hard."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtiow_amd as rt
import wavefront_ref as wr
from rtiow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_camera_rays_device", "rt_camera_rays", "rt_scatter_device", "rt_scatter", "rt_accumulate_device", "rt_accumulate")


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_reference_loop_equals_oracle_b(oracle_mod, book1_flat):
    """Book scene, 32 x 18, 4 spp, depth 50, seed 1: camera step -> { closest hit; sky of the misses; scatter; throughput } path by path
    gives Oracle B's u64 sums and its ray count."""
    w, h, spp = 32, 18, 4
    ocam = oracle_mod.book1_camera(w, h)
    want, _, st = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, max_depth=50, seed=1))
    got, rays = wr.render(book1_flat, ocam, w, h, spp, max_depth=50, seed=1)
    assert np.array_equal(got, want)
    assert rays == st["rays_traced"]


@pytest.mark.parametrize("max_depth", [0, 1, 3])
def test_reference_loop_at_small_depths(oracle_mod, book1_flat, max_depth):
    w, h, spp = 16, 9, 2
    ocam = oracle_mod.book1_camera(w, h)
    want, _, st = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, max_depth=max_depth, seed=3, sample_begin=5))
    got, rays = wr.render(book1_flat, ocam, w, h, spp, max_depth=max_depth, seed=3, sample_begin=5)
    assert np.array_equal(got, want) and rays == st["rays_traced"]


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------

def _err(lib):
    return lib.rt_last_error().decode()


def test_the_symbols_resolve():
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert lib.rt_abi_version() == 5
    for f in (rt.camera_rays_torch, rt.scatter_torch, rt.accumulate_torch, rt.render_wavefront_torch):
        assert callable(f)
    for m in ("camera_rays", "scatter", "accumulate", "camera_rays_device", "scatter_device", "accumulate_device"):
        assert callable(getattr(rt.Renderer, m))
    assert (_ffi.RT_SCATTER_ABSORBED, _ffi.RT_SCATTER_SCATTERED, _ffi.RT_SCATTER_MISS, _ffi.RT_SCATTER_BAD_INDEX) == (0, 1, 2, 3)


SENTINEL = 0x5A


class Arrays:
    """Four paths' worth of arrays for every field of the three batch structs, filled with a sentinel byte (no call here reads or
    writes them: every call ends in validation)."""
    FIELDS = {"camera": ("pixel", "sample", "origin", "dir", "event"),
              "scatter": ("dir", "index", "point", "normal", "front_face", "pixel", "sample", "event", "out_origin", "out_dir", "attenuation", "status"),
              "accumulate": ("pixel", "weight", "sky_dir", "select")}

    def __init__(self, step, n=4, null=()):
        self.keep = {f: np.full(4 * 3 * 8, SENTINEL, dtype=np.uint8) for f in self.FIELDS[step]}
        self.fix = np.full(6 * 3 * 8, SENTINEL, dtype=np.uint8)
        cls = {"camera": _ffi.rt_camera_batch, "scatter": _ffi.rt_scatter_batch, "accumulate": _ffi.rt_accumulate_batch}[step]
        self.batch = cls(*[None if f in null else self.keep[f].ctypes.data for f in self.FIELDS[step]], n)

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.keep.values()) and (self.fix == SENTINEL).all()


def _call(form, a, *, cam=True, width=8, height=8, flags=0, batch=True, fix=True, npix=6, ctx=None):
    lib = _ffi.load()
    step, host = form.rsplit("_", 1)
    camera = rt.book1_camera(8, 8).to_rt_camera()
    b = C.byref(a.batch) if batch else None
    last = C.byref(C.c_float(-1.0)) if host == "host" else None                 # kernel_ms, or the NULL stream
    if step == "camera":
        fn = lib.rt_camera_rays if host == "host" else lib.rt_camera_rays_device
        return fn(ctx, C.byref(camera) if cam else None, width, height, 1, flags, b, last)
    if step == "scatter":
        fn = lib.rt_scatter if host == "host" else lib.rt_scatter_device
        return fn(ctx, 1, flags, b, last)
    fn = lib.rt_accumulate if host == "host" else lib.rt_accumulate_device
    return fn(ctx, b, a.fix.ctypes.data if fix else None, npix, last)


REQUIRED = {"camera": Arrays.FIELDS["camera"], "scatter": Arrays.FIELDS["scatter"], "accumulate": ("pixel", "weight")}
COMMON = [(dict(batch=False), {}, "batch is NULL"),
          ({}, dict(n=-1), "n must be in [0, 2^31]"),
          ({}, dict(n=2 ** 31 + 1), "n must be in [0, 2^31]"),
          ({}, {}, "ctx is NULL"),
          ({}, dict(n=2 ** 31), "ctx is NULL")]                                 # the largest batch is legal
FLAGS = [(dict(flags=rt.RT_FLAG_UNIFORM53), {}, "RT_FLAG_UNIFORM53 is not built"), (dict(flags=0x1), {}, "unknown flags 0x1"),
         (dict(flags=0x80000000), {}, "unknown flags 0x80000000")]
CASES = ([("camera", *c) for c in COMMON + FLAGS] + [("scatter", *c) for c in COMMON + FLAGS] + [("accumulate", *c) for c in COMMON]
         + [("camera", dict(cam=False), {}, "cam is NULL"), ("camera", dict(width=1), {}, "width and height must be >= 2"),
            ("camera", dict(height=1), {}, "width and height must be >= 2"), ("accumulate", dict(fix=False), {}, "fix is NULL"),
            ("accumulate", dict(npix=0), {}, "npix must be in [1, 2^32]"), ("accumulate", dict(npix=-5), {}, "npix must be in [1, 2^32]"),
            ("accumulate", dict(npix=2 ** 32 + 1), {}, "npix must be in [1, 2^32]"),
            ("accumulate", {}, dict(null=("sky_dir", "select")), "ctx is NULL")]                # the optional arrays may be NULL
         + [(step, {}, dict(null=(f,)), f"batch->{f} is NULL") for step in REQUIRED for f in REQUIRED[step]]
         + [(step, {}, dict(n=0, null=REQUIRED[step]), "ctx is NULL") for step in REQUIRED])    # n == 0 needs no array


@pytest.mark.parametrize("host", ["device", "host"])
@pytest.mark.parametrize("step,call_kw,array_kw,msg", CASES, ids=[f"{c[0]}-{c[3]}-{i}" for i, c in enumerate(CASES)])
def test_context_free_validation(host, step, call_kw, array_kw, msg):
    """Every reason comes before the context is looked at (the call passes a NULL one), and nothing is touched."""
    lib = _ffi.load()
    a = Arrays(step, **array_kw)
    assert _call(f"{step}_{host}", a, **call_kw) == -1
    assert msg in _err(lib), _err(lib)
    assert a.untouched()


def test_the_order_of_the_checks():
    """NULL structs, then n, then the arrays, then width / height or npix, then the flags, then the context."""
    lib = _ffi.load()
    a = Arrays("camera", n=-1, null=("pixel",))
    assert _call("camera_device", a, cam=False, width=1, flags=8) == -1 and "cam is NULL" in _err(lib)
    assert _call("camera_device", a, width=1, flags=8) == -1 and "n must be" in _err(lib)
    a = Arrays("camera", null=("pixel",))
    assert _call("camera_device", a, width=1, flags=8) == -1 and "batch->pixel is NULL" in _err(lib)
    a = Arrays("camera")
    assert _call("camera_device", a, width=1, flags=8) == -1 and "width and height" in _err(lib)
    assert _call("camera_device", a, flags=8) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
    a = Arrays("accumulate", null=("weight",))
    assert _call("accumulate_host", a, npix=0) == -1 and "batch->weight is NULL" in _err(lib)


def _header_struct(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, src).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            for item in decl.strip().split(","):
                out.append((re.search(r"(\w+)\s*$", item).group(1), "*" in decl))
    return out


@pytest.mark.parametrize("name,size", [("rt_camera_batch", 48), ("rt_scatter_batch", 104), ("rt_accumulate_batch", 40)])
def test_struct_layouts_match_the_header(name, size):
    """Every field of the header's struct, in order: pointers, then n as an int64."""
    fields = _header_struct(name)
    cls = getattr(_ffi, name)
    assert [f for f, _ in cls._fields_] == [f for f, _ in fields]
    assert all(is_ptr for _, is_ptr in fields[:-1]) and fields[-1] == ("n", False)
    assert all(t is C.c_void_p for _, t in cls._fields_[:-1]) and cls._fields_[-1][1] is C.c_int64
    assert C.sizeof(cls) == size and cls.n.offset == size - 8
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    body = re.search(r"pub struct %s \{(.*?)\n\}" % name, rs, flags=re.S).group(1)
    assert [m.group(1) for m in re.finditer(r"pub (\w+):", body)] == [f for f, _ in fields]
    assert f"{size} == size_of::<{name}>()" in rs
    for k, v in (("ABSORBED", 0), ("SCATTERED", 1), ("MISS", 2), ("BAD_INDEX", 3)):
        assert f"pub const RT_SCATTER_{k}: u8 = {v};" in rs


# ---- the GPU tests' inputs are hard -------------------------------------------------------------------------------------------------

def test_the_scatter_cases_are_hard(oracle_mod):
    """Conditions on the inputs of tests/test_gpu_wavefront.py, checked with the reference alone."""
    flat, inp, want = wr.scatter_cases()
    n = wr.N_CASES
    kind = np.array([int(flat[i]["kind"]) if 0 <= i < len(flat) else -1 for i in inp["index"]])
    fuzz = np.array([float(flat[i]["param"]) if 0 <= i < len(flat) else -1.0 for i in inp["index"]])
    status, tries, mode = want["status"], want["tries"], np.array(want["mode"])
    advance = want["event"].astype(np.int64) - inp["event"].astype(np.int64)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    zero = lambda v: (np.abs(v) < 1e-8).all(axis=1)
    # one of each, already among the first 63 (the smallest batch that holds them all)
    for first in (63, n):
        s = slice(0, first)
        lam = (kind[s] == wr.LAMBERTIAN)
        near = lam & (bits(want["out_dir"][s]) == bits(inp["normal"][s])).all(axis=1)
        assert (lam & ~near).any() and near.any()                                       # Lambertian ordinary; the near-zero fallback
        assert ((kind[s] == wr.METAL) & (status[s] == wr.SCATTERED)).any() and ((kind[s] == wr.METAL) & (status[s] == wr.ABSORBED)).any()
        assert ((kind[s] == wr.METAL) & (fuzz[s] == 0.0)).any()
        glass = kind[s] == wr.DIALECTRIC
        assert (glass & (inp["front_face"][s] == 1) & (mode[s] == "refract")).any() and (glass & (mode[s] == "reflect")).any()
        assert (glass & (inp["front_face"][s] == 0) & (mode[s] == "tir") & (advance[s] == 0)).any()
        assert (tries[s] >= 5).any()                                                    # crosses the three-block period of the stream
        assert (status[s] == wr.MISS).any() and ((status[s] == wr.BAD_INDEX) & (inp["index"][s] < -1)).any()
        assert ((status[s] == wr.BAD_INDEX) & (inp["index"][s] >= len(flat))).any()
    # the near-zero case really is one: normal + unit vector is zero, and only there
    near_all = (kind == wr.LAMBERTIAN) & (bits(want["out_dir"]) == bits(inp["normal"])).all(axis=1)
    assert near_all.sum() == 1 and near_all[1]
    # the event arithmetic and the untouched fields, as the header states them
    solid = (kind == wr.LAMBERTIAN) | (kind == wr.METAL)
    assert np.array_equal(advance[solid], (3 * tries[solid] + 3) // 4) and set(advance[kind == wr.DIALECTRIC]) == {0, 1}
    assert (advance[(status == wr.MISS) | (status == wr.BAD_INDEX)] == 0).all()
    unwritten = (status == wr.MISS) | (status == wr.BAD_INDEX)
    for name in ("out_origin", "out_dir", "attenuation"):
        assert (want[name][unwritten] == wr.F64_SENTINEL).all()
    absorbed = status == wr.ABSORBED
    assert absorbed.sum() >= 5 and (want["attenuation"][absorbed] == 0.0).all() and (advance[absorbed] >= 1).all()
    assert (want["out_origin"][absorbed] == wr.F64_SENTINEL).all() and (want["out_dir"][absorbed] == wr.F64_SENTINEL).all()
    assert np.array_equal(want["out_origin"][status == wr.SCATTERED], inp["point"][status == wr.SCATTERED])
    assert (want["attenuation"][kind == wr.DIALECTRIC] == 1.0).all()                    # materials.rs:103, whatever the flat albedo holds
    assert not zero(want["out_dir"][status == wr.SCATTERED]).any()
    assert {wr.LAMBERTIAN, wr.METAL, wr.DIALECTRIC} <= set(kind[:63]) and (status == wr.MISS).sum() >= 10
    assert (inp["pixel"] >= 1 << 16).any() and (inp["event"] > 4).any()


def test_the_camera_cases_are_hard(oracle_mod):
    cam, pixel, sample, want = wr.camera_cases()
    tries = want["tries"]
    for first in (63, wr.N_CASES):
        assert (tries[:first] >= 2).any() and (tries[:first] == 1).any()
    assert (tries >= 4).any() and np.array_equal(want["event"], 1 + tries // 2) and want["event"].max() >= 3
    assert {0, wr.CW - 1, wr.CW * wr.CH - 1} <= set(int(p) for p in pixel) and (sample >= 1 << 30).any()
    assert float(cam.lens_radius) > 0.2                                                   # the lens draws matter
    assert np.unique(want["origin"], axis=0).shape[0] > 200
