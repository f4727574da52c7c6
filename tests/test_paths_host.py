"""The device path queue without a GPU (include/rtiow_hip.h "path queue"): the reference loop of tests/paths_ref.py
against Oracle B over a whole frame in ragged batches (which pins the restatement: item order, stable compaction, the event and
throughput a survivor carries), the context-free validation of the entry points in the stated order, rt_path_scratch_words, the struct
layouts against the header, and that the hand-built step queue the GPU tests use is hard."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import paths_ref as pr
import rtiow_amd as rt
from rtiow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_path_scratch_words", "rt_paths_begin_device", "rt_paths_step_device", "rt_render_wavefront_device", "rt_render_wavefront")


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_reference_loop_equals_oracle_b(oracle_mod, book1_flat, golden_small):
    """Book scene, 32 x 18, 4 spp, depth 50, seed 1, in batches of 257 items (nine, the last ragged): begin, then 50 steps per batch give
    Oracle B's u64 sums and its ray count."""
    w, h, spp = 32, 18, 4
    ocam = oracle_mod.book1_camera(w, h)
    want, _, st = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, max_depth=50, seed=1))
    got, rays = pr.render(book1_flat, ocam, w, h, spp, max_depth=50, seed=1, batch=257)
    assert np.array_equal(got, want)
    assert rays == st["rays_traced"]


def test_reference_begin_is_pixel_major(oracle_mod):
    ocam = oracle_mod.book1_camera(8, 8)
    q = pr.begin(ocam, 8, 8, 3, 4, 10, 5, 9)                                    # items 5 .. 13 of a 4-spp frame, samples from 10
    assert q["pixel"].tolist() == [1, 1, 1, 2, 2, 2, 2, 3, 3] and q["sample"].tolist() == [11, 12, 13, 10, 11, 12, 13, 10, 11]
    assert (q["throughput"] == 1.0).all() and (q["event"] >= 1).all()


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------

def _err(lib):
    return lib.rt_last_error().decode()


def test_the_symbols_resolve():
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert lib.rt_abi_version() == 5
    for f in (rt.PathQueue, rt.paths_begin_torch, rt.paths_step_torch):
        assert callable(f)
    for m in ("paths_begin_device", "paths_step_device", "render_wavefront", "render_wavefront_device"):
        assert callable(getattr(rt.Renderer, m))


@pytest.mark.parametrize("capacity,words", [(1, 3), (64, 3), (65, 6), (256, 12), (257, 15), (1 << 24, 3 << 18), (0, 0), (-1, 0), ((1 << 24) + 1, 0)])
def test_scratch_words(capacity, words):
    """Three words per 64 slots; 0 for a capacity no queue may have."""
    assert _ffi.load().rt_path_scratch_words(capacity) == words


SENTINEL = 0x5A
QFIELDS = ("count", "pixel", "sample", "event", "origin", "dir", "throughput", "scratch")


class Queue:
    """Host arrays behind every pointer of an rt_path_queue, sentinel-filled (no call here reads or writes them: every call ends in
    validation)."""

    def __init__(self, capacity=4, null=()):
        self.keep = {f: np.full(4 * 3 * 8, SENTINEL, dtype=np.uint8) for f in QFIELDS}
        self.q = _ffi.rt_path_queue(capacity, *[None if f in null else self.keep[f].ctypes.data for f in QFIELDS])

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.keep.values())


FIX = np.full(6 * 3 * 8, SENTINEL, dtype=np.uint8)
RAYS = np.full(8, SENTINEL, dtype=np.uint8)


def _begin(q, *, cam=True, width=8, height=8, flags=0, spp=2, sample_begin=0, first_item=0, n=4, ctx=None):
    camera = rt.book1_camera(8, 8).to_rt_camera()
    return _ffi.load().rt_paths_begin_device(ctx, C.byref(camera) if cam else None, width, height, 1, flags, spp, sample_begin, first_item, n,
                                             C.byref(q.q) if q else None, None)


def _step(qin, qout, *, flags=0, t_min=1e-4, fix=True, npix=6, ctx=None):
    return _ffi.load().rt_paths_step_device(ctx, 1, flags, t_min, C.byref(qin.q) if qin else None, C.byref(qout.q) if qout else None,
                                            FIX.ctypes.data if fix else None, npix, RAYS.ctypes.data, None)


def _render(form, *, cam=True, params=True, fix=True, ctx=None, **kw):
    lib = _ffi.load()
    camera = rt.book1_camera(8, 8).to_rt_camera()
    p = rt.make_params(8, 8, 2)
    for k, v in kw.items():
        setattr(p, k, v)
    c, pp, f = C.byref(camera) if cam else None, C.byref(p) if params else None, FIX.ctypes.data if fix else None
    if form == "device":
        return lib.rt_render_wavefront_device(ctx, c, pp, f, RAYS.ctypes.data, None)
    return lib.rt_render_wavefront(ctx, c, pp, f, RAYS.ctypes.data_as(C.POINTER(C.c_uint64)), None)


BEGIN_CASES = [(dict(cam=False), {}, "cam is NULL"), (dict(q=False), {}, "queue is NULL")] \
    + [({}, dict(null=(f,)), f"queue->{f} is NULL") for f in QFIELDS] \
    + [({}, dict(capacity=0), "capacity must be in [1, 2^24]"), ({}, dict(capacity=(1 << 24) + 1), "capacity must be in [1, 2^24]"),
       (dict(n=-1), {}, "n must be in [0, capacity"), (dict(n=5), {}, "n must be in [0, capacity"),
       (dict(width=1), {}, "width and height must be >= 2"), (dict(height=1), {}, "width and height must be >= 2"),
       (dict(spp=0), {}, "spp must be >= 1"), (dict(sample_begin=-1), {}, "spp must be >= 1"),
       (dict(first_item=-1), {}, "must lie in [0, width * height * spp)"), (dict(first_item=8 * 8 * 2 - 3), {}, "must lie in [0, width * height * spp)"),
       (dict(flags=rt.RT_FLAG_UNIFORM53), {}, "RT_FLAG_UNIFORM53 is not built"), (dict(flags=0x1), {}, "unknown flags 0x1"),
       ({}, {}, "ctx is NULL"), (dict(n=0), {}, "ctx is NULL"), (dict(first_item=8 * 8 * 2 - 4), {}, "ctx is NULL"),
       ({}, dict(capacity=1 << 24), "ctx is NULL")]


@pytest.mark.parametrize("call_kw,queue_kw,msg", BEGIN_CASES, ids=[f"{c[2]}-{i}" for i, c in enumerate(BEGIN_CASES)])
def test_begin_validation_needs_no_context(call_kw, queue_kw, msg):
    lib = _ffi.load()
    q = Queue(**queue_kw)
    call_kw = dict(call_kw)
    assert _begin(q if call_kw.pop("q", True) else None, **call_kw) == -1
    assert msg in _err(lib), _err(lib)
    assert q.untouched()


STEP_CASES = [(dict(qin=False), {}, {}, "in is NULL"), (dict(qout=False), {}, {}, "out is NULL")] \
    + [({}, dict(null=(f,)), {}, f"in->{f} is NULL") for f in QFIELDS] + [({}, {}, dict(null=(f,)), f"out->{f} is NULL") for f in QFIELDS] \
    + [({}, dict(capacity=0), {}, "in->capacity must be in [1, 2^24]"), ({}, {}, dict(capacity=(1 << 24) + 1), "out->capacity must be in [1, 2^24]"),
       (dict(fix=False), {}, {}, "d_fix is NULL"),
       (dict(same=True), {}, {}, "in and out must be distinct queues"), (dict(share="dir"), {}, {}, "in and out share an array"),
       (dict(share="count"), {}, {}, "in and out share an array"),
       ({}, dict(capacity=4), dict(capacity=3), "out->capacity (3) must be >= in->capacity (4)"),
       (dict(npix=0), {}, {}, "npix must be in [1, 2^32]"), (dict(npix=2 ** 32 + 1), {}, {}, "npix must be in [1, 2^32]"),
       (dict(flags=rt.RT_FLAG_UNIFORM53), {}, {}, "RT_FLAG_UNIFORM53 is not built"), (dict(flags=0x80000000), {}, {}, "unknown flags 0x80000000"),
       (dict(t_min=0.0), {}, {}, "t_min must be > 0 and finite"), (dict(t_min=float("inf")), {}, {}, "t_min must be > 0 and finite"),
       (dict(t_min=float("nan")), {}, {}, "t_min must be > 0 and finite"), (dict(t_min=-1.0), {}, {}, "t_min must be > 0 and finite"),
       ({}, {}, {}, "ctx is NULL"), ({}, dict(capacity=3), dict(capacity=1 << 24), "ctx is NULL"), (dict(npix=2 ** 32), {}, {}, "ctx is NULL")]


@pytest.mark.parametrize("call_kw,in_kw,out_kw,msg", STEP_CASES, ids=[f"{c[3]}-{i}" for i, c in enumerate(STEP_CASES)])
def test_step_validation_needs_no_context(call_kw, in_kw, out_kw, msg):
    lib = _ffi.load()
    qin, qout = Queue(**in_kw), Queue(**out_kw)
    call_kw = dict(call_kw)
    if call_kw.pop("same", False):
        qout = qin
    share = call_kw.pop("share", None)
    if share:
        setattr(qout.q, share, getattr(qin.q, share))
    a = qin if call_kw.pop("qin", True) else None
    b = qout if call_kw.pop("qout", True) else None
    before = (FIX.copy(), RAYS.copy())
    assert _step(a, b, **call_kw) == -1
    assert msg in _err(lib), _err(lib)
    assert qin.untouched() and qout.untouched() and np.array_equal(FIX, before[0]) and np.array_equal(RAYS, before[1])


RENDER_CASES = [(dict(cam=False), "cam is NULL"), (dict(params=False), "params is NULL"), (dict(fix=False), "fix is NULL"),
                (dict(width=1), "width and height must be >= 2"), (dict(flags=rt.RT_FLAG_UNIFORM53), "RT_FLAG_UNIFORM53 is not built"),
                (dict(flags=rt.RT_FLAG_ACCUMULATE), "unknown flags 0x1"), (dict(shard_count=2), "shard_count must be 1"),
                (dict(t_min=0.0), "t_min must be > 0"), (dict(t_min=float("inf")), "t_min must be > 0 and finite"), ({}, "ctx is NULL")]


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("kw,msg", RENDER_CASES, ids=[c[1] for c in RENDER_CASES])
def test_render_validation_needs_no_context(form, kw, msg):
    lib = _ffi.load()
    before = (FIX.copy(), RAYS.copy())
    assert _render(form, **kw) == -1
    assert msg in _err(lib), _err(lib)
    assert np.array_equal(FIX, before[0]) and np.array_equal(RAYS, before[1])


def test_the_order_of_the_checks():
    """NULL structs and arrays, the capacity, n, distinct queues, the capacities' order, width / height, npix, the flags, t_min, then the
    context."""
    lib = _ffi.load()
    bad = dict(width=1, flags=8, n=9)
    assert _begin(Queue(capacity=0, null=("dir",)), cam=False, **bad) == -1 and "cam is NULL" in _err(lib)
    assert _begin(Queue(capacity=0, null=("dir",)), **bad) == -1 and "queue->dir is NULL" in _err(lib)
    assert _begin(Queue(capacity=0), **bad) == -1 and "capacity must be" in _err(lib)
    assert _begin(Queue(), **bad) == -1 and "n must be" in _err(lib)
    assert _begin(Queue(), width=1, flags=8) == -1 and "width and height" in _err(lib)
    assert _begin(Queue(), flags=8) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
    assert _begin(Queue()) == -1 and "ctx is NULL" in _err(lib)
    bad = dict(npix=0, flags=8, t_min=0.0)
    q = Queue(null=("event",))
    assert _step(q, q, fix=False, **bad) == -1 and "in->event is NULL" in _err(lib)
    q = Queue()
    assert _step(q, q, fix=False, **bad) == -1 and "d_fix is NULL" in _err(lib)
    assert _step(q, q, **bad) == -1 and "distinct queues" in _err(lib)
    assert _step(Queue(capacity=4), Queue(capacity=2), **bad) == -1 and "out->capacity (2)" in _err(lib)
    assert _step(Queue(), Queue(), **bad) == -1 and "npix must be" in _err(lib)
    assert _step(Queue(), Queue(), flags=8, t_min=0.0) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
    assert _step(Queue(), Queue(), t_min=0.0) == -1 and "t_min must be" in _err(lib)
    assert _step(Queue(), Queue()) == -1 and "ctx is NULL" in _err(lib)


def test_struct_layout_matches_the_header():
    """Every field of the header's struct, in order: capacity as an int64, then eight pointers; ctypes and Rust agree."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct rt_path_queue \{([^}]*)\}\s*rt_path_queue;", src).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype = decl.split()[0]
            for item in decl.strip().split(",")[0:]:
                fields.append((re.search(r"(\w+)\s*$", item).group(1), "*" in item, ctype))
    assert [f for f, _, _ in fields] == [f for f, _ in _ffi.rt_path_queue._fields_] == ["capacity", *QFIELDS]
    assert fields[0] == ("capacity", False, "int64_t") and all(is_ptr for _, is_ptr, _ in fields[1:])
    assert _ffi.rt_path_queue._fields_[0][1] is C.c_int64 and all(t is C.c_void_p for _, t in _ffi.rt_path_queue._fields_[1:])
    assert C.sizeof(_ffi.rt_path_queue) == 72 and _ffi.rt_path_queue.count.offset == 8 and _ffi.rt_path_queue.scratch.offset == 64
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct rt_path_queue \{(.*?)\n\}", rs, flags=re.S).group(1)
    rust = [(m.group(1), m.group(2).strip()) for m in re.finditer(r"pub (\w+):\s*([^,\n]+),", rbody)]
    to_rust = {"uint32_t": "*mut u32", "double": "*mut f64"}
    assert rust == [("capacity", "i64")] + [(f, to_rust[t]) for f, _, t in fields[1:]]
    assert "72 == size_of::<rt_path_queue>()" in rs and re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct rt_path_queue ", rs)
    for name in ENTRY_POINTS:
        assert f"pub fn {name}(" in rs


def test_the_unit_does_not_read_the_render_kernel():
    """wavefront/rt_paths.hip compiles from rt_host.hpp, rt_first_hit.hpp and rt_shade_core.hpp; neither rt_kernels.hpp nor rt_launch.hpp is
    among the files its compilation reads.  rt_shade.hip reads the shared bodies too."""
    csrc = os.path.join(ROOT, "rtiow_amd", "csrc")
    for unit, needs in (("rt_paths.hip", {"rt_host.hpp", "rt_first_hit.hpp", "rt_shade_core.hpp"}), ("rt_shade.hip", {"rt_host.hpp", "rt_shade_core.hpp"})):
        run = subprocess.run(["hipcc", "-MM", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              os.path.join(csrc, "wavefront", unit)], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        deps = {os.path.basename(d) for d in run.stdout.replace("\\\n", " ").split() if not d.endswith(":")}
        assert needs <= deps, (unit, sorted(deps))
        assert "rt_kernels.hpp" not in deps and "rt_launch.hpp" not in deps, (unit, sorted(deps))
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"wavefront/rt_paths.hip"' in entry


def test_the_cli_knows_the_switch():
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert '"--wavefront"' in src and "rt_render_wavefront(" in src


# ---- the GPU tests' inputs are hard -------------------------------------------------------------------------------------------------

def test_the_hand_queue_is_hard(oracle_mod):
    """Conditions on the step input of tests/test_gpu_paths.py, checked with the reference alone."""
    flat, q, fates = pr.hand_queue()
    alive = np.array([f not in ("miss", "absorbed") for f in fates])
    assert len(fates) == pr.HAND_N == 513 and set(fates) == set(pr.FATES)         # a miss, an absorption, every way to survive
    assert set(pr.FATES) <= set(fates[:63])                                       # ... already in the smallest batch that runs a bounce of many
    waves = [alive[k:k + 64] for k in range(0, 512, 64)]
    assert not waves[2].any()                                                     # a wave with no survivor
    assert waves[1].all()                                                         # a wave where all 64 survive
    assert alive[63] and alive[64]                                                # the last slot of one wave, the first of the next
    assert not alive[256:512].any() and alive[255::-1].any()                      # a workgroup (256 slots) with none, after one with some
    assert alive[512]                                                             # ... and a survivor behind it
    assert 0 < waves[0].sum() < 64 and 0 < waves[3].sum() < 64                    # ragged waves
    # total internal reflection takes no draw; every other survivor and every absorption advances the event
    out, adds, live = pr.hand_step(pr.HAND_N)
    before = q["event"][alive].astype(np.int64)
    advance = out["event"].astype(np.int64) - before
    kinds = np.array(fates)[alive]
    assert (advance[kinds == "tir"] == 0).all() and (advance[kinds != "tir"] >= 1).all()
    assert np.array_equal(out["pixel"], q["pixel"][alive]) and np.array_equal(out["sample"], q["sample"][alive])     # stable
    # glass leaves the throughput alone, everything else tints it
    same_thr = (out["throughput"] == q["throughput"][alive]).all(axis=1)
    assert same_thr[np.isin(kinds, ("tir", "refract", "reflect"))].all() and not same_thr[np.isin(kinds, ("lambertian", "metal"))].any()
    # misses inside the frame add, the two outside it do not
    missed = np.array([f == "miss" for f in fates])
    assert (q["pixel"][missed] >= pr.HAND_NPIX).sum() == 2 and adds.any(axis=1).sum() > 100
    assert live == pr.HAND_N and len(out["pixel"]) == alive.sum()
    for count in (0, 1, 63, 64, 65, 256, 257, 513):
        o, _, lv = pr.hand_step(count)
        assert lv == count and len(o["pixel"]) == alive[:count].sum()
