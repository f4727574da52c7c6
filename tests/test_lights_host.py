"""The lit path queue without a GPU (include/rtiow_hip.h "lighting"): the statement of tests/lights_ref.py against
Oracle B where lighting changes nothing, the context-free validation of the three entry points and its order, the rt_lighting layout in
ctypes and Rust against the header, the CLI's switches, and that the hand-built lit queue and the lit book frame the GPU tests use are
hard."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import lights_ref as lr
import paths_ref as pr
import rtiow_amd as rt
from rtiow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_paths_step_lit_device", "rt_render_wavefront_lit_device", "rt_render_wavefront_lit")
Q48 = 1 << 48                                     # quantize(x) for x >= RT_SAMPLE_CLAMP = 2^16: 2^16 * 2^32


# ---- the statement -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["none", "zeros", "negative_nan"])
def test_statement_without_lights_equals_oracle_b(oracle_mod, book1_flat, table):
    """Book scene, 32 x 18, 4 spp, depth 50, seed 1, in batches of 257: under the reference's sky, with no table, an all-zero one or one
    whose only non-zero entries are negative or NaN, the lit loop gives Oracle B's u64 sums and its ray count."""
    w, h, spp = 32, 18, 4
    ocam = oracle_mod.book1_camera(w, h)
    want, _, st = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, max_depth=50, seed=1))
    emission = lr.dark_tables(len(book1_flat))[table]
    assert emission is None or (emission != 0).any() == (table == "negative_nan")
    got, rays = lr.render_lit(book1_flat, ocam, w, h, spp, lr.Light(*lr.REFERENCE_SKY, emission), max_depth=50, seed=1, batch=257)
    assert np.array_equal(got, want)
    assert rays == st["rays_traced"]


def test_which_entries_are_lights():
    nan, inf = float("nan"), float("inf")
    for e in ((1, 0, 0), (0, 1e-300, 0), (-1, -1, 5e-324), (nan, nan, 2), (-inf, 0, inf)):
        assert lr.is_light(e), e
    for e in ((0, 0, 0), (-0.0, 0, 0), (-1, -2, -3), (nan, nan, nan), (nan, 0, -inf)):
        assert not lr.is_light(e), e


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------------

def _err(lib):
    return lib.rt_last_error().decode()


SENTINEL = 0x5A
QFIELDS = ("count", "pixel", "sample", "event", "origin", "dir", "throughput", "scratch")


class Queue:
    """Host arrays behind every pointer of an rt_path_queue, sentinel-filled (no call here reads or writes them: every call ends in
    validation)."""

    def __init__(self, capacity=4):
        self.keep = {f: np.full(4 * 3 * 8, SENTINEL, dtype=np.uint8) for f in QFIELDS}
        self.q = _ffi.rt_path_queue(capacity, *[self.keep[f].ctypes.data for f in QFIELDS])

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.keep.values())


FIX = np.full(6 * 3 * 8, SENTINEL, dtype=np.uint8)
RAYS = np.full(8, SENTINEL, dtype=np.uint8)
TABLE = np.zeros((4, 3))
DEFAULT = object()


def lighting(*, sky_bottom=(1, 1, 1), sky_top=(0.5, 0.7, 1.0), emission=None, n_emission=0, flags=0):
    return _ffi.rt_lighting((C.c_double * 3)(*sky_bottom), (C.c_double * 3)(*sky_top), emission.ctypes.data if emission is not None else None,
                            n_emission, flags)


def _step(qin, qout, light=DEFAULT, *, flags=0, t_min=1e-4, fix=True, npix=6, ctx=None):
    light = lighting() if light is DEFAULT else light
    return _ffi.load().rt_paths_step_lit_device(ctx, 1, flags, t_min, C.byref(qin.q) if qin else None, C.byref(qout.q) if qout else None,
                                                FIX.ctypes.data if fix else None, npix, RAYS.ctypes.data,
                                                C.byref(light) if light is not None else None, None)


def _render(form, light=DEFAULT, *, cam=True, params=True, fix=True, ctx=None, **kw):
    lib = _ffi.load()
    light = lighting() if light is DEFAULT else light
    camera = rt.book1_camera(8, 8).to_rt_camera()
    p = rt.make_params(8, 8, 2)
    for k, v in kw.items():
        setattr(p, k, v)
    c, pp, f = C.byref(camera) if cam else None, C.byref(p) if params else None, FIX.ctypes.data if fix else None
    ll = C.byref(light) if light is not None else None
    if form == "device":
        return lib.rt_render_wavefront_lit_device(ctx, c, pp, ll, f, RAYS.ctypes.data, None)
    return lib.rt_render_wavefront_lit(ctx, c, pp, ll, f, RAYS.ctypes.data_as(C.POINTER(C.c_uint64)), None)


def test_the_symbols_resolve():
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert lib.rt_abi_version() == 5
    assert callable(rt.Lighting)


NAN, INF = float("nan"), float("inf")
LIGHT_CASES = [
    (None, "light is NULL"),
    (dict(flags=1), "unknown light->flags 0x1"),
    (dict(sky_bottom=(1, NAN, 1)), "light->sky_bottom[1] must be finite and >= 0"),
    (dict(sky_bottom=(-1e-300, 0, 0)), "light->sky_bottom[0] must be finite and >= 0"),
    (dict(sky_top=(1, 1, INF)), "light->sky_top[2] must be finite and >= 0"),
    (dict(sky_top=(1, -INF, 1)), "light->sky_top[1] must be finite and >= 0"),
    (dict(n_emission=4), "light->n_emission must be 0 when light->emission is NULL"),
    (dict(n_emission=-4), "light->n_emission must be 0 when light->emission is NULL"),
    (dict(emission=TABLE, n_emission=-1), "light->n_emission must be >= 0"),
    (dict(), "ctx is NULL"),
    (dict(sky_bottom=(0, 0, 0), sky_top=(0, 0, 0)), "ctx is NULL"),
    (dict(sky_bottom=(-0.0, 1e300, 5e-324)), "ctx is NULL"),
    (dict(emission=TABLE, n_emission=4), "ctx is NULL"),
]
LIGHT_IDS = [f"{c[1]}-{i}" for i, c in enumerate(LIGHT_CASES)]


def _light_of(kw):
    return None if kw is None else lighting(**kw)


@pytest.mark.parametrize("kw,msg", LIGHT_CASES, ids=LIGHT_IDS)
def test_step_rejections_need_no_context(kw, msg):
    lib = _ffi.load()
    qin, qout = Queue(), Queue()
    before = (FIX.copy(), RAYS.copy(), TABLE.copy())
    assert _step(qin, qout, _light_of(kw)) == -1
    assert msg in _err(lib) and "rt_paths_step_lit" in _err(lib) or msg == "ctx is NULL" and msg in _err(lib), _err(lib)
    assert qin.untouched() and qout.untouched() and np.array_equal(FIX, before[0]) and np.array_equal(RAYS, before[1]) and np.array_equal(TABLE, before[2])


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("kw,msg", LIGHT_CASES, ids=LIGHT_IDS)
def test_render_rejections_need_no_context(form, kw, msg):
    lib = _ffi.load()
    before = (FIX.copy(), RAYS.copy())
    assert _render(form, _light_of(kw)) == -1
    assert msg in _err(lib), _err(lib)
    assert np.array_equal(FIX, before[0]) and np.array_equal(RAYS, before[1])


@pytest.mark.parametrize("entry,msg", [((1, 0, NAN), "light->emission[2][2]"), ((INF, 0, 0), "light->emission[2][0]"), ((0, -1e-9, 0), "light->emission[2][1]")])
def test_the_host_form_rejects_a_table_entry_it_can_see(entry, msg):
    """... and the device form, whose table is device memory it does not read, goes on to the context check."""
    lib = _ffi.load()
    table = np.zeros((4, 3))
    table[2] = entry
    before = (FIX.copy(), RAYS.copy())
    assert _render("host", lighting(emission=table, n_emission=4)) == -1
    assert msg in _err(lib) and "must be finite and >= 0" in _err(lib), _err(lib)
    assert _render("device", lighting(emission=table, n_emission=4)) == -1 and "ctx is NULL" in _err(lib)
    assert np.array_equal(FIX, before[0]) and np.array_equal(RAYS, before[1])


def test_the_order_of_the_checks():
    """Every context-free check of the unlit form first, in its order (its last: t_min); then the light: NULL, flags, sky, a count without
    a table, a negative count, (host form) the entries; then the context."""
    lib = _ffi.load()
    bad_table = np.full((4, 3), -1.0)
    worst = dict(flags=2, sky_bottom=(NAN, 0, 0), n_emission=3)
    q = Queue()
    assert _step(q, q, None, fix=False, npix=0, flags=8, t_min=0.0) == -1 and "d_fix is NULL" in _err(lib)
    assert _step(Queue(), Queue(), None, npix=0, flags=8, t_min=0.0) == -1 and "npix must be" in _err(lib)
    assert _step(Queue(), Queue(), None, flags=8, t_min=0.0) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
    assert _step(Queue(), Queue(), None, t_min=0.0) == -1 and "t_min must be" in _err(lib)
    assert _step(Queue(), Queue(), None) == -1 and "light is NULL" in _err(lib)
    assert _step(Queue(), Queue(), lighting(**worst)) == -1 and "light->flags" in _err(lib)
    worst.pop("flags")
    assert _step(Queue(), Queue(), lighting(**worst)) == -1 and "sky_bottom[0]" in _err(lib)
    worst.pop("sky_bottom")
    assert _step(Queue(), Queue(), lighting(sky_top=(0, -1, 0), **worst)) == -1 and "sky_top[1]" in _err(lib)
    assert _step(Queue(), Queue(), lighting(**worst)) == -1 and "n_emission must be 0" in _err(lib)
    assert _step(Queue(), Queue(), lighting(emission=bad_table, n_emission=-2)) == -1 and "n_emission must be >= 0" in _err(lib)
    assert _step(Queue(), Queue(), lighting(emission=bad_table, n_emission=4)) == -1 and "ctx is NULL" in _err(lib)
    for form in ("device", "host"):
        assert _render(form, None, params=False) == -1 and "params is NULL" in _err(lib)
        assert _render(form, None, fix=False, width=1) == -1 and "fix is NULL" in _err(lib)
        assert _render(form, None, width=1, shard_count=2, t_min=INF) == -1 and "width and height" in _err(lib)
        assert _render(form, None, shard_count=2, t_min=INF) == -1 and "shard_count must be 1" in _err(lib)
        assert _render(form, None, t_min=INF) == -1 and "t_min must be" in _err(lib)
        assert _render(form, None) == -1 and "light is NULL" in _err(lib)
        assert _render(form, lighting(flags=4, sky_top=(-1, 0, 0), emission=bad_table, n_emission=-1)) == -1 and "light->flags" in _err(lib)
        assert _render(form, lighting(sky_top=(-1, 0, 0), emission=bad_table, n_emission=-1)) == -1 and "sky_top[0]" in _err(lib)
        assert _render(form, lighting(emission=bad_table, n_emission=-1)) == -1 and "n_emission must be >= 0" in _err(lib)
    assert _render("host", lighting(emission=bad_table, n_emission=4)) == -1 and "light->emission[0][0]" in _err(lib)
    assert _render("device", lighting(emission=bad_table, n_emission=4)) == -1 and "ctx is NULL" in _err(lib)


def test_struct_layout_matches_the_header():
    """rt_lighting: 64 bytes; two colours of three doubles, the table's pointer, its length, the flags -- in the header, ctypes and Rust."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*rt_lighting;", src).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["double sky_bottom[3]", "double sky_top[3]", "const double *emission", "int32_t n_emission", "uint32_t flags"]
    L = _ffi.rt_lighting
    assert [f for f, _ in L._fields_] == ["sky_bottom", "sky_top", "emission", "n_emission", "flags"]
    assert [t for _, t in L._fields_][2:] == [C.c_void_p, C.c_int32, C.c_uint32] and C.sizeof(L._fields_[0][1]) == C.sizeof(L._fields_[1][1]) == 24
    assert C.sizeof(L) == 64
    assert (L.sky_bottom.offset, L.sky_top.offset, L.emission.offset, L.n_emission.offset, L.flags.offset) == (0, 24, 48, 56, 60)
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct rt_lighting \{(.*?)\n\}", rs, flags=re.S).group(1)
    rust = [(m.group(1), m.group(2).strip()) for m in re.finditer(r"pub (\w+):\s*([^\n]+),", rbody)]
    assert rust == [("sky_bottom", "[f64; 3]"), ("sky_top", "[f64; 3]"), ("emission", "*const f64"), ("n_emission", "i32"), ("flags", "u32")]
    assert "64 == size_of::<rt_lighting>()" in rs and re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct rt_lighting ", rs)
    for field, offset in (("sky_top", 24), ("emission", 48), ("n_emission", 56), ("flags", 60)):
        assert f"offset_of!(rt_lighting, {field}) == {offset}" in rs
    for name in ENTRY_POINTS:
        assert f"pub fn {name}(" in rs
        assert re.search(rf"\bint {name}\(", src)
    assert "#define RTIOW_HIP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", src)


def test_the_cli_knows_the_switches():
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert '"--sky"' in src and '"--emit"' in src and "rt_render_wavefront_lit(" in src and "need --wavefront" in src


def test_the_python_lighting_value():
    """Lighting's defaults are the reference's; a dict is expanded against the scene's length; an array passes as it is."""
    light = rt.Lighting()
    assert (light.sky_bottom, light.sky_top, light.emission) == (*lr.REFERENCE_SKY, None) and light.table(5) is None
    s = light.struct()
    assert tuple(s.sky_bottom) == (1.0, 1.0, 1.0) and tuple(s.sky_top) == (0.5, 0.7, 1.0) and not s.emission and s.n_emission == 0 and s.flags == 0
    t = rt.Lighting(emission={3: (1, 2, 3), 0: (0.5, 0, 0)}).table(5)
    assert t.shape == (5, 3) and t.dtype == np.float64 and t[3].tolist() == [1, 2, 3] and t[0].tolist() == [0.5, 0, 0] and not t[[1, 2, 4]].any()
    with pytest.raises(ValueError, match="sphere 5"):
        rt.Lighting(emission={5: (1, 1, 1)}).table(5)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        rt.Lighting(emission=np.zeros((4, 2))).table(4)
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert np.array_equal(rt.Lighting((0, 0, 0), (0, 0, 0), a).table(4), a.astype(np.float64))


# ---- the GPU tests' inputs are hard ------------------------------------------------------------------------------------------------------

def _one(k):
    """The statement on path k of the hand queue alone -> (fate, its additions at its pixel as ints or None outside the frame, path)."""
    flat, q, light = lr.hand_queue()
    sub = {f: q[f][[k]] for f in pr.FIELDS}
    _, fates, adds = lr.bounce_lit(flat, sub, lr.SEED, lr.HAND_NPIX, light)
    pixel = int(q["pixel"][k])
    assert int(adds.any(axis=1).sum()) <= 1
    return fates[0], [int(x) for x in adds[pixel]] if pixel < lr.HAND_NPIX else None, sub


def _quantize(oracle_mod, x):
    return int(oracle_mod.load().oracle_b_quantize(float(x)))


def test_the_hand_queue_is_hard(oracle_mod):
    """Conditions on the step input of tests/test_gpu_lights.py, checked with the statement alone.  Every case asked of a single path sits
    below slot 63, the smallest count at which the GPU tests run a bounce of many."""
    from trace_ref import Scene, fast_hit
    flat, q, light = lr.hand_queue()
    scene = Scene(flat)
    E = light.emission
    assert len(q["pixel"]) == 513 and len(E) == len(flat) == 14
    _, fates, adds = lr.bounce_lit(scene, q, lr.SEED, lr.HAND_NPIX, light)
    _, base_fates, _ = pr.bounce(scene, q, lr.SEED, lr.HAND_NPIX)                 # the same paths with no lighting at all
    hit = [fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), 1e-4) for k in range(513)]
    thr = q["throughput"]
    quant = lambda x: _quantize(oracle_mod, x)
    assert all(max(lr.SLOTS) <= 63 and (k < 63 or what == "front") for k, what in lr.SLOTS.items())

    # a path that ends on a light's front face: throughput * e, per channel
    fate, add, _ = _one(6)
    assert fate == "light" and hit[6][0] == 5 and hit[6][4] == 1 and add == [quant(thr[6][c] * E[5][c]) for c in range(3)] and all(add)
    # one that starts inside a light and ends on its back face
    fate, add, _ = _one(7)
    assert fate == "light" and hit[7][0] == 6 and hit[7][4] == 0 and add == [quant(thr[7][c] * E[6][c]) for c in range(3)] and all(add)
    # a light hit outside the frame adds nothing and still ends
    fate, add, _ = _one(8)
    assert fate == "light" and int(q["pixel"][8]) >= lr.HAND_NPIX and add is None and not lr.bounce_lit(scene, {f: q[f][[8]] for f in pr.FIELDS}, lr.SEED, lr.HAND_NPIX, light)[2].any()
    # a light whose material is Dialectric (its front face: unlit, the path would refract or reflect) ...
    assert _one(9)[0] == "light" and hit[9][0] == 6 and hit[9][4] == 1 and int(flat[6]["kind"]) == 2 and base_fates[9] in ("refract", "reflect")
    # ... and one that is Metal where it would have absorbed: it adds all the same
    fate, add, _ = _one(10)
    assert fate == "light" and hit[10][0] == 7 and int(flat[7]["kind"]) == 1 and base_fates[10] == "absorbed" and all(add)
    # spheres with an entry that lights nothing scatter: (0, 0, 0), a NaN channel and two zeros, only negative / -0
    assert E[3].tolist() == [0, 0, 0] and fates[3] in ("refract", "reflect") and hit[3][0] == 3
    assert math.isnan(E[2][0]) and E[2][1:].tolist() == [0, 0] and fates[2] == "metal" and hit[2][0] == 2
    assert E[0].tolist() == [-1, 0, 0] and fates[1] == "lambertian" and hit[1][0] == 0
    assert fates[5] == "absorbed" and hit[5][0] == 4 and not lr.is_light(E[4])
    # one negative and one positive channel (and a NaN one): the negative and the NaN channel add 0
    fate, add, _ = _one(11)
    assert fate == "light" and hit[11][0] == 8 and E[8][0] < 0 and math.isnan(E[8][2]) and add == [0, quant(thr[11][1] * 0.75), 0] and add[1] > 0
    # throughput * e above 65 536 in one channel: exactly 2^48
    fate, add, _ = _one(12)
    assert fate == "light" and hit[12][0] == 9 and thr[12][0] * E[9][0] > 65536.0 and add[0] == Q48 and 0 < add[1] < Q48 and 0 < add[2] < Q48
    # a light and a non-light at equal t: the later one of the list wins, both ways round
    assert flat[10]["center"].tolist() == flat[11]["center"].tolist() and not lr.is_light(E[10]) and lr.is_light(E[11])
    assert hit[13][0] == 11 and _one(13)[0] == "light"
    assert flat[12]["center"].tolist() == flat[13]["center"].tolist() and lr.is_light(E[12]) and not lr.is_light(E[13])
    fate, add, _ = _one(14)
    assert hit[14][0] == 13 and fate == "metal" and add == [0, 0, 0]
    for a, b in ((10, 11), (12, 13)):                                            # (equal roots indeed: either sphere alone gives the same t)
        for k in (13, 14):
            o, d = q["origin"][k].tolist(), q["dir"][k].tolist()
            ta, tb = fast_hit(Scene(flat[[a]]), o, d, 1e-4)[1], fast_hit(Scene(flat[[b]]), o, d, 1e-4)[1]
            assert ta == tb
    # by waves: 128 .. 191 all end on lights (no survivor), 64 .. 127 none does (all survive), slot 63 a light and slot 64 a survivor
    assert fates[128:192] == ["light"] * 64 and {hit[k][0] for k in range(128, 192)} == {5, 6, 8, 9, 11}
    assert "light" not in fates[64:128] and all(f in lr.SURVIVES for f in fates[64:128])
    assert fates[63] == "light" and fates[64] in lr.SURVIVES
    assert "light" not in fates[192:] and fates[512] in lr.SURVIVES
    # what lighting does not touch: every path that does not end on a light has the fate the unlit statement gives it
    assert all(f == b for f, b in zip(fates, base_fates) if f != "light")
    assert set(pr.FATES) <= set(fates[:63]) and fates[:63].count("light") == 8
    # the misses see the hand sky, not the reference's
    k = fates.index("miss", 1)
    assert int(q["pixel"][k]) < lr.HAND_NPIX
    _, _, sky_adds = lr.bounce_lit(scene, {f: q[f][[k]] for f in pr.FIELDS}, lr.SEED, lr.HAND_NPIX, light)
    _, _, ref_adds = pr.bounce(scene, {f: q[f][[k]] for f in pr.FIELDS}, lr.SEED, lr.HAND_NPIX)
    assert sky_adds.any() and not np.array_equal(sky_adds, ref_adds)
    for count in (0, 1, 63, 64, 65, 256, 257, 513):
        out, _, live = lr.hand_step(count)
        assert live == count and len(out["pixel"]) == sum(f in lr.SURVIVES for f in fates[:count])
    # the whole step with a table that lights nothing and the reference's sky is the unlit statement's, bit for bit
    for table in lr.dark_tables(len(flat)).values():
        out, dark_adds, _ = lr.step_lit(scene, q, lr.SEED, lr.HAND_NPIX, lr.Light(*lr.REFERENCE_SKY, table))
        want, want_adds, _ = pr.step(scene, q, lr.SEED, lr.HAND_NPIX)
        assert np.array_equal(dark_adds, want_adds) and all(np.array_equal(out[f].view(np.uint8), want[f].view(np.uint8)) for f in pr.FIELDS)


def test_the_lit_book_frame_is_lit_directly_and_indirectly(oracle_mod):
    """The lights of lights_ref.book_case(): the large Lambertian sphere and five small ones.  With the statement alone: some pixels see
    a light with a camera ray, and some are brighter than under the dim sky alone although none of their camera rays does."""
    flat, light, first = lr.book_case()
    lights = [k for k in range(len(flat)) if lr.is_light(light.emission[k])]
    assert len(lights) == 6 and sum(float(flat[k]["radius"]) == 1.0 for k in lights) == 1 and sum(float(flat[k]["radius"]) < 0.5 for k in lights) == 5
    direct = np.isin(first, lights).reshape(lr.BH, lr.BW, lr.BSPP).any(axis=2)
    for k in lights:
        assert (first == k).any(), k                                             # every light is seen by some camera ray
    lit, rays = lr.book_frame(50)
    dark, dark_rays = lr.book_frame(50, lit=False)
    brighter = (lit.astype(object) > dark.astype(object)).any(axis=2)
    assert direct.sum() > 20 and (brighter & ~direct).sum() > 20
    assert rays < dark_rays                                                      # paths end on the lights
    # at depth 1 only the direct light and the sky arrive; the rays are one per sample
    one, rays1 = lr.book_frame(1)
    assert rays1 == lr.BW * lr.BH * lr.BSPP and np.array_equal(one.any(axis=2), (first.reshape(lr.BH, lr.BW, lr.BSPP) < 0).any(axis=2) | direct)
    assert not np.array_equal(lr.book_frame(3)[0], lit) and not np.array_equal(lr.book_frame(3)[0], one)


# ---- the kernels, without a GPU ------------------------------------------------------------------------------------------------------------

def test_the_path_kernels_keep_their_machine_code_and_the_lit_one_is_pinned():
    """tools/isa_fingerprint.py --paths: the four lines of profiles/isa_fingerprint_paths.txt exactly -- bounce_kernel, whose loop body
    became a template function, among them -- and the one new line of profiles/isa_fingerprint_lights.txt."""
    import subprocess
    import sys
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--paths"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [ln for ln in run.stdout.splitlines() if re.match(r"rt::(path_begin|bounce|bounce_lit|queue_scan|queue_compact)_kernel ", ln)]
    pinned = lambda name: [ln for ln in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if ln.startswith("rt::")]
    before = [ln for ln in pinned("isa_fingerprint_paths.txt") if not re.match(r"rt::(camera_rays|scatter|accumulate)_kernel ", ln)]
    assert len(before) == 4 and any("rt::bounce_kernel " in ln and "n= 2436" in ln and "ops-sha=3c28b1d6df30" in ln for ln in before)
    assert [ln for ln in got if "bounce_lit_kernel" not in ln] == before
    assert got == pinned("isa_fingerprint_lights.txt") and sum("bounce_lit_kernel" in ln for ln in got) == 1


def test_the_lit_kernel_keeps_occupancy_4_and_uses_no_scratch_memory():
    """The compiler's own resource remarks for wavefront/rt_paths.hip, with the flags tools/kernel_resources.py passes."""
    import subprocess
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
    lit = [r for name, r in rows.items() if "bounce_lit_kernel" in name]
    unlit = [r for name, r in rows.items() if "bounce_kernel" in name]
    assert len(lit) == 1 and len(unlit) == 1
    for r in lit + unlit:
        assert int(r["Occupancy [waves/SIMD]"]) >= 4 and int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
    assert int(lit[0]["VGPRs"]) <= 128
