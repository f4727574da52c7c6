"""Next-event estimation in the lit path queue without a GPU (include/rtiow_hip.h "direct lighting"): rt_light_list
against lights_ref.is_light, the context-free validation of the three entry points and its order behind the lit forms', the rt_direct
layout in ctypes and Rust against the header, the CLI's switch and its exit codes, the statement of tests/nee_ref.py against Oracle B
where direct lighting changes nothing, that the hand-built NEE queue the GPU tests use is hard, and what the compiler says of the three
bounce kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lights_ref as lr
import nee_ref as nr
import paths_ref as pr
import rtiow_amd as rt
from rtiow_amd import _ffi
from test_lights_host import FIX, RAYS, TABLE, Queue, lighting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_light_list", "rt_paths_step_nee_device", "rt_render_wavefront_nee_device", "rt_render_wavefront_nee")
Q48 = 1 << 48                                     # quantize(x) for x >= RT_SAMPLE_CLAMP = 2^16
NAN, INF = float("nan"), float("inf")
SHADOW = np.full(8, 0x5A, dtype=np.uint8)
LIST = np.array([0, 2, 3], dtype=np.int32)
DEFAULT = object()


def _err(lib):
    return lib.rt_last_error().decode()


# ---- rt_light_list -------------------------------------------------------------------------------------------------------------------------

def _light_list(table):
    lib = _ffi.load()
    n = 0 if table is None else len(table)
    out = np.full(max(n, 1) + 1, -7, dtype=np.int32)
    count = C.c_int32(-7)
    rc = lib.rt_light_list(table.ctypes.data if n else None, n, out.ctypes.data, C.byref(count))
    assert rc == 0, _err(lib)
    assert (out[count.value:] == -7).all()                                       # nothing past the list is written
    return out[:count.value].tolist()


def test_light_list_is_the_lit_steps_notion_of_a_light():
    rows = [(0, 0, 0), (1, 0, 0), (-0.0, 0, 0), (0, 1e-300, 0), (-1, -2, -3), (-1, -1, 5e-324), (NAN, NAN, NAN), (NAN, NAN, 2), (NAN, 0, -INF),
            (-INF, 0, INF), (0, 0, 0), (4, 3.2, 2.4)]
    table = np.array(rows, dtype=np.float64)
    want = [s for s in range(len(rows)) if lr.is_light(table[s])]
    assert want == [1, 3, 5, 7, 9, 11]
    assert _light_list(table) == want == nr.light_list(table)
    assert _light_list(None) == [] and _light_list(np.zeros((5, 3))) == []
    for name, t in lr.dark_tables(9).items():
        assert _light_list(t) == [], name
    flat, _, light, _ = nr.hand_queue()
    assert _light_list(np.array(light.emission)) == nr.light_list(light.emission) == [5, 6, 7, 8, 9, 11, 12, 14, 16]
    assert rt.Lighting(emission=np.array(light.emission)).light_list(len(flat)).tolist() == [5, 6, 7, 8, 9, 11, 12, 14, 16]
    assert rt.Lighting().light_list(4).tolist() == [] and rt.Lighting(emission={2: (0, 1, 0), 0: (-1, 0, 0)}).light_list(4).tolist() == [2]


def test_light_list_rejections():
    lib = _ffi.load()
    out, n = np.full(4, -7, dtype=np.int32), C.c_int32(-7)
    assert lib.rt_light_list(TABLE.ctypes.data, -1, out.ctypes.data, C.byref(n)) == -1 and "n_emission must be >= 0" in _err(lib)
    assert lib.rt_light_list(TABLE.ctypes.data, 4, out.ctypes.data, None) == -1 and "n_lights_out is NULL" in _err(lib)
    assert lib.rt_light_list(None, 4, out.ctypes.data, C.byref(n)) == -1 and "emission is NULL" in _err(lib)
    assert lib.rt_light_list(TABLE.ctypes.data, 4, None, C.byref(n)) == -1 and "lights_out is NULL" in _err(lib)
    assert (out == -7).all() and n.value == -7


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------------

def direct(*, lights=LIST, n_lights=3, flags=0):
    return _ffi.rt_direct(lights.ctypes.data if lights is not None else None, n_lights, flags)


def _step(qin, qout, light=DEFAULT, d=DEFAULT, *, step_flags=0, flags=0, t_min=1e-4, fix=True, npix=6):
    light = lighting() if light is DEFAULT else light
    d = direct() if d is DEFAULT else d
    return _ffi.load().rt_paths_step_nee_device(None, 1, flags, t_min, C.byref(qin.q) if qin else None, C.byref(qout.q) if qout else None,
                                                FIX.ctypes.data if fix else None, npix, RAYS.ctypes.data,
                                                C.byref(light) if light is not None else None, C.byref(d) if d is not None else None, step_flags,
                                                SHADOW.ctypes.data, None)


def _render(form, light=DEFAULT, d=DEFAULT, *, params=True, fix=True, **kw):
    lib = _ffi.load()
    light = lighting() if light is DEFAULT else light
    d = direct() if d is DEFAULT else d
    camera = rt.book1_camera(8, 8).to_rt_camera()
    p = rt.make_params(8, 8, 2)
    for k, v in kw.items():
        setattr(p, k, v)
    pp, f = C.byref(p) if params else None, FIX.ctypes.data if fix else None
    ll = C.byref(light) if light is not None else None
    if form == "device":
        return lib.rt_render_wavefront_nee_device(None, C.byref(camera), pp, ll, C.byref(d) if d is not None else None, f, RAYS.ctypes.data,
                                                  SHADOW.ctypes.data, None)
    return lib.rt_render_wavefront_nee(None, C.byref(camera), pp, ll, f, RAYS.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       SHADOW.ctypes.data_as(C.POINTER(C.c_uint64)), None)


def test_the_symbols_resolve():
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert lib.rt_abi_version() == 5                                             # the change only adds
    assert _ffi.RT_PATH_EVENT_DIRECT == 1 << 31 == nr.DIRECT and _ffi.RT_STEP_NO_DIRECT == 1 == nr.NO_DIRECT


# (what is passed, what the message holds); the last rows pass every context-free check
DIRECT_CASES = [
    (dict(d=None), "direct is NULL"),
    (dict(d=dict(flags=1)), "unknown direct->flags 0x1"),
    (dict(d=dict(n_lights=-1)), "direct->n_lights must be >= 0"),
    (dict(d=dict(lights=None, n_lights=2)), "direct->n_lights must be 0 when direct->lights is NULL"),
    (dict(d=dict()), "ctx is NULL"),
    (dict(d=dict(lights=None, n_lights=0)), "ctx is NULL"),
    (dict(d=dict(n_lights=0)), "ctx is NULL"),
    (dict(d=dict(n_lights=1 << 30)), "ctx is NULL"),                             # (n_lights > n_spheres needs the uploaded scene)
]
STEP_CASES = DIRECT_CASES[:4] + [(dict(d=dict(), step_flags=2), "unknown step_flags 0x2"), (dict(d=dict(), step_flags=3), "unknown step_flags 0x3"),
                                 (dict(d=dict(), step_flags=0x80000000), "unknown step_flags 0x80000000"), (dict(d=dict(), step_flags=1), "ctx is NULL")] \
    + DIRECT_CASES[4:]


def _untouched(before):
    return all(np.array_equal(a, b) for a, b in zip((FIX, RAYS, SHADOW, TABLE, LIST), before))


def _snapshot():
    return tuple(a.copy() for a in (FIX, RAYS, SHADOW, TABLE, LIST))


@pytest.mark.parametrize("case,msg", STEP_CASES, ids=[f"{m}-{i}" for i, (_, m) in enumerate(STEP_CASES)])
def test_step_rejections_need_no_context(case, msg):
    lib = _ffi.load()
    qin, qout, before = Queue(), Queue(), _snapshot()
    d = None if case["d"] is None else direct(**case["d"])
    assert _step(qin, qout, DEFAULT, d, step_flags=case.get("step_flags", 0)) == -1
    assert msg in _err(lib) and ("rt_paths_step_nee" in _err(lib) or msg == "ctx is NULL"), _err(lib)
    assert qin.untouched() and qout.untouched() and _untouched(before)


@pytest.mark.parametrize("case,msg", DIRECT_CASES, ids=[f"{m}-{i}" for i, (_, m) in enumerate(DIRECT_CASES)])
def test_device_frame_rejections_need_no_context(case, msg):
    lib = _ffi.load()
    before = _snapshot()
    assert _render("device", DEFAULT, None if case["d"] is None else direct(**case["d"])) == -1
    assert msg in _err(lib) and ("rt_render_wavefront_nee" in _err(lib) or msg == "ctx is NULL"), _err(lib)
    assert _untouched(before)


def test_the_order_of_the_checks():
    """Every context-free check of the lit form first, in its order (its last: a negative n_emission, in the host form the table's
    entries); then the direct argument: NULL, flags, a negative count, a count without a list; then the step flag; then the context.  The
    host form takes no list: behind the lit form's checks comes the context."""
    lib = _ffi.load()
    bad_table = np.full((4, 3), -1.0)
    worst = dict(flags=4, n_lights=-3, lights=None)
    assert _step(Queue(), Queue(), None, None, fix=False, step_flags=6, t_min=0.0) == -1 and "d_fix is NULL" in _err(lib)
    assert _step(Queue(), Queue(), None, None, step_flags=6, flags=8, t_min=0.0) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
    assert _step(Queue(), Queue(), None, None, step_flags=6, t_min=0.0) == -1 and "t_min must be" in _err(lib)
    assert _step(Queue(), Queue(), None, None, step_flags=6) == -1 and "light is NULL" in _err(lib)
    assert _step(Queue(), Queue(), lighting(flags=2), None, step_flags=6) == -1 and "light->flags" in _err(lib)
    assert _step(Queue(), Queue(), lighting(sky_top=(0, -1, 0)), None, step_flags=6) == -1 and "sky_top[1]" in _err(lib)
    assert _step(Queue(), Queue(), lighting(n_emission=3), None, step_flags=6) == -1 and "n_emission must be 0" in _err(lib)
    assert _step(Queue(), Queue(), lighting(emission=bad_table, n_emission=-2), None, step_flags=6) == -1 and "n_emission must be >= 0" in _err(lib)
    assert _step(Queue(), Queue(), lighting(emission=bad_table, n_emission=4), None, step_flags=6) == -1 and "direct is NULL" in _err(lib)
    assert _step(Queue(), Queue(), DEFAULT, direct(**worst), step_flags=6) == -1 and "direct->flags" in _err(lib)
    worst.pop("flags")
    assert _step(Queue(), Queue(), DEFAULT, direct(**worst), step_flags=6) == -1 and "n_lights must be >= 0" in _err(lib)
    assert _step(Queue(), Queue(), DEFAULT, direct(lights=None, n_lights=3), step_flags=6) == -1 and "n_lights must be 0" in _err(lib)
    assert _step(Queue(), Queue(), DEFAULT, direct(), step_flags=6) == -1 and "step_flags 0x6" in _err(lib)
    assert _step(Queue(), Queue(), DEFAULT, direct(), step_flags=1) == -1 and "ctx is NULL" in _err(lib)
    for form in ("device", "host"):
        assert _render(form, None, None, params=False) == -1 and "params is NULL" in _err(lib)
        assert _render(form, None, None, fix=False) == -1 and "fix is NULL" in _err(lib)
        assert _render(form, None, None, shard_count=2, t_min=INF) == -1 and "shard_count must be 1" in _err(lib)
        assert _render(form, None, None, t_min=INF) == -1 and "t_min must be" in _err(lib)
        assert _render(form, None, None) == -1 and "light is NULL" in _err(lib)
        assert _render(form, lighting(flags=4, sky_top=(-1, 0, 0)), None) == -1 and "light->flags" in _err(lib)
        assert _render(form, lighting(emission=bad_table, n_emission=-1), None) == -1 and "n_emission must be >= 0" in _err(lib)
    assert _render("host", lighting(emission=bad_table, n_emission=4), None) == -1 and "light->emission[0][0]" in _err(lib)
    assert _render("host", lighting(emission=TABLE, n_emission=4), None) == -1 and "ctx is NULL" in _err(lib)
    assert _render("device", lighting(emission=bad_table, n_emission=4), None) == -1 and "direct is NULL" in _err(lib)
    assert _render("device", lighting(emission=bad_table, n_emission=4), direct(flags=1, n_lights=-1)) == -1 and "direct->flags" in _err(lib)
    assert _render("device", lighting(emission=bad_table, n_emission=4), direct()) == -1 and "ctx is NULL" in _err(lib)


def test_struct_layout_matches_the_header():
    """rt_direct: 16 bytes; the list's pointer, its length, the flags -- in the header, ctypes and Rust; the two constants likewise."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*rt_direct;", src).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["const int32_t *lights", "int32_t n_lights", "uint32_t flags"]
    D = _ffi.rt_direct
    assert D._fields_ == [("lights", C.c_void_p), ("n_lights", C.c_int32), ("flags", C.c_uint32)]
    assert C.sizeof(D) == 16 and (D.lights.offset, D.n_lights.offset, D.flags.offset) == (0, 8, 12)
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct rt_direct \{(.*?)\n\}", rs, flags=re.S).group(1)
    rust = [(m.group(1), m.group(2).strip()) for m in re.finditer(r"pub (\w+):\s*([^\n]+),", rbody)]
    assert rust == [("lights", "*const i32"), ("n_lights", "i32"), ("flags", "u32")]
    assert "16 == size_of::<rt_direct>()" in rs and re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct rt_direct ", rs)
    for field, offset in (("n_lights", 8), ("flags", 12)):
        assert f"offset_of!(rt_direct, {field}) == {offset}" in rs
    for name in ENTRY_POINTS:
        assert f"pub fn {name}(" in rs
        assert re.search(rf"\bint {name}\(", src)
    flat_src = re.sub(r"[ \t]+", " ", src)
    assert "#define RT_PATH_EVENT_DIRECT 0x80000000u" in flat_src and "#define RT_STEP_NO_DIRECT 1u" in flat_src
    assert "pub const RT_PATH_EVENT_DIRECT: u32 = 0x8000_0000;" in rs and "pub const RT_STEP_NO_DIRECT: u32 = 1;" in rs
    assert "#define RTIOW_HIP_ABI_VERSION 5" in flat_src


def test_the_cli_knows_the_switch_and_refuses_it_alone(tmp_path, book1_flat):
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert '"--direct"' in src and "rt_render_wavefront_nee(" in src
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    base = [exe, "--scene", scene_file, "--width", "8", "--height", "8", "--spp", "1", "--out", str(tmp_path / "o.ppm")]
    # (every one is refused while the arguments are read: no device is asked for)
    for args, word in ((["--direct"], "--wavefront"), (["--direct", "--emit", "0:1,1,1"], "--wavefront"), (["--wavefront", "--direct"], "--emit"),
                       (["--wavefront", "--direct", "--sky", "0,0,0:0,0,0"], "--emit")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.returncode, bad.stderr)


# ---- the statement -----------------------------------------------------------------------------------------------------------------------

def test_statement_without_lights_equals_oracle_b(oracle_mod, book1_flat):
    """Book scene, 32 x 18, 4 spp, depth 50, seed 1, in batches of 257, the reference's sky and a table that lights nothing: render_nee gives
    Oracle B's u64 sums and its ray count, and traces no shadow ray."""
    w, h, spp = 32, 18, 4
    ocam = oracle_mod.book1_camera(w, h)
    want, _, st = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, max_depth=50, seed=1))
    emission = lr.dark_tables(len(book1_flat))["negative_nan"]
    got, rays, shadow = nr.render_nee(book1_flat, ocam, w, h, spp, lr.Light(*lr.REFERENCE_SKY, emission), max_depth=50, seed=1, batch=257)
    assert np.array_equal(got, want)
    assert rays == st["rays_traced"] and shadow == 0


def _one(k, **kw):
    """The statement on path k of the hand queue alone -> (fate, its additions at its pixel as ints, the out event or None, the sample)."""
    flat, q, light, lights = nr.hand_queue()
    sub = {f: q[f][[k]] for f in pr.FIELDS}
    new, fates, adds, samples = nr.bounce_nee(flat, sub, nr.SEED, nr.HAND_NPIX, light, kw.pop("lights", lights), **kw)
    pixel = int(q["pixel"][k])
    assert int(adds.any(axis=1).sum()) <= 1
    event = int(new["event"][0]) if fates[0] in lr.SURVIVES else None
    return fates[0], [int(x) for x in adds[pixel]] if pixel < nr.HAND_NPIX else None, event, samples[0]


def test_the_hand_queue_is_hard(oracle_mod):
    """Conditions on the step input of tests/test_gpu_nee.py, checked with the statement alone.  Every case asked of a single path sits
    below slot 63, the smallest count at which the GPU tests run a bounce of many."""
    from trace_ref import Scene, fast_hit
    flat, q, light, lights = nr.hand_queue()
    scene = Scene(flat)
    E = light.emission
    quant = lambda x: int(oracle_mod.load().oracle_b_quantize(float(x)))
    assert len(q["pixel"]) == 513 and len(E) == len(flat) == 17 and len(lights) == 11 <= len(flat)
    assert max(nr.CASES) < 63 and max(nr.DIRECT_SLOTS) < 63
    new, fates, adds, samples = nr.bounce_nee(scene, q, nr.SEED, nr.HAND_NPIX, light, lights)
    _, lit_fates, lit_adds = lr.bounce_lit(scene, q, nr.SEED, nr.HAND_NPIX, light)
    hit = [fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), 1e-4) for k in range(513)]
    blockers = set()

    def shadow_hit(k):
        return fast_hit(scene, list(hit[k][2]), samples[k]["dv"], 1e-4)[0]

    # a light chosen at each end of the list, both visible
    s = _one(1)[3]
    assert s["j"] == 0 and s["li"] == lights[0] == 14 and s["visible"] and s["word"] <= (1 << 32) // len(lights)
    s = _one(19)[3]
    assert s["j"] == len(lights) - 1 and s["li"] == lights[-1] == 16 and s["visible"] and s["word"] >= (1 << 32) - (1 << 32) // len(lights)
    # a shadow ray blocked by another sphere: the closest hit is the occluder, and the path adds nothing
    fate, add, event, s = _one(25)
    assert fate == "lambertian" and s["shadow"] and not s["visible"] and shadow_hit(25) == 15 and add == [0, 0, 0] and event & nr.DIRECT
    # the sampled point lies on the light's far side: nl <= 0, no shadow ray
    fate, add, event, s = _one(31)
    assert s["ns"] > 0.0 and s["nl"] <= 0.0 and not s["shadow"] and add == [0, 0, 0] and event & nr.DIRECT
    # ... below the hit's own horizon: ns <= 0
    fate, add, event, s = _one(37)
    assert s["ns"] <= 0.0 and not s["shadow"] and add == [0, 0, 0] and event & nr.DIRECT
    # a try accepted first, and one accepted only in a later block (the third try or later: block 2 of the sample's own counter)
    assert _one(61)[3]["tries"] == 1 and _one(61)[3]["visible"] and any(_one(61)[1])
    assert _one(43)[3]["tries"] >= 3 and _one(43)[3]["visible"] and any(_one(43)[1])
    # a list entry that names no sphere: no contribution, no shadow ray, the bit still set
    fate, add, event, s = _one(49)
    assert s["li"] in (99, -1) and not s["shadow"] and add == [0, 0, 0] and event & nr.DIRECT
    assert {samples[k]["li"] for k in range(513) if samples[k] is not None} >= {99, -1}
    # a contribution above the clamp adds exactly 2^48
    fate, add, event, s = _one(55)
    assert s["visible"] and s["c"][0] > 65536.0 and add[0] == Q48 and 0 < add[1] < Q48 and 0 < add[2] < Q48
    assert add == [quant(c) for c in s["c"]]
    # a DIRECT path on a light's front face adds nothing; the same path without the bit adds; slot 63, without the bit, adds
    assert q["event"][6] & nr.DIRECT and hit[6][0] == 5 and hit[6][4] == 1
    assert _one(6)[:2] == ("light_counted", [0, 0, 0])
    plain = {f: q[f][[6]].copy() for f in pr.FIELDS}
    plain["event"] &= np.uint32(0x7FFFFFFF)
    _, f6, a6, _ = nr.bounce_nee(scene, plain, nr.SEED, nr.HAND_NPIX, light, lights)
    assert f6 == ["light"] and [int(x) for x in a6[int(q["pixel"][6])]] == [quant(q["throughput"][6][c] * E[5][c]) for c in range(3)] and a6.any()
    assert not q["event"][63] & nr.DIRECT and hit[63][4] == 1 and _one(63)[0] == "light" and all(_one(63)[1])
    # a DIRECT path that meets a light's back face from inside adds
    assert q["event"][7] & nr.DIRECT and hit[7][0] == 6 and hit[7][4] == 0
    fate, add, _, _ = _one(7)
    assert fate == "light" and add == [quant(q["throughput"][7][c] * E[6][c]) for c in range(3)] and all(add)
    # a Metal and a Dialectric hit clear the bit; a Lambertian one that samples keeps it set; without lights or with NO_DIRECT it is cleared
    assert q["event"][2] & nr.DIRECT and _one(2)[0] == "metal" and not _one(2)[2] & nr.DIRECT and _one(2)[3] is None
    assert q["event"][3] & nr.DIRECT and _one(3)[0] in ("refract", "reflect") and not _one(3)[2] & nr.DIRECT and _one(3)[3] is None
    assert q["event"][17] & nr.DIRECT and fates[17] == "lambertian" and _one(17)[2] & nr.DIRECT
    assert not _one(17, no_direct=True)[2] & nr.DIRECT and not _one(17, lights=())[2] & nr.DIRECT
    # the bit is masked off before any Philox use: the DIRECT paths scatter as the same paths without it
    for k in (2, 3, 17):
        plain = {f: q[f][[k]].copy() for f in pr.FIELDS}
        plain["event"] &= np.uint32(0x7FFFFFFF)
        base, base_fate, _ = lr.bounce_lit(scene, plain, nr.SEED, nr.HAND_NPIX, light)
        assert base_fate == [fates[k]] and np.array_equal(base["dir"][0], new["dir"][k]) and int(base["event"][0]) == int(new["event"][k]) & 0x7FFFFFFF
    # by waves: all 64 lanes with a shadow ray; none (the wave that ends on lights whole, and the waves of misses); only lane 63
    assert all(samples[k] is not None and samples[k]["shadow"] for k in nr.ALL_WAVE)
    assert not any(samples[k] is not None for k in range(128, 192)) and not any(samples[k] is not None for k in range(256, 320))
    lone = [k for k in nr.LAST_LANE_WAVE if samples[k] is not None and samples[k]["shadow"]]
    assert lone == [447] and 447 % 64 == 63
    assert any(samples[k]["visible"] for k in nr.ALL_WAVE) and any(not samples[k]["visible"] for k in nr.ALL_WAVE)
    # NEE changes what is added, never where paths go: every array of the lit statement but bit 31 of the event, for the paths whose events agree
    same_event = [k for k in range(513) if not q["event"][k] & nr.DIRECT]
    for k in same_event:
        assert fates[k] == lit_fates[k], k
    lit_new = lr.bounce_lit(scene, q, nr.SEED, nr.HAND_NPIX, light)[0]
    for f in pr.FIELDS:
        a, b = new[f][same_event], lit_new[f][same_event]
        if f == "event":
            a = a & np.uint32(0x7FFFFFFF)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f
    assert not np.array_equal(adds, lit_adds)
    # with no list, or NO_DIRECT, on the paths without the bit the statement is the lit one, bit for bit
    sub = {f: q[f][same_event] for f in pr.FIELDS}
    want, want_adds, _ = lr.step_lit(scene, sub, nr.SEED, nr.HAND_NPIX, light)
    for kw in (dict(lights=()), dict(lights=lights, no_direct=True)):
        out, dark_adds, _, shadow = nr.step_nee(scene, sub, nr.SEED, nr.HAND_NPIX, light, kw["lights"], kw.get("no_direct", False))
        assert shadow == 0 and np.array_equal(dark_adds, want_adds) and all(np.array_equal(out[f].view(np.uint8), want[f].view(np.uint8)) for f in pr.FIELDS)
    for count in (0, 1, 63, 64, 65, 256, 257, 513):
        out, _, live, shadow = nr.hand_step(count)
        assert live == count and len(out["pixel"]) == sum(f in lr.SURVIVES for f in fates[:count])
        assert shadow == sum(1 for s in samples[:count] if s is not None and s["shadow"])
    assert nr.hand_step(513)[3] > 64 and nr.hand_step(1)[3] == 0 and nr.hand_step(63)[3] > 0


# ---- the kernels, without a GPU ------------------------------------------------------------------------------------------------------------

def test_the_path_kernels_keep_their_machine_code_and_the_nee_one_is_pinned():
    """tools/isa_fingerprint.py --paths: the five lines of profiles/isa_fingerprint_lights.txt exactly -- bounce_kernel and bounce_lit_kernel,
    whose trip gained a third mode, among them -- and the one new line of profiles/isa_fingerprint_nee.txt."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--paths"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [ln for ln in run.stdout.splitlines() if re.match(r"rt::(path_begin|bounce|bounce_lit|bounce_nee|queue_scan|queue_compact)_kernel ", ln)]
    pinned = lambda name: [ln for ln in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if ln.startswith("rt::")]
    before = pinned("isa_fingerprint_lights.txt")
    assert len(before) == 5 and any("rt::bounce_lit_kernel " in ln and "ops-sha=cd9b07f2e329" in ln for ln in before)
    assert [ln for ln in got if "bounce_nee_kernel" not in ln] == before
    assert [ln for ln in got if "bounce_nee_kernel" in ln] == pinned("isa_fingerprint_nee.txt") and len(pinned("isa_fingerprint_nee.txt")) == 1


def test_the_bounce_kernels_use_no_scratch_memory_and_spill_no_vector_register():
    """The compiler's own resource remarks for wavefront/rt_paths.hip, with the flags tools/kernel_resources.py passes.  The occupancy
    of the NEE kernel is reported, not promised."""
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
    bounce = {kind: [r for name, r in rows.items() if f"{kind}E" in name] for kind in ("bounce_kernel", "bounce_lit_kernel", "bounce_nee_kernel")}
    for kind, found in bounce.items():
        assert len(found) == 1, kind
        r = found[0]
        print(kind, "VGPRs", r["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "SGPR spills", r["SGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, (kind, r)
