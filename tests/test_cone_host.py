"""Direct lighting by solid angle without a GPU (include/rtiow_hip.h "direct lighting by solid angle"): that the
hand-built cone queue the GPU tests use is hard, the statement of tests/cone_ref.py against Oracle B where direct lighting changes nothing
and against tests/nee_ref.py where the flag is 0, the one bound of the estimator, the new rejections of the loaded library and their
order, the header against ctypes and Rust, the CLI's switch and its exit codes, and what the compiler says of bounce_cone_kernel."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cone_ref as cr
import lights_ref as lr
import nee_ref as nr
import paths_ref as pr
import rtiow_amd as rt
import test_nee_host as tnh
from rtiow_amd import _ffi
from test_lights_host import FIX, RAYS, TABLE, Queue, lighting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADOW = tnh.SHADOW
INF = float("inf")


def _err(lib):
    return lib.rt_last_error().decode()


# ---- the statement -----------------------------------------------------------------------------------------------------------------------

def _one(k, **kw):
    """The statement on path k of the hand queue alone -> (fate, its additions at its pixel as ints, the out event or None, the sample)."""
    flat, q, light, lights = cr.hand_queue()
    sub = {f: q[f][[k]] for f in pr.FIELDS}
    new, fates, adds, samples = cr.bounce_cone(flat, sub, cr.SEED, cr.HAND_NPIX, light, kw.pop("lights", lights), **kw)
    pixel = int(q["pixel"][k])
    assert int(adds.any(axis=1).sum()) <= 1
    event = int(new["event"][0]) if fates[0] in lr.SURVIVES else None
    return fates[0], [int(x) for x in adds[pixel]] if pixel < cr.HAND_NPIX else None, event, samples[0]


def test_the_hand_queue_is_hard(oracle_mod):
    """Conditions on the step input of tests/test_gpu_cone.py, checked with the statement alone.  Every case asked of a single path sits
    below slot 63, the smallest count at which the GPU tests run a bounce of many."""
    from trace_ref import Scene, fast_hit
    flat, q, light, lights = cr.hand_queue()
    scene = Scene(flat)
    E = light.emission
    quant = lambda x: int(oracle_mod.load().oracle_b_quantize(float(x)))
    assert len(q["pixel"]) == 513 and len(E) == len(flat) == 21 and len(lights) == 15 <= len(flat)
    assert max(cr.CASES) < 63 and max(cr.DIRECT_SLOTS) < 63
    new, fates, adds, samples = cr.bounce_cone(scene, q, cr.SEED, cr.HAND_NPIX, light, lights)
    hit = [fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), 1e-4) for k in range(513)]

    def shadow_hit(k):
        return fast_hit(scene, list(hit[k][2]), samples[k]["dv"], 1e-4)

    # a hit point inside a light (d2 <= r2): no ray, the bit still set; the path never met the light (it started inside it)
    fate, add, event, s = _one(1)
    assert fate == "lambertian" and hit[1][0] == 0 and s["li"] == 19 and 0.0 < s["d2"] <= s["r2"] and not s["shadow"] and add == [0, 0, 0] and event & nr.DIRECT
    # a sample below the hit's own horizon: ns <= 0
    fate, add, event, s = _one(19)
    assert s["ns"] <= 0.0 and not s["shadow"] and s["c"] is None and add == [0, 0, 0] and event & nr.DIRECT
    # a disk try accepted first, and one accepted only in a later block (the third try: block 2 of the sample's own counter)
    assert _one(31)[3]["tries"] == 1 and _one(31)[3]["visible"] and any(_one(31)[1])
    assert _one(37)[3]["tries"] >= 3 and _one(37)[3]["visible"] and any(_one(37)[1])
    # both branches of step 7: the tangent frame is built from (1, 0, 0), and from (0, 1, 0) where w is nearly that
    assert abs(_one(23)[3]["wx"]) < 0.9 and _one(23)[3]["visible"] and all(_one(23)[1])
    assert abs(_one(43)[3]["wx"]) > 0.9 and _one(43)[3]["li"] == 18 and _one(43)[3]["visible"] and all(_one(43)[1])
    # a shadow ray blocked by another sphere: the closest hit is the occluder, and the path adds nothing
    fate, add, event, s = _one(25)
    assert s["li"] == 14 and s["shadow"] and not s["visible"] and shadow_hit(25)[0] == 15 and add == [0, 0, 0] and event & nr.DIRECT
    # the light overlaps the shaded sphere and passes 5e-5 from the hit point: the near root lies below t_min, the closest hit is the
    # light's INNER face, and it counts
    fate, add, event, s = _one(cr.NEAR_SLOT)
    gap = np.sqrt(s["d2"]) - np.sqrt(s["r2"])
    assert s["li"] == 20 and 0.0 < gap < 1e-4 and s["visible"] and s["front"] == 0 and shadow_hit(cr.NEAR_SLOT)[1] > 1e-4
    assert add == [quant(c) for c in s["c"]] and all(add) and s["k"] > 0.9
    centre0 = np.array(flat[0]["center"], dtype=np.float64)
    assert np.linalg.norm(np.array(flat[20]["center"]) - centre0) < float(flat[0]["radius"]) + float(flat[20]["radius"])      # they overlap
    # a list entry that names no sphere: no contribution, no shadow ray, the bit still set
    fate, add, event, s = _one(49)
    assert s["li"] in (99, -1) and not s["shadow"] and add == [0, 0, 0] and event & nr.DIRECT
    assert {samples[k]["li"] for k in range(513) if samples[k] is not None} >= {99, -1}
    # a light at r / d = 1e-6: k = q / (1 + cm) is 5e-13 to full precision, where 1 - cm keeps four digits; the sample adds
    fate, add, event, s = _one(61)
    ratio = np.sqrt(s["r2"] / s["d2"])
    assert s["li"] == 17 and 0.99e-6 < ratio < 1.01e-6 and s["visible"] and all(add)
    qq = np.float64(s["r2"]) / np.float64(s["d2"])
    naive = np.float64(1.0) - np.sqrt(np.float64(1.0) - qq)
    assert abs(s["k"] / (0.5 * qq) - 1.0) < 1e-12 and abs(naive / s["k"] - 1.0) > 1e-6
    # a DIRECT path on a light's front face adds nothing; on a back face it adds (nee_ref's slots, whatever the sampler)
    assert q["event"][6] & nr.DIRECT and hit[6][0] == 5 and hit[6][4] == 1 and _one(6)[:2] == ("light_counted", [0, 0, 0])
    assert q["event"][7] & nr.DIRECT and hit[7][0] == 6 and hit[7][4] == 0
    fate, add, _, _ = _one(7)
    assert fate == "light" and add == [quant(q["throughput"][7][c] * E[6][c]) for c in range(3)] and all(add)
    # the bit is set when the sample yields nothing, and cleared with NO_DIRECT or without lights
    assert not _one(19, no_direct=True)[2] & nr.DIRECT and not _one(19, lights=())[2] & nr.DIRECT and _one(19, no_direct=True)[3] is None
    # by waves: all 64 lanes with a shadow ray; none (the wave that ends on lights whole, and the waves of misses); only lane 63
    assert all(samples[k] is not None and samples[k]["shadow"] for k in cr.ALL_WAVE)
    assert not any(samples[k] is not None for k in range(128, 192)) and not any(samples[k] is not None for k in range(256, 320))
    lone = [k for k in cr.LAST_LANE_WAVE if samples[k] is not None and samples[k]["shadow"]]
    assert lone == [447] and 447 % 64 == 63
    assert any(samples[k]["visible"] for k in cr.ALL_WAVE) and any(not samples[k]["visible"] for k in cr.ALL_WAVE)
    # the sampler changes what is added, never where paths go: every array of the area statement on the same queue
    area_new, area_fates, area_adds, area_samples = nr.bounce_nee(scene, q, cr.SEED, cr.HAND_NPIX, light, lights)
    assert area_fates == fates and not np.array_equal(area_adds, adds)
    for f in pr.FIELDS:
        assert np.array_equal(new[f].view(np.uint8), area_new[f].view(np.uint8)), f
    n_cone, n_area = sum(1 for s in samples if s is not None and s["shadow"]), sum(1 for s in area_samples if s is not None and s["shadow"])
    assert n_cone != n_area
    for count in (0, 1, 63, 64, 65, 256, 257, 513):
        out, _, live, shadow = cr.hand_step(count)
        assert live == count and len(out["pixel"]) == sum(f in lr.SURVIVES for f in fates[:count])
        assert shadow == sum(1 for s in samples[:count] if s is not None and s["shadow"])
    assert cr.hand_step(513)[3] > 64 and cr.hand_step(1)[3] == 0 and cr.hand_step(63)[3] > 0


def test_no_sample_of_the_hand_queue_exceeds_the_bound():
    """cadd <= cone_sample_bound() * throughput per channel, throughput the path's on entry (no albedo exceeds 1), for every sample of
    the hand queue -- the light 5e-5 from the hit point and the light that would pass the clamp under area sampling among them."""
    flat, q, light, lights = cr.hand_queue()
    bound = cr.cone_sample_bound(np.where(np.isfinite(light.emission), light.emission, 0.0))
    assert bound == 3.0e7 * 2 * 13                                              # (thirteen entries of the table are lights)
    _, _, _, samples = cr.bounce_cone(flat, q, cr.SEED, cr.HAND_NPIX, light, lights)
    seen = 0
    for k, s in enumerate(samples):
        if s is None or s["c"] is None:
            continue
        e_max = max(x for x in light.emission[s["li"]] if x == x)
        for c in range(3):
            if s["c"][c] == s["c"][c]:
                # the bound of one light: 2 n_lights e, n_lights the LIST's length; the frame's bound takes the table's largest e
                assert s["c"][c] <= 2.0 * len(lights) * max(e_max, 0.0) * float(q["throughput"][k][c]) * (1.0 + 1e-12), (k, c, s)
        seen += 1
    assert seen > 64
    # ... and with the list the frame forms build from the table, the frame's bound holds for every sample
    table_list = nr.light_list(light.emission)
    _, _, _, samples = cr.bounce_cone(flat, q, cr.SEED, cr.HAND_NPIX, light, table_list)
    for k, s in enumerate(samples):
        if s is not None and s["c"] is not None:
            assert all(not x > bound * float(q["throughput"][k][c]) for c, x in enumerate(s["c"])), (k, s)


def test_statement_without_lights_equals_oracle_b(oracle_mod, book1_flat):
    """Book scene, 32 x 18, 4 spp, depth 50, seed 1, in batches of 257, the reference's sky and a table that lights nothing: render_cone
    gives Oracle B's u64 sums and its ray count, and traces no shadow ray."""
    w, h, spp = 32, 18, 4
    ocam = oracle_mod.book1_camera(w, h)
    want, _, st = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, max_depth=50, seed=1))
    emission = lr.dark_tables(len(book1_flat))["negative_nan"]
    got, rays, shadow = cr.render_cone(book1_flat, ocam, w, h, spp, lr.Light(*lr.REFERENCE_SKY, emission), max_depth=50, seed=1, batch=257)
    assert np.array_equal(got, want)
    assert rays == st["rays_traced"] and shadow == 0


def test_with_flags_zero_the_statement_is_nee_refs():
    """direct->flags = 0: step_cone is nee_ref.step_nee, on nee_ref's hand queue and on this one -- every array, the sums, both counts."""
    for source in (nr, cr):
        flat, q, light, lights = source.hand_queue()
        for no_direct in (False, True):
            want = nr.step_nee(flat, q, nr.SEED, nr.HAND_NPIX, light, lights, no_direct)
            got = cr.step_cone(flat, q, nr.SEED, nr.HAND_NPIX, light, lights, no_direct, flags=0)
            assert all(np.array_equal(got[0][f].view(np.uint8), want[0][f].view(np.uint8)) for f in pr.FIELDS)
            assert np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    assert not np.array_equal(cr.hand_step(513)[1], cr.hand_step(513, flags=0)[1])


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------------

def _render_sampled(direct_flags, light=tnh.DEFAULT, *, params=True, fix=True, **kw):
    lib = _ffi.load()
    light = lighting() if light is tnh.DEFAULT else light
    camera = rt.book1_camera(8, 8).to_rt_camera()
    p = rt.make_params(8, 8, 2)
    for k, v in kw.items():
        setattr(p, k, v)
    return lib.rt_render_wavefront_nee_sampled(None, C.byref(camera), C.byref(p) if params else None, C.byref(light) if light is not None else None,
                                               direct_flags, FIX.ctypes.data if fix else None, RAYS.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               SHADOW.ctypes.data_as(C.POINTER(C.c_uint64)), None)


def test_the_symbol_resolves_and_the_abi_version_stays():
    lib = _ffi.load()
    assert "rt_render_wavefront_nee_sampled" in [n for n, _, _ in _ffi.SYMBOLS] and lib.rt_render_wavefront_nee_sampled
    assert lib.rt_abi_version() == 5                                             # the change only adds
    assert _ffi.RT_DIRECT_CONE == 2 == cr.CONE


@pytest.mark.parametrize("flags", [1, 3, 4, 6, 0x80000002])
def test_other_flags_are_still_rejected(flags):
    """In the three forms that take an rt_direct or its flags: the message used before, nothing touched, no context needed."""
    lib = _ffi.load()
    qin, qout, before = Queue(), Queue(), tnh._snapshot()
    assert tnh._step(qin, qout, tnh.DEFAULT, tnh.direct(flags=flags)) == -1
    assert f"rt_paths_step_nee: unknown direct->flags 0x{flags:x}" in _err(lib)
    assert tnh._render("device", tnh.DEFAULT, tnh.direct(flags=flags)) == -1
    assert f"rt_render_wavefront_nee: unknown direct->flags 0x{flags:x}" in _err(lib)
    assert _render_sampled(flags) == -1
    assert f"rt_render_wavefront_nee_sampled: unknown direct->flags 0x{flags:x}" in _err(lib)
    assert qin.untouched() and qout.untouched() and tnh._untouched(before)


def test_the_cone_flag_passes_on_to_the_context_check():
    lib = _ffi.load()
    qin, qout, before = Queue(), Queue(), tnh._snapshot()
    for step_flags in (0, 1):
        assert tnh._step(qin, qout, tnh.DEFAULT, tnh.direct(flags=2), step_flags=step_flags) == -1 and "ctx is NULL" in _err(lib)
    assert tnh._render("device", tnh.DEFAULT, tnh.direct(flags=2)) == -1 and "ctx is NULL" in _err(lib)
    for flags in (0, 2):
        assert _render_sampled(flags) == -1 and "ctx is NULL" in _err(lib)
        assert _render_sampled(flags, lighting(emission=TABLE, n_emission=4)) == -1 and "ctx is NULL" in _err(lib)
    assert qin.untouched() and qout.untouched() and tnh._untouched(before)


def test_the_order_of_the_checks():
    """The flags sit where direct->flags != 0 sat: behind every context-free check of the lit form (in the host form: the table's entries
    last), before the count checks of the list, the step flag and the context."""
    lib = _ffi.load()
    bad_table = np.full((4, 3), -1.0)
    assert tnh._step(Queue(), Queue(), lighting(emission=bad_table, n_emission=-2), tnh.direct(flags=2), step_flags=6) == -1 and "n_emission must be >= 0" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=3, n_lights=-3, lights=None), step_flags=6) == -1 and "direct->flags 0x3" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=2, n_lights=-3, lights=None), step_flags=6) == -1 and "n_lights must be >= 0" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=2, n_lights=3, lights=None), step_flags=6) == -1 and "n_lights must be 0" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=2), step_flags=6) == -1 and "step_flags 0x6" in _err(lib)
    assert tnh._render("device", lighting(emission=bad_table, n_emission=4), tnh.direct(flags=6, n_lights=-1)) == -1 and "direct->flags 0x6" in _err(lib)
    assert tnh._render("device", lighting(emission=bad_table, n_emission=4), tnh.direct(flags=2, n_lights=-1)) == -1 and "n_lights must be >= 0" in _err(lib)
    before = tnh._snapshot()
    assert _render_sampled(1, None, params=False) == -1 and "params is NULL" in _err(lib)
    assert _render_sampled(1, None, fix=False) == -1 and "fix is NULL" in _err(lib)
    assert _render_sampled(1, None, shard_count=2, t_min=INF) == -1 and "shard_count must be 1" in _err(lib)
    assert _render_sampled(1, None, t_min=INF) == -1 and "t_min must be" in _err(lib)
    assert _render_sampled(1, None) == -1 and "light is NULL" in _err(lib)
    assert _render_sampled(1, lighting(flags=4, sky_top=(-1, 0, 0))) == -1 and "light->flags" in _err(lib)
    assert _render_sampled(1, lighting(sky_top=(0, -1, 0))) == -1 and "sky_top[1]" in _err(lib)
    assert _render_sampled(1, lighting(emission=bad_table, n_emission=-1)) == -1 and "n_emission must be >= 0" in _err(lib)
    assert _render_sampled(1, lighting(emission=bad_table, n_emission=4)) == -1 and "light->emission[0][0]" in _err(lib)
    assert _render_sampled(1, lighting(emission=TABLE, n_emission=4)) == -1 and "direct->flags 0x1" in _err(lib)
    assert _render_sampled(2, lighting(emission=TABLE, n_emission=4)) == -1 and "ctx is NULL" in _err(lib)
    assert tnh._untouched(before)


def test_header_ctypes_and_rust_agree():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    flat_src = re.sub(r"\s+", " ", src)
    assert "#define RT_DIRECT_CONE 2u" in flat_src and "#define RTIOW_HIP_ABI_VERSION 5" in flat_src
    decl = re.search(r"\bint rt_render_wavefront_nee_sampled\(([^)]*)\)", flat_src).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "rt_context *ctx", "const rt_camera *cam", "const rt_params *p", "const rt_lighting *light", "uint32_t direct_flags", "uint64_t *fix",
        "uint64_t *rays_traced", "uint64_t *shadow_rays", "float *kernel_ms"]
    sym = {n: (r, a) for n, r, a in _ffi.SYMBOLS}["rt_render_wavefront_nee_sampled"]
    plain = {n: (r, a) for n, r, a in _ffi.SYMBOLS}["rt_render_wavefront_nee"]
    assert sym[0] is C.c_int and sym[1] == plain[1][:4] + [C.c_uint32] + plain[1][4:]
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub const RT_DIRECT_CONE: u32 = 2;" in rs
    rdecl = re.sub(r"\s+", " ", re.search(r"pub fn rt_render_wavefront_nee_sampled\((.*?)\) -> i32;", rs, flags=re.S).group(1))
    assert [a.strip() for a in rdecl.split(",")] == [
        "ctx: *mut rt_context", "cam: *const rt_camera", "p: *const rt_params", "light: *const rt_lighting", "direct_flags: u32", "fix: *mut u64",
        "rays_traced: *mut u64", "shadow_rays: *mut u64", "kernel_ms: *mut f32"]


def test_the_python_forms_know_the_sampling():
    import inspect
    for f in (rt.Renderer.render_wavefront, rt.Renderer.render_wavefront_device, rt.Renderer.paths_step_device, rt.paths_step_torch):
        assert inspect.signature(f).parameters["sampling"].default == "area", f
    from rtiow_amd.render import _direct_flags
    assert _direct_flags("area", True) == 0 == _direct_flags("area", False) and _direct_flags("cone", True) == 2 == _direct_flags("cone", [3])
    with pytest.raises(ValueError, match="sampling must be"):
        _direct_flags("solid", True)
    with pytest.raises(ValueError, match="belongs to direct lighting"):
        _direct_flags("cone", False)


def test_the_cli_knows_the_switch_and_its_exit_codes(tmp_path, book1_flat):
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert '"--direct-cone"' in src and "rt_render_wavefront_nee_sampled(" in src and "RT_DIRECT_CONE" in src
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    base = [exe, "--scene", scene_file, "--width", "8", "--height", "8", "--spp", "1", "--out", str(tmp_path / "o.ppm")]
    # (every one is refused while the arguments are read: no device is asked for)
    for args, word in ((["--direct-cone"], "--wavefront"), (["--direct-cone", "--emit", "0:1,1,1"], "--wavefront"), (["--wavefront", "--direct-cone"], "--emit"),
                       (["--wavefront", "--direct-cone", "--sky", "0,0,0:0,0,0"], "--emit"),
                       (["--wavefront", "--direct", "--direct-cone", "--emit", "0:1,1,1"], "one of them"),
                       (["--wavefront", "--direct-cone", "--direct", "--emit", "0:1,1,1"], "one of them")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.returncode, bad.stderr)


# ---- the kernels, without a GPU ------------------------------------------------------------------------------------------------------------

def test_the_six_path_kernels_keep_their_machine_code_and_the_cone_one_is_pinned():
    """tools/isa_fingerprint.py --paths: the five lines of profiles/isa_fingerprint_lights.txt and the one of profiles/isa_fingerprint_nee.txt
    exactly, in their places, and behind bounce_nee_kernel's the one new line of profiles/isa_fingerprint_cone.txt."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--paths"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [ln for ln in run.stdout.splitlines() if re.match(r"rt::\w+_kernel ", ln)]
    pinned = lambda name: [ln for ln in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if ln.startswith("rt::")]
    lights, nee, cone = pinned("isa_fingerprint_lights.txt"), pinned("isa_fingerprint_nee.txt"), pinned("isa_fingerprint_cone.txt")
    assert len(lights) == 5 and len(nee) == 1 and len(cone) == 1 and cone[0].startswith("rt::bounce_cone_kernel ")
    assert got[-7:] == lights[:3] + nee + cone + lights[3:]                      # (not the last kernel: the padding behind that one is counted)
    assert not any("_kernel " in ln and "render_kernel" not in ln and "resolve" not in ln for ln in got[:-7])


def test_the_cone_kernel_uses_no_scratch_memory_and_spills_no_vector_register():
    """The compiler's own resource remarks for wavefront/rt_paths.hip, with the flags tools/kernel_resources.py passes.  The occupancy is
    reported, not promised."""
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
    found = [r for name, r in rows.items() if "bounce_cone_kernelE" in name]
    assert len(found) == 1
    r = found[0]
    print("bounce_cone_kernel VGPRs", r["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "SGPR spills", r["SGPRs Spill"])
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
