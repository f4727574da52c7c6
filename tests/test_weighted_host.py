"""Direct lighting with a weighted choice of the light, without a GPU (include/rtiow_hip.h "direct lighting with a weighted choice of
the light"): that the hand-built queue the GPU tests use is hard, the statement of tests/weighted_ref.py against
tests/cone_ref.py where the list holds one light and against Oracle B where direct lighting changes nothing, the one bound of the
estimator, the new flag's rejections in the loaded library and their order, the header against ctypes and Rust, the CLI's switch and its
exit codes, what the compiler says of bounce_weighted_kernel, and on the eight-light scene -- with the statement alone -- the same
expectation as the random walk and as the uniform choice, at less variance than the uniform choice."""
import functools
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
import test_cone_host as tch
import test_nee_host as tnh
import weighted_ref as wt
from rtiow_amd import _ffi
from test_lights_host import TABLE, Queue, lighting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err(lib):
    return lib.rt_last_error().decode()


# ---- the statement -----------------------------------------------------------------------------------------------------------------------

def _one(k, **kw):
    """The statement on path k of the hand queue alone -> (fate, its additions at its pixel as ints, the out event or None, the sample)."""
    flat, q, light, lights = wt.hand_queue()
    sub = {f: q[f][[k]] for f in pr.FIELDS}
    new, fates, adds, samples = wt.bounce_weighted(flat, sub, wt.SEED, wt.HAND_NPIX, light, kw.pop("lights", lights), **kw)
    pixel = int(q["pixel"][k])
    assert int(adds.any(axis=1).sum()) <= 1
    event = int(new["event"][0]) if fates[0] in lr.SURVIVES else None
    return fates[0], [int(x) for x in adds[pixel]] if pixel < wt.HAND_NPIX else None, event, samples[0]


def test_the_hand_queue_is_hard(oracle_mod, monkeypatch):
    """Conditions on the step input of tests/test_gpu_weighted.py, checked with the statement alone.  Every case asked of a single path
    sits below slot 63, the smallest count at which the GPU tests run a bounce of many."""
    from trace_ref import Scene, fast_hit
    flat, q, light, lights = wt.hand_queue()
    scene = Scene(flat)
    E = light.emission
    quant = lambda x: int(oracle_mod.load().oracle_b_quantize(float(x)))
    assert len(q["pixel"]) == 513 and len(E) == len(flat) == 21 and lights == cr.LIGHTS + (15,) and len(lights) == 16 <= len(flat)
    assert max(wt.CASES) < 63 and max(wt.DIRECT_SLOTS) < 63
    new, fates, adds, samples = wt.bounce_weighted(scene, q, wt.SEED, wt.HAND_NPIX, light, lights)
    hit = [fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), 1e-4) for k in range(513)]
    taken = [s for s in samples if s is not None]

    def shadow_hit(k):
        return fast_hit(scene, list(hit[k][2]), samples[k]["dv"], 1e-4)

    # entries never chosen: the two that name no sphere (99, -1), the sphere that does not emit (15), the light whose largest channel
    # is a NaN on the right of a comparison (8: e = (-2, 0.75, NaN)); each has the weight 0 at every hit point, and the list's last
    # entry is not its last positive one
    never = [lights.index(s) for s in (99, -1, 15, 8)]
    assert all(s["imp"][i] == 0.0 for s in taken for i in never) and not {s["j"] for s in taken} & set(never)
    assert lights[wt.FIRST_POSITIVE] == 14 and lights[wt.LAST_POSITIVE] == 20 and wt.LAST_POSITIVE == len(lights) - 2
    assert all(s["imp"][wt.FIRST_POSITIVE] > 0.0 for s in taken)
    assert len({s["li"] for s in taken}) >= 6                                    # the choice is spread over the list
    # a hit point inside light 19 (d2 <= r2): its weight is 0 there, another light is chosen and a ray traced -- which ends on 19's
    # inner face; under the uniform choice this path chose 19 and traced nothing (cone_ref's slot 1)
    fate, add, event, s = _one(1)
    i19 = lights.index(19)
    centre19, r19 = np.array(flat[19]["center"], dtype=np.float64), float(flat[19]["radius"])
    assert fate == "lambertian" and hit[1][0] == 0 and np.linalg.norm(np.array(hit[1][2]) - centre19) < r19
    assert s["imp"][i19] == 0.0 and s["li"] not in (None, 19) and s["shadow"] and not s["visible"] and shadow_hit(1)[0] == 19
    assert add == [0, 0, 0] and event & nr.DIRECT and s["tot"] > 0.0
    # ... and inside every light the list can reach (the light that holds it, no sphere, no emitter): tot = 0, no ray, the bit still set
    fate, add, event, s = _one(1, lights=wt.INNER_LIGHTS)
    assert fate == "lambertian" and s["tot"] == 0.0 and s["imp"] == [0.0, 0.0, 0.0] and s["j"] is None and not s["shadow"]
    assert add == [0, 0, 0] and event & nr.DIRECT
    # the first and the last positive entry chosen, each seen and adding; the last one 5e-5 from the hit point, on its inner face
    fate, add, event, s = _one(19)
    assert s["j"] == wt.FIRST_POSITIVE and s["li"] == 14 and s["visible"] and not s["fallback"] and add == [quant(c) for c in s["c"]] and all(add)
    fate, add, event, s = _one(cr.NEAR_SLOT)
    assert s["j"] == wt.LAST_POSITIVE and s["li"] == 20 and s["visible"] and s["front"] == 0 and not s["fallback"]
    assert add == [quant(c) for c in s["c"]] and all(add) and s["imp"][wt.LAST_POSITIVE] > 0.9 * s["tot"]
    # the fallback of 1c: the draw no word gives, 1.0, makes x = tot, no partial sum exceeds it, and the last POSITIVE entry is taken --
    # not the last entry -- with the weight tot / imp_j of that entry
    usual = _one(19)[3]
    monkeypatch.setattr(wt, "choice_draw", lambda word: 1.0)
    fate, add, event, s = _one(19)
    monkeypatch.undo()
    assert s["fallback"] and s["j"] == wt.LAST_POSITIVE and s["li"] == 20 and s["tot"] == usual["tot"] and s["imp"] == usual["imp"]
    assert event & nr.DIRECT and (s["c"] is None or all(c >= 0.0 for c in s["c"]))
    just_below = np.float64(wt.choice_draw(0xFFFFFFFF)) * np.float64(usual["tot"])
    assert just_below < usual["tot"]                                             # (no word of the generator reaches the fallback here)
    # a sample below the hit's own horizon: ns <= 0
    fate, add, event, s = _one(23)
    assert s["ns"] <= 0.0 and not s["shadow"] and s["c"] is None and add == [0, 0, 0] and event & nr.DIRECT
    # a shadow ray blocked by another sphere: the closest hit is the occluder, and the path adds nothing
    fate, add, event, s = _one(25)
    assert s["li"] == 14 and s["shadow"] and not s["visible"] and shadow_hit(25)[0] == 15 and add == [0, 0, 0] and event & nr.DIRECT
    # a disk try accepted first, and one accepted only in a later block (the third try: block 2 of the sample's own counter)
    assert _one(31)[3]["tries"] == 1 and _one(31)[3]["visible"] and any(_one(31)[1])
    assert _one(37)[3]["tries"] >= 3 and _one(37)[3]["visible"] and any(_one(37)[1])
    # the other tangent frame of the cone sample
    assert abs(_one(43)[3]["wx"]) > 0.9 and _one(43)[3]["li"] == 18 and _one(43)[3]["visible"] and all(_one(43)[1])
    # a DIRECT path on a light's front face adds nothing; on a back face it adds (nee_ref's slots, whatever the sampler)
    assert q["event"][6] & nr.DIRECT and hit[6][0] == 5 and hit[6][4] == 1 and _one(6)[:2] == ("light_counted", [0, 0, 0])
    assert q["event"][7] & nr.DIRECT and hit[7][0] == 6 and hit[7][4] == 0
    fate, add, _, _ = _one(7)
    assert fate == "light" and add == [quant(q["throughput"][7][c] * E[6][c]) for c in range(3)] and all(add)
    # the bit is set when the sample yields nothing, and cleared with NO_DIRECT or without lights
    assert not _one(23, no_direct=True)[2] & nr.DIRECT and not _one(23, lights=())[2] & nr.DIRECT and _one(23, no_direct=True)[3] is None
    # by waves: all 64 lanes with a shadow ray; none (the wave that ends on lights whole, and the waves of misses); only lane 63
    assert all(samples[k] is not None and samples[k]["shadow"] for k in wt.ALL_WAVE)
    assert not any(samples[k] is not None for k in range(128, 192)) and not any(samples[k] is not None for k in range(256, 320))
    lone = [k for k in wt.LAST_LANE_WAVE if samples[k] is not None and samples[k]["shadow"]]
    assert lone == [447] and 447 % 64 == 63
    assert any(samples[k]["visible"] for k in wt.ALL_WAVE) and any(not samples[k]["visible"] for k in wt.ALL_WAVE)
    # the choice changes what is added, never where paths go: every array of the cone statement on the same queue, table and list
    cone_new, cone_fates, cone_adds, cone_samples = cr.bounce_cone(scene, q, wt.SEED, wt.HAND_NPIX, light, lights)
    assert cone_fates == fates and not np.array_equal(cone_adds, adds)
    for f in pr.FIELDS:
        assert np.array_equal(new[f].view(np.uint8), cone_new[f].view(np.uint8)), f
    n_weighted, n_cone = sum(1 for s in taken if s["shadow"]), sum(1 for s in cone_samples if s is not None and s["shadow"])
    assert n_weighted > n_cone                                                   # (no sample is lost on an entry that can give nothing)
    for count in (0, 1, 63, 64, 65, 256, 257, 513):
        out, _, live, shadow = wt.hand_step(count)
        assert live == count and len(out["pixel"]) == sum(f in lr.SURVIVES for f in fates[:count])
        assert shadow == sum(1 for s in samples[:count] if s is not None and s["shadow"])
    assert wt.hand_step(513)[3] > 64 and wt.hand_step(1)[3] == 0 and wt.hand_step(63)[3] > 0
    # under the inner list every hit point outside light 19 chooses it -- the one positive entry, in the middle of the list -- and finds
    # it below its horizon (19 hangs on sphere 0's side): no ray at all, the bit set on every Lambertian survivor
    out, inner_adds, live, shadow = wt.hand_step(513, lights=wt.INNER_LIGHTS)
    _, _, _, inner = wt.bounce_weighted(scene, q, wt.SEED, wt.HAND_NPIX, light, wt.INNER_LIGHTS)
    assert shadow == 0 and (out["event"] & np.uint32(nr.DIRECT)).any() and not np.array_equal(inner_adds, adds)
    assert {s["j"] for s in inner if s is not None} == {None, 1} and sum(1 for s in inner if s is not None and s["j"] is None) == 1


def test_no_sample_of_the_hand_queue_exceeds_the_bound():
    """cadd <= 2 tot * throughput <= weighted_sample_bound() * throughput per channel, throughput the path's on entry (no albedo exceeds
    1), for every sample of the hand queue -- the light 5e-5 from the hit point among them --, under the queue's table and under
    cone_ref's, whose lights of 2e6 and 3e7 the choice then takes almost always."""
    flat, q, light, lights = wt.hand_queue()
    for table in (light, cr.hand_queue()[2]):
        bound = wt.weighted_sample_bound(table.emission, lights)
        positive = [max(x for x in table.emission[s] if x == x) for s in lights if 0 <= s < len(flat) and lr.is_light(table.emission[s])]
        assert bound == 2.0 * sum(positive) and len(positive) == 13
        _, _, _, samples = wt.bounce_weighted(flat, q, wt.SEED, wt.HAND_NPIX, table, lights)
        seen = 0
        for k, s in enumerate(samples):
            if s is None or s["c"] is None:
                continue
            for c in range(3):
                if s["c"][c] == s["c"][c]:
                    assert s["c"][c] <= 2.0 * s["tot"] * float(q["throughput"][k][c]) * (1.0 + 1e-12), (k, c, s)
                    assert s["c"][c] <= bound * float(q["throughput"][k][c]), (k, c, s)
            seen += 1
        assert seen > 64
    assert wt.weighted_sample_bound() == 2.0 * (20 + 30 + 30 + 30 + 20 + 16 + 30 + 40) == 432.0


def test_with_one_light_the_statement_is_cone_refs():
    """A list of one valid light: tot / imp_j is exactly 1.0 and ((2 k) 1) ns == ((2 k) ns) 1, so the step is the cone step bit for bit
    -- every array, the sums, both counts -- on the hand queue for a far light, a near one, the one that holds slot 1's hit point (no hit point
    sees it above its horizon: no ray either way) and the one at r / d = 1e-6,
    and the frame of nee_ref's stat scene (one light in the table) is cone_ref's."""
    flat, q, light, _ = wt.hand_queue()
    for one in (14, 20, 19, 17):
        for no_direct in (False, True):
            want = cr.step_cone(flat, q, wt.SEED, wt.HAND_NPIX, light, (one,), no_direct)
            got = wt.step_weighted(flat, q, wt.SEED, wt.HAND_NPIX, light, (one,), no_direct)
            assert all(np.array_equal(got[0][f].view(np.uint8), want[0][f].view(np.uint8)) for f in pr.FIELDS), one
            assert np.array_equal(got[1], want[1]) and got[2:] == want[2:] and (got[3] > 0) == (not no_direct and one != 19), one
    import oracle
    sflat, slight = nr.stat_scene()
    ocam = oracle.camera_from_host(nr.stat_camera())
    want = cr.render_cone(sflat, ocam, nr.STAT_W, nr.STAT_H, 4, slight, max_depth=4, seed=101)
    got = wt.render_weighted(sflat, ocam, nr.STAT_W, nr.STAT_H, 4, slight, max_depth=4, seed=101)
    assert np.array_equal(got[0], want[0]) and got[0].any() and got[1:] == want[1:] and got[2] > 0
    # ... and with the hand queue's sixteen entries it is not
    assert not np.array_equal(wt.hand_step(513)[1], cr.step_cone(flat, q, wt.SEED, wt.HAND_NPIX, light, wt.LIGHTS)[1])


def test_statement_without_lights_equals_oracle_b(oracle_mod, book1_flat):
    """Book scene, 32 x 18, 4 spp, depth 50, seed 1, in batches of 257, the reference's sky and a table that lights nothing:
    render_weighted gives Oracle B's u64 sums and its ray count, and traces no shadow ray."""
    w, h, spp = 32, 18, 4
    ocam = oracle_mod.book1_camera(w, h)
    want, _, st = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, max_depth=50, seed=1))
    emission = lr.dark_tables(len(book1_flat))["negative_nan"]
    got, rays, shadow = wt.render_weighted(book1_flat, ocam, w, h, spp, lr.Light(*lr.REFERENCE_SKY, emission), max_depth=50, seed=1, batch=257)
    assert np.array_equal(got, want)
    assert rays == st["rays_traced"] and shadow == 0


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------------

def test_the_constants_agree_and_the_abi_version_stays():
    lib = _ffi.load()
    assert lib.rt_abi_version() == 5                                             # the change only adds
    assert _ffi.RT_DIRECT_WEIGHTED == 8 == wt.WEIGHTED and (_ffi.RT_DIRECT_WEIGHTED | _ffi.RT_DIRECT_CONE) == 10 == wt.FLAGS


def test_the_weighted_flags_pass_on_to_the_context_check():
    """10 in the three forms that take an rt_direct or its flags: on to "ctx is NULL", nothing touched."""
    lib = _ffi.load()
    qin, qout, before = Queue(), Queue(), tnh._snapshot()
    for step_flags in (0, 1):
        assert tnh._step(qin, qout, tnh.DEFAULT, tnh.direct(flags=10), step_flags=step_flags) == -1 and "ctx is NULL" in _err(lib)
    assert tnh._render("device", tnh.DEFAULT, tnh.direct(flags=10)) == -1 and "ctx is NULL" in _err(lib)
    assert tch._render_sampled(10) == -1 and "ctx is NULL" in _err(lib)
    assert tch._render_sampled(10, lighting(emission=TABLE, n_emission=4)) == -1 and "ctx is NULL" in _err(lib)
    assert qin.untouched() and qout.untouched() and tnh._untouched(before)


@pytest.mark.parametrize("flags", [8, 9, 11, 12, 14])
def test_the_weighted_bit_alone_and_with_other_bits_is_rejected(flags):
    """RT_DIRECT_WEIGHTED without RT_DIRECT_CONE, and with any further bit: the message used before, nothing touched, no context needed."""
    lib = _ffi.load()
    qin, qout, before = Queue(), Queue(), tnh._snapshot()
    assert tnh._step(qin, qout, tnh.DEFAULT, tnh.direct(flags=flags)) == -1
    assert f"rt_paths_step_nee: unknown direct->flags 0x{flags:x}" in _err(lib)
    assert tnh._render("device", tnh.DEFAULT, tnh.direct(flags=flags)) == -1
    assert f"rt_render_wavefront_nee: unknown direct->flags 0x{flags:x}" in _err(lib)
    assert tch._render_sampled(flags) == -1
    assert f"rt_render_wavefront_nee_sampled: unknown direct->flags 0x{flags:x}" in _err(lib)
    assert qin.untouched() and qout.untouched() and tnh._untouched(before)


def test_the_order_of_the_checks():
    """The flags sit where they sat: behind every context-free check of the lit form (in the host form: the table's entries last), before
    the count checks of the list, the step flag and the context -- for 8, which is rejected, and for 10, which passes on."""
    lib = _ffi.load()
    bad_table = np.full((4, 3), -1.0)
    assert tnh._step(Queue(), Queue(), lighting(emission=bad_table, n_emission=-2), tnh.direct(flags=8), step_flags=6) == -1 and "n_emission must be >= 0" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=8, n_lights=-3, lights=None), step_flags=6) == -1 and "direct->flags 0x8" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=10, n_lights=-3, lights=None), step_flags=6) == -1 and "n_lights must be >= 0" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=10, n_lights=3, lights=None), step_flags=6) == -1 and "n_lights must be 0" in _err(lib)
    assert tnh._step(Queue(), Queue(), tnh.DEFAULT, tnh.direct(flags=10), step_flags=6) == -1 and "step_flags 0x6" in _err(lib)
    assert tnh._render("device", lighting(emission=bad_table, n_emission=4), tnh.direct(flags=12, n_lights=-1)) == -1 and "direct->flags 0xc" in _err(lib)
    assert tnh._render("device", lighting(emission=bad_table, n_emission=4), tnh.direct(flags=10, n_lights=-1)) == -1 and "n_lights must be >= 0" in _err(lib)
    before = tnh._snapshot()
    assert tch._render_sampled(8, None, params=False) == -1 and "params is NULL" in _err(lib)
    assert tch._render_sampled(8, None, fix=False) == -1 and "fix is NULL" in _err(lib)
    assert tch._render_sampled(8, None) == -1 and "light is NULL" in _err(lib)
    assert tch._render_sampled(8, lighting(emission=bad_table, n_emission=4)) == -1 and "light->emission[0][0]" in _err(lib)
    assert tch._render_sampled(8, lighting(emission=TABLE, n_emission=4)) == -1 and "direct->flags 0x8" in _err(lib)
    assert tch._render_sampled(10, lighting(emission=bad_table, n_emission=4)) == -1 and "light->emission[0][0]" in _err(lib)
    assert tch._render_sampled(10, lighting(emission=TABLE, n_emission=4)) == -1 and "ctx is NULL" in _err(lib)
    assert tnh._untouched(before)


def test_header_ctypes_and_rust_agree():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    flat_src = re.sub(r"\s+", " ", src)
    assert "#define RT_DIRECT_WEIGHTED 8u" in flat_src and "#define RT_DIRECT_CONE 2u" in flat_src and "#define RTIOW_HIP_ABI_VERSION 5" in flat_src
    assert _ffi.RT_DIRECT_WEIGHTED == 8
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub const RT_DIRECT_WEIGHTED: u32 = 8;" in rs and "pub const RT_DIRECT_CONE: u32 = 2;" in rs
    # no new entry point: the header declares what it declared
    assert len(re.findall(r"\bint rt_render_wavefront_nee\w*\(", flat_src)) == 3 and "weighted" not in " ".join(n for n, _, _ in _ffi.SYMBOLS)


def test_the_python_forms_know_the_sampling():
    from rtiow_amd.render import _direct_flags
    assert _direct_flags("weighted", True) == 10 == _direct_flags("weighted", [3])
    assert _direct_flags("area", True) == 0 == _direct_flags("area", False) and _direct_flags("cone", True) == 2
    with pytest.raises(ValueError, match="sampling must be"):
        _direct_flags("importance", True)
    with pytest.raises(ValueError, match="belongs to direct lighting"):
        _direct_flags("weighted", False)
    r = rt.Renderer.__new__(rt.Renderer)                                         # (the check comes before the handle is looked at)
    with pytest.raises(ValueError, match="belongs to direct lighting"):
        rt.Renderer.render_wavefront(r, None, None, lighting=None, direct=False, sampling="weighted")


def test_the_cli_knows_the_switch_and_its_exit_codes(tmp_path, book1_flat):
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert '"--direct-weighted"' in src and "RT_DIRECT_WEIGHTED | RT_DIRECT_CONE" in src
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    base = [exe, "--scene", scene_file, "--width", "8", "--height", "8", "--spp", "1", "--out", str(tmp_path / "o.ppm")]
    emit = ["--emit", "0:1,1,1"]
    # (every one is refused while the arguments are read: no device is asked for)
    for args, word in ((["--direct-weighted"], "--wavefront"), (["--direct-weighted"] + emit, "--wavefront"), (["--wavefront", "--direct-weighted"], "--emit"),
                       (["--wavefront", "--direct-weighted", "--sky", "0,0,0:0,0,0"], "--emit"),
                       (["--wavefront", "--direct", "--direct-weighted"] + emit, "one of them"),
                       (["--wavefront", "--direct-weighted", "--direct-cone"] + emit, "one of them"),
                       (["--wavefront", "--direct-cone", "--direct-weighted"] + emit, "one of them"),
                       (["--wavefront", "--direct-cone", "--direct"] + emit, "one of them"),
                       (["--wavefront", "--direct", "--direct-cone", "--direct-weighted"] + emit, "one of them")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.returncode, bad.stderr)


# ---- the kernels, without a GPU ------------------------------------------------------------------------------------------------------------

def test_the_seven_path_kernels_keep_their_machine_code_and_the_weighted_one_is_pinned():
    """tools/isa_fingerprint.py --paths --weighted: the seven lines --paths alone prints (profiles/isa_fingerprint_lights.txt, _nee.txt and
    _cone.txt) exactly, in their places, and behind bounce_cone_kernel's the one new line of profiles/isa_fingerprint_weighted.txt."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--paths", "--weighted"], capture_output=True, text=True,
                         cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [ln for ln in run.stdout.splitlines() if re.match(r"rt::\w+_kernel ", ln)]
    pinned = lambda name: [ln for ln in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if ln.startswith("rt::")]
    lights, nee, cone, weighted = (pinned(f"isa_fingerprint_{n}.txt") for n in ("lights", "nee", "cone", "weighted"))
    assert len(lights) == 5 and len(nee) == 1 and len(cone) == 1 and len(weighted) == 1 and weighted[0].startswith("rt::bounce_weighted_kernel ")
    assert got[-8:] == lights[:3] + nee + cone + weighted + lights[3:]           # (not the last kernel: the padding behind that one is counted)
    assert not any("_kernel " in ln and "render_kernel" not in ln and "resolve" not in ln for ln in got[:-8])


def test_the_weighted_kernel_uses_no_scratch_memory_and_spills_no_vector_register():
    """The compiler's own resource remarks for wavefront/rt_paths.hip, with the flags tools/kernel_resources.py passes.  Registers and
    occupancy are reported, not promised."""
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
    found = [r for name, r in rows.items() if "bounce_weighted_kernelE" in name]
    assert len(found) == 1
    r = found[0]
    print("bounce_weighted_kernel VGPRs", r["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "SGPR spills", r["SGPRs Spill"])
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r


# ---- the eight-light scene, with the statement alone ----------------------------------------------------------------------------------------

@functools.lru_cache(None)
def many_light_statement_frames():
    """-> (weighted, cone, lit: 16 frames each at depth 8, one per seed; the indirect pixels from the 16 lit frames at depth 1)."""
    import oracle
    flat, light = wt.many_light_scene()
    ocam = oracle.camera_from_host(nr.stat_camera())
    size = (wt.MANY_W, wt.MANY_H, wt.MANY_SPP)
    weighted, cone, lit, first = [], [], [], []
    for seed in wt.MANY_SEEDS:
        weighted.append(wt.render_weighted(flat, ocam, *size, light, max_depth=wt.MANY_DEPTH, seed=seed)[0])
        cone.append(cr.render_cone(flat, ocam, *size, light, max_depth=wt.MANY_DEPTH, seed=seed)[0])
        lit.append(lr.render_lit(flat, ocam, *size, light, max_depth=wt.MANY_DEPTH, seed=seed)[0])
        first.append(lr.render_lit(flat, ocam, *size, light, max_depth=1, seed=seed)[0])
    return weighted, cone, lit, wt.indirect_pixels(first)


def test_many_lights_same_expectation_less_variance():
    """The eight-light scene, 16 x 12, 64 spp, depth 8, seeds 101 .. 116, the statement alone.  On the pixels that see no light directly,
    per seed the energy of weighted minus lit, and of weighted minus cone: |mean| <= 5 standard errors of the 16 differences; and the
    per-pixel variance over the seeds, summed over those pixels, of the weighted choice is strictly below the uniform choice's.  (The
    figures of DESIGN.md section 23: 177 of 192 pixels; lit 20 504.9, cone 19 964.0, weighted 5 294.1.)"""
    weighted, cone, lit, mask = many_light_statement_frames()
    assert 100 < int(mask.sum()) < wt.MANY_W * wt.MANY_H
    everywhere = np.ones_like(mask)
    for name, other in (("lit", lit), ("cone", cone)):
        for where, m in (("indirect pixels", mask), ("whole frame", everywhere)):
            mean, stderr, var_w, var_o, all_w, all_o = wt.many_numbers(weighted, other, m)
            print(f"weighted - {name}, {where} ({int(m.sum())}): mean {mean:.4f}, standard error {stderr:.4f}, |mean| / stderr {abs(mean) / stderr:.3f}; "
                  f"variance weighted {var_w:.1f}, {name} {var_o:.1f}")
            assert stderr > 0.0 and abs(mean) <= 5.0 * stderr, (name, where)
    _, _, var_w, var_cone, _, _ = wt.many_numbers(weighted, cone, mask)
    assert 0.0 < var_w < var_cone
