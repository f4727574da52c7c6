"""The variance-guided denoiser without a GPU (rt_denoise_var_host): the library's CPU statement against the numpy
statement of the contract (tests/denoise_var_ref.py), bit for bit; two known answers; the context-free validation of the entry points in
the documented order; the declarations in the header, ctypes and the Rust binding; the command line's refusals;
rt_denoise_var_core.hpp alone under ASan + UBSan in a stand-alone program; and the compiler's resource remarks for the new kernels."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as vr
import rtiow_amd as rt
from isa_pins import fingerprint_lines
from rtiow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtiow_amd", "csrc")
SIZES = [(1, 1), (5, 3), (37, 19), (70, 45)]
WIDE_COLOR = 64.0
NAMES = ("rt_denoise_var_workspace_bytes", "rt_denoise_var_device", "rt_denoise_var", "rt_denoise_var_host")


def differing(got, want):
    return f"{int((got != want).any(axis=-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


@pytest.fixture(scope="module")
def cases():
    """The synthetic frames, built once and left unchanged."""
    out = {}
    for w, h in SIZES + [(150, 9)]:
        case = vr.synthetic_case(w, h)
        for a in (case[0], case[1], case[2], case[4]):
            a.setflags(write=False)
        out[(w, h)] = case
    return out


def run_both(case, levels, demodulate, with_count, sigmas=(vr.SIGMA_COLOR, 1.0, 0.2)):
    fix, half, count, spp, feat, feat_spp = case
    cnt = count if with_count else None
    got = rt.denoise_var_host(fix, half, spp, feat, feat_spp, rt.make_denoise_var(levels, *sigmas, demodulate), count=cnt)
    want = vr.denoise_var(fix, half, spp, feat, feat_spp, levels=levels, sigma_color=sigmas[0], sigma_normal=sigmas[1], sigma_depth=sigmas[2],
                          demodulate=demodulate, count=cnt)
    return got, want


def test_the_declarations():
    """The four functions: in the header, in ctypes (and the library resolves them), in the Rust binding; the struct is rt_denoise's."""
    lib = _ffi.load()
    hdr = open(os.path.join(ROOT, "include", "rtiow_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert "#define RTIOW_HIP_ABI_VERSION 5" in hdr and C.sizeof(_ffi.rt_denoise) == 32
    args = {n: a for n, _, a in _ffi.SYMBOLS}
    assert len(args["rt_denoise_var_device"]) == 13 and len(args["rt_denoise_var"]) == 12 and len(args["rt_denoise_var_host"]) == 10
    d = rt.make_denoise_var()
    assert (d.levels, d.flags, d.sigma_color, d.sigma_normal, d.sigma_depth) == (4, _ffi.RT_DENOISE_DEMODULATE, vr.SIGMA_COLOR, 1.0, 0.2)
    assert rt.make_denoise_var(demodulate=False).flags == 0 and rt.Renderer.denoise_var_host is rt.denoise_var_host
    # the workspace: 19 doubles per pixel, from the one call that says so
    assert rt.Renderer.denoise_var_workspace_bytes(37, 19) == 37 * 19 * 19 * 8
    n = C.c_int64(-7)
    for w, h in ((0, 4), (4, 0), (65536, 32769)):
        assert lib.rt_denoise_var_workspace_bytes(w, h, C.byref(n)) == -1 and n.value == -7
    assert lib.rt_denoise_var_workspace_bytes(4, 4, None) == -1
    assert lib.rt_denoise_var_workspace_bytes(65536, 32768, C.byref(n)) == 0 and n.value == (1 << 31) * 19 * 8


def test_the_synthetic_frames_exercise_the_contract(cases):
    fix, half, count, spp, feat, feat_spp = cases[(37, 19)]
    d = (half * np.uint64(2) - fix).view(np.int64)
    assert (d == 0).all(axis=-1).any() and (half == 0).all(axis=-1).any() and (half == fix).all(axis=-1).any()      # zero variance, half = 0, half = fix
    assert (half > fix).all(axis=-1).any() and (d < 0).any() and (half >= np.uint64(1 << 63)).any()                 # half > fix; the wrapping cases
    assert int(fix.max()) > 1 << 53 and int(np.abs(d).max()) > 1 << 53 and (count % 2 == 0).all() and len(np.unique(count)) > 10 and spp % 2 == 0
    # the colour stop is neither idle nor shut: the filter moves the frame, and its width matters at both ends
    c, m, n, z = dr.prepare(fix, None, spp, feat, feat_spp, True)
    base = vr.denoise_var(fix, half, spp, feat, feat_spp)
    assert (base != dr.quantize(c * m)).any()
    assert (vr.denoise_var(fix, half, spp, feat, feat_spp, sigma_color=0.25) != base).any()
    assert (vr.denoise_var(fix, half, spp, feat, feat_spp, sigma_color=1e6) != base).any()
    assert (vr.denoise_var(fix, half, spp, feat, feat_spp, count=count) != base).any()
    # the half buffer matters, and so does the propagated variance: with the input variance at every level the frame is another
    assert (vr.denoise_var(fix, fix >> np.uint64(1), spp, feat, feat_spp) != base).any()
    with np.errstate(all="ignore"):
        var0 = vr.prepare_var(fix, half, None, spp, m)
        cc, var = c, var0
        for l in range(4):
            cc, var = vr.level(cc, var0, n, z, l, vr.SIGMA_COLOR, 1.0, 0.2)
    assert (dr.quantize(cc * m) != base).any()


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_numpy_on_synthetic_frames(cases, size, levels):
    """From 70 x 45 down, 4 s exceeds the frame on both sides; demodulate on and off; spp and a count buffer."""
    for demodulate in (True, False):
        for with_count in (False, True):
            got, want = run_both(cases[size], levels, demodulate, with_count)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (demodulate, with_count, differing(got, want))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_numpy_with_other_sigmas(cases, size):
    for levels, sc, sn, sd in ((4, 0.25, 1.0, 0.2), (3, 1e6, 0.1, 5.0), (2, 1e-3, 1e-3, 1e-3), (5, 1.5, 2.0, 1e6)):
        got, want = run_both(cases[size], levels, True, True, (sc, sn, sd))
        assert np.array_equal(got, want), (levels, sc, sn, sd, differing(got, want))


@pytest.mark.parametrize("levels", [6, 7, 8])
def test_host_equals_numpy_at_levels_six_to_eight_on_a_wide_frame(cases, levels):
    """150 x 9, hole steps 32, 64 and 128: the taps at +-128 of the columns 0..21 and 128..149 are inside the frame.  The variance shrinks
    from level to level and the colour stop with it: at the default width the eighth level returns its input on this frame, so the same
    is asked at 64 standard deviations, where each of these levels moves pixels -- asserted."""
    fix, half, count, spp, feat, feat_spp = cases[(150, 9)]
    for sigma_color in (vr.SIGMA_COLOR, WIDE_COLOR):
        for demodulate in (True, False):
            for with_count in (False, True):
                got, want = run_both(cases[(150, 9)], levels, demodulate, with_count, (sigma_color, 1.0, 0.2))
                assert np.array_equal(got, want), (sigma_color, demodulate, with_count, differing(got, want))
    wide = lambda n: vr.denoise_var(fix, half, spp, feat, feat_spp, levels=n, sigma_color=WIDE_COLOR)
    assert (wide(levels) != wide(levels - 1)).any()


def test_known_answer_zero_variance_returns_the_prepared_mean():
    """half = fix / 2 everywhere: var = 0, so icv = 1e12 and every tap whose box mean differs from the centre's by more than 2^-10 has
    xc > 2^-20 * 1e12 > 1 and weight 0; the centre tap alone remains, w = 9/64, and (9/64 c) / (9/64) = c exactly for a c of few bits.
    Without demodulation the filter returns quantize(v(fix) / count)."""
    w, h = 13, 11
    jj, ii = np.mgrid[0:h, 0:w]
    count = np.where((ii + jj) % 3 == 0, 4, 2).astype(np.uint32)
    units = (1 + ii + 40 * jj).astype(np.uint64)                                 # c = units / 64 in the red channel: at most 9 bits
    fix = np.zeros((h, w, 3), dtype=np.uint64)
    fix[..., 0] = units * np.uint64(1 << 26) * count.astype(np.uint64)
    half = fix >> np.uint64(1)
    assert np.array_equal(half * np.uint64(2), fix)
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    want = dr.quantize(dr.mean_of(fix, count=count))
    assert np.array_equal(want[..., 0], units << np.uint64(26))
    # the premise: at every tap distance of the levels used, the 3x3 box means of two different in-frame pixels differ by more than 2^-10
    g = dr.box_mean(dr.mean_of(fix, count=count))[..., 0]
    for l in range(3):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy << l if dy >= 0 else -((-dy) << l), dx << l if dx >= 0 else -((-dx) << l)
                if (dx, dy) == (0, 0) or abs(oy) >= h or abs(ox) >= w:
                    continue
                (dj, sj), (di, si) = dr._shift(h, oy), dr._shift(w, ox)
                assert (np.abs(g[dj, di] - g[sj, si]) > 2.0 ** -10).all(), (l, dx, dy)
    for levels in (1, 2, 3):
        dn = rt.make_denoise_var(levels, demodulate=False)
        assert np.array_equal(rt.denoise_var_host(fix, half, 0, feat, 1, dn, count=count), want), levels
        assert np.array_equal(vr.denoise_var(fix, half, 0, feat, 1, levels=levels, demodulate=False, count=count), want), levels
    # (the same frame with a variance is filtered: the answer above is the variance's doing)
    assert not np.array_equal(rt.denoise_var_host(fix, fix, 0, feat, 1, rt.make_denoise_var(3, demodulate=False), count=count), want)


@pytest.mark.parametrize("size", [(9, 11), (150, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_known_answer_a_constant_frame_is_a_fixed_point(size):
    """Colour, guides and variance constant: every difference is 0, so every stop is 1 - 0 = 1 and w = k exactly; with a colour that is a
    power of two every product k c is exact, the sums of the dyadic k are exact, and acc / ws = c.  The variance changes from level to
    level (and differs at the borders, where fewer taps lie in the frame), which the colour never sees: d = 0 times any icv is 0."""
    w, h = size
    q1 = dr.Q1
    fix = np.full((h, w, 3), 2 * q1, dtype=np.uint64)                            # c = 2 / 2 = 1
    half = fix.copy()                                                            # d = fix: e = 1 per channel without demodulation, var = 3
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    feat[..., 0:3] = q1 // 2                                                     # albedo 1/2, alpha 1: m = 1/2, c0 = 2
    feat[..., 3] = q1
    feat[..., 6] = 5 * q1
    feat[..., 7] = 1
    want = np.full((h, w, 3), q1, dtype=np.uint64)
    for levels in range(1, 9):
        for demodulate in (True, False):
            for sigma_color in (vr.SIGMA_COLOR, 1e-3):
                dn = rt.make_denoise_var(levels, sigma_color, demodulate=demodulate)
                assert np.array_equal(rt.denoise_var_host(fix, half, 2, feat, 1, dn), want), (levels, demodulate, sigma_color)
    assert np.array_equal(vr.denoise_var(fix, half, 2, feat, 1, levels=8), want)


BAD = [
    (dict(dn=None), "dn is NULL"), (dict(fix=None), "NULL (fix)"), (dict(half=None), "NULL (half)"), (dict(feat=None), "NULL (feat or out)"),
    (dict(out=None), "NULL (feat or out)"), (dict(levels=0), "levels must be 1..8"), (dict(levels=9), "levels must be 1..8"), (dict(flags=2), "unknown flags"),
    (dict(flags=0x80000001), "unknown flags"), (dict(sigma_color=0.0), "sigma"), (dict(sigma_normal=-1.0), "sigma"), (dict(sigma_depth=math.inf), "sigma"),
    (dict(sigma_color=math.nan), "sigma"), (dict(width=0), "bad width/height"), (dict(height=-3), "bad width/height"),
    (dict(width=65536, height=32769), "<= 2^31"), (dict(spp=0), "spp >= 1 without a count"), (dict(feat_spp=0), "feat_spp >= 1"),
]
# two faults at once: the one the documented order names first is reported
ORDER = [
    (dict(dn=None, fix=None), "dn is NULL"), (dict(fix=None, half=None), "NULL (fix)"), (dict(half=None, feat=None), "NULL (half)"),
    (dict(out=None, levels=0), "NULL (feat or out)"), (dict(levels=0, flags=2), "levels must be"), (dict(flags=2, sigma_color=0.0), "unknown flags"),
    (dict(sigma_depth=0.0, width=0), "sigma"), (dict(width=0, spp=0), "bad width/height"), (dict(width=65536, height=32769, spp=0), "<= 2^31"),
    (dict(spp=0, feat_spp=0), "spp >= 1 without a count"),
]


def call_form(lib, form, kw, out):
    w, h = 4, 3
    fix = np.full((h, w, 3), 1 << 32, dtype=np.uint64)
    half = np.full((h, w, 3), 1 << 31, dtype=np.uint64)
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    work = np.zeros(h * w * 19, dtype=np.float64)
    dn = rt.make_denoise_var()
    for k in ("levels", "flags", "sigma_color", "sigma_normal", "sigma_depth"):
        if k in kw:
            setattr(dn, k, kw[k])
    ptr = lambda name, a: None if name in kw and kw[name] is None else a.ctypes.data_as(C.c_void_p)
    dnp = None if "dn" in kw else C.byref(dn)
    common = (kw.get("spp", 8), ptr("feat", feat), kw.get("feat_spp", 8), kw.get("width", w), kw.get("height", h), dnp)
    if form == "host":
        return lib.rt_denoise_var_host(ptr("fix", fix), ptr("half", half), None, *common, ptr("out", out))
    if form == "buffers":
        return lib.rt_denoise_var(None, ptr("fix", fix), ptr("half", half), None, *common, ptr("out", out), None)
    return lib.rt_denoise_var_device(None, ptr("fix", fix), ptr("half", half), None, *common, ptr("work", work), ptr("out", out), None)


@pytest.mark.parametrize("form", ["host", "device", "buffers"])
@pytest.mark.parametrize("kw,msg", BAD + ORDER, ids=[",".join(f"{a}={b}" for a, b in k.items()) for k, _ in BAD + ORDER])
def test_rejections_touch_nothing_and_come_in_the_documented_order(kw, msg, form):
    """Every rejection, from every form, without a context: RT_ERR_INVALID_ARGUMENT, the reason, and out_fix untouched."""
    lib = _ffi.load()
    out = np.full((3, 4, 3), 0xABCD, dtype=np.uint64)
    rc = call_form(lib, form, kw, out)
    assert rc == -1 and msg in lib.rt_last_error().decode() and "denoise_var" in lib.rt_last_error().decode(), lib.rt_last_error().decode()
    assert (out == 0xABCD).all()


def test_the_forms_with_a_context_name_what_is_missing():
    lib = _ffi.load()
    out = np.full((3, 4, 3), 0xABCD, dtype=np.uint64)
    err = lambda: lib.rt_last_error().decode()
    assert call_form(lib, "device", dict(feat_spp=0, work=None), out) == -1 and "feat_spp" in err()
    assert call_form(lib, "device", dict(work=None), out) == -1 and "workspace is NULL" in err()         # ... before the missing context
    assert call_form(lib, "device", {}, out) == -1 and "ctx is NULL" in err()
    assert call_form(lib, "buffers", {}, out) == -1 and "ctx is NULL" in err()
    assert (out == 0xABCD).all()
    assert call_form(lib, "host", {}, out) == 0 and (out != 0xABCD).all()
    # a count buffer stands in for spp; odd counts are not rejected
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    cnt = np.array([3], dtype=np.uint32)
    one = np.zeros(3, dtype=np.uint64)
    dn = rt.make_denoise_var()
    assert lib.rt_denoise_var_host(p, p, cnt.ctypes.data_as(C.c_void_p), 0, p, 1, 1, 1, C.byref(dn), one.ctypes.data_as(C.c_void_p)) == 0


def test_the_cli_refuses_what_it_must(tmp_path, book1_flat):
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert "rt_denoise_var(" in src and "--denoise-variance" in src.split("#include")[0]                 # ... and the usage comment names it
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    base = [exe, "--scene", scene_file, "--width", "8", "--height", "8", "--out", str(tmp_path / "o.ppm")]
    for args, word in ((["--spp", "8", "--denoise-variance", "--denoise"], "give one of them"),
                       (["--spp", "7", "--denoise-variance"], "--spp must be even"),
                       (["--spp", "7", "--wavefront", "--denoise-variance"], "--spp must be even"),
                       (["--spp", "8", "--wavefront", "--denoise"], "goes with none of"),
                       (["--spp", "8", "--wavefront", "--denoise", "--denoise-variance"], "give one of them"),
                       (["--spp", "8", "--denoise-variance", "--uniform53"], "goes with none of"),
                       (["--spp", "8", "--denoise-variance", "--orbit", "2"], "goes with none of")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.returncode, bad.stderr)
    # accepted by the argument checks: what fails now is the device (here there may be none) or nothing at all, never a refusal's exit code
    for args in (["--spp", "8", "--wavefront", "--sky", "0,0,0:0,0,0", "--emit", "0:4,3.2,2.4", "--direct-weighted", "--denoise-variance"],
                 ["--spp", "16", "--adaptive", "0.05", "--step", "4", "--denoise-variance"]):
        ok = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert ok.returncode in (0, 1) and "goes with none of" not in ok.stderr and "give one" not in ok.stderr, (args, ok.returncode, ok.stderr)


def test_core_header_alone_under_asan_and_ubsan(cases, tmp_path):
    """tests/denoise_var_san_main.cpp includes rt_denoise_var_core.hpp and nothing else of the library; the sanitizers watch it filter the
    1 x 1, 5 x 3 and 37 x 19 frames (buffers of exactly the size the filter may touch), and its checksum is numpy's."""
    assert shutil.which("g++")
    src = open(os.path.join(CSRC, "rt_denoise_var_core.hpp")).read()
    assert "#include <hip" not in src and re.findall(r"#include (\S+)", src) == ['"rt_denoise_core.hpp"']
    for name in ("double value(", "uint64_t quantize(", "void prepare(", "void box_mean(", "double edge_stop(", "void finish(", "LevelConst level_const("):
        assert name not in src, name                                                 # reused, not restated
    exe = str(tmp_path / "denoise_var_san_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "denoise_var_san_main.cpp")], check=True, timeout=300)
    for (w, h), levels, demodulate, with_count in (((1, 1), 3, True, False), ((5, 3), 5, True, True), ((37, 19), 5, False, True), ((37, 19), 4, True, False)):
        fix, half, count, spp, feat, feat_spp = cases[(w, h)]
        path = str(tmp_path / f"case_{w}x{h}_{levels}.bin")
        with open(path, "wb") as f:
            f.write(np.array([w, h, spp, feat_spp, levels, int(demodulate), int(with_count)], dtype="<i8").tobytes())
            f.write(np.array([vr.SIGMA_COLOR, 1.0, 0.2], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(fix, dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(half, dtype="<u8").tobytes())
            if with_count:
                f.write(np.ascontiguousarray(count, dtype="<u4").tobytes())
            f.write(np.ascontiguousarray(feat, dtype="<u8").tobytes())
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and not run.stderr, run.stderr
        want = vr.denoise_var(fix, half, spp, feat, feat_spp, levels=levels, demodulate=demodulate, count=count if with_count else None)
        assert int(run.stdout.strip(), 16) == dr.checksum(want), (w, h, levels)


def test_the_kernels_use_no_scratch_memory_and_spill_no_vector_register():
    """The compiler's own resource remarks for denoise/rt_denoise_var.hip with the product's flags.  Registers and occupancy are reported
    (DESIGN.md section 25), not promised; the tile form's LDS is the eleven planes of 400 doubles the header of the file states."""
    import tempfile
    unit = os.path.join(CSRC, "denoise", "rt_denoise_var.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                              "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-c", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "denoise_var.o"), unit],
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
    kinds = ("denoise_var_prepare_kernel", "denoise_var_stats_kernel", "denoise_var_level_gather_kernel", "denoise_var_level_tile_kernel",
             "denoise_var_finish_kernel")
    assert len(rows) == len(kinds), sorted(rows)
    for kind in kinds:
        found = [r for name, r in rows.items() if f"{kind}E" in name]
        assert len(found) == 1, kind
        r = found[0]
        print(kind, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "occupancy", r["Occupancy [waves/SIMD]"], "SGPR spills", r["SGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, (kind, r)
        assert int(r["LDS Size [bytes/block]"]) == (11 * 400 * 8 if kind == "denoise_var_level_tile_kernel" else 0), (kind, r)


def test_the_old_denoiser_is_untouched_by_the_new_unit():
    """Both units state what they share once, in rt_denoise_shared.hpp; the new one includes neither rt_denoise.hip nor a render kernel's
    header."""
    def deps_of(unit):
        run = subprocess.run(["hipcc", "-MM", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                              os.path.join(CSRC, unit)], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        return {os.path.basename(d) for d in run.stdout.replace("\\\n", " ").split() if not d.endswith(":")}
    deps = deps_of(os.path.join("denoise", "rt_denoise_var.hip"))
    assert {"rt_host.hpp", "rt_denoise_core.hpp", "rt_denoise_var_core.hpp", "rt_denoise_shared.hpp", "rt_denoise_tile.inc"} <= deps, deps
    assert not {"rt_kernels.hpp", "rt_launch.hpp", "rt_device.hpp", "rt_denoise.hip"} & deps, sorted(deps)
    assert {"rt_denoise_shared.hpp", "rt_denoise_tile.inc"} <= deps_of("rt_denoise.hip")
    import __graft_entry__ as g
    import inspect
    assert inspect.getsource(g.build_hip_library).count(".hip\"") >= 12 and "denoise/rt_denoise_var.hip" in inspect.getsource(g.build_hip_library)


def test_the_kernels_have_the_machine_code_they_had_before_the_shared_header():
    """tools/isa_fingerprint.py --denoise-var = profiles/isa_fingerprint_denoise_var.txt, printed by the same flag on the commit before
    the two denoisers shared a header: the five kernels, by name, instruction counts and opcode hash."""
    pinned = fingerprint_lines(open(os.path.join(ROOT, "profiles", "isa_fingerprint_denoise_var.txt")).read())
    assert len(pinned) == 5, sorted(pinned)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--denoise-var"], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    now = fingerprint_lines(run.stdout)
    assert sorted(now) == sorted(pinned)
    for name in pinned:
        assert now[name] == pinned[name], (name, now[name], pinned[name])
