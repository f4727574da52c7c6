"""The environment cube map of the lit path queue without a GPU (include/rtiow_hip.h "environment"):
rt_environment_cdf against the statement of tests/env_ref.py bit for bit and alone under ASan + UBSan, the lookup rule, the estimator
against a quadrature of the integral it estimates, the two frames with answers that need no device, that the hand-built queue the GPU
tests use is hard, the context-free validation of the four entry points and its order, the rt_environment layout in ctypes and Rust
against the header, the Python class, the CLI's switches, and what the compiler says of the new kernel."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import env_ref as er
import lights_ref as lr
import paths_ref as pr
import rtiow_amd as rt
from rtiow_amd import _ffi
from test_lights_host import FIX, RAYS, TABLE, Queue, lighting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_environment_cdf", "rt_paths_step_env_device", "rt_render_wavefront_env_device", "rt_render_wavefront_env")
NAN, INF = float("nan"), float("inf")
SHADOW = np.full(8, 0x5A, dtype=np.uint8)
TEXELS = np.full((6, 2, 2, 3), 0.5)
CDF = np.arange(1.0, 25.0)
DEFAULT = object()
SIZES = (1, 2, 8)


def _err(lib):
    return lib.rt_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def _cdf(texels, size):
    lib = _ffi.load()
    t = np.ascontiguousarray(texels, dtype=np.float64)
    out = np.full(6 * size * size + 1, -7.0)
    assert lib.rt_environment_cdf(t.ctypes.data, size, out.ctypes.data) == 0, _err(lib)
    assert out[-1] == -7.0                                                       # nothing past the table is written
    return out[:-1]


def hard_texels(size):
    """Seeded texels with NaN, negative, -0, zero, tiny and huge entries among them."""
    rng = np.random.default_rng(100 + size)
    t = rng.uniform(0.0, 4.0, (6, size, size, 3))
    flat = t.reshape(-1, 3)
    for k, row in enumerate(((NAN, 0.5, -1.0), (-2.0, -0.0, NAN), (0.0, 0.0, 0.0), (1e-300, 0.0, 0.0), (NAN, NAN, NAN), (3.0, 3.0, 3.0))):
        flat[(k * 5) % len(flat)] = row
    return t


@pytest.mark.parametrize("size", SIZES)
def test_the_table_equals_the_statement_bit_for_bit(size):
    for texels in (er.hand_env(size)[0], hard_texels(size), np.zeros((6, size, size, 3)), np.full((6, size, size, 3), 1.0)):
        want = er.environment_cdf(texels, size)
        assert np.array_equal(bits(_cdf(texels, size)), bits(want))
        assert np.array_equal(bits(rt.Environment(np.array(texels)).cdf()), bits(want))
    ones = _cdf(np.full((6, size, size, 3), 1.0), size)
    # the weights are solid angles up to s^2: they sum to 4 pi / s^2 as the map gets finer (size 1: the centre's, 6 exactly)
    assert ones[-1] == 6.0 if size == 1 else abs(ones[-1] * (2.0 / size) ** 2 - 4.0 * math.pi) < 0.5
    assert (np.diff(ones) > 0.0).all()


def test_table_rejections():
    lib = _ffi.load()
    out = np.full(24, -7.0)
    assert lib.rt_environment_cdf(None, 2, out.ctypes.data) == -1 and "texels is NULL" in _err(lib)
    assert lib.rt_environment_cdf(TEXELS.ctypes.data, 2, None) == -1 and "cdf_out is NULL" in _err(lib)
    for size in (0, -1, 3, 6, 1025, 2048, -(1 << 31)):
        assert lib.rt_environment_cdf(TEXELS.ctypes.data, size, out.ctypes.data) == -1 and "power of two" in _err(lib), size
    assert (out == -7.0).all()


def test_core_header_alone_under_asan_and_ubsan(tmp_path):
    """tests/env_cdf_san_main.cpp includes rt_env_core.hpp and nothing else of the library; the sanitizers watch it build tables in
    buffers of exactly their size, and what it prints is the statement's table bit for bit."""
    assert shutil.which("g++")
    src = open(os.path.join(ROOT, "rtiow_amd", "csrc", "rt_env_core.hpp")).read()
    assert "#include <hip" not in src and '#include "' not in src and "getenv" not in src
    main = open(os.path.join(ROOT, "tests", "env_cdf_san_main.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', main) == ["rt_env_core.hpp"]
    exe = str(tmp_path / "env_cdf_san_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "env_cdf_san_main.cpp")], check=True, timeout=300)
    for size in SIZES:
        texels = hard_texels(size)
        path = str(tmp_path / f"case_{size}.bin")
        with open(path, "wb") as f:
            f.write(np.array([size], dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(texels, dtype="<f8").tobytes())
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and not run.stderr, run.stderr
        got = np.array([int(x, 16) for x in run.stdout.split()], dtype=np.uint64)
        assert np.array_equal(got, bits(er.environment_cdf(texels, size)))


# ---- the lookup --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
def test_every_sampled_direction_looks_up_its_own_texel(size):
    """For power-of-two sizes every step of a and b' is exact: env_lookup(dv) == k for every texel at both ends of the offset words --
    with ONE exception the contract's own rules make, and which is pinned here exactly: offset word 0 in row 0 gives the coordinate
    -1.0 exactly, the cube's edge, where |coordinate| ties with the face's own +-1.0; the lookup's strict comparisons give a tie to the
    LOWER axis, so on a y or z face such a direction looks up the texel of the -x (or -y) face across that edge.  (One word in 2^32 per
    coordinate; the sample still takes texels[k], so the estimator does not see it.)"""
    n = 6 * size * size
    texels = np.ones((6, size, size, 3))
    # a table with which word x chooses texel k exactly: equal weights
    cdf = np.arange(1.0, n + 1.0)
    edges = 0
    for k in range(n):
        x = (k * (1 << 32)) // n + 1
        f, i, j = er.texel_of(k, size)
        for word in (0, 0xFFFFFFFF):
            s = er.sample_words(texels, cdf, size, (x, word, word), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
            assert s["k"] == k and s["P"] > 0.0 and s["dv"][f >> 1] == (-1.0 if f & 1 else 1.0), (k, word)
            got = er.env_lookup(s["dv"], size)
            # the coordinates on axes below the face's own that sit on the edge -1.0
            lower = [c for c, row in zip([a for a in range(3) if a != f >> 1], (i, j)) if c < f >> 1 and row == 0 and word == 0]
            if not lower:
                assert got == k, (k, word)
            else:
                edges += 1
                assert s["dv"][lower[0]] == -1.0 and got != k and er.texel_of(got, size)[0] == 2 * lower[0] + 1, (k, word)
    assert edges == 2 * size + 2 * (2 * size - 1)     # the two y faces: row i = 0; the two z faces: row i = 0 or column j = 0


def test_the_lookup_of_degenerate_directions():
    """Equal components: x wins over y, y over z; +-0 components; the zero, infinite and NaN directions: the texel the rule names."""
    k = lambda f, i, j, size=8: (f * size + i) * size + j
    L = lambda *d: er.env_lookup(d, 8)
    assert L(1.0, 1.0, 1.0) == k(0, 7, 7) and L(-1.0, -1.0, -1.0) == k(1, 0, 0) and L(1.0, -1.0, 1.0) == k(0, 0, 7)
    assert L(0.0, 2.0, 2.0) == k(2, 4, 7) and L(0.0, -3.0, 3.0) == k(3, 4, 7) and L(2.0, 0.0, -2.0) == k(0, 4, 0)
    assert L(0.0, 0.0, 1.0) == k(4, 4, 4) and L(-0.0, -0.0, 1.0) == k(4, 4, 4) and L(0.0, 0.0, -1.0) == k(5, 4, 4)
    assert L(-0.0, 1.0, 0.0) == k(2, 4, 4) and L(-1.0, 0.0, -0.0) == k(1, 4, 4)
    # the zero direction: axis x, not negative (-0.0 < 0.0 is false), 0 / 0 = NaN gives row 0
    assert L(0.0, 0.0, 0.0) == k(0, 0, 0) == L(-0.0, -0.0, -0.0)
    # infinite: the face of the first infinite component; finite / inf = 0 is the middle, inf / inf = NaN row 0
    assert L(INF, 1.0, 1.0) == k(0, 4, 4) and L(-INF, INF, 0.0) == k(1, 0, 4) and L(1.0, INF, -INF) == k(2, 4, 0) and L(INF, INF, INF) == k(0, 0, 0)
    # a NaN never wins an axis; in the first place it stays (no comparison replaces it) and makes both coordinates NaN
    assert L(1.0, NAN, 0.5) == k(0, 0, 6) and L(0.5, 1.0, NAN) == k(2, 6, 0) and L(NAN, 1.0, 0.5) == k(0, 0, 0) and L(NAN, NAN, NAN) == k(0, 0, 0)
    assert L(0.0, NAN, 0.0) == k(0, 0, 0)
    # beyond the range of a finite quotient: the clamp to the last row
    assert L(1e300, 1e300, 1e-300) == k(0, 7, 4) and L(-2.0, 1.0, -2.0) == k(1, 6, 0)
    for size in SIZES:
        rng = np.random.default_rng(size)
        for d in list(rng.normal(size=(200, 3))) + [d for d in er.degenerate_queue()[1]]:
            assert 0 <= er.env_lookup(d, size) < 6 * size * size


# ---- the estimator -------------------------------------------------------------------------------------------------------------------------

def estimator_case():
    rng = np.random.default_rng(8)
    texels = rng.uniform(0.0, 1.0, (6, 8, 8, 3))
    texels[2, 5, 2] = 400.0
    return texels, er.environment_cdf(texels, 8)


def test_the_vector_form_of_the_sample_is_the_statement():
    texels, cdf = estimator_case()
    words = np.random.default_rng(9).integers(0, 1 << 32, (1500, 3), dtype=np.uint64)
    n = (0.6, 0.0, 0.8)
    k, c = er.sample_many(texels, cdf, 8, words, n)
    for m in range(len(words)):
        s = er.sample_words(texels, cdf, 8, words[m], n, (1.0, 1.0, 1.0))
        assert s["k"] == k[m] and np.array_equal(bits(c[m]), bits(s["c"] if s["shadow"] else [0.0, 0.0, 0.0])), m


@pytest.mark.parametrize("normal", [(0.0, 1.0, 0.0), (0.6, 0.0, 0.8), (-2.0 / 3.0, -1.0 / 3.0, 2.0 / 3.0)], ids=["up", "side", "down"])
def test_the_estimator_against_a_quadrature(normal):
    """Size 8, one texel of 400 among random ones, an unoccluded point: the mean of 10^5 samples from fixed words against a 16 x 16 per
    texel quadrature of the integral of L cos(theta) / pi, within 4 standard errors taken from the samples themselves."""
    texels, cdf = estimator_case()
    words = np.random.default_rng(10).integers(0, 1 << 32, (100000, 3), dtype=np.uint64)
    _, c = er.sample_many(texels, cdf, 8, words, normal)
    mean, stderr = c.mean(axis=0), c.std(axis=0, ddof=1) / math.sqrt(len(c))
    want = er.quadrature(texels, 8, normal)
    print(f"normal {normal}: mean {mean}, quadrature {want}, standard error {stderr}")
    assert (stderr > 0.0).all() and (np.abs(mean - want) <= 4.0 * stderr).all()


# ---- frames with answers that need no device ------------------------------------------------------------------------------------------------

def test_a_black_environment_gives_the_black_sky_lit_frame(oracle_mod):
    """The golden book frame (32 x 18, 4 spp) with lights_ref.book_case()'s lights: under a black environment, not sampled, render_env is
    the lit statement under a black sky, bit for bit."""
    flat, light, _ = lr.book_case()
    black = lr.Light((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), light.emission)
    cam = oracle_mod.book1_camera(lr.BW, lr.BH)
    want, want_rays = lr.render_lit(flat, cam, lr.BW, lr.BH, lr.BSPP, black, max_depth=50, seed=1, batch=257)
    got, rays, shadow = er.render_env(flat, cam, lr.BW, lr.BH, lr.BSPP, light, (np.zeros((6, 2, 2, 3)), None), 2, max_depth=50, seed=1, batch=257)
    assert np.array_equal(got, want) and want.any() and rays == want_rays and shadow == 0


def test_a_constant_environment_seen_by_rays_that_all_miss(oracle_mod):
    """One sphere behind the camera: every camera ray misses and adds quantize(c), c a power of two."""
    flat = np.zeros(1, dtype=rt.SPHERE_DTYPE)
    flat[0]["center"], flat[0]["radius"], flat[0]["albedo"] = (13.0, 2.0, 30.0), 0.5, (0.5, 0.5, 0.5)
    w, h, spp, c = 8, 6, 3, 0.25
    texels = np.full((6, 4, 4, 3), c)
    for env in ((texels, None), (texels, er.environment_cdf(texels, 4))):
        got, rays, shadow = er.render_env(flat, oracle_mod.book1_camera(w, h), w, h, spp, lr.REFERENCE, env, 4, max_depth=5, seed=3)
        assert (got == spp * (1 << 30)).all() and rays == w * h * spp and shadow == 0


# ---- the hand queue is hard -----------------------------------------------------------------------------------------------------------------

def _one(k, env=None, size=8, **kw):
    """The statement on path k of the hand queue alone -> (fate, its additions at its pixel as ints, the out event or None, the sample)."""
    flat, q, light = er.hand_queue()
    sub = {f: q[f][[k]] for f in pr.FIELDS}
    new, fates, adds, got = er.bounce_env(flat, sub, er.SEED, er.HAND_NPIX, light, env if env is not None else er.hand_env(size), size, **kw)
    pixel = int(q["pixel"][k])
    assert int(adds.any(axis=1).sum()) <= 1
    event = int(new["event"][0]) if fates[0] in lr.SURVIVES else None
    return fates[0], [int(x) for x in adds[pixel]] if pixel < er.HAND_NPIX else None, event, got[0]


def test_the_hand_queue_is_hard(oracle_mod):
    """Conditions on the step input of tests/test_gpu_env.py, checked with the statement alone.  Every case asked of a single path sits
    below slot 63, the smallest count at which the GPU tests run a bounce of many."""
    from trace_ref import Scene, fast_hit
    flat, q, light = er.hand_queue()
    scene = Scene(flat)
    texels, cdf = er.hand_env(8)
    flat_texels = texels.reshape(-1, 3)
    quant = lambda x: int(oracle_mod.load().oracle_b_quantize(float(x)))
    index = lambda t: (t[0] * 8 + t[1]) * 8 + t[2]
    assert len(q["pixel"]) == 513 and len(flat) == 15 and max(er.CASES) < 63 and max(er.DIRECT_SLOTS) < 63 and er.PLAIN_MISS < 63
    new, fates, adds, got = er.bounce_env(scene, q, er.SEED, er.HAND_NPIX, light, (texels, cdf), 8)
    plain_new, plain_fates, plain_adds, plain_got = er.bounce_env(scene, q, er.SEED, er.HAND_NPIX, light, (texels, None), 8)
    hit = [fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), 1e-4) for k in range(513)]
    # a miss without the bit adds throughput * texel; with it, nothing
    fate, add, _, _ = _one(er.PLAIN_MISS)
    e = flat_texels[er.env_lookup(q["dir"][er.PLAIN_MISS].tolist(), 8)]
    assert fate == "miss" and not q["event"][er.PLAIN_MISS] & er.DIRECT and add == [quant(q["throughput"][er.PLAIN_MISS][c] * e[c]) for c in range(3)] and all(add)
    assert q["event"][18] & er.DIRECT and _one(18)[:2] == ("miss", [0, 0, 0])
    plain = {f: q[f][[18]].copy() for f in pr.FIELDS}
    plain["event"] &= np.uint32(0x7FFFFFFF)
    assert er.bounce_env(scene, plain, er.SEED, er.HAND_NPIX, light, (texels, cdf), 8)[2].any()
    # a sample below the horizon: no shadow ray, the bit still set
    fate, add, event, s = _one(25)
    assert fate == "lambertian" and s["ns"] <= 0.0 and not s["shadow"] and add == [0, 0, 0] and event & er.DIRECT
    # an occluded shadow ray (the sphere above) and a visible one
    fate, add, event, s = _one(19)
    assert s["shadow"] and not s["visible"] and add == [0, 0, 0] and event & er.DIRECT
    assert fast_hit(scene, list(hit[19][2]), s["dv"], 1e-4)[0] == 14
    fate, add, event, s = _one(1)
    assert s["visible"] and add == [quant(c) for c in s["c"]] and any(add) and event & er.DIRECT
    # the sun: the texel of 400 is found, and seen past the occluder
    fate, add, event, s = _one(37)
    assert s["k"] == index(er.SUN) and s["visible"] and all(add) and s["P"] > 0.5
    # a texel with a NaN and a negative channel, chosen by its green one: the other two add 0
    fate, add, event, s = _one(43)
    assert s["k"] == index(er.NAN_TEXEL) and s["visible"] and add[0] == 0 and add[1] > 0 and add[2] == 0 and math.isnan(s["c"][0]) and s["c"][2] < 0.0
    # a light hit carrying the bit still adds (sphere lights are not sampled in this mode)
    assert q["event"][6] & er.DIRECT and hit[6][0] == 5 and _one(6)[0] == "light"
    assert _one(6)[1] == [quant(q["throughput"][6][c] * light.emission[5][c]) for c in range(3)] and all(_one(6)[1])
    # a pixel outside the frame: the shadow ray is traced and visible, nothing is added
    fate, add, event, s = _one(31)
    assert int(q["pixel"][31]) >= er.HAND_NPIX and s["visible"] and add is None and not adds[:, :].any(axis=1)[er.HAND_NPIX - 1:].any()
    # a Metal and a Dialectric hit clear the bit; a Lambertian one keeps it set; without the table or with NO_DIRECT it is cleared
    assert q["event"][2] & er.DIRECT and _one(2)[0] == "metal" and not _one(2)[2] & er.DIRECT and _one(2)[3] is None
    assert q["event"][3] & er.DIRECT and _one(3)[0] in ("refract", "reflect") and not _one(3)[2] & er.DIRECT
    assert q["event"][17] & er.DIRECT and fates[17] == "lambertian" and _one(17)[2] & er.DIRECT
    assert not _one(17, no_direct=True)[2] & er.DIRECT and not _one(17, env=(texels, None))[2] & er.DIRECT
    # the environments that sample at an edge, or not at all
    special = er.special_envs(8)
    lamb = [k for k in range(513) if fates[k] == "lambertian"]
    assert len(lamb) > 90
    for name, want_k in (("first", 0), ("last", 383)):
        _, _, _, g = er.bounce_env(scene, q, er.SEED, er.HAND_NPIX, light, special[name], 8)
        assert all(g[k]["k"] == want_k and g[k]["P"] == 1.0 for k in lamb), name
    for name in ("zero", "nan_table", "inf_table"):
        nw, fs, ad, g = er.bounce_env(scene, q, er.SEED, er.HAND_NPIX, light, special[name], 8)
        assert all(s is None for s in g) and not any(int(nw["event"][k]) & er.DIRECT for k in lamb), name
        base = er.bounce_env(scene, q, er.SEED, er.HAND_NPIX, light, (special[name][0], None), 8)
        assert np.array_equal(ad, base[2]) and all(np.array_equal(nw[f].view(np.uint8), base[0][f].view(np.uint8)) for f in pr.FIELDS), name
    # a zero-weight texel between positive ones is never chosen, whatever the word
    zeros = {index(z) for z in er.ZERO_TEXELS}
    assert all(cdf[z] == cdf[z - 1] and cdf[z + 1] > cdf[z] for z in zeros)
    chosen = {s["k"] for s in got if s is not None}
    assert not chosen & zeros and len(chosen) > 20
    for z in zeros:
        for x in (cdf[z - 1], np.nextafter(cdf[z - 1], 0.0), np.nextafter(cdf[z], INF)):
            word = min(0xFFFFFFFF, max(0, int(x / cdf[-1] * 4294967296.0)))
            for w in (word - 1, word, word + 1):
                assert er.sample_words(texels, cdf, 8, (w & 0xFFFFFFFF, 0, 0), (0.0, 1.0, 0.0), (1.0, 1.0, 1.0))["k"] not in zeros
    # by waves: all 64 lanes with a shadow ray; none (the wave that ends on lights whole, and the waves of misses)
    assert all(got[k] is not None and got[k]["shadow"] for k in er.ALL_WAVE)
    assert any(got[k]["visible"] for k in er.ALL_WAVE) and any(not got[k]["visible"] for k in er.ALL_WAVE)
    assert not any(got[k] is not None for k in range(128, 192)) and not any(got[k] is not None for k in range(256, 320))
    # sampling changes what is added, never where paths go: every array of the unsampled statement but bit 31 of the event
    assert fates == plain_fates and all(s is None for s in plain_got)
    for f in pr.FIELDS:
        a, b = new[f], plain_new[f]
        if f == "event":
            assert not (b & np.uint32(er.DIRECT)).any() and (a & np.uint32(er.DIRECT)).any()
            a = a & np.uint32(0x7FFFFFFF)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f
    assert not np.array_equal(adds, plain_adds)
    for count in (0, 1, 63, 64, 65, 256, 257, 513):
        out, _, live, shadow = er.hand_step(count)
        assert live == count and len(out["pixel"]) == sum(f in lr.SURVIVES for f in fates[:count])
        assert shadow == sum(1 for s in got[:count] if s is not None and s["shadow"])
    assert er.hand_step(513)[3] > 64 and er.hand_step(1)[3] == 0 and er.hand_step(63)[3] > 0
    assert er.hand_step(513, sampled=False)[3] == 0 == er.hand_step(513, no_direct=True)[3]


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------------

def environment(*, texels=TEXELS, cdf=CDF, size=2, flags=0):
    return _ffi.rt_environment(texels.ctypes.data if texels is not None else None, cdf.ctypes.data if cdf is not None else None, size, flags)


def _step(qin, qout, light=DEFAULT, env=DEFAULT, *, step_flags=0, flags=0, t_min=1e-4, fix=True, npix=6):
    light = lighting() if light is DEFAULT else light
    env = environment() if env is DEFAULT else env
    return _ffi.load().rt_paths_step_env_device(None, 1, flags, t_min, C.byref(qin.q) if qin else None, C.byref(qout.q) if qout else None,
                                                FIX.ctypes.data if fix else None, npix, RAYS.ctypes.data,
                                                C.byref(light) if light is not None else None, C.byref(env) if env is not None else None, step_flags,
                                                SHADOW.ctypes.data, None)


def _render(form, light=DEFAULT, env=DEFAULT, *, params=True, fix=True, sample=1, **kw):
    lib = _ffi.load()
    light = lighting() if light is DEFAULT else light
    env = environment() if env is DEFAULT else env
    camera = rt.book1_camera(8, 8).to_rt_camera()
    p = rt.make_params(8, 8, 2)
    for k, v in kw.items():
        setattr(p, k, v)
    pp, f = C.byref(p) if params else None, FIX.ctypes.data if fix else None
    ll, ee = C.byref(light) if light is not None else None, C.byref(env) if env is not None else None
    if form == "device":
        return lib.rt_render_wavefront_env_device(None, C.byref(camera), pp, ll, ee, f, RAYS.ctypes.data, SHADOW.ctypes.data, None)
    return lib.rt_render_wavefront_env(None, C.byref(camera), pp, ll, ee, sample, f, RAYS.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       SHADOW.ctypes.data_as(C.POINTER(C.c_uint64)), None)


def test_the_symbols_resolve():
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert lib.rt_abi_version() == 5                                             # the change only adds
    assert _ffi.RT_ENV_MAX_SIZE == 1024


# (what is passed, what the message holds); the last rows pass every context-free check
ENV_CASES = [
    (dict(env=None), "env is NULL"),
    (dict(env=dict(flags=1)), "unknown env->flags 0x1"),
    (dict(env=dict(size=0)), "env->size must be a power of two"),
    (dict(env=dict(size=3)), "env->size must be a power of two"),
    (dict(env=dict(size=2048)), "env->size must be a power of two"),
    (dict(env=dict(size=-2)), "env->size must be a power of two"),
    (dict(env=dict(texels=None)), "env->texels is NULL"),
    (dict(env=dict()), "ctx is NULL"),
    (dict(env=dict(cdf=None)), "ctx is NULL"),
]
STEP_CASES = ENV_CASES[:7] + [(dict(env=dict(), step_flags=2), "unknown step_flags 0x2"), (dict(env=dict(), step_flags=3), "unknown step_flags 0x3"),
                              (dict(env=dict(), step_flags=0x80000000), "unknown step_flags 0x80000000"), (dict(env=dict(), step_flags=1), "ctx is NULL")] \
    + ENV_CASES[7:]


def _snapshot():
    return tuple(a.copy() for a in (FIX, RAYS, SHADOW, TABLE, TEXELS, CDF))


def _untouched(before):
    return all(np.array_equal(a, b) for a, b in zip((FIX, RAYS, SHADOW, TABLE, TEXELS, CDF), before))


@pytest.mark.parametrize("case,msg", STEP_CASES, ids=[f"{m}-{i}" for i, (_, m) in enumerate(STEP_CASES)])
def test_step_rejections_need_no_context(case, msg):
    lib = _ffi.load()
    qin, qout, before = Queue(), Queue(), _snapshot()
    env = None if case["env"] is None else environment(**case["env"])
    assert _step(qin, qout, DEFAULT, env, step_flags=case.get("step_flags", 0)) == -1
    assert msg in _err(lib) and ("rt_paths_step_env" in _err(lib) or msg == "ctx is NULL"), _err(lib)
    assert qin.untouched() and qout.untouched() and _untouched(before)


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("case,msg", ENV_CASES, ids=[f"{m}-{i}" for i, (_, m) in enumerate(ENV_CASES)])
def test_frame_rejections_need_no_context(form, case, msg):
    lib = _ffi.load()
    before = _snapshot()
    assert _render(form, DEFAULT, None if case["env"] is None else environment(**case["env"])) == -1
    assert msg in _err(lib) and ("rt_render_wavefront_env" in _err(lib) or msg == "ctx is NULL"), _err(lib)
    assert _untouched(before)


def test_the_host_form_rejects_texels_it_can_see():
    lib = _ffi.load()
    before = _snapshot()
    for value, at in ((NAN, (0, 0, 0, 0)), (INF, (3, 1, 0, 2)), (-1.0, (5, 1, 1, 2)), (-INF, (2, 0, 1, 1))):
        bad = TEXELS.copy()
        bad[at] = value
        k = ((at[0] * 2 + at[1]) * 2 + at[2])
        for sample in (0, 1):
            assert _render("host", DEFAULT, environment(texels=bad), sample=sample) == -1
            assert f"env->texels[{k}][{at[3]}] must be finite and >= 0" in _err(lib), _err(lib)
        assert _render("device", DEFAULT, environment(texels=bad)) == -1 and "ctx is NULL" in _err(lib)       # the device forms validate no texel
    bad = TEXELS.copy()
    bad[0, 0, 0, 1] = -0.0                                                      # (-0.0 >= 0.0: passes)
    assert _render("host", DEFAULT, environment(texels=bad)) == -1 and "ctx is NULL" in _err(lib)
    assert _untouched(before)


def test_the_order_of_the_checks():
    """Every context-free check of the lit form first, in its order; then the environment: NULL, flags, size, texels; then the step flag;
    in the host form then the texels' values; then the context."""
    lib = _ffi.load()
    bad_table = np.full((4, 3), -1.0)
    bad_texels = np.full((6, 2, 2, 3), -1.0)
    worst = dict(flags=4, size=5, texels=None)
    assert _step(Queue(), Queue(), None, None, fix=False, step_flags=6, t_min=0.0) == -1 and "d_fix is NULL" in _err(lib)
    assert _step(Queue(), Queue(), None, None, step_flags=6, flags=8, t_min=0.0) == -1 and "RT_FLAG_UNIFORM53" in _err(lib)
    assert _step(Queue(), Queue(), None, None, step_flags=6, t_min=0.0) == -1 and "t_min must be" in _err(lib)
    assert _step(Queue(), Queue(), None, None, step_flags=6) == -1 and "light is NULL" in _err(lib)
    assert _step(Queue(), Queue(), lighting(flags=2), None, step_flags=6) == -1 and "light->flags" in _err(lib)
    assert _step(Queue(), Queue(), lighting(sky_top=(0, -1, 0)), None, step_flags=6) == -1 and "sky_top[1]" in _err(lib)
    assert _step(Queue(), Queue(), lighting(emission=bad_table, n_emission=-2), None, step_flags=6) == -1 and "n_emission must be >= 0" in _err(lib)
    assert _step(Queue(), Queue(), lighting(emission=bad_table, n_emission=4), None, step_flags=6) == -1 and "env is NULL" in _err(lib)
    assert _step(Queue(), Queue(), DEFAULT, environment(**worst), step_flags=6) == -1 and "env->flags" in _err(lib)
    worst.pop("flags")
    assert _step(Queue(), Queue(), DEFAULT, environment(**worst), step_flags=6) == -1 and "env->size" in _err(lib)
    worst.pop("size")
    assert _step(Queue(), Queue(), DEFAULT, environment(**worst), step_flags=6) == -1 and "env->texels is NULL" in _err(lib)
    assert _step(Queue(), Queue(), DEFAULT, environment(texels=bad_texels), step_flags=6) == -1 and "step_flags 0x6" in _err(lib)
    assert _step(Queue(), Queue(), DEFAULT, environment(texels=bad_texels), step_flags=1) == -1 and "ctx is NULL" in _err(lib)
    for form in ("device", "host"):
        assert _render(form, None, None, params=False) == -1 and "params is NULL" in _err(lib)
        assert _render(form, None, None, fix=False) == -1 and "fix is NULL" in _err(lib)
        assert _render(form, None, None, shard_count=2, t_min=INF) == -1 and "shard_count must be 1" in _err(lib)
        assert _render(form, None, None, t_min=INF) == -1 and "t_min must be" in _err(lib)
        assert _render(form, None, None) == -1 and "light is NULL" in _err(lib)
        assert _render(form, lighting(flags=4, sky_top=(-1, 0, 0)), None) == -1 and "light->flags" in _err(lib)
        assert _render(form, lighting(), None) == -1 and "env is NULL" in _err(lib)
        assert _render(form, lighting(), environment(flags=2, size=7, texels=bad_texels)) == -1 and "env->flags" in _err(lib)
        assert _render(form, lighting(), environment(size=7, texels=bad_texels)) == -1 and "env->size" in _err(lib)
    assert _render("host", lighting(emission=bad_table, n_emission=4), environment(texels=bad_texels)) == -1 and "light->emission[0][0]" in _err(lib)
    assert _render("host", lighting(), environment(texels=bad_texels)) == -1 and "env->texels[0][0]" in _err(lib)
    assert _render("device", lighting(emission=bad_table, n_emission=4), environment(texels=bad_texels)) == -1 and "ctx is NULL" in _err(lib)


def test_struct_layout_matches_the_header():
    """rt_environment: 24 bytes; the two pointers, the size, the flags -- in the header, ctypes and Rust; the limit likewise."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*rt_environment;", src).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["const double *texels", "const double *cdf", "int32_t size", "uint32_t flags"]
    E = _ffi.rt_environment
    assert E._fields_ == [("texels", C.c_void_p), ("cdf", C.c_void_p), ("size", C.c_int32), ("flags", C.c_uint32)]
    assert C.sizeof(E) == 24 and (E.texels.offset, E.cdf.offset, E.size.offset, E.flags.offset) == (0, 8, 16, 20)
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct rt_environment \{(.*?)\n\}", rs, flags=re.S).group(1)
    rust = [(m.group(1), m.group(2).strip()) for m in re.finditer(r"pub (\w+):\s*([^\n]+),", rbody)]
    assert rust == [("texels", "*const f64"), ("cdf", "*const f64"), ("size", "i32"), ("flags", "u32")]
    assert "24 == size_of::<rt_environment>()" in rs and re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct rt_environment ", rs)
    for field, offset in (("cdf", 8), ("size", 16), ("flags", 20)):
        assert f"offset_of!(rt_environment, {field}) == {offset}" in rs
    for name in ENTRY_POINTS:
        assert f"pub fn {name}(" in rs
        assert re.search(rf"\bint {name}\(", src)
    flat_src = re.sub(r"[ \t]+", " ", src)
    assert "#define RT_ENV_MAX_SIZE 1024" in flat_src and "pub const RT_ENV_MAX_SIZE: i32 = 1024;" in rs
    assert "#define RTIOW_HIP_ABI_VERSION 5" in flat_src
    args = {n: a for n, _, a in _ffi.SYMBOLS}
    for name in ENTRY_POINTS:
        decl = re.search(rf"\bint {name}\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(args[name]), name


# ---- the Python class ------------------------------------------------------------------------------------------------------------------------

def test_the_environment_class(tmp_path):
    env = rt.Environment.sun_sky(8, sun_dir=(0.3, 0.8, 0.6), cos_radius=0.99)
    t = env.table()
    assert t.shape == (6, 8, 8, 3) and env.size == 8 and env.sample and (t >= 0.0).all() and np.isfinite(t).all()
    sun = t.max(axis=-1) > 100.0
    assert 1 <= sun.sum() <= 4 and sun[2].any()                                  # the sun is on the +y face
    k = er.env_lookup((0.3, 0.8, 0.6), 8)
    assert t.reshape(-1, 3)[k].max() > 100.0                                     # where its direction looks it up
    tiny = rt.Environment.sun_sky(4, sun_dir=(0.0, 0.2, -1.0), cos_radius=0.99999)     # a sun smaller than a texel still gets one
    assert (tiny.table().max(axis=-1) > 100.0).sum() == 1 and tiny.table().reshape(-1, 3)[er.env_lookup((0.0, 0.2, -1.0), 4)].max() > 100.0
    sky = rt.Environment.sun_sky(2, sun_radiance=(0, 0, 0)).table()
    assert np.allclose(sky[2].mean(axis=(0, 1)), sky[2, 0, 0]) and sky[2, 0, 0, 0] < sky[3, 0, 0, 0]          # top colour above, bottom below
    path = str(tmp_path / "env.bin")
    env.save(path)
    assert os.path.getsize(path) == 6 * 8 * 8 * 3 * 8
    back = rt.Environment.load(path, sample=False)
    assert np.array_equal(bits(back.table()), bits(t)) and back.size == 8 and not back.sample
    assert np.array_equal(bits(env.cdf()), bits(er.environment_cdf(t, 8)))
    with open(path, "ab") as f:
        f.write(b"\0" * 8)
    with pytest.raises(ValueError, match="not 6"):
        rt.Environment.load(path)
    for shape in ((6, 3, 3, 3), (5, 2, 2, 3), (6, 2, 4, 3), (6, 2, 2, 4), (6, 2048, 1, 3)):
        with pytest.raises(ValueError):
            rt.Environment(np.zeros(shape))
    st = env.struct(1234, 0)
    assert (st.texels, st.cdf, st.size, st.flags) == (1234, None, 8, 0)


def test_environment_does_not_combine_with_direct():
    class Stub(rt.Renderer):
        def __init__(self):
            self.n_spheres = 3
    r = Stub()
    env = rt.Environment(np.zeros((6, 1, 1, 3)))
    for direct in (True, [0, 1]):
        with pytest.raises(ValueError, match="does not combine"):
            r._env_lighting(rt.Lighting(), direct, env)
    assert isinstance(r._env_lighting(None, False, env), rt.Lighting)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------

def test_the_cli_knows_the_switches_and_refuses_them_alone(tmp_path, book1_flat):
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert '"--env"' in src and '"--env-sample"' in src and "rt_render_wavefront_env(" in src
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    scene_file, env_file = str(tmp_path / "scene.bin"), str(tmp_path / "env.bin")
    rt.save_scene(scene_file, book1_flat)
    rt.Environment.sun_sky(4).save(env_file)
    base = [exe, "--scene", scene_file, "--width", "8", "--height", "8", "--spp", "1", "--out", str(tmp_path / "o.ppm")]
    # (every one is refused while the arguments are read: no device is asked for)
    for args, word in ((["--env", env_file], "--wavefront"), (["--env", env_file, "--env-sample"], "--wavefront"),
                       (["--wavefront", "--env-sample"], "--env"),
                       (["--wavefront", "--env", env_file, "--direct", "--emit", "0:1,1,1"], "--direct"),
                       (["--wavefront", "--env", env_file, "--env-sample", "--direct-cone", "--emit", "0:1,1,1"], "--direct"),
                       (["--wavefront", "--env", env_file, "--direct-weighted", "--emit", "0:1,1,1"], "--direct"),
                       (["--wavefront", "--env", env_file, "--adaptive", "0.1"], "--adaptive")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.returncode, bad.stderr)
    short = str(tmp_path / "short.bin")
    with open(short, "wb") as f:
        f.write(b"\0" * (6 * 3 * 3 * 3 * 8))                                     # a face edge of 3: no power of two
    bad = subprocess.run(base + ["--wavefront", "--env", short], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "power of two" in bad.stderr, (bad.returncode, bad.stderr)


# ---- the kernels, without a GPU ------------------------------------------------------------------------------------------------------------

def _fingerprint(*flags):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), *flags], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout.splitlines()


def _pinned(name):
    return [ln for ln in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if ln.startswith(("rt::", "void rt::"))]


def test_the_path_kernels_keep_their_machine_code_and_the_env_one_is_pinned():
    """tools/isa_fingerprint.py: --paths --weighted prints what it printed -- the five kernels of profiles/isa_fingerprint_lights.txt and
    the NEE, cone and weighted kernels, whose trip gained a sixth mode -- and no line for the new kernel; --env prints the one line of
    profiles/isa_fingerprint_env.txt."""
    got = [ln for ln in _fingerprint("--paths", "--weighted") if re.match(r"rt::(path_begin|bounce\w*|queue_scan|queue_compact)_kernel ", ln)]
    want = _pinned("isa_fingerprint_lights.txt")
    names = [ln.split()[0] for ln in got]
    assert names == ["rt::path_begin_kernel", "rt::bounce_kernel", "rt::bounce_lit_kernel", "rt::bounce_nee_kernel", "rt::bounce_cone_kernel",
                     "rt::bounce_weighted_kernel", "rt::queue_scan_kernel", "rt::queue_compact_kernel"]
    assert [ln for ln in got if not re.match(r"rt::bounce_(nee|cone|weighted)_kernel ", ln)] == want and len(want) == 5
    for kernel, name in (("nee", "isa_fingerprint_nee.txt"), ("cone", "isa_fingerprint_cone.txt"), ("weighted", "isa_fingerprint_weighted.txt")):
        assert [ln for ln in got if f"bounce_{kernel}_kernel" in ln] == [ln for ln in _pinned(name) if f"bounce_{kernel}_kernel" in ln], kernel
    env = [ln for ln in _fingerprint("--env") if "bounce_" in ln or "queue_" in ln or "path_begin" in ln]
    assert env == _pinned("isa_fingerprint_env.txt") and len(env) == 1 and env[0].startswith("rt::bounce_env_kernel ")
    both = [ln.split()[0] for ln in _fingerprint("--paths", "--env") if "bounce_" in ln]
    assert both == ["rt::bounce_kernel", "rt::bounce_lit_kernel", "rt::bounce_nee_kernel", "rt::bounce_cone_kernel", "rt::bounce_env_kernel"]


def test_the_shade_kernels_keep_their_machine_code():
    """--shade prints its pinned lines (profiles/isa_fingerprint_paths.txt): the header the new sampler went into is that unit's too.
    (--all lists no kernel of the wavefront folder; tests/test_source_layout_host.py holds it to its pinned lines.)"""
    shade = [ln for ln in _fingerprint("--shade") if re.match(r"rt::(camera_rays|scatter|accumulate)_kernel ", ln)]
    assert shade == [ln for ln in _pinned("isa_fingerprint_paths.txt") if re.match(r"rt::(camera_rays|scatter|accumulate)_kernel ", ln)] and len(shade) == 3


def test_the_env_kernel_uses_no_scratch_memory_spills_no_vector_register_and_keeps_occupancy_4():
    """The compiler's own resource remarks for wavefront/rt_paths.hip, with the flags tools/kernel_resources.py passes."""
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
    found = [r for name, r in rows.items() if "bounce_env_kernelE" in name]
    assert len(found) == 1
    r = found[0]
    print("bounce_env_kernel VGPRs", r["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "SGPR spills", r["SGPRs Spill"])
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["Occupancy [waves/SIMD]"]) >= 4, r


# ---- the same expectation, less variance -----------------------------------------------------------------------------------------------------

def test_the_stat_scene_has_the_same_expectation_and_less_variance_when_sampled(oracle_mod):
    """A Lambertian ground, a Metal, a Dialectric and an occluder under a sun_sky map whose sun is out of view; 16 x 12 pixels, 64 spp,
    depth 8, seeds 1..16, with the statement.  Per seed the frame-total energy sampled minus unsampled: |mean| <= 4 standard errors of
    the 16 differences; the per-pixel variance over the seeds, summed over the frame, is lower sampled.  The numbers are recorded in
    env_ref.STAT_EXPECTED, which tests/test_gpu_env.py holds the device's frames to.  No sample reaches the 2^16 clamp: the largest
    texel is 400 and a sample's weight is at most tot s^2 / (pi mx) of it, so the u64 sums are unbiased for both estimators."""
    assert er.STAT_SEEDS == tuple(range(1, 17))
    texels = er.stat_environment().table()
    cdf = er.environment_cdf(texels, er.STAT_ENV_SIZE)
    s = 2.0 / er.STAT_ENV_SIZE
    assert float(texels.max()) * max(1.0, cdf[-1] * s * s / math.pi) < 65536.0 / 10.0
    # the sun is behind the camera: no camera ray looks it up
    sun = np.argwhere(texels.max(axis=-1) > 100.0)
    assert len(sun) >= 1 and all(f == 2 for f, _, _ in sun)
    sampled, plain = er.stat_reference()
    mean, stderr, var_sampled, var_plain = er.stat_numbers(sampled, plain)
    print(f"energy sampled - unsampled: mean {mean:.6g}, standard error {stderr:.6g}, |mean| / stderr {abs(mean) / stderr:.3f}; "
          f"variance unsampled {var_plain:.6g}, sampled {var_sampled:.6g}, unsampled / sampled {var_plain / var_sampled:.3f}")
    assert stderr > 0.0 and abs(mean) <= 4.0 * stderr
    assert 0.0 < var_sampled < var_plain
    assert all(math.isclose(a, b, rel_tol=1e-9) for a, b in zip((mean, stderr, var_sampled, var_plain), er.STAT_EXPECTED))
