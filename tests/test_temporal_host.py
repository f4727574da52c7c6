"""Temporal accumulation without a GPU (rt_temporal_host): the library's CPU statement against the numpy statement
of the contract (tests/temporal_ref.py), bit for bit, both out_fix and out_len; two pins that do not rest on that restatement (the
constants, the geometry of the reprojection); the context-free validation of the three entry points; and rt_temporal_core.hpp alone under
ASan + UBSan in a stand-alone program."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import features_ref as fr
import rtiow_amd as rt
import temporal_ref as tr
from rtiow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def differing(got, want):
    return f"{int((got[0] != want[0]).any(axis=-1).sum())} sums and {int((got[1] != want[1]).sum())} lengths of {got[1].size} pixels differ"


def same(got, want):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def cases():
    """size -> (frame, history), built once and left unchanged."""
    out = {}
    for w, h in tr.SIZES:
        frame, hist = tr.synthetic_frame(w, h, 3), tr.synthetic_history(w, h, 3)
        for a in (frame[0], frame[1], frame[3], hist[0], hist[1], hist[2]):
            a.setflags(write=False)
        out[(w, h)] = (frame, hist)
    return out


def test_the_abi_surface():
    lib = _ffi.load()
    for name in ("rt_temporal_device", "rt_temporal", "rt_temporal_host"):
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert C.sizeof(_ffi.rt_temporal) == 40 and _ffi.rt_temporal.alpha_min.offset == 8 and _ffi.rt_temporal.clamp_scale.offset == 32
    t = rt.make_temporal()
    assert (t.flags, t.alpha_min, t.sigma_normal, t.sigma_depth, t.clamp_scale) == (rt.RT_TEMPORAL_CLAMP, 0.1, 0.5, 0.1, 1.0)
    assert rt.make_temporal(clamp=False).flags == 0 and rt.RT_TEMPORAL_MAX_LEN == 65535 == tr.MAX_LEN
    assert lib.rt_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "rtiow_hip.h")).read()
    assert "#define RT_TEMPORAL_CLAMP   0x1u" in hdr and "#define RT_TEMPORAL_MAX_LEN 65535" in hdr


def test_the_synthetic_cases_exercise_the_contract(cases):
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp) = cases[(37, 19)]
    assert (feat[..., 7] == 0).any() and (feat[..., 3:6].view(np.int64) < 0).any() and int(fix.max()) > 1 << 53 and int(feat[..., 6].max()) > 1 << 53
    assert {0, 1, 65535}.issubset(set(int(x) for x in np.unique(plen))) and int(plen.max()) > 65535
    cur, prev = tr.camera_pairs(37, 19)["subpixel_pan"]
    hist = (pfix, plen, pfeat, pspp, prev)
    out, length = tr.accumulate(fix, spp, feat, feat_spp, cur, hist)
    first, _ = tr.accumulate(fix, spp, feat, feat_spp, cur, None)
    hit = feat[..., 7] != 0
    assert (length[~hit] == 1).all() and np.array_equal(out[~hit], first[~hit])                 # the sky takes the current frame
    assert (length[hit] == 1).any() and (length[hit] == 2).any() and (length == 65535).any()       # rejected, accepted, saturated
    assert 0.2 < (length[hit] >= 2).mean() < 0.98
    # each test and the clamp decide something
    for other in (dict(sigma_depth=5.0), dict(sigma_normal=5.0), dict(clamp=False), dict(clamp_scale=0.0), dict(alpha_min=0.5)):
        o2, l2 = tr.accumulate(fix, spp, feat, feat_spp, cur, hist, **dict(tr.DEFAULTS, **other))
        assert (o2 != out).any() or (l2 != length).any(), other
    # clamp_scale 0 leaves the centre of the neighbourhood's box, whatever the history holds
    o0, _ = tr.accumulate(fix, spp, feat, feat_spp, cur, hist, **dict(tr.DEFAULTS, clamp_scale=0.0))
    o1, _ = tr.accumulate(fix, spp, feat, feat_spp, cur, (np.zeros_like(pfix), plen, pfeat, pspp, prev), **dict(tr.DEFAULTS, clamp_scale=0.0))
    assert np.array_equal(o0, o1)


@pytest.mark.parametrize("pair", ["identical", "subpixel_pan", "wide_pan", "facing_away", "roll_90", "fov", "nan_prev", "lens_radius", "orbit_step"])
@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_numpy_on_synthetic_frames(cases, size, pair):
    w, h = size
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp) = cases[size]
    cur, prev = tr.camera_pairs(w, h)[pair]
    hist = (pfix, plen, pfeat, pspp, prev)
    accepted = 0
    for options in tr.OPTION_SETS:
        for cnt in (None, count):
            got = rt.temporal_host(fix, spp, feat, feat_spp, cur, hist, tr.make_options(**options), count=cnt)
            want = tr.accumulate(fix, spp, feat, feat_spp, cur, hist, count=cnt, **options)
            assert same(got, want), (options, cnt is not None, differing(got, want))
            accepted += int((want[1] >= 2).sum())
    if pair in ("wide_pan", "facing_away", "nan_prev"):
        assert accepted == 0                                            # every tap out of frame; s <= 0; a NaN fails every comparison
    elif size != (2, 2):
        assert accepted > 0


def test_lens_radius_does_not_matter(cases):
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp) = cases[(37, 19)]
    a = tr.camera_pairs(37, 19)["subpixel_pan"]
    b = tr.camera_pairs(37, 19)["lens_radius"]
    assert a[0].lens_radius != b[0].lens_radius and a[1].lens_radius != b[1].lens_radius
    assert same(rt.temporal_host(fix, spp, feat, feat_spp, a[0], (pfix, plen, pfeat, pspp, a[1])),
                rt.temporal_host(fix, spp, feat, feat_spp, b[0], (pfix, plen, pfeat, pspp, b[1])))


@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_first_frame(cases, size):
    (fix, count, spp, feat, feat_spp), _ = cases[size]
    cam = tr.camera(*size)
    for cnt in (None, count):
        got = rt.temporal_host(fix, spp, feat, feat_spp, cam, None, count=cnt)
        assert same(got, tr.accumulate(fix, spp, feat, feat_spp, cam, None, count=cnt))
        assert (got[1] == 1).all() and np.array_equal(got[0], tr.quantize(tr.colour(fix, spp, cnt)))


@pytest.fixture(scope="module")
def book_chain(oracle_mod, book1_flat):
    """The book scene at 37 x 19, the first 3 cameras of orbit_cameras(180), 4 spp with streams of their own: Oracle B's sums and the
    reference's feature sums of the same samples."""
    w, h, spp = 37, 19, 4
    frames = []
    for f, cam in enumerate(rt.orbit_cameras(180, w, h)[:3]):
        ocam = oracle_mod.camera_from_host(cam)
        fix, _, _ = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, sample_begin=f * spp, seed=1))
        feat, _ = fr.render_features(ocam, book1_flat, w, h, spp, sample_begin=f * spp, seed=1)
        frames.append((fix, spp, feat, spp, cam))
    return frames


def test_host_equals_numpy_on_a_chain_of_oracle_renders(book_chain):
    want = tr.chain(book_chain)
    history = None
    for k, (fix, spp, feat, feat_spp, cam) in enumerate(book_chain):
        got = rt.temporal_host(fix, spp, feat, feat_spp, cam, history)
        assert same(got, want[k]), (k, differing(got, want[k]))
        history = (got[0], got[1], feat, feat_spp, cam)
    hit = book_chain[2][2][..., 7] != 0
    assert (want[2][1][hit] == 3).mean() > 0.5 and (want[2][0] != want[0][0]).any()


def pinhole(look_from, look_at, fov, w, h):
    return rt.Camera(rt.Point3(*look_from), rt.Point3(*look_at), rt.Vec3(0, 1, 0), fov, float(w) / float(h), 0.0, 1.0)


def test_pin_constants():
    """Identical pinhole cameras, history 0.5 everywhere with length 3, current colour 0.25: powers of two scale exactly through the weighted
    mean, so every hit pixel gives exactly quantize(0.5 + 0.25 * (0.25 - 0.5)) and length 4 -- whatever the rounding of fx does to a and b."""
    w, h = 37, 19
    cam = pinhole((13, 2, 3), (0, 0, 0), 20.0, w, h)
    fix = np.full((h, w, 3), tr.Q1 // 4 * 2, dtype=np.uint64)                   # 2 samples of 0.25
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    feat[..., 7] = 2
    feat[..., 6] = 2 * tr.Q1                                                    # z = 1.0: the focus plane
    feat[..., 4] = 2 * tr.Q1                                                    # normal (0, 1, 0)
    feat[3:6, 5:9] = 0                                                          # a patch of sky
    pfix = np.full((h, w, 3), tr.Q1 // 2, dtype=np.uint64)
    plen = np.full((h, w), 3, dtype=np.uint32)
    out, length = rt.temporal_host(fix, 2, feat, 2, cam, (pfix, plen, feat, 2, pinhole((13, 2, 3), (0, 0, 0), 20.0, w, h)), rt.make_temporal(clamp=False))
    hit = feat[..., 7] != 0
    want = int(math.floor((0.5 + 0.25 * (0.25 - 0.5)) * 4294967296.0))
    assert want == 7 * tr.Q1 // 16
    assert (length[hit] == 4).all() and (out[hit] == want).all()
    assert (length[~hit] == 1).all() and (out[~hit] == tr.Q1 // 4).all()
    # a tap of a sky pixel of the previous frame is skipped; the mean over the others is still 0.5
    edge = np.zeros((h, w), dtype=bool)
    edge[2:7, 4:10] = True
    assert (out[edge & hit] == want).all()


def ground_case(w=32, h=16, shift=0.4):
    """One huge ground sphere, a pinhole camera looking down at it and the same camera translated sideways: the feature sums of both
    frames from the analytic intersection of the pixel-centre rays, and where each pixel's first-hit point lies in the previous image by
    plain perspective projection from look_from / look_at / the camera's own axes."""
    fov, centre, radius = 40.0, np.array([0.0, -1000.0, 0.0]), 1000.0
    frm, at = np.array([0.0, 4.0, 6.0]), np.array([0.0, 0.0, 0.0])
    side = np.array([shift, 0.0, 0.0])
    th, aspect = math.tan(math.radians(fov) / 2.0), float(w) / float(h)

    def axes(frm, at):
        wv = (frm - at) / np.linalg.norm(frm - at)
        uv = np.cross(np.array([0.0, 1.0, 0.0]), wv)
        uv /= np.linalg.norm(uv)
        return uv, np.cross(wv, uv), wv

    def first_hits(frm, at):
        uv, vv, wv = axes(frm, at)
        jj, ii = np.mgrid[0:h, 0:w]
        su = 2.0 * (ii + 0.5) / (w - 1) - 1.0
        sv = 2.0 * (jj + 0.5) / (h - 1) - 1.0
        d = -wv + (su * th * aspect)[..., None] * uv + (sv * th)[..., None] * vv
        oc = frm - centre
        a, hb, c = (d * d).sum(-1), (d * oc).sum(-1), float(oc @ oc) - radius * radius
        disc = hb * hb - a * c
        assert (disc > 0).all()
        t = (-hb - np.sqrt(disc)) / a
        assert (t > 0).all()
        P = frm + t[..., None] * d
        nrm = (P - centre) / radius
        feat = np.zeros((h, w, 8), dtype=np.uint64)
        feat[..., 3:6] = np.floor(nrm * tr.Q1).astype(np.int64).view(np.uint64)
        feat[..., 6] = np.floor(t * tr.Q1).astype(np.uint64)
        feat[..., 7] = 1
        return feat, P

    feat, P = first_hits(frm, at)
    prev_feat, _ = first_hits(frm + side, at + side)
    uv, vv, wv = axes(frm + side, at + side)
    e = P - (frm + side)
    xc, yc, zc = e @ uv, e @ vv, -(e @ wv)
    fx = (xc / zc / (th * aspect) + 1.0) / 2.0 * (w - 1) - 0.5
    fy = (yc / zc / th + 1.0) / 2.0 * (h - 1) - 0.5
    return pinhole(frm, at, fov, w, h), pinhole(frm + side, at + side, fov, w, h), feat, prev_feat, fx, fy


def test_pin_geometry():
    """The history is a ramp i / W in red with length 1, the current colour 0: a pixel that reports length 2 holds half the ramp's
    bilinear value at (fx, fy), so 2 out_red W is fx -- where all four taps lie in the frame; where a column of taps falls outside it the
    weights renormalise over the other column, and the value is that column's (within one pixel of fx)."""
    w, h = 32, 16
    cur, prev, feat, prev_feat, fx, fy = ground_case(w, h)
    fix = np.zeros((h, w, 3), dtype=np.uint64)
    pfix = np.zeros((h, w, 3), dtype=np.uint64)
    pfix[..., 0] = (np.arange(w, dtype=np.uint64) * np.uint64(tr.Q1 // w))[None, :]
    plen = np.ones((h, w), dtype=np.uint32)
    tp = rt.make_temporal(alpha_min=0.1, sigma_normal=10.0, sigma_depth=10.0, clamp=False)
    out, length = rt.temporal_host(fix, 1, feat, 1, cur, (pfix, plen, prev_feat, 1, prev), tp)
    got = 2.0 * fr.fix_to_f64(out[..., 0]) * w
    two = length == 2
    inside = (fx >= 0.0) & (fx <= w - 1.0) & (fy >= 0.0) & (fy <= h - 1.0)
    reachable = (fx >= -1.0 + 1e-9) & (fx < w - 1e-9) & (fy >= -1.0 + 1e-9) & (fy < h - 1e-9)
    assert np.array_equal(two, reachable), (int(two.sum()), int(reachable.sum()))
    assert (two & inside).sum() > 0.8 * w * h and (two & ~inside).sum() > 0
    assert np.abs(got - fx)[two & inside].max() < 1e-6, np.abs(got - fx)[two & inside].max()
    assert np.abs(got - fx)[two & ~inside].max() <= 1.0 + 1e-6
    assert 0.3 < np.abs(fx - np.arange(w)[None, :]).max() < 4.0 and np.ptp(fx - np.arange(w)[None, :]) > 0.2    # a parallax that varies with depth
    assert (out[~two] == 0).all() and (out[..., 1:] == 0).all()


@pytest.mark.parametrize("form", ["host", "device", "buffers"])
@pytest.mark.parametrize("kw,msg", tr.BAD, ids=tr.BAD_IDS)
def test_rejections_touch_nothing(kw, msg, form):
    """Every rejection, from every form, without a context: RT_ERR_INVALID_ARGUMENT, the reason, and the outputs untouched."""
    lib = _ffi.load()
    arrays = tr.rejection_arrays()
    rc = tr.call_form(lib, form, kw, {k: a.ctypes.data for k, a in arrays.items()})
    assert rc == -1 and msg in lib.rt_last_error().decode(), lib.rt_last_error().decode()
    assert (arrays["out"] == 0xABCD).all() and (arrays["olen"] == 0xABCD).all()


def test_the_forms_with_a_context_name_what_is_missing():
    lib = _ffi.load()
    w, h = 4, 3
    arrays = dict(fix=np.zeros((h, w, 3), dtype=np.uint64), feat=np.zeros((h, w, 8), dtype=np.uint64), pfix=np.zeros((h, w, 3), dtype=np.uint64),
                  plen=np.ones((h, w), dtype=np.uint32), pfeat=np.zeros((h, w, 8), dtype=np.uint64), out=np.zeros((h, w, 3), dtype=np.uint64),
                  olen=np.zeros((h, w), dtype=np.uint32))
    bufs = {k: a.ctypes.data for k, a in arrays.items()}
    for form in ("device", "buffers"):
        assert tr.call_form(lib, form, {}, bufs) == -1 and "ctx is NULL" in lib.rt_last_error().decode()
    assert tr.call_form(lib, "host", {}, bufs) == 0 and (arrays["olen"] == 1).all()
    # no history at all is the first frame; prev_feat_spp is not looked at then
    assert tr.call_form(lib, "host", dict(pfix=None, plen=None, pfeat=None, pcam=None, pspp=0), bufs) == 0


def test_core_header_alone_under_asan_and_ubsan(cases, tmp_path):
    """tests/temporal_san_main.cpp includes rt_temporal_core.hpp (which includes rt_denoise_core.hpp) and nothing else of the library; the
    sanitizers watch it chain three frames of 2 x 2, 5 x 3 and 37 x 19 (buffers of exactly the size the filter may touch), and its checksum is
    numpy's."""
    assert shutil.which("g++")
    src = open(os.path.join(ROOT, "rtiow_amd", "csrc", "rt_temporal_core.hpp")).read()
    assert "#include <hip" not in src and src.count("#include") == 2 and '#include "rt_denoise_core.hpp"' in src
    exe = str(tmp_path / "temporal_san_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "temporal_san_main.cpp")], check=True, timeout=300)
    for (w, h), options, with_count, pair in (((5, 3), tr.OPTION_SETS[0], True, "subpixel_pan"), ((37, 19), tr.OPTION_SETS[0], False, "orbit_step"),
                                              ((37, 19), tr.OPTION_SETS[3], True, "fov"), ((2, 2), tr.OPTION_SETS[1], False, "identical")):
        cur, prev = tr.camera_pairs(w, h)[pair]
        frames = []
        for k, cam in enumerate((prev, cur, prev)):
            fix, count, spp, feat, feat_spp = tr.synthetic_frame(w, h, 20 + k)
            frames.append((fix, count if with_count else None, spp, feat, feat_spp, cam))
        path = str(tmp_path / f"case_{w}x{h}_{pair}.bin")
        with open(path, "wb") as f:
            f.write(np.array([w, h, len(frames), frames[0][2], frames[0][4], rt.RT_TEMPORAL_CLAMP if options["clamp"] else 0, int(with_count)], dtype="<i8").tobytes())
            f.write(np.array([options["alpha_min"], options["sigma_normal"], options["sigma_depth"], options["clamp_scale"]], dtype="<f8").tobytes())
            for fix, count, spp, feat, feat_spp, cam in frames:
                f.write(np.array([x for v in tr.cam_vectors(cam) for x in v], dtype="<f8").tobytes())
                f.write(np.ascontiguousarray(fix, dtype="<u8").tobytes())
                if with_count:
                    f.write(np.ascontiguousarray(count, dtype="<u4").tobytes())
                f.write(np.ascontiguousarray(feat, dtype="<u8").tobytes())
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and not run.stderr, run.stderr
        history = None
        for fix, count, spp, feat, feat_spp, cam in frames:
            out, length = tr.accumulate(fix, spp, feat, feat_spp, cam, history, count=count, **options)
            history = (out, length, feat, feat_spp, cam)
        assert int(run.stdout.strip(), 16) == tr.checksum(out, length), (w, h, pair)
