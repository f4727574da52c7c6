"""Temporal accumulation with second moments and the variance-guided denoiser fed by a given variance, without a GPU
(rt_temporal_var_host, rt_denoise_var_given_host): the library's CPU statements against the numpy statement of the
contract (tests/temporal_var_ref.py), bit for bit on all outputs -- doubles compared as u64, so NaN and -0 count --; out_fix and out_len
against rt_temporal_host's own arrays; known answers that do not rest on the restatement; the cross-pin of the shared levels against
rt_denoise_var_host; the context-free validation of the six entry points in the documented order; the declarations; the fingerprints;
the two core headers alone under ASan + UBSan in a stand-alone program; and the command line's exit codes."""
import ctypes as C
import itertools
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import denoise_var_ref as vr
import features_ref as fr
import rtiow_amd as rt
import temporal_ref as tr
import temporal_var_ref as tv
from isa_pins import fingerprint_lines
from rtiow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtiow_amd", "csrc")
PAIRS = ["identical", "subpixel_pan", "wide_pan", "facing_away", "roll_90", "fov", "nan_prev", "lens_radius", "orbit_step"]
FILTER_SIZES = [(1, 1), (5, 3), (37, 19), (70, 45)]
NAMES = ("rt_temporal_var_device", "rt_temporal_var", "rt_temporal_var_host", "rt_denoise_var_given_device", "rt_denoise_var_given",
         "rt_denoise_var_given_host")


def same(got, want):
    """(out_fix, out_len, out_m2, out_var) bit for bit"""
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float64 and got[3].dtype == np.float64
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(tv.bits(got[2]), tv.bits(want[2]))
            and np.array_equal(tv.bits(got[3]), tv.bits(want[3])))


def differing(got, want):
    return (f"{int((got[0] != want[0]).any(axis=-1).sum())} sums, {int((got[1] != want[1]).sum())} lengths, "
            f"{int((tv.bits(got[2]) != tv.bits(want[2])).any(axis=-1).sum())} moments and "
            f"{int((tv.bits(got[3]) != tv.bits(want[3])).any(axis=-1).sum())} variances of {got[1].size} pixels differ")


@pytest.fixture(scope="module")
def cases():
    """size -> (frame, history with prev_m2 as its last entry), built once and left unchanged."""
    out = {}
    for w, h in tr.SIZES:
        frame, hist = tr.synthetic_frame(w, h, 3), tr.synthetic_history(w, h, 3)
        hist = hist + (tv.synthetic_m2(hist[0], 3),)
        for a in (frame[0], frame[1], frame[3], hist[0], hist[1], hist[2], hist[4]):
            a.setflags(write=False)
        out[(w, h)] = (frame, hist)
    return out


@pytest.fixture(scope="module")
def filter_cases():
    out = {}
    for w, h in FILTER_SIZES + [(150, 9)]:
        fix, _, count, spp, feat, feat_spp = vr.synthetic_case(w, h)
        case = (fix, tv.synthetic_var(fix, None, spp, 5), tv.synthetic_var(fix, count, spp, 6), count, spp, feat, feat_spp)
        for a in case[:4] + (feat,):
            a.setflags(write=False)
        out[(w, h)] = case
    return out


def test_the_declarations():
    """The six functions: in the header, in ctypes (and the library resolves them), in the Rust binding; the ABI version stays 5."""
    lib = _ffi.load()
    hdr = open(os.path.join(ROOT, "include", "rtiow_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert "#define RTIOW_HIP_ABI_VERSION 5" in hdr and lib.rt_abi_version() == 5
    assert "#define RT_TEMPORAL_VAR_MIN_LEN 4" in hdr and rt.RT_TEMPORAL_VAR_MIN_LEN == 4 == tv.MIN_LEN
    args = {n: a for n, _, a in _ffi.SYMBOLS}
    assert [len(args[n]) for n in NAMES] == [21, 21, 19, 13, 12, 10]
    # three more arguments than rt_temporal's, the same as rt_denoise_var's
    assert len(args["rt_temporal_var_host"]) == len(args["rt_temporal_host"]) + 3 and args["rt_denoise_var_given_host"] == args["rt_denoise_var_host"]
    assert rt.Renderer.temporal_var_host is rt.temporal_var_host and rt.Renderer.denoise_var_given_host is rt.denoise_var_given_host
    from rtiow_amd import render
    assert render.TEMPORAL_VAR_SIGMA_COLOR == tv.SIGMA_COLOR
    import inspect
    assert list(inspect.signature(rt.Renderer.render_sequence_var).parameters) == [
        "self", "cams", "params", "sample_stride", "feature_spp", "temporal", "denoise", "lighting", "direct", "sampling", "flip"]


def test_the_synthetic_moments_exercise_the_contract(cases):
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp, pm2) = cases[(37, 19)]
    hcol = fr.fix_to_f64(pfix)
    assert np.isnan(pm2).any() and (pm2 == 0.0).any() and (pm2 == 1e12).any() and (pm2 < hcol * hcol).any() and (pm2 > hcol * hcol).any()
    for size in tr.SIZES:
        m = cases[size][1][4]
        assert np.isnan(m).any() and (m == 0.0).any() and (m == 1e12).any() and (m < fr.fix_to_f64(cases[size][1][0]) ** 2).any(), size
    cur, prev = tr.camera_pairs(37, 19)["subpixel_pan"]
    out, length, m2, var = tv.accumulate(fix, spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev, pm2))
    acc = length >= 2
    assert np.isnan(m2[acc]).any() and (var[acc & (length >= 4)] == 0.0).any() and (var[acc & (length >= 4)] > 0.0).any()
    assert (length[acc] < 4).any() and (length[acc] >= 4).any() and not np.isnan(var).any() and (var >= 0.0).all()
    # the moment matters, and so does the clamp's rule for it
    other = tv.accumulate(fix, spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev, pm2 * 0.5))
    assert np.array_equal(other[0], out) and (tv.bits(other[2]) != tv.bits(m2)).any() and (tv.bits(other[3]) != tv.bits(var)).any()
    off = tv.accumulate(fix, spp, feat, feat_spp, cur, (pfix, plen, pfeat, pspp, prev, pm2), **dict(tr.DEFAULTS, clamp=False))
    assert (tv.bits(off[2]) != tv.bits(m2)).any()


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_numpy_and_rt_temporal_on_synthetic_frames(cases, size, pair):
    """All four outputs against numpy; out_fix and out_len against rt_temporal_host's arrays for the same inputs."""
    w, h = size
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp, pm2) = cases[size]
    cur, prev = tr.camera_pairs(w, h)[pair]
    hist = (pfix, plen, pfeat, pspp, prev, pm2)
    accepted = 0
    for options in tr.OPTION_SETS:
        for cnt in (None, count):
            got = rt.temporal_var_host(fix, spp, feat, feat_spp, cur, hist, tr.make_options(**options), count=cnt)
            want = tv.accumulate(fix, spp, feat, feat_spp, cur, hist, count=cnt, **options)
            assert same(got, want), (options, cnt is not None, differing(got, want))
            old = rt.temporal_host(fix, spp, feat, feat_spp, cur, hist[:5], tr.make_options(**options), count=cnt)
            assert np.array_equal(got[0], old[0]) and np.array_equal(got[1], old[1]), (options, cnt is not None)
            accepted += int((want[1] >= 2).sum())
    if pair in ("wide_pan", "facing_away", "nan_prev"):
        assert accepted == 0
    elif size != (2, 2):
        assert accepted > 0


@pytest.mark.parametrize("size", tr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_first_frame_returns_the_spatial_estimate(cases, size):
    (fix, count, spp, feat, feat_spp), _ = cases[size]
    cam = tr.camera(*size)
    for cnt in (None, count):
        got = rt.temporal_var_host(fix, spp, feat, feat_spp, cam, None, count=cnt)
        assert same(got, tv.accumulate(fix, spp, feat, feat_spp, cam, None, count=cnt))
        c = tr.colour(fix, spp, cnt)
        assert (got[1] == 1).all() and np.array_equal(got[0], tr.quantize(c)) and np.array_equal(tv.bits(got[2]), tv.bits(c * c))
        assert np.array_equal(tv.bits(got[3]), tv.bits(tv.neighbourhood(c)[2]))
        old = rt.temporal_host(fix, spp, feat, feat_spp, cam, None, count=cnt)
        assert np.array_equal(got[0], old[0]) and np.array_equal(got[1], old[1])


def test_first_frame_at_a_corner_of_a_2x2_frame_counts_four():
    """Dyadic colours 1, 2, 3, 6 in red: every pixel of a 2 x 2 frame sees all four, a1 = 12, a2 = 50, cnt = 4: vs = 50 / 4 - 9 = 3.5."""
    fix = np.zeros((2, 2, 3), dtype=np.uint64)
    fix[..., 0] = np.array([[1, 2], [3, 6]], dtype=np.uint64) * np.uint64(tr.Q1)
    feat = np.zeros((2, 2, 8), dtype=np.uint64)
    out, length, m2, var = rt.temporal_var_host(fix, 1, feat, 1, tr.camera(2, 2), None)
    assert (length == 1).all() and (var[..., 0] == 3.5).all() and (var[..., 1:] == 0.0).all()
    assert np.array_equal(m2[..., 0], np.array([[1.0, 4.0], [9.0, 36.0]])) and np.array_equal(out, fix)


def exact_pinhole():
    """An rt_camera whose reprojection onto itself is exact at 33 x 17: origin (0, 0, 4), the image plane 4 x 2 at distance 1, every
    component a small integer, and W - 1 = 32, H - 1 = 16 powers of two.  Then u = (i + 0.5) / 32 and v = (j + 0.5) / 16 are exact, e = L + u H
    + v V is exact, s = 1, up = u, fx = i and fy = j exactly: a = b = 0, ONE tap with kw = 1.  (0.3125 is no power of two: through four
    taps with rounded weights the mean of a constant 0.3125 is only within an ulp of it, so the pin needs a camera whose weights are exact.)"""
    cam = _ffi.rt_camera()
    cam.origin[:] = (0.0, 0.0, 4.0)
    cam.lower_left_corner[:] = (-2.0, -1.0, 3.0)
    cam.horizontal[:] = (4.0, 0.0, 0.0)
    cam.vertical[:] = (0.0, 2.0, 0.0)
    cam.u[:] = (1.0, 0.0, 0.0)
    cam.v[:] = (0.0, 1.0, 0.0)
    cam.lens_radius = 0.0
    return cam


def known_answer_case(w=33, h=17):
    fix = np.full((h, w, 3), tr.Q1 // 4 * 2, dtype=np.uint64)                   # 2 samples of 0.25
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    feat[..., 7] = 2
    feat[..., 6] = 2 * tr.Q1                                                    # z = 1.0: the image plane
    feat[..., 5] = 2 * tr.Q1                                                    # normal (0, 0, 1)
    feat[3:6, 5:9] = 0                                                          # a patch of sky
    pfix = np.full((h, w, 3), tr.Q1 // 2, dtype=np.uint64)
    plen = np.full((h, w), 3, dtype=np.uint32)
    pm2 = np.full((h, w, 3), 0.3125, dtype=np.float64)
    return exact_pinhole(), fix, feat, (pfix, plen, feat, 2, exact_pinhole(), pm2), feat[..., 7] != 0


def test_known_answers_that_do_not_rest_on_the_restatement():
    """Identical pinhole cameras, history colour 0.5 with length 3 and second moment 0.3125, current colour 0.25 everywhere; by hand,
    every value dyadic, on EVERY hit pixel (exact_pinhole: each pixel reprojects onto itself).  at = 1/4, s2 = 0.0625.
    Clamp off: o = 0.5 + (0.25 - 0.5) / 4 = 0.4375; m2 = 0.3125 + (0.0625 - 0.3125) / 4 = 0.25; vt = 0.25 - 0.4375^2 = 0.05859375; len = 4,
    so out_var = vt / 4 = 0.0146484375.
    Clamp on at scale 1: the box is the point 0.25, so h = 0.25 and h2 = (0.3125 - 0.25) + 0.0625 = 0.125; o = 0.25;
    m2 = 0.125 + (0.0625 - 0.125) / 4 = 0.109375; vt = 0.109375 - 0.0625 = 0.046875; out_var = 0.01171875."""
    cam, fix, feat, hist, hit = known_answer_case()
    assert hit.sum() == 33 * 17 - 12
    out, length, m2, var = rt.temporal_var_host(fix, 2, feat, 2, cam, hist, rt.make_temporal(clamp=False))
    assert (length[hit] == 4).all() and (out[hit] == tr.quantize(np.float64(0.4375))).all() and tr.quantize(np.float64(0.4375)) == 7 * tr.Q1 // 16
    assert (m2[hit] == 0.25).all() and (var[hit] == 0.0146484375).all()
    assert same((out, length, m2, var), tv.accumulate(fix, 2, feat, 2, cam, hist, **dict(tr.DEFAULTS, clamp=False)))
    out, length, m2, var = rt.temporal_var_host(fix, 2, feat, 2, cam, hist, rt.make_temporal(clamp=True, clamp_scale=1.0))
    assert (length[hit] == 4).all() and (out[hit] == tr.Q1 // 4).all()
    assert (m2[hit] == 0.109375).all() and (var[hit] == 0.01171875).all()
    # the sky: no history, the frame's own square, and a flat neighbourhood
    assert (length[~hit] == 1).all() and (m2[~hit] == 0.0625).all() and (var[~hit] == 0.0).all()
    # the book camera's weights are rounded: the sums and the lengths are still exact (powers of two), the moment within an ulp
    w, h = 37, 19
    book = lambda: rt.Camera(rt.Point3(13, 2, 3), rt.Point3(0, 0, 0), rt.Vec3(0, 1, 0), 20.0, float(w) / float(h), 0.0, 1.0)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a[0, 0], (h, w) + a.shape[2:]))
    feat2 = tile(feat)
    out, length, m2, var = rt.temporal_var_host(tile(fix), 2, feat2, 2, book(), (tile(hist[0]), tile(hist[1]), feat2, 2, book(), tile(hist[5])),
                                                rt.make_temporal(clamp=False))
    inner = np.zeros((h, w), dtype=bool)
    inner[1:h - 1, 1:w - 1] = True
    assert (length[inner] == 4).all() and (out[inner] == 7 * tr.Q1 // 16).all()
    assert np.abs(m2[inner] - 0.25).max() <= 2.0 ** -53 and np.abs(var[inner] - 0.0146484375).max() <= 2.0 ** -55


def test_a_chain_of_five_constant_frames_ends_without_variance():
    """The same colour five times along an orbit: wherever the history is accepted, the weighted mean of a constant power of two is that
    constant whatever the weights round to, so h = c, h2 = c c, m2 = c c and vt = m2 - o o is exactly 0 -- with the clamp (its box is the
    point c) and without it; a pixel younger than four frames takes the flat 3 x 3 neighbourhood's 0.  Colours (0.5, 0.25, 2.0)."""
    w, h = 37, 19
    cams = rt.orbit_cameras(180, w, h)[:5]
    c = np.array([0.5, 0.25, 2.0])
    fix = np.zeros((h, w, 3), dtype=np.uint64)
    fix[...] = (c * 4.0 * tr.Q1).astype(np.uint64)
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    feat[..., 7] = 2
    feat[..., 6] = 2 * tr.Q1
    feat[..., 4] = 2 * tr.Q1
    for clamp in (True, False):
        history = None
        for cam in cams:
            out, length, m2, var = rt.temporal_var_host(fix, 4, feat, 2, cam, history, rt.make_temporal(sigma_depth=1.0, clamp=clamp))
            history = (out, length, feat, 2, cam, m2)
        old = length >= 4
        assert old.sum() > 0.5 * w * h and int(length.max()) == 5
        assert (var[old] == 0.0).all() and (var == 0.0).all(), clamp
        assert (out == fix // np.uint64(4)).all() and (m2 == c * c).all()


@pytest.fixture(scope="module")
def book_chain(oracle_mod, book1_flat):
    """The book scene at 37 x 19, the first 3 cameras of orbit_cameras(180), 4 spp with streams of their own (tests/test_temporal_host.py)."""
    w, h, spp = 37, 19, 4
    frames = []
    for f, cam in enumerate(rt.orbit_cameras(180, w, h)[:3]):
        ocam = oracle_mod.camera_from_host(cam)
        fix, _, _ = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, sample_begin=f * spp, seed=1))
        feat, _ = fr.render_features(ocam, book1_flat, w, h, spp, sample_begin=f * spp, seed=1)
        frames.append((fix, spp, feat, spp, cam))
    return frames


def test_host_equals_numpy_on_a_chain_of_oracle_renders(book_chain):
    want = tv.chain(book_chain)
    history = None
    for k, (fix, spp, feat, feat_spp, cam) in enumerate(book_chain):
        got = rt.temporal_var_host(fix, spp, feat, feat_spp, cam, history)
        assert same(got, want[k]), (k, differing(got, want[k]))
        history = (got[0], got[1], feat, feat_spp, cam, got[2])
    assert (want[2][1] == 3).mean() > 0.3 and (want[2][3] > 0.0).any()
    shown = rt.denoise_var_given_host(got[0], got[3], 1, feat, feat_spp)
    assert np.array_equal(shown, tv.denoise_var_given(got[0], got[3], 1, feat, feat_spp)) and (shown != got[0]).any()


def run_filter(case, levels, demodulate, with_count, sigma_color=vr.SIGMA_COLOR):
    fix, var_spp, var_count, count, spp, feat, feat_spp = case
    cnt, var = (count, var_count) if with_count else (None, var_spp)
    got = rt.denoise_var_given_host(fix, var, spp, feat, feat_spp, rt.make_denoise_var(levels, sigma_color, demodulate=demodulate), count=cnt)
    want = tv.denoise_var_given(fix, var, spp, feat, feat_spp, levels=levels, sigma_color=sigma_color, demodulate=demodulate, count=cnt)
    return got, want


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("size", FILTER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_filter_equals_numpy_on_synthetic_frames(filter_cases, size, levels):
    for demodulate in (True, False):
        for with_count in (False, True):
            got, want = run_filter(filter_cases[size], levels, demodulate, with_count)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (demodulate, with_count, int((got != want).any(axis=-1).sum()))


def test_the_filter_equals_numpy_at_six_levels_on_a_wide_frame(filter_cases):
    fix, var, _, _, spp, feat, feat_spp = filter_cases[(150, 9)]
    assert np.isnan(var).any() and (var < 0.0).any() and (var == 0.0).any() and (var == 1e-300).any() and (var == 1e12).any()
    for sigma_color in (vr.SIGMA_COLOR, 64.0):
        for demodulate in (True, False):
            for with_count in (False, True):
                got, want = run_filter(filter_cases[(150, 9)], 6, demodulate, with_count, sigma_color)
                assert np.array_equal(got, want), (sigma_color, demodulate, with_count)
    # the variance decides: another one gives another frame, and negatives and NaN count as 0
    base = tv.denoise_var_given(fix, var, spp, feat, feat_spp, levels=6)
    assert (tv.denoise_var_given(fix, var * 4.0, spp, feat, feat_spp, levels=6) != base).any()
    bad = ~(var > 0.0)
    assert np.array_equal(tv.denoise_var_given(fix, np.where(bad, 0.0, var), spp, feat, feat_spp, levels=6), base)


@pytest.mark.parametrize("size", [(37, 19), (70, 45)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_pin_of_the_shared_levels(size):
    """Without demodulation m = 1: var_ch = e_ch e_ch with e_ch = v(|2 half - fix|) / samples is what rt_denoise_var's Prepare squares
    itself ((x / 1) / 1 = x, and a square is never negative), so the two entries return the same bits."""
    fix, half, count, spp, feat, feat_spp = vr.synthetic_case(*size)
    dn = rt.make_denoise_var(4, demodulate=False)
    for cnt in (None, count):
        d = half * np.uint64(2) - fix
        d = np.where(d.view(np.int64) < 0, (~d) + np.uint64(1), d)
        e = fr.fix_to_f64(d) / (np.float64(spp) if cnt is None else cnt.astype(np.float64)[..., None])
        got = rt.denoise_var_given_host(fix, e * e, spp, feat, feat_spp, dn, count=cnt)
        assert np.array_equal(got, rt.denoise_var_host(fix, half, spp, feat, feat_spp, dn, count=cnt)), cnt is not None


# ---- the rejections every form makes before it touches anything ----

HIST = ("pfix", "plen", "pfeat", "pcam", "pm2")
PARTIAL = [dict.fromkeys(left_out) for n in (1, 2, 3, 4) for left_out in itertools.combinations(HIST, n)][::3] + [dict.fromkeys(HIST[:4])]
TP_BAD = ([(kw, msg) for kw, msg in tr.BAD if "partial" not in msg] + [(dict(om2=None), "a buffer is NULL"), (dict(ovar=None), "a buffer is NULL")]
          + [(kw, "partial history") for kw in PARTIAL])
# two faults at once: the one the documented order names first is reported
TP_ORDER = [
    (dict(tp=None, fix=None), "options are NULL"), (dict(ovar=None, pm2=None), "a buffer is NULL"), (dict(pm2=None, flags=2), "partial history"),
    (dict(flags=2, alpha_min=0.0), "unknown flags"), (dict(alpha_min=0.0, sigma_normal=0.0), "alpha_min"), (dict(sigma_depth=0.0, clamp_scale=-1.0), "sigma"),
    (dict(clamp_scale=-1.0, width=1), "clamp_scale"), (dict(width=1, spp=0), "must be >= 2"), (dict(width=65536, height=32769, spp=0), "<= 2^31"),
    (dict(spp=0, feat_spp=0), "spp >= 1 without a count"), (dict(feat_spp=0, pspp=0), "feat_spp >= 1"),
]
TP_IDS = ["-".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in TP_BAD + TP_ORDER]


def temporal_var_arrays(w=4, h=3):
    a = tr.rejection_arrays(w, h)
    a.update(pm2=np.zeros((h, w, 3), dtype=np.float64), om2=np.full((h, w, 3), 1234.5, dtype=np.float64), ovar=np.full((h, w, 3), 1234.5, dtype=np.float64))
    return a


def call_temporal_var(lib, form, kw, arrays):
    tp = rt.make_temporal()
    for k in ("flags", "alpha_min", "sigma_normal", "sigma_depth", "clamp_scale"):
        if k in kw:
            setattr(tp, k, kw[k])
    cam, pcam = rt.book1_camera(4, 3).to_rt_camera(), rt.book1_camera(4, 3).to_rt_camera()
    ptr = lambda name: None if name in kw else C.c_void_p(arrays[name].ctypes.data)
    args = [ptr("fix"), None, kw.get("spp", 8), ptr("feat"), kw.get("feat_spp", 8), None if "cam" in kw else C.byref(cam),
            ptr("pfix"), ptr("plen"), ptr("pfeat"), kw.get("pspp", 8), None if "pcam" in kw else C.byref(pcam), ptr("pm2"),
            kw.get("width", 4), kw.get("height", 3), None if "tp" in kw else C.byref(tp), ptr("out"), ptr("olen"), ptr("om2"), ptr("ovar")]
    if form == "host":
        return lib.rt_temporal_var_host(*args)
    if form == "buffers":
        return lib.rt_temporal_var(None, *args, None)
    return lib.rt_temporal_var_device(None, *args, None)


def untouched(arrays):
    return ((arrays["out"] == 0xABCD).all() and (arrays["olen"] == 0xABCD).all() and (arrays["om2"] == 1234.5).all()
            and (arrays["ovar"] == 1234.5).all())


@pytest.mark.parametrize("form", ["host", "device", "buffers"])
@pytest.mark.parametrize("kw,msg", TP_BAD + TP_ORDER, ids=TP_IDS)
def test_temporal_var_rejections_touch_nothing_and_come_in_the_documented_order(kw, msg, form):
    lib = _ffi.load()
    arrays = temporal_var_arrays()
    rc = call_temporal_var(lib, form, kw, arrays)
    err = lib.rt_last_error().decode()
    assert rc == -1 and msg in err and "temporal_var" in err, err
    assert untouched(arrays)


def test_temporal_var_with_everything_names_the_missing_context_last():
    lib = _ffi.load()
    arrays = temporal_var_arrays()
    for form in ("device", "buffers"):
        assert call_temporal_var(lib, form, {}, arrays) == -1 and "ctx is NULL" in lib.rt_last_error().decode()
        assert call_temporal_var(lib, form, dict(pspp=0), arrays) == -1 and "prev_feat_spp" in lib.rt_last_error().decode()
    assert untouched(arrays)
    assert len(PARTIAL) >= 10 and {len(p) for p in PARTIAL} == {1, 2, 3, 4}
    assert call_temporal_var(lib, "host", {}, arrays) == 0 and (arrays["olen"] == 1).all() and not untouched(arrays)
    # no history at all is the first frame; prev_feat_spp is not looked at then
    assert call_temporal_var(lib, "host", dict(pfix=None, plen=None, pfeat=None, pcam=None, pm2=None, pspp=0), arrays) == 0


DN_BAD = [
    (dict(dn=None), "dn is NULL"), (dict(fix=None), "NULL (fix)"), (dict(var=None), "NULL (var)"), (dict(feat=None), "NULL (feat or out)"),
    (dict(out=None), "NULL (feat or out)"), (dict(levels=0), "levels must be 1..8"), (dict(levels=9), "levels must be 1..8"), (dict(flags=2), "unknown flags"),
    (dict(sigma_color=0.0), "sigma"), (dict(sigma_normal=-1.0), "sigma"), (dict(sigma_depth=math.inf), "sigma"), (dict(sigma_color=math.nan), "sigma"),
    (dict(width=0), "bad width/height"), (dict(height=-3), "bad width/height"), (dict(width=65536, height=32769), "<= 2^31"),
    (dict(spp=0), "spp >= 1 without a count"), (dict(feat_spp=0), "feat_spp >= 1"),
]
DN_ORDER = [
    (dict(dn=None, fix=None), "dn is NULL"), (dict(fix=None, var=None), "NULL (fix)"), (dict(var=None, feat=None), "NULL (var)"),
    (dict(out=None, levels=0), "NULL (feat or out)"), (dict(levels=0, flags=2), "levels must be"), (dict(flags=2, sigma_color=0.0), "unknown flags"),
    (dict(sigma_depth=0.0, width=0), "sigma"), (dict(width=0, spp=0), "bad width/height"), (dict(width=65536, height=32769, spp=0), "<= 2^31"),
    (dict(spp=0, feat_spp=0), "spp >= 1 without a count"),
]


def call_filter(lib, form, kw, out):
    w, h = 4, 3
    fix = np.full((h, w, 3), 1 << 32, dtype=np.uint64)
    var = np.full((h, w, 3), 0.25, dtype=np.float64)
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
        return lib.rt_denoise_var_given_host(ptr("fix", fix), ptr("var", var), None, *common, ptr("out", out))
    if form == "buffers":
        return lib.rt_denoise_var_given(None, ptr("fix", fix), ptr("var", var), None, *common, ptr("out", out), None)
    return lib.rt_denoise_var_given_device(None, ptr("fix", fix), ptr("var", var), None, *common, ptr("work", work), ptr("out", out), None)


@pytest.mark.parametrize("form", ["host", "device", "buffers"])
@pytest.mark.parametrize("kw,msg", DN_BAD + DN_ORDER, ids=[",".join(f"{a}={b}" for a, b in k.items()) for k, _ in DN_BAD + DN_ORDER])
def test_filter_rejections_touch_nothing_and_come_in_the_documented_order(kw, msg, form):
    lib = _ffi.load()
    out = np.full((3, 4, 3), 0xABCD, dtype=np.uint64)
    rc = call_filter(lib, form, kw, out)
    err = lib.rt_last_error().decode()
    assert rc == -1 and msg in err and "denoise_var_given" in err, err
    assert (out == 0xABCD).all()


def test_the_filter_with_everything_names_the_workspace_then_the_context():
    lib = _ffi.load()
    out = np.full((3, 4, 3), 0xABCD, dtype=np.uint64)
    err = lambda: lib.rt_last_error().decode()
    assert call_filter(lib, "device", dict(feat_spp=0, work=None), out) == -1 and "feat_spp" in err()
    assert call_filter(lib, "device", dict(work=None), out) == -1 and "workspace is NULL" in err()
    assert call_filter(lib, "device", {}, out) == -1 and "ctx is NULL" in err()
    assert call_filter(lib, "buffers", {}, out) == -1 and "ctx is NULL" in err()
    assert (out == 0xABCD).all()
    assert call_filter(lib, "host", {}, out) == 0 and (out != 0xABCD).all()


# ---- the source layout ----

def test_the_new_kernels_are_pinned_and_the_old_ones_keep_their_lines():
    """tools/isa_fingerprint.py --temporal-var = profiles/isa_fingerprint_temporal_var.txt and names exactly the two new kernels;
    --denoise-var and --all print their pinned lines (the factored host function and the shared checks moved no machine code)."""
    def lines_of(flag):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), flag], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert run.returncode == 0, run.stderr[-2000:]
        return fingerprint_lines(run.stdout)
    for flag, name, kernels in (("--temporal-var", "isa_fingerprint_temporal_var.txt", 2), ("--denoise-var", "isa_fingerprint_denoise_var.txt", 5),
                                ("--all", "isa_fingerprint_source_split.txt", 49)):
        pinned = fingerprint_lines(open(os.path.join(ROOT, "profiles", name)).read())
        now = lines_of(flag)
        assert len(pinned) == kernels and sorted(now) == sorted(pinned), (flag, sorted(now))
        for kernel in pinned:
            assert now[kernel] == pinned[kernel], (flag, kernel, now[kernel], pinned[kernel])
        if flag == "--temporal-var":
            assert sorted(k.split("::")[-1] for k in now) == ["denoise_var_given_prepare_kernel", "temporal_var_kernel"]


def test_the_unit_is_built_and_reads_no_render_kernel():
    import inspect
    import __graft_entry__ as g
    src = inspect.getsource(g.build_hip_library)
    assert "denoise/rt_temporal_var.hip" in src and src.count(".hip\"") >= 13
    run = subprocess.run(["hipcc", "-MM", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                          os.path.join(CSRC, "denoise", "rt_temporal_var.hip")], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    deps = {os.path.basename(d) for d in run.stdout.replace("\\\n", " ").split() if not d.endswith(":")}
    assert {"rt_host.hpp", "rt_temporal_core.hpp", "rt_temporal_var_core.hpp", "rt_temporal_shared.hpp", "rt_denoise_var_core.hpp", "rt_denoise_shared.hpp"} <= deps
    assert not {"rt_kernels.hpp", "rt_launch.hpp", "rt_device.hpp", "rt_denoise_var.hip", "rt_temporal.hip"} & deps, sorted(deps)
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "denoise", "rt_temporal_var.hip")).read())      # (the comments say what is absent)
    assert "__shared__" not in code and "atomic" not in code and "asm" not in code


def test_the_kernels_use_no_scratch_memory_and_no_lds():
    """The compiler's own resource remarks for denoise/rt_temporal_var.hip with the product's flags (DESIGN.md section 26 reports registers and
    occupancy)."""
    import tempfile
    unit = os.path.join(CSRC, "denoise", "rt_temporal_var.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                              "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-c", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "temporal_var.o"), unit],
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
    assert len(rows) == 2, sorted(rows)
    for kind in ("temporal_var_kernel", "denoise_var_given_prepare_kernel"):
        found = [r for name, r in rows.items() if f"{kind}E" in name]
        assert len(found) == 1, kind
        r = found[0]
        print(kind, "VGPRs", r["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "SGPR spills", r["SGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["LDS Size [bytes/block]"]) == 0, (kind, r)


def test_core_headers_alone_under_asan_and_ubsan(tmp_path):
    """tests/temporal_var_san_main.cpp includes the two new core headers and nothing else of the library; the sanitizers watch it chain three
    frames and filter the last (buffers of exactly the size the contract may touch), and its checksum is numpy's."""
    assert shutil.which("g++")
    src = open(os.path.join(CSRC, "rt_temporal_var_core.hpp")).read()
    assert "#include <hip" not in src and re.findall(r"#include (\S+)", src) == ['"rt_temporal_core.hpp"']
    main = open(os.path.join(ROOT, "tests", "temporal_var_san_main.cpp")).read()
    assert re.findall(r'#include "(\S+)"', main) == ["rt_temporal_var_core.hpp", "rt_denoise_var_core.hpp"]
    assert re.findall(r"#include (\S+)", open(os.path.join(CSRC, "rt_denoise_var_core.hpp")).read()) == ['"rt_denoise_core.hpp"']
    exe = str(tmp_path / "temporal_var_san_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "temporal_var_san_main.cpp")], check=True, timeout=300)
    for (w, h), options, with_count, pair, levels, demodulate in (((5, 3), tr.OPTION_SETS[0], True, "subpixel_pan", 3, True),
                                                                  ((37, 19), tr.OPTION_SETS[0], False, "orbit_step", 4, True),
                                                                  ((37, 19), tr.OPTION_SETS[3], True, "fov", 5, False),
                                                                  ((2, 2), tr.OPTION_SETS[1], False, "identical", 2, True)):
        cur, prev = tr.camera_pairs(w, h)[pair]
        frames = []
        for k, cam in enumerate((prev, cur, prev)):
            fix, count, spp, feat, feat_spp = tr.synthetic_frame(w, h, 20 + k)
            frames.append((fix, count if with_count else None, spp, feat, feat_spp, cam))
        path = str(tmp_path / f"case_{w}x{h}_{pair}.bin")
        with open(path, "wb") as f:
            f.write(np.array([w, h, len(frames), frames[0][2], frames[0][4], rt.RT_TEMPORAL_CLAMP if options["clamp"] else 0, int(with_count), levels,
                              int(demodulate)], dtype="<i8").tobytes())
            f.write(np.array([options["alpha_min"], options["sigma_normal"], options["sigma_depth"], options["clamp_scale"], vr.SIGMA_COLOR, 1.0, 0.2],
                             dtype="<f8").tobytes())
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
            out, length, m2, var = tv.accumulate(fix, spp, feat, feat_spp, cam, history, count=count, **options)
            history = (out, length, feat, feat_spp, cam, m2)
        shown = tv.denoise_var_given(out, var, 1, feat, feat_spp, levels=levels, demodulate=demodulate)
        assert int(run.stdout.strip(), 16) == tv.checksum(out, length, m2, var, shown), (w, h, pair)


def test_the_cli_accepts_the_sequence_and_keeps_its_refusals(tmp_path, book1_flat):
    src = open(os.path.join(ROOT, "host", "rtiow_render.cpp")).read()
    assert "rt_temporal_var(" in src and "rt_denoise_var_given(" in src and "--temporal --denoise-variance" in src.split("#include")[0]
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    scene_file = str(tmp_path / "scene.bin")
    rt.save_scene(scene_file, book1_flat)
    base = [exe, "--scene", scene_file, "--width", "8", "--height", "8", "--out", str(tmp_path / "o.ppm")]
    for args, word in ((["--spp", "8", "--denoise-variance", "--orbit", "2"], "goes with none of"),
                       (["--spp", "8", "--denoise-variance", "--temporal"], "--temporal accumulates a frame batch"),
                       (["--spp", "8", "--denoise-variance", "--denoise", "--temporal", "--orbit", "2"], "give one of them"),
                       (["--spp", "8", "--temporal", "--orbit", "2", "--wavefront"], "go with none of"),
                       (["--spp", "8", "--temporal", "--denoise", "--orbit", "2", "--wavefront"], "go with none of"),
                       (["--spp", "8", "--temporal", "--denoise-variance", "--orbit", "2", "--sky", "0,0,0:0,0,0"], "they need --wavefront"),
                       (["--spp", "8", "--temporal", "--denoise-variance", "--orbit", "2", "--wavefront", "--direct"], "at least one --emit")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.returncode, bad.stderr)
    # accepted by the argument checks: what fails now is the device (here there may be none) or nothing at all, never a refusal's exit code
    for args in (["--spp", "7", "--temporal", "--denoise-variance", "--orbit", "2"],
                 ["--spp", "8", "--temporal", "--denoise-variance", "--cameras", str(tmp_path / "cams.bin")],
                 ["--spp", "8", "--temporal", "--denoise-variance", "--orbit", "2", "--wavefront"],
                 ["--spp", "8", "--temporal", "--denoise-variance", "--orbit", "2", "--wavefront", "--sky", "0,0,0:0,0,0", "--emit", "0:4,3.2,2.4",
                  "--direct-weighted"]):
        if "--cameras" in args:
            rt.save_cameras(str(tmp_path / "cams.bin"), rt.orbit_cameras(4, 8, 8)[:2])
        ok = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert ok.returncode in (0, 1) and "none of" not in ok.stderr and "give one" not in ok.stderr and "need" not in ok.stderr, (args, ok.returncode, ok.stderr)
