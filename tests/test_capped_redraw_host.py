"""The capped unit-sphere redraw without a GPU (rt_kernels.hpp, ITEMS = kItemBlockDense / kItemBlockDenseLarge):

* the stream contract makes the resume stateless: "four tries, else ev += 3 and start again" ends with the same accepted words and
  the same event counter as the unbounded loop, for every key -- checked in pure Python on the Philox of rtiow_amd/philox.py with
  the 32-bit acceptance rule of rt_device.hpp (unit_sphere_accepts), on keys that include two and three parks in a row;
* the four kernels of rt_dense.hip are held to profiles/isa_fingerprint_capped_redraw.txt (names, counts, hashes), and compiling
  them leaves the kernels of rt_api.hip and rt_frames.hip what they were;
* rt_last_dense_body is bound outside the C ABI of rtiow_hip.h."""
import os
import re
import subprocess
import sys

import rtiow_amd as rt  # noqa: F401
from rtiow_amd import _ffi
from rtiow_amd.philox import philox4x32_10
from isa_pins import fingerprint_lines as _fingerprint_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = (0x2545F491, 0x9E3779B1)


def _i32(w):
    return w - (1 << 32) if w & 0x80000000 else w


def accepts(wx, wy, wz):
    """rt_device.hpp unit_sphere_accepts: the integer sum of squares decides, the f64 expression of vec3.rs:87-89 only in the band."""
    x, y, z = _i32(wx), _i32(wy), _i32(wz)
    hi = (x * x + y * y + z * z) >> 32
    if hi < 0x3FFFFFFF:
        return True
    if hi - 0x3FFFFFFF < 2:
        fx, fy, fz = x / 2147483648.0, y / 2147483648.0, z / 2147483648.0
        return fx * fx + fy * fy + fz * fz < 1.0
    return False


class Blocks:
    """Block e of the stream of (pixel, sample): philox(pixel, sample, e, 0), cached and counted."""

    def __init__(self, pixel, sample):
        self.pixel, self.sample, self.cache = pixel, sample, {}

    def __call__(self, e):
        if e not in self.cache:
            self.cache[e] = philox4x32_10((self.pixel, self.sample, e & 0xFFFFFFFF, 0), KEY)
        return self.cache[e]


def unbounded(blk, ev):
    """The classic body's loop (rt_kernels.hpp PHASE 4), statement for statement: -> (accepted words, final ev, rejected tries)."""
    w = blk(ev)
    tx, ty, tz, nblk, rejected = w[0], w[1], w[2], 1, 0
    ok = accepts(tx, ty, tz)
    if not ok:
        c0 = w[3]
        while not ok:
            b = blk(ev + nblk); nblk += 1
            tx, ty, tz = c0, b[0], b[1]; rejected += 1                  # try 4m+1
            ok = accepts(tx, ty, tz)
            if not ok:
                c1, c2 = b[2], b[3]
                b = blk(ev + nblk); nblk += 1
                tx, ty, tz = c1, c2, b[0]; rejected += 1                # try 4m+2
                ok = accepts(tx, ty, tz)
                if not ok:
                    tx, ty, tz = b[1], b[2], b[3]; rejected += 1        # try 4m+3
                    ok = accepts(tx, ty, tz)
                    if not ok:
                        b = blk(ev + nblk); nblk += 1
                        tx, ty, tz, c0 = b[0], b[1], b[2], b[3]; rejected += 1   # try 4m+4
                        ok = accepts(tx, ty, tz)
    return (tx, ty, tz), ev + nblk, rejected


def capped_pass(blk, ev):
    """One pass of the capped body: -> (accepted words or None when the lane parks, ev after the pass)."""
    w = blk(ev)
    t, nblk = (w[0], w[1], w[2]), 1
    ok = accepts(*t)
    if not ok:
        b = blk(ev + 1); nblk = 2
        t = (w[3], b[0], b[1])
        ok = accepts(*t)
        if not ok:
            c1, c2 = b[2], b[3]
            b = blk(ev + 2); nblk = 3
            t = (c1, c2, b[0])
            ok = accepts(*t)
            if not ok:
                t = (b[1], b[2], b[3])
                ok = accepts(*t)
    return (t if ok else None), ev + nblk


def capped(blk, ev):
    parks = 0
    while True:
        t, ev = capped_pass(blk, ev)
        if t is not None:
            return t, ev, parks
        parks += 1


def test_four_tries_then_resume_is_the_unbounded_schedule():
    """40 000 keys (pixel, sample, ev) in a fixed order; every one of them through both schedules.  A try is accepted with
    probability pi/6, so 8 rejections in a row (two parks) happen about 2.6 times and 12 (three parks) about 0.14 times per
    thousand keys: the set holds dozens of the first kind and several of the second, asserted below."""
    two = three = total_parks = 0
    n = 0
    for pixel in range(400):
        for k in range(100):
            sample = (k * 7919 + pixel) & 0x7FFFFFFF
            ev = 1 + (pixel * 31 + k * 3) % 97
            blk = Blocks(pixel * 2654435761 & 0xFFFFFFFF, sample)
            t_u, ev_u, rejected = unbounded(blk, ev)
            t_c, ev_c, parks = capped(blk, ev)
            assert t_c == t_u and ev_c == ev_u, (pixel, sample, ev, rejected, parks)
            assert parks == rejected // 4                                   # a park per four rejected tries, nothing else
            # the words of the accepted try are words 3T .. 3T + 2 of the concatenated blocks ev, ev + 1, ...: no word skipped or reused
            stream = [x for e in range(ev, ev_u) for x in blk(e)]
            assert tuple(stream[3 * rejected:3 * rejected + 3]) == t_u and ev_u - ev == (3 * rejected + 2) // 4 + 1
            two += parks >= 2
            three += parks >= 3
            total_parks += parks
            n += 1
    assert n == 40000 and two >= 40 and three >= 2, (two, three)
    # (0.4764^4 = 5.15 % of the scatters park at least once: 2 060 +- 5 sigma of 45)
    assert 1800 < total_parks < 2500, total_parks


NEW = ["void rt::render_kernel<5, false, false, false, -1024>", "void rt::render_kernel<5, false, false, false, -768>",
       "void rt::render_kernel<5, false, true, false, -1024>", "void rt::render_kernel<5, false, true, false, -768>"]


def test_the_capped_kernels_keep_their_machine_code_and_add_nothing_elsewhere():
    """tools/isa_fingerprint.py --frames --dense = the committed profiles/isa_fingerprint_capped_redraw.txt, line for line: the 20
    kernels of rt_api.hip and rt_frames.hip as profiles/isa_fingerprint_after_frame_batches.txt has them, and the four of rt_dense.hip.
    The two small-grid ones are one machine code (as the classic pair is): the block size is a launch parameter there."""
    pinned = _fingerprint_lines(open(os.path.join(ROOT, "profiles", "isa_fingerprint_capped_redraw.txt")).read())
    before = _fingerprint_lines(open(os.path.join(ROOT, "profiles", "isa_fingerprint_after_frame_batches.txt")).read())
    assert len(before) == 20 and {k: v for k, v in pinned.items() if k in before} == before
    assert sorted(set(pinned) - set(before)) == NEW
    assert pinned[NEW[2]] == pinned[NEW[3]] and pinned[NEW[0]] != pinned[NEW[1]]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--frames", "--dense"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    now = _fingerprint_lines(run.stdout)
    assert now == pinned, sorted(set(now.items()) ^ set(pinned.items()))
    # fewer instructions than the classic kernel of the same shape: the loop and its carried word are gone
    count = lambda line: int(re.match(r"n=\s*(\d+)", line).group(1))
    for new, old in ((NEW[2], "void rt::render_kernel<5, false, true, false, 1024>"), (NEW[1], "void rt::render_kernel<5, false, false, false, 256>"),
                     (NEW[0], "void rt::render_kernel<5, false, false, false, 1024>")):
        assert count(pinned[new]) < count(pinned[old]), (new, old)


def test_the_diagnostic_is_bound_outside_the_c_abi():
    lib = _ffi.load()
    assert [n for n, _, _ in _ffi.DIAG_SYMBOLS] == ["rt_last_dense_body"]
    assert "rt_last_dense_body" not in [n for n, _, _ in _ffi.SYMBOLS]
    assert "rt_last_dense_body" not in open(os.path.join(ROOT, "include", "rtiow_hip.h")).read().split("diagnostic knobs")[0]
    assert "rt_last_dense_body" in open(os.path.join(ROOT, "include", "rtiow_hip_diag.h")).read()
    assert lib.rt_last_dense_body(None) == -1 and lib.rt_abi_version() == 5
