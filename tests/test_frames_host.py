"""Frame batches without a GPU: the argument validation of the three entry points (every limit names itself in rt_last_error,
checked before a context is needed), the camera file (save_cameras / load_cameras, and host/rtiow_render --dump-cameras writing
the bytes of orbit_cameras), and the proof that the frame-batch kernel variant left every existing kernel's machine code alone
(tools/isa_fingerprint.py against the parent commit's output, profiles/isa_fingerprint_before_frame_batches.txt)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rtiow_amd as rt
from rtiow_amd import _ffi
from isa_pins import fingerprint_lines as _fingerprint_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _ffi.load().rt_last_error().decode()


@pytest.mark.parametrize("n_frames,stride,kw,msg", [
    (3, 0, dict(flags=_ffi.RT_FLAG_UNIFORM53), "RT_FLAG_UNIFORM53"),
    (3, 0, dict(flags=_ffi.RT_FLAG_DIAG_STATS), "RT_FLAG_DIAG_STATS"),
    (3, 0, dict(flags=_ffi.RT_FLAG_NO_FILTER), "RT_FLAG_NO_FILTER"),
    (3, 0, dict(flags=0x20), "unknown flags 0x20"),
    (3, 0, dict(shard_count=2), "shard_count must be 1"),
    (-1, 0, dict(), "n_frames must be >= 0"),
    (3, -1, dict(), "sample_stride must be >= 0"),
    (2 ** 31 // (16 * 9) + 1, 0, dict(), "pixels in one batch: at most 2^31"),
    (3, 2 ** 30, dict(sample_begin=10), "sample indices must stay below 2^31"),
    (2, 2 ** 31 - 40, dict(sample_begin=8), "sample indices must stay below 2^31"),
    (1, 0, dict(sample_begin=2 ** 31 - 32), "spp/sample_begin"),
    (2 ** 31 // (16 * 9), 0, dict(spp=2000), "work blocks in one batch: at most 2^31 - 1"),
    (3, 0, dict(), "ctx is NULL"),
    (0, 0, dict(), "ctx is NULL"),
    (2 ** 31 // (16 * 9), 0, dict(spp=1), "ctx is NULL"),              # exactly 2^31 pixels (virtual pixel numbers < 2^32) pass the limits
    (2, 2 ** 31 - 41, dict(sample_begin=8), "ctx is NULL"),            # the last sample index is 2^31 - 2
])
def test_every_limit_names_itself_before_a_context_is_needed(n_frames, stride, kw, msg):
    lib = _ffi.load()
    spp = kw.pop("spp", 32)
    p = rt.make_params(16, 9, spp, **kw)
    cams = rt.cameras_to_array(rt.orbit_cameras(2, 16, 9))
    out = np.full(64, 77, dtype=np.uint64)
    cp, op = cams.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for fn, extra in ((lib.rt_render_frames_device, (op, None)), (lib.rt_render_frames, (op, None)), (lib.rt_render_frames_rgba8, (1, op, None))):
        assert fn(None, cp, n_frames, stride, C.byref(p), *extra) == -1
        assert msg in _err(), (fn.__name__, _err())
    assert (out == 77).all()


def test_null_arguments_are_errors_not_crashes():
    lib = _ffi.load()
    assert lib.rt_render_frames_device(None, None, 0, 0, None, None, None) == -1 and "params is NULL" in _err()
    assert lib.rt_render_frames(None, None, 0, 0, None, None, None) == -1
    assert lib.rt_render_frames_rgba8(None, None, 0, 0, None, 1, None, None) == -1
    assert lib.rt_abi_version() == 5 and _ffi.RT_FLAG_KNOWN == 0x1f


def test_camera_file_round_trip_and_a_wrong_length_is_refused(tmp_path):
    w, h = 97, 55
    cams = rt.orbit_cameras(7, w, h) + [rt.book1_camera(w, h)]
    path = str(tmp_path / "cams.bin")
    rt.save_cameras(path, cams)
    assert os.path.getsize(path) == 8 * 152 and C.sizeof(_ffi.rt_camera) == 152
    back = rt.load_cameras(path)
    assert back.shape == (8, 19) and back.dtype == np.float64
    assert np.array_equal(back, rt.cameras_to_array(cams))
    # the records are rt_camera's own layout
    raw = open(path, "rb").read()
    for f, cam in enumerate(cams):
        assert raw[152 * f:152 * (f + 1)] == bytes(cam.to_rt_camera())
    # frame 0 of an orbit is the book camera; a quarter turn later look_from is (3, 2, -13)
    assert np.array_equal(back[0], back[7])
    assert np.allclose(rt.orbit_cameras(4, w, h)[1].origin, (3.0, 2.0, -13.0), atol=1e-12)
    rt.save_cameras(path, back[:3])                                     # arrays are accepted as well
    assert np.array_equal(rt.load_cameras(path), back[:3])
    with open(path, "ab") as f:
        f.write(b"\0" * 8)
    with pytest.raises(ValueError, match="152-byte"):
        rt.load_cameras(path)


def test_cli_dumps_the_cameras_the_python_mirror_builds(tmp_path):
    exe = os.path.join(ROOT, "host", "rtiow_render")
    if not os.path.exists(exe):
        pytest.fail("host/rtiow_render has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    for n, w, h in ((5, 97, 55), (12, 200, 133), (1, 16, 9)):
        path = str(tmp_path / f"orbit{n}.bin")
        run = subprocess.run([exe, "--orbit", str(n), "--width", str(w), "--height", str(h), "--dump-cameras", path], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, run.stderr
        want = rt.cameras_to_array(rt.orbit_cameras(n, w, h))
        assert open(path, "rb").read() == want.tobytes(), (n, w, h)
    # the batch options say what they do not go with, as --adaptive does; a camera file of a wrong length is refused
    bad = str(tmp_path / "bad.bin")
    open(bad, "wb").write(b"\0" * 100)
    run = subprocess.run([exe, "--cameras", bad, "--out", str(tmp_path / "x")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "152-byte" in run.stderr
    for extra in (["--passes", "2"], ["--adaptive", "0.05"], ["--uniform53"], ["--two-calls"], ["--devices", "0"]):
        run = subprocess.run([exe, "--orbit", "3", *extra], capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "go with none of" in run.stderr, extra


# ---- the existing kernels' machine code --------------------------------------------------------------------------------

def test_frame_batches_leave_every_existing_kernel_alone():
    """A fresh run of tools/isa_fingerprint.py (its default output: the kernels of rt_api.hip) equals, line for line, what the tool
    printed on a checkout of the PARENT commit: 18 kernels, none added, none changed.  The frame-batch instantiations are compiled
    from rt_frames.hip and show only with --frames: they are the two lines profiles/isa_fingerprint_after_frame_batches.txt adds."""
    before = _fingerprint_lines(open(os.path.join(ROOT, "profiles", "isa_fingerprint_before_frame_batches.txt")).read())
    assert len(before) == 18 and before["void rt::render_kernel<5, false, true, false, 256>"].endswith("ops-sha=b7a4e26be357")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    now = _fingerprint_lines(run.stdout)
    assert now == before, sorted(set(now.items()) ^ set(before.items()))
    after = _fingerprint_lines(open(os.path.join(ROOT, "profiles", "isa_fingerprint_after_frame_batches.txt")).read())
    assert {k: v for k, v in after.items() if k in before} == before
    assert sorted(set(after) - set(before)) == ["void rt::render_kernel<5, false, false, false, -512>", "void rt::render_kernel<5, false, true, false, -512>"]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--frames"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    assert _fingerprint_lines(run.stdout) == after
