"""Diagnostic: the capped body of the dense kernel against the classic one (RTIOW_DENSE_BODY, read per launch), interleaved in ONE process on
ONE library and ONE context: the classic kernels are the parent commit's machine code (tools/isa_fingerprint.py).  Per configuration a warm-up
pair, then N (default 7) launches of each body alternating, in both orders (classic first / capped first); median kernel time from the library's
own HIP events.  Every launch fills the chip, so nothing in the rotation ends on an idle one.
usage: python tools/dense_body_ab.py [N] > profiles/capped_redraw_ab.txt"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa
import numpy as np
from rtiow_amd import _ffi
import rtiow_amd as rt
n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
lib = _ffi.load()
# (configuration, scene grid, width, height, spp, launches per body as a multiple of N: the sub-millisecond launch takes more)
CONFIGS = [("book 1200x675x500", (-11, 11), 1200, 675, 500, 1), ("book 1200x675x100", (-11, 11), 1200, 675, 100, 1),
           ("book 400x225x10", (-11, 11), 400, 225, 10, 8), ("10k spheres 1920x1080x256", (-50, 49), 1920, 1080, 256, 1),
           ("10k spheres 1920x1080x100", (-50, 49), 1920, 1080, 100, 1)]
print(f"# {lib.rt_backend_name().decode()}, source {lib.rt_build_source_sha().decode()}; median kernel ms of {n} launches per body and order ({8 * n} for 400x225x10), interleaved")
print(f"# {'configuration':28s} {'kernel_variant':>14s} {'order':>14s} {'classic ms':>11s} {'capped ms':>11s} {'capped/classic':>15s} {'min classic':>12s} {'min capped':>11s}")
scenes = {}
for name, grid, w, h, spp, mult in CONFIGS:
    if grid not in scenes:
        scenes[grid] = np.ascontiguousarray(rt.random_scene(1, grid=grid).flatten(), dtype=rt.SPHERE_DTYPE)
    flat = scenes[grid]
    hctx = C.c_void_p()
    assert lib.rt_create(0, C.byref(hctx)) == 0
    assert lib.rt_upload_scene(hctx, flat.ctypes.data_as(C.POINTER(_ffi.rt_sphere)), len(flat)) == 0
    cam = rt.book1_camera(w, h).to_rt_camera()
    p = rt.make_params(w, h, spp)
    out = np.zeros((h, w, 3), dtype=np.float32)
    st = _ffi.rt_stats()
    rays = {}
    for order in (("classic", "capped"), ("capped", "classic")):
        ts = {"classic": [], "capped": []}
        for rnd in range(n * mult + 1):
            for body in order:
                os.environ["RTIOW_DENSE_BODY"] = body
                assert lib.rt_render(hctx, C.byref(cam), C.byref(p), out.ctypes.data_as(C.c_void_p), None, C.byref(st)) == 0
                assert lib.rt_last_dense_body(hctx) == (1 if body == "capped" else 0)
                rays.setdefault(body, st.rays_traced)
                assert rays[body] == st.rays_traced
                if rnd:
                    ts[body].append(st.kernel_ms)
        a, b = statistics.median(ts["classic"]), statistics.median(ts["capped"])
        print(f"  {name:28s} {st.kernel_variant:14d} {order[0] + ' first':>14s} {a:11.3f} {b:11.3f} {100.0 * (b / a - 1.0):+14.2f}% {min(ts['classic']):12.3f} {min(ts['capped']):11.3f}")
    assert rays["classic"] == rays["capped"]
    lib.rt_destroy(hctx)
os.environ.pop("RTIOW_DENSE_BODY", None)
