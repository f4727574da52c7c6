"""Diagnostic (not a test): loads the -DRT_BLOCK_COUNTS -DRT_COUNT_PARKS build (tools/build_diag_libs.sh -> tools/lib_counts_parks.so, or RTIOW_LIB)
and prints, for the classic and the capped body of the dense kernel on 1200x675 x SPP (default 500): bounce-loop passes, unit-sphere redraw
blocks executed per pass after the shared first one (wave level), and the lanes that park per pass."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa
from rtiow_amd import _ffi
_ffi.LIB_PATH = os.environ.get("RTIOW_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib_counts_parks.so"))
import rtiow_amd as rt
r = rt.Renderer(0)
r.upload_scene(rt.random_scene(1).flatten())
w, h, spp = 1200, 675, int(os.environ.get("SPP", "500"))
r._lib.rt_debug_phase_cycles.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
for body in ("classic", "capped"):
    os.environ["RTIOW_DENSE_BODY"] = body
    sm, fix, st = r.render(rt.book1_camera(w, h), rt.make_params(w, h, spp), want_fix=False)
    out = (C.c_ulonglong * 8)()
    r._lib.rt_debug_phase_cycles(r._h, out)
    print(f"{body:8s} body {r._lib.rt_last_dense_body(r._h)} variant {st['kernel_variant']}: kernel {st['kernel_ms']:.2f} ms (counting build), rays {st['rays_traced']}, "
          f"passes {out[0]}, redraw blocks {out[6]} = {out[6] / max(1, out[0]):.3f} per pass, parked lanes {out[1]} = {out[1] / max(1, out[0]):.3f} per pass, "
          f"lanes per pass {(st['rays_traced'] + out[1]) / max(1, out[0]):.2f}")
r.close()
