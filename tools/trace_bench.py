#!/usr/bin/env python3
"""What a ray query costs (profiles/trace.txt).  Needs an MI355X.

Ray sets, made on the device with torch, on the book scene and the 10k-sphere scene of `bench.py --full`:
  A  the camera rays of a 1200 x 675 frame, 16 jitters per pixel (12.96 M rays; order [jitter][row][column]: a wave holds 64 neighbouring
     pixels of one row), from the camera formula (camera.rs:47-54) with torch's own seeded random numbers;
  B  their bounce-1 rays, in order: from A's hit points along normal + a seeded unit vector, the rays whose parent missed dropped --
     what a wavefront integrator holds after one bounce;
  C  B under a fixed random permutation;
  D  C with t_max = 0.5, for occlusion.
Every time is a pair of device events around ONE launch of the device form on a torch stream; a warm-up, then REPS (default 24)
repetitions with the kernels under comparison ALTERNATED within a repetition in one process; median, minimum, maximum and spread =
(max - min) / median.
  1. Set A, outputs index + t, both candidate schemes, beside features_kernel at 16 spp on the same frame (rt_render_features_device)
     plus the query's own streaming time, 68 bytes per ray (48 in, 12 out, 8 for t_max were it given) at 6.3 TB/s: the no-overlap bound.
  2. Sets B and C, both schemes; for scale only the dense render's rays_traced / kernel_ms on the same scene (that kernel also shades).
  3. Set D: occlusion against closest hit on the same rays.

--counts: with the diagnostic library built with -DRT_TRACE_COUNT --
    python -c "import __graft_entry__ as g; g.build_hip_library(count_trace=True)"     # -> tools/lib_trace_count.so
    RTIOW_HIP_LIB=tools/lib_trace_count.so tools/trace_bench.py --counts
-- one launch per set and scheme and the kernel's counters instead of times: tiles scanned and exact tests per wave.

usage: tools/trace_bench.py [--reps N] [--out FILE] [--counts] [--scenes book,tenk]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import rtiow_amd as rt  # noqa: E402

W, H, JITTERS = 1200, 675, 16
STREAM_BYTES, HBM_RATE = 68, 6.3e12


def fmt(xs):
    med = statistics.median(xs)
    return f"{med:8.3f} ms (min {min(xs):.3f}, max {max(xs):.3f}, spread {100 * (max(xs) - min(xs)) / med:.1f} %)"


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def camera_rays(cam, gen):
    """Camera::get_ray for every (jitter, pixel): f64 tensors [n, 3] on the device."""
    c = cam.to_rt_camera()
    v3 = lambda name: torch.tensor(list(getattr(c, name)), dtype=torch.float64, device="cuda")
    i = torch.arange(W, dtype=torch.float64, device="cuda").view(1, 1, W)
    j = torch.arange(H, dtype=torch.float64, device="cuda").view(1, H, 1)
    shape = (JITTERS, H, W)
    u = ((i + torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)) / (W - 1)).reshape(-1, 1)
    v = ((j + torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)) / (H - 1)).reshape(-1, 1)
    ang = torch.rand((u.shape[0], 1), dtype=torch.float64, device="cuda", generator=gen) * (2.0 * torch.pi)
    rad = torch.rand((u.shape[0], 1), dtype=torch.float64, device="cuda", generator=gen).sqrt() * c.lens_radius
    offset = v3("u") * (rad * ang.cos()) + v3("v") * (rad * ang.sin())
    o = v3("origin") + offset
    d = v3("lower_left_corner") + u * v3("horizontal") + v * v3("vertical") - v3("origin") - offset
    return o.contiguous(), d.contiguous()


def unit_vectors(n, gen):
    x = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    return x / x.norm(dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--scenes", default="book,tenk")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    lib = rt._ffi.load()
    if a.counts and not hasattr(lib, "rt_debug_trace_counts"):
        sys.exit("--counts needs a library built with -DRT_TRACE_COUNT (RTIOW_HIP_LIB)")
    out(f"# tools/trace_bench.py --reps {a.reps}{' --counts' if a.counts else ''}: {torch.cuda.get_device_name(0)}")
    stream = torch.cuda.Stream()
    scenes = {"book": ("book scene", lambda: rt.random_scene(1).flatten()), "tenk": ("10k scene", lambda: rt.random_scene(1, grid=(-50, 49)).flatten())}
    for key in a.scenes.split(","):
        name, make = scenes[key]
        flat = make()
        with rt.Renderer(0) as r:
            r.upload_scene(flat)
            (grid_dim, n_global), _, slots = rt.tile_layout_host(flat)
            out(f"{name}: {len(flat)} spheres, grid {grid_dim} x {grid_dim}, {n_global} global tiles, {len(slots) // 32} tiles; {W}x{H}, {JITTERS} jitters")
            cam = rt.book1_camera(W, H)
            gen = torch.Generator(device="cuda").manual_seed(1)
            oa, da = camera_rays(cam, gen)
            n_a = oa.shape[0]
            first = rt.trace_rays_torch(r, oa, da, want=("point", "normal"))
            torch.cuda.synchronize()
            hit = first["index"] >= 0
            ob = first["point"][hit].contiguous()
            db = (first["normal"][hit] + unit_vectors(int(hit.sum()), gen)).contiguous()
            perm = torch.randperm(ob.shape[0], device="cuda", generator=gen)
            oc, dc = ob[perm].contiguous(), db[perm].contiguous()
            td = torch.full((oc.shape[0],), 0.5, dtype=torch.float64, device="cuda")
            del first
            out(f"  A {n_a} camera rays, {int(hit.sum())} of them hit; B / C / D {ob.shape[0]} bounce-1 rays")
            sets = {"A": (oa, da, None), "B": (ob, db, None), "C": (oc, dc, None), "D": (oc, dc, td)}
            index = torch.empty(n_a, dtype=torch.int32, device="cuda")
            t = torch.empty(n_a, dtype=torch.float64, device="cuda")
            occ = torch.empty(n_a, dtype=torch.uint8, device="cuda")

            def launch(which, scheme, any_hit=False):
                o, d, tm = sets[which]
                os.environ["RTIOW_TRACE_CANDIDATES"] = scheme
                if any_hit:
                    r.occluded_device(o.shape[0], o.data_ptr(), d.data_ptr(), occ.data_ptr(), tm.data_ptr() if tm is not None else 0, 1e-4, stream.cuda_stream)
                else:
                    r.trace_rays_device(o.shape[0], o.data_ptr(), d.data_ptr(), index.data_ptr(), tm.data_ptr() if tm is not None else 0, 1e-4,
                                        t.data_ptr(), 0, 0, 0, stream.cuda_stream)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)

            if a.counts:
                import ctypes as C
                c = (C.c_uint64 * 8)()
                for which in ("A", "B", "C", "D"):
                    for scheme in ("wave", "ray"):
                        lib.rt_debug_trace_counts(r._h, c)                  # (zeroes them)
                        launch(which, scheme, any_hit=which == "D")
                        stream.synchronize()
                        assert lib.rt_debug_trace_counts(r._h, c) == 0
                        waves, tiles, tests, lanes, roots = (int(c[k]) for k in range(5))
                        out(f"  set {which} {scheme:4s}{' occluded' if which == 'D' else ''}: {waves} waves; per wave {tiles / waves:.2f} tiles scanned, "
                            f"{tests / waves:.1f} exact tests (lane, column), {lanes / waves:.1f} lanes in range, {roots / waves:.1f} tests with a root >= t_min")
                continue

            # 1. set A against the feature kernel on the same frame
            p16 = rt.make_params(W, H, JITTERS)
            d_feat = torch.zeros((H, W, 8), dtype=torch.int64, device="cuda")
            feats = lambda: r.render_features_device(cam, p16, d_feat.data_ptr(), 0, stream.cuda_stream)
            runs = {"features": feats, "A wave": lambda: launch("A", "wave"), "A ray": lambda: launch("A", "ray")}
            times = {k: [] for k in runs}
            for rep in range(3 + a.reps):
                for k, fn in runs.items():
                    ms = timed(fn)
                    if rep >= 3:
                        times[k].append(ms)
            stream_ms = n_a * STREAM_BYTES / HBM_RATE * 1e3
            mf = statistics.median(times["features"])
            out(f"  1. features_kernel 16 spp {fmt(times['features'])} = {n_a / mf / 1e6:.2f} Gray/s; streaming {STREAM_BYTES} B/ray at 6.3 TB/s = {stream_ms:.3f} ms; "
                f"no-overlap bound {mf + stream_ms:.3f} ms")
            for k in ("A wave", "A ray"):
                m = statistics.median(times[k])
                out(f"     set {k:6s} index + t {fmt(times[k])} = {n_a / m / 1e6:.2f} Gray/s; / bound = {m / (mf + stream_ms):.3f} "
                    f"(larger spread {100 * max(spread(times[k]), spread(times['features'])):.1f} %); its own traffic at that rate {n_a * 60 / m / 1e9:.2f} TB/s")
            # 2. sets B and C
            for which in ("B", "C"):
                n = sets[which][0].shape[0]
                tw, tr_ = [], []
                for rep in range(3 + a.reps):
                    w_ms, r_ms = timed(lambda: launch(which, "wave")), timed(lambda: launch(which, "ray"))
                    if rep >= 3:
                        tw.append(w_ms); tr_.append(r_ms)
                mw, mr = statistics.median(tw), statistics.median(tr_)
                out(f"  2. set {which} wave {fmt(tw)} = {n / mw / 1e6:.2f} Gray/s;  ray {fmt(tr_)} = {n / mr / 1e6:.2f} Gray/s;  ray / wave = {mr / mw:.3f} "
                    f"(larger spread {100 * max(spread(tw), spread(tr_)):.1f} %)")
            d_fix = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda")
            r.render_device(cam, p16, d_fix.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            st = r.last_stats()
            out(f"     for scale only (it also shades): dense render 16 spp {st['rays_traced']} rays in {st['kernel_ms']:.3f} ms = {st['rays_traced'] / st['kernel_ms'] / 1e6:.2f} Gray/s")
            # 3. set D: occlusion against closest hit
            n = oc.shape[0]
            res = {}
            for scheme in ("wave", "ray"):
                tc, to = [], []
                for rep in range(3 + a.reps):
                    c_ms, o_ms = timed(lambda: launch("D", scheme)), timed(lambda: launch("D", scheme, any_hit=True))
                    if rep >= 3:
                        tc.append(c_ms); to.append(o_ms)
                res[scheme] = (tc, to)
                out(f"  3. set D {scheme:4s} closest {fmt(tc)} = {n / statistics.median(tc) / 1e6:.2f} Gray/s;  occluded {fmt(to)} = {n / statistics.median(to) / 1e6:.2f} Gray/s;  "
                    f"occluded / closest = {statistics.median(to) / statistics.median(tc):.3f}; {int(occ[:n].sum())} of {n} occluded")
    os.environ.pop("RTIOW_TRACE_CANDIDATES", None)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
