#!/usr/bin/env python3
"""What the first-hit feature kernel costs (profiles/features.txt).  Needs an MI355X.

For each frame: the kernel time of the feature kernel (rt_render_features' kernel_ms: the pair of HIP events the library records
around the launch inside the call) beside the yardstick, rt_render_device with max_depth = 1 on the same frame (kernel time of
rt_last_stats: the pair of HIP events the library records around the render kernel) -- the megakernel tracing the very same camera
rays, the only way to reach them without this feature.  Both pairs are recorded from C right before and after the launch, so
neither holds Python's call overhead.  REPS repetitions (default 24) after a warm-up, the two ALTERNATED within a repetition in one
process; median, minimum, maximum and spread = (max - min) / median of identical runs.

--counts: with the diagnostic library built with -DRT_FEATURES_COUNT --
    python -c "import __graft_entry__ as g; g.build_hip_library(count_features=True)"     # -> tools/lib_features_count.so
    RTIOW_HIP_LIB=tools/lib_features_count.so tools/features_bench.py --counts
-- one launch per frame and the kernel's counters instead of times: tiles scanned and columns kept per wave-sample (= exact tests every
lane ran), against the tests that found a root.

usage: tools/features_bench.py [--reps N] [--out FILE] [--counts]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import rtiow_amd as rt  # noqa: E402


def fmt(xs):
    med = statistics.median(xs)
    return f"{med:8.3f} ms (min {min(xs):.3f}, max {max(xs):.3f}, spread {100 * (max(xs) - min(xs)) / med:.1f} %)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--counts", action="store_true")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/features_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}, library built from kernel sources {rt._ffi.load().rt_build_source_sha().decode()}")
    out("# feature kernel (rt_render_features, its kernel_ms) against the megakernel on the same camera rays (rt_render_device, max_depth = 1, rt_last_stats); kernel times, HIP events recorded by the library around each launch")
    lib = rt._ffi.load()
    if a.counts and not hasattr(lib, "rt_debug_features_counts"):
        sys.exit("--counts needs a library built with -DRT_FEATURES_COUNT (RTIOW_HIP_LIB)")
    stream = torch.cuda.Stream()
    cases = (("book scene", rt.random_scene(1).flatten(), 1200, 675, (1, 4, 16)),
             ("10k scene", rt.random_scene(1, grid=(-50, 49)).flatten(), 1920, 1080, (1, 4)))
    for name, flat, w, h, spps in cases:
        with rt.Renderer(0) as r:
            r.upload_scene(flat)
            (grid_dim, n_global), _, slots = rt.tile_layout_host(flat)
            out(f"{name}: {len(flat)} spheres, grid {grid_dim} x {grid_dim}, {n_global} global tiles, {len(slots) // 32} tiles; {w}x{h}")
            cam = rt.book1_camera(w, h)
            d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            for spp in spps:
                p = rt.make_params(w, h, spp)
                p1 = rt.make_params(w, h, spp, max_depth=1)

                def features():
                    return r.render_features(cam, p, want_ids=True)

                def dense():
                    r.render_device(cam, p1, d_fix.data_ptr(), stream.cuda_stream)
                    stream.synchronize()
                    return r.last_stats()["kernel_ms"]

                if a.counts:
                    import ctypes as C
                    c = (C.c_uint64 * 8)()
                    lib.rt_debug_features_counts(r._h, c)             # (zeroes them)
                    features()
                    assert lib.rt_debug_features_counts(r._h, c) == 0
                    ws, tiles, cols, lanes, roots = (int(c[k]) for k in range(5))
                    out(f"  spp {spp:2d}: {ws} wave-samples; per wave-sample {tiles / ws:.2f} tiles scanned, {cols / ws:.2f} columns kept = exact tests run by each of "
                        f"{lanes / ws:.1f} lanes ({cols / ws * lanes / ws:.0f} lane-tests), of which {roots / ws:.1f} found a root >= t_min")   # (roots: the always-exact spheres every lane tests included)
                    continue
                for _ in range(3):
                    features()
                    dense()
                tf, td = [], []
                for _ in range(a.reps):
                    feat, _, ms = features()
                    tf.append(ms)
                    td.append(dense())
                mf, md = statistics.median(tf), statistics.median(td)
                spread = max((max(tf) - min(tf)) / mf, (max(td) - min(td)) / md)
                hits = int(feat[..., 7].sum())
                out(f"  spp {spp:2d}: features {fmt(tf)}   depth-1 render {fmt(td)}   features / render = {mf / md:.3f} "
                    f"(larger spread {100 * spread:.1f} %); {w * h * spp / mf / 1e6:.2f} Gray/s; alpha of the frame {hits / (w * h * spp):.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
