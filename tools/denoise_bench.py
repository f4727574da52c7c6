#!/usr/bin/env python3
"""What the denoiser costs (profiles/denoise.txt).  Needs an MI355X.

For each frame, everything on the device and in one process: the time of a whole denoise (rt_denoise_device, 4 levels: prepare, four
box means, four level kernels, finish) beside the yardstick, the two launches whose output it consumes -- rt_render_device at 8 spp
and rt_render_features_device at 8 spp.  Every figure is the time between two events recorded on the stream right before and after
the call (so a figure holds the call's launches and the gaps between them, not Python's overhead before the first one); the three are
ALTERNATED within a repetition; REPS repetitions (default 24) after a warm-up; median, minimum, maximum and spread = (max - min) /
median of identical runs.

Then the two forms of the level kernel per level (RTIOW_DENOISE_LEVEL_KERNEL=gather|tile, read per call): a denoise of L levels minus
a denoise of L - 1 levels is the cost of level L - 1 (its box mean, the same in both, and its level kernel), both measured with the
same form; medians of REPS alternated runs.

usage: tools/denoise_bench.py [--reps N] [--levels L] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import rtiow_amd as rt  # noqa: E402

KNOB = "RTIOW_DENOISE_LEVEL_KERNEL"


def fmt(xs):
    med = statistics.median(xs)
    return f"{med:8.3f} ms (min {min(xs):.3f}, max {max(xs):.3f}, spread {100 * (max(xs) - min(xs)) / med:.1f} %)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--levels", type=int, default=6, help="per-level table: levels 0 .. L - 1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/denoise_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}, library built from kernel sources {rt._ffi.load().rt_build_source_sha().decode()}")
    out("# times between two events on the stream around each call; render = rt_render_device 8 spp, features = rt_render_features_device 8 spp, "
        "denoise = rt_denoise_device 4 levels, sigmas 0.35 / 1.0 / 0.2, demodulated")
    os.environ.pop(KNOB, None)
    stream = torch.cuda.Stream()
    cases = (("book scene", rt.random_scene(1).flatten(), 1200, 675), ("10k scene", rt.random_scene(1, grid=(-50, 49)).flatten(), 1920, 1080))
    for name, flat, w, h in cases:
        with rt.Renderer(0) as r:
            r.upload_scene(flat)
            cam = rt.book1_camera(w, h)
            d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            d_feat = torch.zeros((h, w, 8), dtype=torch.int64, device="cuda")
            d_out = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            work_bytes = rt.Renderer.denoise_workspace_bytes(w, h)
            d_work = torch.zeros(work_bytes // 8, dtype=torch.int64, device="cuda")
            p = rt.make_params(w, h, 8)
            out(f"{name}: {len(flat)} spheres, {w}x{h}, workspace {work_bytes / 1e6:.1f} MB")

            def timed(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1)

            render = lambda: r.render_device(cam, p, d_fix.data_ptr(), stream.cuda_stream)
            features = lambda: r.render_features_device(cam, p, d_feat.data_ptr(), 0, stream.cuda_stream)

            def denoise(levels, form=None):
                if form:
                    os.environ[KNOB] = form
                try:
                    return timed(lambda: r.denoise_device(d_fix.data_ptr(), 8, d_feat.data_ptr(), 8, w, h, rt.make_denoise(levels), d_work.data_ptr(),
                                                          d_out.data_ptr(), stream=stream.cuda_stream))
                finally:
                    os.environ.pop(KNOB, None)

            for _ in range(3):
                timed(render); timed(features); denoise(4)
            tr, tf, td = [], [], []
            for _ in range(a.reps):
                tr.append(timed(render)); tf.append(timed(features)); td.append(denoise(4))
            yard = [x + y for x, y in zip(tr, tf)]
            out(f"  render   {fmt(tr)}")
            out(f"  features {fmt(tf)}")
            out(f"  denoise  {fmt(td)}   denoise / (render + features) = {statistics.median(td) / statistics.median(yard):.3f} "
                f"(render + features {fmt(yard)})")
            # the two forms of the level kernel, level by level
            forms = ("gather", "tile")
            t = {(f, L): [] for f in forms for L in range(0, a.levels + 1)}
            for f in forms:
                for L in range(1, a.levels + 1):
                    denoise(L, f)
            for _ in range(a.reps):
                for L in range(1, a.levels + 1):
                    for f in forms:
                        t[(f, L)].append(denoise(L, f))
            med = {k: (statistics.median(v) if v else None) for k, v in t.items()}
            out(f"  a denoise of 1 level (prepare + box + level 0 + finish): gather {fmt(t[('gather', 1)])}   tile {fmt(t[('tile', 1)])}")
            for L in range(2, a.levels + 1):
                g, ti = med[("gather", L)] - med[("gather", L - 1)], med[("tile", L)] - med[("tile", L - 1)]
                out(f"  level {L - 1} (hole step {1 << (L - 1):3d}), box mean + level kernel: gather {g:7.3f} ms   tile {ti:7.3f} ms   tile / gather = {ti / g:.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
