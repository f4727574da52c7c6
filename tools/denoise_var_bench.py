#!/usr/bin/env python3
"""What the variance-guided denoiser costs (profiles/denoise_var.txt).  Needs an MI355X.

The protocol of tools/denoise_bench.py: everything on the device and in one process, every figure the time between two events recorded on
the stream right before and after the call, the calls ALTERNATED within a repetition, REPS repetitions (default 24) after a warm-up;
median, minimum, maximum and spread = (max - min) / median of identical runs.

For each frame: a whole rt_denoise_var_device (4 levels: prepare, four statistics passes, four level kernels, finish) beside the
yardstick of the same run, rt_denoise_device at 4 levels on the same sums.  The sums are a dense render of 8 spp, `half` its first 4 spp.
Then the two forms of the level kernel per level (RTIOW_DENOISE_LEVEL_KERNEL=gather|tile, read per call): a denoise of L levels minus a
denoise of L - 1 levels is the cost of level L - 1 (its statistics pass, the same in both, and its level kernel), both measured with the
same form; medians of REPS alternated runs.

usage: tools/denoise_var_bench.py [--reps N] [--levels L] [--out FILE]
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

    out(f"# tools/denoise_var_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}, library built from kernel sources {rt._ffi.load().rt_build_source_sha().decode()}")
    out("# times between two events on the stream around each call; denoise = rt_denoise_device 4 levels, sigmas 0.35 / 1.0 / 0.2; "
        f"denoise_var = rt_denoise_var_device 4 levels, sigmas {rt.make_denoise_var().sigma_color:g} / 1.0 / 0.2; both demodulated, the shipped level kernels")
    os.environ.pop(KNOB, None)
    stream = torch.cuda.Stream()
    cases = (("book scene", rt.random_scene(1).flatten(), 1200, 675), ("10k scene", rt.random_scene(1, grid=(-50, 49)).flatten(), 1920, 1080))
    for name, flat, w, h in cases:
        with rt.Renderer(0) as r:
            r.upload_scene(flat)
            cam = rt.book1_camera(w, h)
            d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            d_half = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            d_feat = torch.zeros((h, w, 8), dtype=torch.int64, device="cuda")
            d_out = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            work_bytes = rt.Renderer.denoise_var_workspace_bytes(w, h)
            d_work = torch.zeros(work_bytes // 8, dtype=torch.int64, device="cuda")
            r.render_device(cam, rt.make_params(w, h, 8), d_fix.data_ptr(), stream.cuda_stream)
            r.render_device(cam, rt.make_params(w, h, 4), d_half.data_ptr(), stream.cuda_stream)
            r.render_features_device(cam, rt.make_params(w, h, 8), d_feat.data_ptr(), 0, stream.cuda_stream)
            stream.synchronize()
            out(f"{name}: {len(flat)} spheres, {w}x{h}, workspace {work_bytes / 1e6:.1f} MB (rt_denoise: {rt.Renderer.denoise_workspace_bytes(w, h) / 1e6:.1f} MB)")

            def timed(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1)

            def plain(levels=4):
                return timed(lambda: r.denoise_device(d_fix.data_ptr(), 8, d_feat.data_ptr(), 8, w, h, rt.make_denoise(levels), d_work.data_ptr(),
                                                      d_out.data_ptr(), stream=stream.cuda_stream))

            def var(levels=4, form=None):
                if form:
                    os.environ[KNOB] = form
                try:
                    return timed(lambda: r.denoise_var_device(d_fix.data_ptr(), d_half.data_ptr(), 8, d_feat.data_ptr(), 8, w, h, rt.make_denoise_var(levels),
                                                              d_work.data_ptr(), d_out.data_ptr(), stream=stream.cuda_stream))
                finally:
                    os.environ.pop(KNOB, None)

            for _ in range(3):
                plain(); var()
            tp, tv = [], []
            for _ in range(a.reps):
                tp.append(plain()); tv.append(var())
            out(f"  denoise      {fmt(tp)}")
            out(f"  denoise_var  {fmt(tv)}   denoise_var / denoise = {statistics.median(tv) / statistics.median(tp):.3f}")
            forms = ("gather", "tile")
            t = {(f, L): [] for f in forms for L in range(0, a.levels + 1)}
            for f in forms:
                for L in range(1, a.levels + 1):
                    var(L, f)
            for _ in range(a.reps):
                for L in range(1, a.levels + 1):
                    for f in forms:
                        t[(f, L)].append(var(L, f))
            med = {k: (statistics.median(v) if v else None) for k, v in t.items()}
            out(f"  a denoise_var of 1 level (prepare + statistics + level 0 + finish): gather {fmt(t[('gather', 1)])}   tile {fmt(t[('tile', 1)])}")
            for L in range(2, a.levels + 1):
                g, ti = med[("gather", L)] - med[("gather", L - 1)], med[("tile", L)] - med[("tile", L - 1)]
                out(f"  level {L - 1} (hole step {1 << (L - 1):3d}), statistics + level kernel: gather {g:7.3f} ms   tile {ti:7.3f} ms   tile / gather = {ti / g:.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
