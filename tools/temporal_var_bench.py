#!/usr/bin/env python3
"""What carrying second moments costs (profiles/temporal_var.txt).  Needs an MI355X.

tools/temporal_bench.py's method: for each of its two frames, everything on the device and in one process; every figure is the time between
two events recorded on the stream right before and after the call; the calls are ALTERNATED within a repetition; REPS repetitions (default
24) after a warm-up; median, minimum, maximum and spread = (max - min) / median of identical runs.  Measured: rt_temporal_var_device with a
full history (default options), as a first frame and without the clamp; rt_denoise_var_given_device (4 levels, defaults) on its result;
and, as yardsticks measured again in the same run, rt_temporal_device and rt_denoise_var_device on the same frame.

The traffic model: rt_temporal moves at least 208 B per pixel; this adds 24 B of history moment and 48 B of output
(moment and variance), 280 B: 1.35 x.

usage: tools/temporal_var_bench.py [--reps N] [--out FILE]
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
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/temporal_var_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}, library built from kernel sources {rt._ffi.load().rt_build_source_sha().decode()}")
    out("# times between two events on the stream around each call, all calls alternated in one process; temporal = rt_temporal_device and "
        "temporal_var = rt_temporal_var_device with a full history (defaults: alpha_min 0.1, sigmas 0.5 / 0.1, clamp 1); denoise_var = "
        "rt_denoise_var_device on the 8-spp frame and its half, given = rt_denoise_var_given_device on the accumulated frame and its variance (4 levels, defaults)")
    stream = torch.cuda.Stream()
    cases = (("book scene", rt.random_scene(1).flatten(), 1200, 675), ("10k scene", rt.random_scene(1, grid=(-50, 49)).flatten(), 1920, 1080))
    for name, flat, w, h in cases:
        with rt.Renderer(0) as r:
            r.upload_scene(flat)
            prev_cam, cam = rt.orbit_cameras(180, w, h)[:2]
            zeros = lambda n, t=torch.int64: torch.zeros(n, dtype=t, device="cuda")
            d_fix, d_half, d_feat, d_pfeat, d_dn = zeros(h * w * 3), zeros(h * w * 3), zeros(h * w * 8), zeros(h * w * 8), zeros(h * w * 3)
            d_acc = [zeros(h * w * 3), zeros(h * w * 3)]
            d_len = [zeros(h * w, torch.int32), zeros(h * w, torch.int32)]
            d_m2 = [zeros(h * w * 3, torch.float64), zeros(h * w * 3, torch.float64)]
            d_var = zeros(h * w * 3, torch.float64)
            d_work = zeros(rt.Renderer.denoise_var_workspace_bytes(w, h) // 8)
            p = rt.make_params(w, h, 8)
            s = stream.cuda_stream
            out(f"{name}: {len(flat)} spheres, {w}x{h}")

            def timed(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1)

            # the previous frame: its sums, its features, its (first-frame) accumulation into set 0; then this frame's sums, half and features
            tp, dn = rt.make_temporal(), rt.make_denoise_var(4)
            r.render_device(prev_cam, p, d_fix.data_ptr(), s)
            r.render_features_device(prev_cam, p, d_pfeat.data_ptr(), 0, s)
            r.temporal_var_device(d_fix.data_ptr(), 8, d_pfeat.data_ptr(), 8, prev_cam, w, h, tp, d_acc[0].data_ptr(), d_len[0].data_ptr(),
                                  d_m2[0].data_ptr(), d_var.data_ptr(), stream=s)
            r.render_device(cam, rt.make_params(w, h, 4), d_half.data_ptr(), s)
            r.render_device(cam, p, d_fix.data_ptr(), s)
            r.render_features_device(cam, p, d_feat.data_ptr(), 0, s)
            stream.synchronize()
            hist = (d_acc[0].data_ptr(), d_len[0].data_ptr(), d_pfeat.data_ptr(), 8, prev_cam, d_m2[0].data_ptr())

            def temporal_var(options=tp, history=hist):
                return lambda: r.temporal_var_device(d_fix.data_ptr(), 8, d_feat.data_ptr(), 8, cam, w, h, options, d_acc[1].data_ptr(), d_len[1].data_ptr(),
                                                     d_m2[1].data_ptr(), d_var.data_ptr(), history=history, stream=s)

            calls = (("temporal", lambda: r.temporal_device(d_fix.data_ptr(), 8, d_feat.data_ptr(), 8, cam, w, h, tp, d_acc[1].data_ptr(), d_len[1].data_ptr(),
                                                            history=hist[:5], stream=s)),
                     ("  its first frame", lambda: r.temporal_device(d_fix.data_ptr(), 8, d_feat.data_ptr(), 8, cam, w, h, tp, d_acc[1].data_ptr(),
                                                                     d_len[1].data_ptr(), stream=s)),
                     ("temporal_var", temporal_var()),
                     ("  no clamp", temporal_var(rt.make_temporal(clamp=False))), ("  first frame", temporal_var(history=None)),
                     ("denoise_var", lambda: r.denoise_var_device(d_fix.data_ptr(), d_half.data_ptr(), 8, d_feat.data_ptr(), 8, w, h, dn, d_work.data_ptr(),
                                                                  d_dn.data_ptr(), stream=s)),
                     ("given", lambda: r.denoise_var_given_device(d_acc[1].data_ptr(), d_var.data_ptr(), 1, d_feat.data_ptr(), 8, w, h, dn, d_work.data_ptr(),
                                                                  d_dn.data_ptr(), stream=s)))
            for _ in range(3):
                for _, call in calls:
                    timed(call)
            final = calls[2][1]                                         # (the default call, once more at the end: its lengths are what is counted)
            t = {k: [] for k, _ in calls}
            for _ in range(a.reps):
                for k, call in calls:
                    t[k].append(timed(call))
            for k, _ in calls:
                out(f"  {k:<17} {fmt(t[k])}")
            med = {k: statistics.median(v) for k, v in t.items()}
            out(f"  temporal_var / temporal = {med['temporal_var'] / med['temporal']:.3f} (traffic model 280 / 208 = 1.35)   "
                f"given / denoise_var = {med['given'] / med['denoise_var']:.3f}")
            timed(final)
            hit = (d_feat.view(h * w, 8)[:, 7] != 0)
            found = (d_len[1] >= 2)
            torch.cuda.synchronize()
            moved = h * w * 280
            out(f"  {int(found.sum())} of {int(hit.sum())} hit pixels found history; at least "
                f"{moved / 1e6:.0f} MB moved: {moved / med['temporal_var'] / 1e6:.0f} GB/s at the median")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
