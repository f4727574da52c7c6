#!/usr/bin/env python3
"""What temporal accumulation costs (profiles/temporal.txt).  Needs an MI355X.

For each frame size, everything on the device and in one process: the time of one accumulation (rt_temporal_device with a full history,
default options) beside the yardsticks of profiles/denoise.txt measured again in the same run -- a whole denoise (rt_denoise_device, 4
levels) and the two launches whose output both consume, rt_render_device at 8 spp and rt_render_features_device at 8 spp.  Every figure is
the time between two events recorded on the stream right before and after the call; the four are ALTERNATED within a repetition; REPS
repetitions (default 24) after a warm-up; median, minimum, maximum and spread = (max - min) / median of identical runs.

The history is the previous camera of a 2-degree orbit (orbit_cameras(180)), its features rendered and its result accumulated once before
the timing starts, so the taps land where they do in an animation.  Then the same call without the clamp, and as a first frame (no
history: what the prepare and the store alone cost), and the bytes a call must move at least against the time it takes.

usage: tools/temporal_bench.py [--reps N] [--out FILE]
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

    out(f"# tools/temporal_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}, library built from kernel sources {rt._ffi.load().rt_build_source_sha().decode()}")
    out("# times between two events on the stream around each call; render = rt_render_device 8 spp, features = rt_render_features_device 8 spp, "
        "denoise = rt_denoise_device 4 levels (defaults), temporal = rt_temporal_device with a full history (defaults: alpha_min 0.1, sigmas 0.5 / 0.1, clamp 1)")
    stream = torch.cuda.Stream()
    cases = (("book scene", rt.random_scene(1).flatten(), 1200, 675), ("10k scene", rt.random_scene(1, grid=(-50, 49)).flatten(), 1920, 1080))
    for name, flat, w, h in cases:
        with rt.Renderer(0) as r:
            r.upload_scene(flat)
            prev_cam, cam = rt.orbit_cameras(180, w, h)[:2]
            zeros = lambda n, t=torch.int64: torch.zeros(n, dtype=t, device="cuda")
            d_fix, d_feat, d_pfeat, d_dn = zeros(h * w * 3), zeros(h * w * 8), zeros(h * w * 8), zeros(h * w * 3)
            d_acc = [zeros(h * w * 3), zeros(h * w * 3)]
            d_len = [zeros(h * w, torch.int32), zeros(h * w, torch.int32)]
            d_work = zeros(rt.Renderer.denoise_workspace_bytes(w, h) // 8)
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

            # the previous frame: its sums, its features, its (first-frame) accumulation into pair 0
            r.render_device(prev_cam, p, d_fix.data_ptr(), s)
            r.render_features_device(prev_cam, p, d_pfeat.data_ptr(), 0, s)
            r.temporal_device(d_fix.data_ptr(), 8, d_pfeat.data_ptr(), 8, prev_cam, w, h, rt.make_temporal(), d_acc[0].data_ptr(), d_len[0].data_ptr(), stream=s)
            stream.synchronize()
            history = (d_acc[0].data_ptr(), d_len[0].data_ptr(), d_pfeat.data_ptr(), 8, prev_cam)
            render = lambda: r.render_device(cam, p, d_fix.data_ptr(), s)
            features = lambda: r.render_features_device(cam, p, d_feat.data_ptr(), 0, s)
            denoise = lambda: r.denoise_device(d_fix.data_ptr(), 8, d_feat.data_ptr(), 8, w, h, rt.make_denoise(4), d_work.data_ptr(), d_dn.data_ptr(), stream=s)

            def temporal(tp=None, hist=history):
                return lambda: r.temporal_device(d_fix.data_ptr(), 8, d_feat.data_ptr(), 8, cam, w, h, tp if tp is not None else rt.make_temporal(),
                                                 d_acc[1].data_ptr(), d_len[1].data_ptr(), history=hist, stream=s)

            variants = (("temporal", temporal()), ("  no clamp", temporal(rt.make_temporal(clamp=False))), ("  first frame", temporal(hist=None)))
            for _ in range(3):
                timed(render); timed(features); timed(denoise)
                for _, call in variants:
                    timed(call)
            tr, tf, td = [], [], []
            tv = {k: [] for k, _ in variants}
            for _ in range(a.reps):
                tr.append(timed(render)); tf.append(timed(features)); td.append(timed(denoise))
                for k, call in variants:
                    tv[k].append(timed(call))
            yard = [x + y for x, y in zip(tr, tf)]
            mt, md = statistics.median(tv["temporal"]), statistics.median(td)
            out(f"  render       {fmt(tr)}")
            out(f"  features     {fmt(tf)}")
            out(f"  denoise      {fmt(td)}   one level of four ~ {md / 4:.3f} ms")
            for k, _ in variants:
                out(f"  {k:<12} {fmt(tv[k])}")
            out(f"  temporal / denoise = {mt / md:.3f}   temporal / (render + features) = {mt / statistics.median(yard):.4f}")
            timed(variants[0][1])                                       # (the default call once more: its lengths are what is counted)
            hit = (d_feat.view(h * w, 8)[:, 7] != 0)
            found = (d_len[1] >= 2)
            torch.cuda.synchronize()
            # the least a call moves: 24 + 64 B of the pixel's own sums, 24 + 4 + 64 B of a history pixel (every one is some lane's tap), 24 + 4 B out
            moved = h * w * 208
            out(f"  {int(found.sum())} of {int(hit.sum())} hit pixels found history; at least {moved / 1e6:.0f} MB moved: {moved / mt / 1e6:.0f} GB/s at the median")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
