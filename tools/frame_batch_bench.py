#!/usr/bin/env python3
"""What a frame batch (rt_render_frames_device: n cameras, ONE launch) buys over the same frames rendered one launch each
(profiles/frame_batches.txt).  Needs an MI355X.

A  small frames, the case the feature is for: F orbit cameras of the book scene, rendered
     batch   in one rt_render_frames_device launch (sample_stride = spp),
     loop    as F rt_render_device launches back to back on one stream (sample_begin = f * spp: the same frames),
     loop2   the same launches alternated over two streams with RT_FLAG_OVERLAPPED,
   timed from the first launch to the last event (HIP events; the second stream waits for the start event) and as the wall
   time of the call sequence up to the final synchronisation.
B  what the variant costs per sample: 1 and 4 frames of 1200x675x100 as a batch against dense rt_render_device launches of the
   same frames, kernel time (rt_last_stats) per pixel-sample.

Every figure: REPS repetitions (default 12) after a warm-up, the variants ALTERNATED within a repetition in one process;
median, minimum, maximum, and spread = (max - min) / median.

usage: tools/frame_batch_bench.py [--reps N] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtiow_amd as rt  # noqa: E402


def summary(xs):
    med = statistics.median(xs)
    return med, min(xs), max(xs), (max(xs) - min(xs)) / med


def fmt(xs, unit="ms"):
    med, lo, hi, spread = summary(xs)
    return f"{med:9.3f} {unit} (min {lo:.3f}, max {hi:.3f}, spread {100 * spread:.1f} %)"


class Sequence:
    """One way of rendering the F frames; run() issues the launches and returns (gpu ms first launch -> last event, wall ms)."""

    def __init__(self, r, cams, w, h, spp, kind, streams):
        self.r, self.cams, self.w, self.h, self.spp, self.kind, self.streams = r, cams, w, h, spp, kind, streams
        self.F = len(cams)
        self.d_cams = torch.from_numpy(rt.cameras_to_array(cams)).cuda()
        self.d_fix = torch.zeros((self.F, h, w, 3), dtype=torch.int64, device="cuda")
        self.rc = [c.to_rt_camera() for c in cams]
        flags = rt.RT_FLAG_OVERLAPPED if kind == "loop2" else 0
        self.p_batch = rt.make_params(w, h, spp)
        self.p_frame = [rt.make_params(w, h, spp, sample_begin=f * spp, flags=flags) for f in range(self.F)]
        self.frame_ptr = [self.d_fix[f].data_ptr() for f in range(self.F)]

    def run(self):
        s0, s1 = self.streams
        start, e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record(s0)
        if self.kind == "batch":
            self.r.render_frames_device(self.d_cams.data_ptr(), self.F, self.spp, self.p_batch, self.d_fix.data_ptr(), s0.cuda_stream)
        elif self.kind == "loop":
            for f in range(self.F):
                self.r.render_device(self.rc[f], self.p_frame[f], self.frame_ptr[f], s0.cuda_stream)
        else:
            s1.wait_event(start)
            for f in range(self.F):
                self.r.render_device(self.rc[f], self.p_frame[f], self.frame_ptr[f], (s0, s1)[f & 1].cuda_stream)
        e0.record(s0)
        e1.record(s1)
        s0.synchronize()
        s1.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return max(start.elapsed_time(e0), start.elapsed_time(e1)), wall


def case_a(r, out, reps, streams):
    out("A. F small frames of the book scene (depth 50): one batch launch against F launches; Gsample/s from the median GPU time")
    for w, h, spp, F in ((200, 133, 100, 32), (200, 133, 100, 8), (200, 133, 100, 2), (400, 225, 16, 32), (400, 225, 16, 8), (400, 225, 16, 2)):
        cams = rt.orbit_cameras(F, w, h)
        seqs = {k: Sequence(r, cams, w, h, spp, k, streams) for k in ("batch", "loop", "loop2")}
        ref = None
        for k, s in seqs.items():                     # warm-up, and the three ways render the same frames
            s.run()
            got = s.d_fix.cpu().numpy()
            ref = got if ref is None else ref
            assert np.array_equal(got, ref), k
        gpu = {k: [] for k in seqs}
        wall = {k: [] for k in seqs}
        for _ in range(reps):
            for k, s in seqs.items():
                g, wl = s.run()
                gpu[k].append(g)
                wall[k].append(wl)
        samples = F * w * h * spp
        out(f"  {w}x{h} x {spp} spp x {F} frames = {samples / 1e6:.2f} M pixel-samples, {reps} repetitions, variants alternated")
        for k, label in (("batch", "batch, 1 launch          "), ("loop", f"loop, {F:2d} launches, 1 stream"), ("loop2", f"loop, {F:2d} launches, 2 streams")):
            med = statistics.median(gpu[k])
            out(f"    {label}  gpu {fmt(gpu[k])}  wall {fmt(wall[k])}  {samples / med / 1e6:6.2f} Gsample/s")
        best = min(("loop", "loop2"), key=lambda k: statistics.median(gpu[k]))
        mb, ml = statistics.median(gpu["batch"]), statistics.median(gpu[best])
        spread = max(summary(gpu["batch"])[3], summary(gpu[best])[3])
        out(f"    batch / better loop ({best}): {mb / ml:.3f} x the GPU time ({ml / mb:.2f} x as fast); wall {statistics.median(wall['batch']) / statistics.median(wall[best]):.3f} x; "
            f"larger run-to-run spread of the two: {100 * spread:.1f} %  ->  "
            f"{'the batch wins by more than the spread' if (ml - mb) / ml > spread else 'within the spread or slower'}")


def case_b(r, out, reps, streams):
    w, h, spp = 1200, 675, 100
    out(f"B. the variant's cost per sample: {w}x{h}x{spp} frames, kernel time (rt_last_stats) per pixel-sample, batch against dense launches of the same frames")
    s0 = streams[0]
    for F in (1, 4):
        cams = rt.orbit_cameras(F, w, h)
        d_cams = torch.from_numpy(rt.cameras_to_array(cams)).cuda()
        d_fix = torch.zeros((F, h, w, 3), dtype=torch.int64, device="cuda")
        p = rt.make_params(w, h, spp)

        def batch():
            r.render_frames_device(d_cams.data_ptr(), F, spp, p, d_fix.data_ptr(), s0.cuda_stream)
            s0.synchronize()
            return r.last_stats()["kernel_ms"]

        def dense():
            ms = 0.0
            for f in range(F):
                r.render_device(cams[f], rt.make_params(w, h, spp, sample_begin=f * spp), d_fix[f].data_ptr(), s0.cuda_stream)
                s0.synchronize()
                ms += r.last_stats()["kernel_ms"]
            return ms

        batch()
        got = d_fix.cpu().numpy().copy()
        dense()
        assert np.array_equal(d_fix.cpu().numpy(), got)
        tb, td = [], []
        for _ in range(reps):
            tb.append(batch())
            td.append(dense())
        n = F * w * h * spp
        mb, md = statistics.median(tb), statistics.median(td)
        out(f"  n_frames = {F}: batch {fmt(tb)} = {1e6 * mb / n:.4f} ns/sample; dense x {F} {fmt(td)} = {1e6 * md / n:.4f} ns/sample; "
            f"batch / dense = {mb / md:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/frame_batch_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}, library built from kernel sources {rt._ffi.load().rt_build_source_sha().decode()}")
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    with rt.Renderer(0) as r:
        r.upload_scene(rt.random_scene(1).flatten())
        case_a(r, out, a.reps, streams)
        case_b(r, out, a.reps, streams)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
