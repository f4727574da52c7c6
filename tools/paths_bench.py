#!/usr/bin/env python3
"""What the device path queue costs (profiles/paths.txt).  Needs an MI355X.  The protocol of tools/shade_bench.py.

  (c) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, BEFORE this process opens the GPU.
  (a) The frame, 1200 x 675 x 16 spp on the book scene, through rt_render_device, rtiow_amd.render_wavefront_torch and
      rt_render_wavefront_device (batch 1 << 20 both), alternated in one process; host clock around work that ends in a device synchronise;
      one warm-up, medians of --frame-reps, spreads printed.  The three frames are compared bit for bit.
  (b) One batch of 2^20 items: the begin kernel, and the three kernels of a step -- issued one by one through the diagnostic knob
      RTIOW_PATHS_STEP_PARTS, the in queue restored before every repetition -- at bounce 1 and at the first bounce that holds fewer than
      10 000 paths.  A pair of device events around ONE launch; three warm-ups, then --reps repetitions, the kernels alternated within a
      repetition; each next to its own bytes at 6.3 TB/s (the rate sections 17 and 18 use).  Bytes: a path's state is 84 (three 32-bit
      words, nine doubles); begin writes 84 per path; the bounce reads 84 per live path and writes 76 per survivor (origin, dir,
      throughput, event) or 24 of atomic adds per path that ends (every ended path counted as a miss), plus 12 per wave of scratch; the
      scan reads and writes 4 per wave; the compaction reads 12 per wave and moves 84 + 84 per survivor.
  (d) The live count per bounce of that batch (read back between steps: this tool may wait, the integrator does not), per batch of the
      frame the number of steps that run on an empty queue, when rt_render_wavefront_device returns against when the device is done,
      and what a step on an empty queue costs: --reps groups of 50 steps on an empty queue of 2^20 slots
      between one pair of events.

usage: tools/paths_bench.py [--reps N] [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SPP = 1200, 675, 16
HBM_RATE = 6.3e12
BATCH = 1 << 20
STATE = 84


def fmt(xs, unit="ms", scale=1.0):
    med = statistics.median(xs)
    return f"{med * scale:9.3f} {unit} (min {min(xs) * scale:.3f}, max {max(xs) * scale:.3f}, spread {100 * (max(xs) - min(xs)) / med:.1f} %)"


def headline(tree, steps, warmup):
    run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        sys.exit(f"bench.py failed in {tree}: {run.stderr[-2000:]}")
    line = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    value = float(line["value"])
    return value, W * H * 500 / value / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--frame-reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.parent_tree:
        out("## (c) bench.py --gpus 1 --steps 10 --warmup 3: the parent commit's tree and this one, alternated, fresh processes (Msamples/s, ms per step)")
        vals = {"parent": [], "tree": []}
        for rnd in range(1, a.rounds + 1):
            for name, tree in (("parent", a.parent_tree), ("tree", ROOT)):
                v, ms = headline(tree, 10, 3)
                vals[name].append(v)
                out(f"{name} round {rnd}".ljust(18) + f" {v:8.2f} Msamples/s  {ms:.3f} ms")
                save()
        sp = lambda xs: 100 * (max(xs) - min(xs)) / statistics.median(xs)
        out(f"parent median {statistics.median(vals['parent']):.2f} (run-to-run spread {sp(vals['parent']):.2f} %), tree median "
            f"{statistics.median(vals['tree']):.2f} (spread {sp(vals['tree']):.2f} %), tree / parent = "
            f"{statistics.median(vals['tree']) / statistics.median(vals['parent']):.4f}")
        save()

    import torch
    import rtiow_amd as rt

    out(f"# tools/paths_bench.py --reps {a.reps} --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    dev = torch.device("cuda", 0)
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    seed = 1
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    os.environ.pop("RTIOW_PATHS_STEP_PARTS", None)

    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        n = W * H * SPP
        out(f"book scene: {len(flat)} spheres; {W}x{H}, {SPP} samples per pixel: {n} paths, pixel-major, {-(-n // BATCH)} batches of {BATCH}")

        # ---- (a) the frame
        p = rt.make_params(W, H, SPP, seed=seed)
        d_fix = torch.zeros((H, W, 3), dtype=torch.int64, device=dev)
        n_fix = torch.zeros((H, W, 3), dtype=torch.int64, device=dev)
        n_rays = torch.zeros(1, dtype=torch.int64, device=dev)

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res

        cur = lambda: torch.cuda.current_stream().cuda_stream
        td, tw, tn = [], [], []
        for rep in range(1 + a.frame_reps):
            ms_d, _ = clock(lambda: r.render_device(cam, p, d_fix.data_ptr(), cur()))
            ms_w, (wf, w_rays) = clock(lambda: rt.render_wavefront_torch(r, cam, p, batch=BATCH))
            ms_n, _ = clock(lambda: r.render_wavefront_device(cam, p, n_fix.data_ptr(), n_rays.data_ptr(), cur()))
            if rep >= 1:
                td.append(ms_d); tw.append(ms_w); tn.append(ms_n)
        st = r.last_stats()
        med = statistics.median
        out(f"## (a) the frame, {W}x{H}x{SPP}, host clock around work that ends in a synchronise, alternated, medians of {a.frame_reps}")
        out(f"  rt_render_device              {fmt(td)}  (kernel {st['kernel_ms']:.3f} ms, {st['rays_traced']} rays)")
        out(f"  render_wavefront_torch        {fmt(tw)}  ({w_rays} rays)")
        out(f"  rt_render_wavefront_device    {fmt(tn)}  ({int(n_rays.item())} rays)")
        gain, spreads = med(tw) - med(tn), (max(tw) - min(tw)) + (max(tn) - min(tn))
        out(f"  torch / native = {med(tw) / med(tn):.2f}; the gain {gain:.3f} ms against the two spreads together {spreads:.3f} ms: "
            f"{'FASTER by more than the spreads' if gain > spreads else 'NOT faster by more than the spreads'}; native / megakernel = {med(tn) / med(td):.2f}")
        out(f"  the three frames are {'EQUAL bit for bit' if torch.equal(wf, d_fix) and torch.equal(n_fix, d_fix) else 'DIFFERENT'}; ray counts "
            f"{'equal' if w_rays == st['rays_traced'] == int(n_rays.item()) else 'DIFFER'}")
        save()
        del wf

        # ---- (d) first half: the live count per bounce of the first batch, and the queues of the two bounces to time
        A, B = rt.PathQueue(BATCH, dev), rt.PathQueue(BATCH, dev)
        rt.paths_begin_torch(r, cam, W, H, seed, SPP, 0, 0, BATCH, A)
        snap = {}
        counts = []
        keep = lambda Q: {f: getattr(Q, f).clone() for f in rt.PathQueue.FIELDS if f != "scratch"}
        q = [A, B]
        small_at = None
        for depth in range(int(p.max_depth)):
            live = int(q[depth & 1].count.item())
            counts.append(live)
            if depth == 0:
                snap[1] = keep(q[0])
            if small_at is None and 0 < live < 10000:
                small_at = depth + 1
                snap[small_at] = keep(q[depth & 1])
            rt.paths_step_torch(r, seed, q[depth & 1], q[(depth + 1) & 1], n_fix)
        torch.cuda.synchronize()
        last = max(k for k, c in enumerate(counts) if c > 0) + 1
        out(f"## (d) batch 0 of {BATCH}: live paths entering bounce 1, 2, ...: {counts[:last + 1]}")
        # every batch of the frame: the first bounce that finds its queue empty
        first_empty = []
        for first in range(0, n, BATCH):
            rt.paths_begin_torch(r, cam, W, H, seed, SPP, 0, first, min(BATCH, n - first), A)
            depth = 0
            while depth < int(p.max_depth) and int(q[depth & 1].count.item()) > 0:
                rt.paths_step_torch(r, seed, q[depth & 1], q[(depth + 1) & 1], n_fix)
                depth += 1
            first_empty.append(depth)
        empty_steps = sum(int(p.max_depth) - d for d in first_empty)
        out(f"  steps that find a live path, per batch: {first_empty}: {empty_steps} of the frame's {len(first_empty) * int(p.max_depth)} steps run on an empty queue")
        # how far ahead of the device the host runs: the host clock until the call returns, and until the device is done
        t_issue, t_done = [], []
        for rep in range(1 + a.frame_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.render_wavefront_device(cam, p, n_fix.data_ptr(), n_rays.data_ptr(), cur())
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rep >= 1:
                t_issue.append((t1 - t0) * 1e3); t_done.append((time.perf_counter() - t0) * 1e3)
        out(f"  rt_render_wavefront_device returns after {fmt(t_issue)}; the device is done after {fmt(t_done)}")

        # ---- (b) the kernels one by one
        stream = torch.cuda.Stream()

        def timed(fn, before=None):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if before:
                before()
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def restore(state):
            for f, t in state.items():
                getattr(A, f).copy_(t)

        def part(mask):
            def run():
                os.environ["RTIOW_PATHS_STEP_PARTS"] = str(mask)
                try:
                    rt.paths_step_torch(r, seed, A, B, n_fix)
                finally:
                    os.environ.pop("RTIOW_PATHS_STEP_PARTS")
            return run

        out("## (b) one batch, the kernels one launch each, beside their own bytes at 6.3 TB/s (the no-overlap streaming bound)")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            tb = []
            for rep in range(3 + a.reps):
                ms = timed(lambda: rt.paths_begin_torch(r, cam, W, H, seed, SPP, 0, 0, BATCH, A))
                if rep >= 3:
                    tb.append(ms)
            bytes_b = BATCH * STATE
            out(f"  path_begin_kernel     {BATCH} paths".ljust(64) + f"{fmt(tb, 'us', 1e3)}; {bytes_b / 1e6:.1f} MB = {bytes_b / HBM_RATE * 1e6:.1f} us at 6.3 TB/s; "
                f"time / bound = {med(tb) / (bytes_b / HBM_RATE * 1e3):.2f}")
            for bounce, state in sorted(snap.items()):
                live = int(state["count"].item())
                times = {"bounce_kernel": [], "queue_scan_kernel": [], "queue_compact_kernel": []}
                for rep in range(3 + a.reps):
                    for (name, mask) in (("bounce_kernel", 1), ("queue_scan_kernel", 2), ("queue_compact_kernel", 4)):
                        ms = timed(part(mask), before=(lambda: restore(state)) if mask == 1 else None)
                        if rep >= 3:
                            times[name].append(ms)
                stream.synchronize()
                m = int(B.count.item())
                waves = -(-live // 64)
                bounds = {"bounce_kernel": live * STATE + m * 76 + (live - m) * 24 + waves * 12, "queue_scan_kernel": waves * 8,
                          "queue_compact_kernel": waves * 12 + m * 2 * STATE}
                out(f"  bounce {bounce}: {live} live paths, {m} survive")
                for name, ts in times.items():
                    b_us = bounds[name] / HBM_RATE * 1e6
                    out(f"    {name:22s}".ljust(64) + f"{fmt(ts, 'us', 1e3)}; {bounds[name] / 1e6:.3f} MB = {b_us:.2f} us at 6.3 TB/s; "
                        f"time / bound = {med(ts) * 1e3 / b_us:.1f}; {bounds[name] / live:.1f} bytes per live path")
                save()

            # ---- (d) second half: what a step on an empty queue costs
            A.count.zero_()
            te = []
            for rep in range(3 + a.reps):
                def fifty():
                    for k in range(50):
                        rt.paths_step_torch(r, seed, q[k & 1], q[(k + 1) & 1], n_fix)
                ms = timed(fifty)
                if rep >= 3:
                    te.append(ms / 50)
        cost = med(te) * empty_steps
        spread_n = max(tn) - min(tn)
        out(f"  a step on an empty queue of {BATCH} slots (three launches; 50 between one pair of events): {fmt(te, 'us', 1e3)}")
        out(f"  {empty_steps} empty steps x {med(te) * 1e3:.1f} us = {cost:.3f} ms of the native frame's {med(tn):.3f} ms "
            f"({100 * cost / med(tn):.1f} %); the frame's spread is {spread_n:.3f} ms: the empty launches cost "
            f"{'MORE' if cost > spread_n else 'LESS'} than the spread")
        out(f"  the call returns {med(t_done) - med(t_issue):.1f} ms before the device is done: a count copied to pinned memory is "
            f"{'NOT yet there' if med(t_issue) < 0.5 * med(t_done) else 'there'} when the host issues the steps it could spare")
    save()


if __name__ == "__main__":
    main()
