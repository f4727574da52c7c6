#!/usr/bin/env python3
"""What lighting costs the device path queue (profiles/lights.txt).  Needs an MI355X.  The protocol of
tools/paths_bench.py, whose sibling this is.

  (h) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, BEFORE this process opens the GPU (tools/paths_bench.py's own section (c)).
  The frame, 1200 x 675 x 16 spp on the book scene, host clock around work that ends in a device synchronise, one warm-up, medians of
  --frame-reps, alternated in one process:
  (a) rt_render_wavefront_device -- the yardstick;
  (b) rt_render_wavefront_lit_device with the reference's sky and no table;
  (c) ... with an all-zero table of the scene's size;
  (d) ... the night frame: a black sky, the large Lambertian sphere radiating (4, 3.2, 2.4) (no identity: for the reader's interest).
  (a), (b) and (c) are compared bit for bit, sums and ray counts.

usage: tools/lights_bench.py [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from paths_bench import H, SPP, W, fmt, headline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame-reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.parent_tree:
        out("## (h) bench.py --gpus 1 --steps 10 --warmup 3: the parent commit's tree and this one, alternated, fresh processes (Msamples/s, ms per step)")
        vals = {"parent": [], "tree": []}
        for rnd in range(1, a.rounds + 1):
            for name, tree in (("parent", a.parent_tree), ("tree", ROOT)):
                v, ms = headline(tree, 10, 3)
                vals[name].append(v)
                out(f"{name} round {rnd}".ljust(18) + f" {v:8.2f} Msamples/s  {ms:.3f} ms")
        sp = lambda xs: 100 * (max(xs) - min(xs)) / statistics.median(xs)
        out(f"parent median {statistics.median(vals['parent']):.2f} (run-to-run spread {sp(vals['parent']):.2f} %), tree median "
            f"{statistics.median(vals['tree']):.2f} (spread {sp(vals['tree']):.2f} %), tree / parent = "
            f"{statistics.median(vals['tree']) / statistics.median(vals['parent']):.4f}")

    import numpy as np
    import torch
    import rtiow_amd as rt

    out(f"# tools/lights_bench.py --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    dev = torch.device("cuda", 0)
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    os.environ.pop("RTIOW_PATHS_STEP_PARTS", None)
    big = [k for k in range(len(flat)) if int(flat[k]["kind"]) == 0 and float(flat[k]["radius"]) == 1.0][0]
    zeros = torch.zeros((len(flat), 3), dtype=torch.float64, device=dev)
    night = torch.zeros((len(flat), 3), dtype=torch.float64, device=dev)
    night[big] = torch.tensor([4.0, 3.2, 2.4], dtype=torch.float64)
    cases = [("(a) rt_render_wavefront_device", None),
             ("(b) lit, reference sky, no table", rt.Lighting()),
             ("(c) lit, reference sky, zero table", rt.Lighting(emission=zeros)),
             ("(d) lit, black sky, one light", rt.Lighting((0, 0, 0), (0, 0, 0), night))]

    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        out(f"book scene: {len(flat)} spheres (the large Lambertian sphere is number {big}); {W}x{H}, {SPP} samples per pixel: {W * H * SPP} paths")
        p = rt.make_params(W, H, SPP, seed=1)
        fix = [torch.zeros((H, W, 3), dtype=torch.int64, device=dev) for _ in cases]
        rays = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in cases]
        times = [[] for _ in cases]
        cur = lambda: torch.cuda.current_stream().cuda_stream
        for rep in range(1 + a.frame_reps):
            for k, (_, light) in enumerate(cases):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.render_wavefront_device(cam, p, fix[k].data_ptr(), rays[k].data_ptr(), cur(), lighting=light)
                torch.cuda.synchronize()
                if rep >= 1:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        med = statistics.median
        out(f"## the frame, {W}x{H}x{SPP}, host clock around work that ends in a synchronise, alternated, medians of {a.frame_reps}")
        for k, (name, _) in enumerate(cases):
            out(f"  {name:38s} {fmt(times[k])}  ({int(rays[k].item())} rays)")
        spread_a = max(times[0]) - min(times[0])
        for k in (1, 2):
            extra = med(times[k]) - med(times[0])
            out(f"  {cases[k][0][:3]} - (a) = {extra:+.3f} ms ({100 * extra / med(times[0]):+.2f} %); (a)'s own spread is {spread_a:.3f} ms: "
                f"{'SLOWER by more than the spread' if extra > spread_a else 'within the spread'}")
        same = all(torch.equal(fix[k], fix[0]) and int(rays[k].item()) == int(rays[0].item()) for k in (1, 2))
        out(f"  (a), (b) and (c) are {'EQUAL bit for bit, sums and ray counts' if same else 'DIFFERENT'}")
        lit = np.count_nonzero(fix[3].cpu().numpy().any(axis=2))
        out(f"  (d): {lit} of {W * H} pixels receive light")


if __name__ == "__main__":
    main()
