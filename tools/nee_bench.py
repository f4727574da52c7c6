#!/usr/bin/env python3
"""What next-event estimation costs the lit path queue, and what it buys (profiles/nee.txt).  Needs an MI355X.
The protocol of tools/paths_bench.py; a sibling of tools/lights_bench.py.

  (h) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, BEFORE this process opens the GPU (tools/paths_bench.py's own section (c)).
  The frame, 1200 x 675 x 16 spp on the book scene, host clock around work that ends in a device synchronise, one warm-up, medians of
  --frame-reps, alternated in one process:
  (d) rt_render_wavefront_lit_device, the night frame of tools/lights_bench.py: a black sky, the large Lambertian sphere radiating
      (4, 3.2, 2.4) -- the yardstick;
  (e) rt_render_wavefront_nee_device with the same lighting and its light list;
  (f) ... with n_lights = 0 (compared with (d) bit for bit, sums and ray counts).
  (v) the variance at equal samples per pixel: the scene, the 16 seeds and the numbers of tests/test_gpu_nee.py's variance test
      (tests/nee_ref.py: stat_scene, stat_numbers), and the time of its frames both ways; from the two the equal-time efficiency.

usage: tools/nee_bench.py [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

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

    out(f"# tools/nee_bench.py --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    dev = torch.device("cuda", 0)
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    os.environ.pop("RTIOW_PATHS_STEP_PARTS", None)
    big = [k for k in range(len(flat)) if int(flat[k]["kind"]) == 0 and float(flat[k]["radius"]) == 1.0][0]
    night = torch.zeros((len(flat), 3), dtype=torch.float64, device=dev)
    night[big] = torch.tensor([4.0, 3.2, 2.4], dtype=torch.float64)
    L = rt.Lighting((0, 0, 0), (0, 0, 0), night)
    cases = [("(d) lit, black sky, one light", False), ("(e) NEE, the same lighting", True), ("(f) NEE, n_lights = 0", [])]
    med = statistics.median

    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        out(f"book scene: {len(flat)} spheres (the large Lambertian sphere is number {big}); {W}x{H}, {SPP} samples per pixel: {W * H * SPP} paths")
        p = rt.make_params(W, H, SPP, seed=1)
        fix = [torch.zeros((H, W, 3), dtype=torch.int64, device=dev) for _ in cases]
        rays = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in cases]
        shadow = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in cases]
        times = [[] for _ in cases]
        cur = lambda: torch.cuda.current_stream().cuda_stream
        for rep in range(1 + a.frame_reps):
            for k, (_, direct) in enumerate(cases):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.render_wavefront_device(cam, p, fix[k].data_ptr(), rays[k].data_ptr(), cur(), lighting=L, direct=direct,
                                          d_shadow_rays_ptr=shadow[k].data_ptr() if direct is not False else 0)
                torch.cuda.synchronize()
                if rep >= 1:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        out(f"## the frame, {W}x{H}x{SPP}, host clock around work that ends in a synchronise, alternated, medians of {a.frame_reps}")
        for k, (name, _) in enumerate(cases):
            out(f"  {name:38s} {fmt(times[k])}  ({int(rays[k].item())} rays, {int(shadow[k].item())} shadow rays)")
        spread_d = max(times[0]) - min(times[0])
        extra = med(times[1]) - med(times[0])
        n_shadow = int(shadow[1].item())
        out(f"  (e) - (d) = {extra:+.3f} ms ({100 * extra / med(times[0]):+.2f} %): {1e6 * extra / max(n_shadow, 1):.3f} ns per shadow ray; "
            f"(d) itself: {1e6 * med(times[0]) / int(rays[0].item()):.3f} ns per path ray")
        extra_f = med(times[2]) - med(times[0])
        out(f"  (f) - (d) = {extra_f:+.3f} ms ({100 * extra_f / med(times[0]):+.2f} %); (d)'s own spread is {spread_d:.3f} ms: "
            f"{'SLOWER by more than the spread' if extra_f > spread_d else 'within the spread'}")
        same = torch.equal(fix[2], fix[0]) and int(rays[2].item()) == int(rays[0].item())
        out(f"  (d) and (f) are {'EQUAL bit for bit, sums and ray counts' if same else 'DIFFERENT'}; (e) traces the path rays of (d): "
            f"{int(rays[1].item()) == int(rays[0].item())}")
        lit_px = [np.count_nonzero(fix[k].cpu().numpy().any(axis=2)) for k in (0, 1)]
        out(f"  pixels that receive light: (d) {lit_px[0]}, (e) {lit_px[1]} of {W * H}")

    import lights_ref as lr  # noqa: F401  (nee_ref composes it)
    import nee_ref as nr
    sflat, slight = nr.stat_scene()
    scam = nr.stat_camera()
    with rt.Renderer(0) as r:
        r.upload_scene(sflat)
        SL = rt.Lighting(slight.sky_bottom, slight.sky_top, np.array(slight.emission))
        frames = {True: [], False: []}
        stimes = {True: [], False: []}
        for rep in range(2):                                                     # (the first pass is the warm-up)
            for seed in nr.STAT_SEEDS:
                sp_ = rt.make_params(nr.STAT_W, nr.STAT_H, nr.STAT_SPP, max_depth=nr.STAT_DEPTH, seed=seed)
                for direct in (True, False):
                    t0 = time.perf_counter()
                    res = r.render_wavefront(scam, sp_, lighting=SL, direct=direct)
                    if rep:
                        stimes[direct].append((time.perf_counter() - t0) * 1e3)
                        frames[direct].append(res[0])
    mean, stderr, var_nee, var_lit = nr.stat_numbers(frames[True], frames[False])
    out(f"## (v) the stat scene of tests/nee_ref.py: {nr.STAT_W}x{nr.STAT_H}, {nr.STAT_SPP} spp, depth {nr.STAT_DEPTH}, {len(nr.STAT_SEEDS)} seeds")
    out(f"  frame-total energy, NEE - lit: mean {mean:+.4f}, standard error {stderr:.4f}: |mean| / stderr = {abs(mean) / stderr:.3f}")
    out(f"  per-pixel variance over the seeds, summed over the frame: lit {var_lit:.4f}, NEE {var_nee:.4f}: lit / NEE = {var_lit / var_nee:.3f} at equal spp")
    t_ratio = med(stimes[False]) / med(stimes[True])
    out(f"  host form, whole call: lit {fmt(stimes[False])}, NEE {fmt(stimes[True])}")
    out(f"  equal-time efficiency (variance ratio x time ratio lit / NEE): {var_lit / var_nee:.3f} x {t_ratio:.3f} = {var_lit / var_nee * t_ratio:.3f}")
    frame_ratio = med(times[0]) / med(times[1])
    out(f"  ... with the book frame's time ratio (d) / (e) = {frame_ratio:.3f} instead (the stat frame is too small to time a kernel by): "
        f"{var_lit / var_nee * frame_ratio:.3f}")


if __name__ == "__main__":
    main()
