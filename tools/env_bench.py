#!/usr/bin/env python3
"""What an environment cube map costs the lit path queue, and what sampling it buys (profiles/env.txt).  Needs an
MI355X.  The protocol of tools/paths_bench.py; a sibling of tools/nee_bench.py.

  (h) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, BEFORE this process opens the GPU (tools/paths_bench.py's own section (c)).
  The frame, 1200 x 675 x 16 spp on the book scene, host clock around work that ends in a device synchronise, one warm-up, medians of
  --frame-reps, alternated in one process:
  (a) rt_render_wavefront_lit_device under the reference sky, no light: the yardstick;
  (b) rt_render_wavefront_env_device under a size-64 Environment.sun_sky, not sampled;
  (c) the same environment, sampled;
  (d) (c) at size 512.
  (v) the variance at equal samples per pixel: the scene, the 16 seeds and the numbers of tests/test_gpu_env.py's variance test
      (tests/env_ref.py: stat_scene, stat_numbers), and the time of its frames both ways.

usage: tools/env_bench.py [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
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

SUN = dict(sun_dir=(0.3, 0.8, 0.6), sun_radiance=(400.0, 360.0, 300.0), cos_radius=0.999)


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

    out(f"# tools/env_bench.py --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    dev = torch.device("cuda", 0)
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    os.environ.pop("RTIOW_PATHS_STEP_PARTS", None)
    L = rt.Lighting()
    small, large = rt.Environment.sun_sky(64, **SUN).table(), rt.Environment.sun_sky(512, **SUN).table()
    cases = [("(a) lit, the reference sky", None), ("(b) environment 64, looked up", rt.Environment(small, sample=False)),
             ("(c) environment 64, sampled", rt.Environment(small, sample=True)), ("(d) environment 512, sampled", rt.Environment(large, sample=True))]
    med = statistics.median

    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        out(f"book scene: {len(flat)} spheres; {W}x{H}, {SPP} samples per pixel: {W * H * SPP} paths; the sun: {SUN}")
        p = rt.make_params(W, H, SPP, seed=1)
        fix = [torch.zeros((H, W, 3), dtype=torch.int64, device=dev) for _ in cases]
        rays = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in cases]
        shadow = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in cases]
        times = [[] for _ in cases]
        cur = lambda: torch.cuda.current_stream().cuda_stream
        for rep in range(1 + a.frame_reps):
            for k, (_, env) in enumerate(cases):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.render_wavefront_device(cam, p, fix[k].data_ptr(), rays[k].data_ptr(), cur(), lighting=L, environment=env,
                                          d_shadow_rays_ptr=shadow[k].data_ptr() if env is not None else 0)
                torch.cuda.synchronize()
                if rep >= 1:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        out(f"## the frame, {W}x{H}x{SPP}, host clock around work that ends in a synchronise, alternated, medians of {a.frame_reps}")
        for k, (name, _) in enumerate(cases):
            out(f"  {name:38s} {fmt(times[k])}  ({int(rays[k].item())} rays, {int(shadow[k].item())} shadow rays)")
        spread_a = max(times[0]) - min(times[0])
        for k, tag in ((1, "(b)"), (2, "(c)"), (3, "(d)")):
            extra = med(times[k]) - med(times[0])
            out(f"  {tag} - (a) = {extra:+.3f} ms ({100 * extra / med(times[0]):+.2f} %); (a)'s own spread is {spread_a:.3f} ms: "
                f"{'SLOWER by more than the spread' if extra > spread_a else 'not slower'}")
        n_shadow = int(shadow[2].item())
        extra_c = med(times[2]) - med(times[1])
        out(f"  (c) - (b) = {extra_c:+.3f} ms: {1e6 * extra_c / max(n_shadow, 1):.3f} ns per shadow ray, the search of {6 * 64 * 64} running sums "
            f"included; (b) itself: {1e6 * med(times[1]) / int(rays[1].item()):.3f} ns per path ray")
        extra_d = med(times[3]) - med(times[2])
        out(f"  (d) - (c) = {extra_d:+.3f} ms: {1e6 * extra_d / max(int(shadow[3].item()), 1):.3f} ns per shadow ray for 6 more steps of the search "
            f"in a table of {6 * 512 * 512 * 8 / 2 ** 20:.0f} MiB")
        out(f"  (b) and (c) trace the same path rays: {int(rays[1].item()) == int(rays[2].item())}")

    import env_ref as er
    sflat, slight = er.stat_scene()
    scam = er.stat_camera()
    texels = er.stat_environment().table()
    with rt.Renderer(0) as r:
        r.upload_scene(sflat)
        SL = rt.Lighting(slight.sky_bottom, slight.sky_top, None)
        frames = {True: [], False: []}
        stimes = {True: [], False: []}
        for rep in range(2):                                                     # (the first pass is the warm-up)
            for seed in er.STAT_SEEDS:
                sp_ = rt.make_params(er.STAT_W, er.STAT_H, er.STAT_SPP, max_depth=er.STAT_DEPTH, seed=seed)
                for sample in (True, False):
                    t0 = time.perf_counter()
                    res = r.render_wavefront(scam, sp_, lighting=SL, environment=rt.Environment(texels, sample=sample))
                    if rep:
                        stimes[sample].append((time.perf_counter() - t0) * 1e3)
                        frames[sample].append(res[0])
    mean, stderr, var_s, var_p = er.stat_numbers(frames[True], frames[False])
    out(f"## (v) the stat scene of tests/env_ref.py: {er.STAT_W}x{er.STAT_H}, {er.STAT_SPP} spp, depth {er.STAT_DEPTH}, {len(er.STAT_SEEDS)} seeds")
    out(f"  frame-total energy, sampled - unsampled: mean {mean:+.4f}, standard error {stderr:.4f}: |mean| / stderr = {abs(mean) / stderr:.3f}")
    out(f"  per-pixel variance over the seeds, summed over the frame: unsampled {var_p:.4f}, sampled {var_s:.4f}: unsampled / sampled = "
        f"{var_p / var_s:.3f} at equal spp")
    out(f"  host form, whole call: unsampled {fmt(stimes[False])}, sampled {fmt(stimes[True])}")
    frame_ratio = med(times[1]) / med(times[2])
    out(f"  equal-time efficiency with the book frame's time ratio (b) / (c) = {frame_ratio:.3f} (the stat frame is too small to time a kernel by): "
        f"{var_p / var_s * frame_ratio:.3f}")


if __name__ == "__main__":
    main()
