#!/usr/bin/env python3
"""What the adaptive loop over the wavefront frame buys against the uniform NEE frame, and what a pass over a list costs when the list is
short (profiles/wavefront_adaptive.txt).  Needs an MI355X.  The protocol of tools/nee_bench.py: one warm-up, medians
of --frame-reps, alternated in one process, host clock around work that ends in a device synchronise.

  (h) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, BEFORE this process opens the GPU; and
  (n) rt_render_wavefront_nee_device (1200 x 675 x 16 spp, the frame below, RT_DIRECT_WEIGHTED | RT_DIRECT_CONE) from fresh processes
      of both trees, alternated likewise: the existing frames are not slower (this script with --nee-frame-only --tree DIR).
  The frame: the book scene at night (a black sky) lit by its large Lambertian sphere radiating (4, 3.2, 2.4), the light chosen by its
  contribution and sampled by solid angle (rtiow_render --wavefront --sky 0,0,0:0,0,0 --emit K:4,3.2,2.4 --direct-weighted), 1200 x 675:
  (a) the uniform NEE frame at 64 spp (rt_render_wavefront_nee_sampled);
  (b) the adaptive frame with cap 64, step 8 and threshold 0.05 (rt_render_wavefront_adaptive), and the histogram of its counts;
  (c) the fixed cost of one pass: a one-pixel list, 8 spp (rt_render_wavefront_pixels).
  For each: time, samples, path rays, shadow rays.

usage: tools/wavefront_adaptive_bench.py [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = ROOT
if "--tree" in sys.argv:
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from paths_bench import H, W, fmt, headline  # noqa: E402

sys.path.insert(0, TREE)                           # (paths_bench puts its own tree first: the package comes from --tree)

EMIT = (4.0, 3.2, 2.4)
CAP, STEP, THRESHOLD = 64, 8, 0.05


def night(rt):
    """(flat, the index of the large Lambertian sphere, the Lighting)."""
    flat = rt.random_scene(1).flatten()
    big = next(k for k in range(len(flat)) if int(flat[k]["kind"]) == 0 and float(flat[k]["radius"]) == 1.0)
    return flat, big, rt.Lighting((0, 0, 0), (0, 0, 0), {big: EMIT})


def nee_frame_only(reps):
    """One line: the median host-clock time of the NEE device frame at 16 spp in this process's tree."""
    import torch
    import rtiow_amd as rt
    dev = torch.device("cuda", 0)
    flat, big, L = night(rt)
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        p = rt.make_params(W, H, 16, seed=1)
        fix = torch.zeros((H, W, 3), dtype=torch.int64, device=dev)
        rays, shadow = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        times = []
        for rep in range(1 + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.render_wavefront_device(rt.book1_camera(W, H), p, fix.data_ptr(), rays.data_ptr(), torch.cuda.current_stream().cuda_stream, lighting=L,
                                      direct=True, d_shadow_rays_ptr=shadow.data_ptr(), sampling="weighted")
            torch.cuda.synchronize()
            if rep >= 1:
                times.append((time.perf_counter() - t0) * 1e3)
    assert os.path.dirname(os.path.dirname(os.path.abspath(rt.__file__))) == TREE, (rt.__file__, TREE)
    print(f"NEE_FRAME_MS {statistics.median(times):.4f} {int(rays.item())} {int(shadow.item())} {int(fix.sum().item())}")


def nee_frame_of(tree, reps):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--nee-frame-only", "--tree", tree, "--frame-reps", str(reps)], cwd=tree,
                         capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        sys.exit(f"--nee-frame-only failed in {tree}: {run.stderr[-2000:]}")
    word = [ln for ln in run.stdout.splitlines() if ln.startswith("NEE_FRAME_MS")][-1].split()
    return float(word[1]), tuple(int(x) for x in word[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame-reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nee-frame-only", action="store_true")
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    if a.nee_frame_only:
        return nee_frame_only(a.frame_reps)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    sp = lambda xs: 100 * (max(xs) - min(xs)) / statistics.median(xs)
    if a.parent_tree:
        out("## (h) bench.py --gpus 1 --steps 10 --warmup 3: the parent commit's tree and this one, alternated, fresh processes (Msamples/s, ms per step)")
        vals = {"parent": [], "tree": []}
        for rnd in range(1, a.rounds + 1):
            for name, tree in (("parent", a.parent_tree), ("tree", ROOT)):
                v, ms = headline(tree, 10, 3)
                vals[name].append(v)
                out(f"{name} round {rnd}".ljust(18) + f" {v:8.2f} Msamples/s  {ms:.3f} ms")
        out(f"parent median {statistics.median(vals['parent']):.2f} (run-to-run spread {sp(vals['parent']):.2f} %), tree median "
            f"{statistics.median(vals['tree']):.2f} (spread {sp(vals['tree']):.2f} %), tree / parent = "
            f"{statistics.median(vals['tree']) / statistics.median(vals['parent']):.4f}")
        out(f"## (n) rt_render_wavefront_nee_device, {W}x{H}x16, weighted: both trees, alternated, fresh processes, the median of {a.frame_reps} in each (ms)")
        vals, results = {"parent": [], "tree": []}, set()
        for rnd in range(1, a.rounds + 1):
            for name, tree in (("parent", a.parent_tree), ("tree", ROOT)):
                ms, result = nee_frame_of(tree, a.frame_reps)
                vals[name].append(ms)
                results.add(result)
                out(f"{name} round {rnd}".ljust(18) + f" {ms:9.3f} ms")
        out(f"parent median {statistics.median(vals['parent']):.3f} ms (run-to-run spread {sp(vals['parent']):.2f} %), tree median "
            f"{statistics.median(vals['tree']):.3f} ms (spread {sp(vals['tree']):.2f} %), tree / parent = "
            f"{statistics.median(vals['tree']) / statistics.median(vals['parent']):.4f}; rays, shadow rays and the sum of the sums agree in all "
            f"{2 * a.rounds} runs: {len(results) == 1}")

    import numpy as np
    import torch
    import rtiow_amd as rt

    out(f"# tools/wavefront_adaptive_bench.py --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    flat, big, L = night(rt)
    cam = rt.book1_camera(W, H)
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    os.environ.pop("RTIOW_PATHS_STEP_PARTS", None)
    one_pixel = np.array([(H // 2) * W + W // 2], dtype=np.uint32)
    times, kernel = {"a": [], "b": [], "c": []}, {"a": [], "b": [], "c": []}
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        out(f"book scene at night: {len(flat)} spheres, sphere {big} radiates {EMIT}; {W}x{H}; direct lighting weighted, by solid angle")
        p, p_pass = rt.make_params(W, H, CAP, seed=1), rt.make_params(W, H, STEP, seed=1)
        ad = rt.make_adaptive(STEP, THRESHOLD, 0.01)
        for rep in range(1 + a.frame_reps):
            t0 = time.perf_counter()
            fa, sa = r.render_wavefront_pixels(cam, p, None, lighting=L, direct=True, sampling="weighted")
            t1 = time.perf_counter()
            fb, _, count, sb = r.render_wavefront_adaptive(cam, p, ad, lighting=L, direct=True, sampling="weighted", want_half=False)
            t2 = time.perf_counter()
            fc, sc = r.render_wavefront_pixels(cam, p_pass, one_pixel, lighting=L, direct=True, sampling="weighted")
            t3 = time.perf_counter()
            if rep >= 1:
                for key, dt, st in (("a", t1 - t0, sa), ("b", t2 - t1, sb), ("c", t3 - t2, sc)):
                    times[key].append(dt * 1e3)
                    kernel[key].append(st["kernel_ms"])
        dense_fix, dense_rays, dense_st = r.render_wavefront(cam, p, lighting=L, direct=True, sampling="weighted")
    out(f"## host form, whole call (the copies of the {W * H * 24 / 1e6:.1f} MB frame included) and the device time inside it, alternated, medians of {a.frame_reps}")
    npix = W * H
    out(f"  (a) uniform NEE, {CAP} spp            whole call {fmt(times['a'])}; device {fmt(kernel['a'])}")
    out(f"      {npix * CAP} samples, {sa['rays_traced']} path rays, {sa['shadow_rays']} shadow rays; equals rt_render_wavefront_nee_sampled bit for bit: "
        f"{bool(np.array_equal(fa, dense_fix)) and sa['rays_traced'] == dense_rays and sa['shadow_rays'] == dense_st['shadow_rays']}")
    out(f"  (b) adaptive, cap {CAP} step {STEP} thr {THRESHOLD}  whole call {fmt(times['b'])}; device {fmt(kernel['b'])}")
    out(f"      {sb['samples']} samples ({sb['samples'] / npix:.2f} per pixel), {sb['rays']} path rays, {sb['shadow_rays']} shadow rays")
    values, pixels = np.unique(count, return_counts=True)
    out("      count histogram: " + ", ".join(f"{int(v)}: {int(n)} ({100 * n / npix:.1f} %)" for v, n in zip(values, pixels)))
    med = statistics.median
    out(f"      (b) / (a): device time {med(kernel['b']) / med(kernel['a']):.3f}, whole call {med(times['b']) / med(times['a']):.3f}, samples "
        f"{sb['samples'] / (npix * CAP):.3f}, path rays {sb['rays'] / sa['rays_traced']:.3f}, shadow rays {sb['shadow_rays'] / max(sa['shadow_rays'], 1):.3f}")
    out(f"      device time per million samples: (a) {1e6 * med(kernel['a']) / (npix * CAP):.3f} ms, (b) {1e6 * med(kernel['b']) / sb['samples']:.3f} ms")
    out(f"  (c) one pixel, {STEP} spp: one pass      whole call {fmt(times['c'])}; device {fmt(kernel['c'])}")
    out(f"      {STEP} samples, {sc['rays_traced']} path rays, {sc['shadow_rays']} shadow rays: one begin and {p_pass.max_depth} steps of three launches, and the zeroing of the frame")


if __name__ == "__main__":
    main()
