#!/usr/bin/env python3
"""What sampling a light by solid angle costs the lit path queue against sampling it by area, and what it buys (profiles/cone.txt,
DESIGN.md section 22).  Needs an MI355X.  The protocol of tools/paths_bench.py; a sibling of tools/nee_bench.py.

  (h) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, BEFORE this process opens the GPU (tools/paths_bench.py's own section (c)).
  The frame, 1200 x 675 x 16 spp on the book scene at night (a black sky), host clock around work that ends in a device synchronise, one
  warm-up, medians of --frame-reps, alternated in one process; once with the large Lambertian sphere radiating (4, 3.2, 2.4), once
  with one small sphere radiating (40, 32, 24) instead:
  (d) rt_render_wavefront_lit_device -- the yardstick;
  (e) rt_render_wavefront_nee_device, the light sampled by area;
  (g) ... by solid angle (RT_DIRECT_CONE).
  (v) the variance at equal samples per pixel on the two 16 x 12 scenes of tests/test_gpu_cone.py (tests/cone_ref.py: big_light_scene;
      tests/nee_ref.py: stat_scene), 16 seeds, all three ways, and from it and the frames' times the equal-time efficiency of cone against
      area and against lit.

usage: tools/cone_bench.py [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
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

    out(f"# tools/cone_bench.py --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    dev = torch.device("cuda", 0)
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    os.environ.pop("RTIOW_PATHS_STEP_PARTS", None)
    big = [k for k in range(len(flat)) if int(flat[k]["kind"]) == 0 and float(flat[k]["radius"]) == 1.0][0]
    # the small light: the Lambertian sphere of radius < 0.5 nearest to the point (4, 0.2, 3), in front of the camera beside the large spheres
    small = min((k for k in range(len(flat)) if int(flat[k]["kind"]) == 0 and float(flat[k]["radius"]) < 0.5),
                key=lambda k: float(np.linalg.norm(np.array(flat[k]["center"]) - np.array((4.0, 0.2, 3.0)))))
    cases = [("(d) lit", False, "area"), ("(e) NEE by area", True, "area"), ("(g) NEE by cone", True, "cone")]
    med = statistics.median
    ratios = {}                                        # light -> (t_area / t_cone, t_lit / t_cone) of the book frame

    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        out(f"book scene: {len(flat)} spheres; {W}x{H}, {SPP} samples per pixel: {W * H * SPP} paths; a black sky")
        p = rt.make_params(W, H, SPP, seed=1)
        cur = lambda: torch.cuda.current_stream().cuda_stream
        for light_name, index, e in (("the large sphere", big, (4.0, 3.2, 2.4)), ("one small sphere", small, (40.0, 32.0, 24.0))):
            table = torch.zeros((len(flat), 3), dtype=torch.float64, device=dev)
            table[index] = torch.tensor(e, dtype=torch.float64)
            L = rt.Lighting((0, 0, 0), (0, 0, 0), table)
            fix = [torch.zeros((H, W, 3), dtype=torch.int64, device=dev) for _ in cases]
            rays = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in cases]
            shadow = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in cases]
            times = [[] for _ in cases]
            for rep in range(1 + a.frame_reps):
                for k, (_, direct, sampling) in enumerate(cases):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r.render_wavefront_device(cam, p, fix[k].data_ptr(), rays[k].data_ptr(), cur(), lighting=L, direct=direct,
                                              d_shadow_rays_ptr=shadow[k].data_ptr() if direct else 0, sampling=sampling)
                    torch.cuda.synchronize()
                    if rep >= 1:
                        times[k].append((time.perf_counter() - t0) * 1e3)
            c = flat[index]["center"]
            out(f"## the frame lit by {light_name} (number {index}, centre ({c[0]:.2f}, {c[1]:.2f}, {c[2]:.2f}), radius {float(flat[index]['radius']):.2f}, "
                f"e = {e}), {W}x{H}x{SPP}, host clock around work that ends in a synchronise, alternated, medians of {a.frame_reps}")
            for k, (name, _, _) in enumerate(cases):
                out(f"  {name:20s} {fmt(times[k])}  ({int(rays[k].item())} rays, {int(shadow[k].item())} shadow rays)")
            for k in (1, 2):
                extra, n_shadow = med(times[k]) - med(times[0]), int(shadow[k].item())
                out(f"  {cases[k][0][:3]} - (d) = {extra:+.3f} ms ({100 * extra / med(times[0]):+.2f} %): {1e6 * extra / max(n_shadow, 1):.3f} ns per shadow ray")
            out(f"  (d) itself: {1e6 * med(times[0]) / int(rays[0].item()):.3f} ns per path ray; (g) / (e) = {med(times[2]) / med(times[1]):.3f} in time, "
                f"{int(shadow[2].item()) / max(int(shadow[1].item()), 1):.3f} in shadow rays; all three trace the same path rays: "
                f"{int(rays[0].item()) == int(rays[1].item()) == int(rays[2].item())}")
            lit_px = [np.count_nonzero(fix[k].cpu().numpy().any(axis=2)) for k in range(3)]
            out(f"  pixels that receive light: (d) {lit_px[0]}, (e) {lit_px[1]}, (g) {lit_px[2]} of {W * H}")
            ratios[light_name] = (med(times[1]) / med(times[2]), med(times[0]) / med(times[2]))

    import cone_ref as cr
    import nee_ref as nr
    scenes = [("the big-light scene of tests/cone_ref.py", cr.big_light_scene(), cr.big_light_camera(), "the large sphere",
               "53606.8 / 6547.7 / 9360.5"),
              ("the stat scene of tests/nee_ref.py (a small far light)", nr.stat_scene(), nr.stat_camera(), "one small sphere",
               "1377.6 / 1270.3 / 20371.5")]
    for title, (sflat, slight), scam, book_light, statement in scenes:
        ways = (("cone", True, "cone"), ("area", True, "area"), ("lit", False, "area"))
        frames, stimes, nshadow = {w: [] for w, _, _ in ways}, {w: [] for w, _, _ in ways}, {w: 0 for w, _, _ in ways}
        with rt.Renderer(0) as r:
            r.upload_scene(sflat)
            SL = rt.Lighting(slight.sky_bottom, slight.sky_top, np.array(slight.emission))
            for rep in range(2):                                                     # (the first pass is the warm-up)
                for seed in nr.STAT_SEEDS:
                    sp_ = rt.make_params(nr.STAT_W, nr.STAT_H, nr.STAT_SPP, max_depth=nr.STAT_DEPTH, seed=seed)
                    for way, direct, sampling in ways:
                        t0 = time.perf_counter()
                        res = r.render_wavefront(scam, sp_, lighting=SL, direct=direct, sampling=sampling)
                        if rep:
                            stimes[way].append((time.perf_counter() - t0) * 1e3)
                            frames[way].append(res[0])
                            nshadow[way] += res[2]["shadow_rays"] if direct else 0
        out(f"## (v) {title}: {nr.STAT_W}x{nr.STAT_H}, {nr.STAT_SPP} spp, depth {nr.STAT_DEPTH}, {len(nr.STAT_SEEDS)} seeds")
        for other in ("lit", "area"):
            mean, stderr, _, _ = nr.stat_numbers(frames["cone"], frames[other])
            out(f"  frame-total energy, cone - {other}: mean {mean:+.4f}, standard error {stderr:.4f}: |mean| / stderr = {abs(mean) / stderr:.3f}")
        var = {w: nr.stat_numbers(frames[w], frames[w])[2] for w in frames}
        out(f"  per-pixel variance over the seeds, summed over the frame: area {var['area']:.1f}, cone {var['cone']:.1f}, lit {var['lit']:.1f} "
            f"(the statement alone: {statement}); shadow rays area {nshadow['area']}, cone {nshadow['cone']}")
        out(f"  at equal spp: area / cone = {var['area'] / var['cone']:.3f}, lit / cone = {var['lit'] / var['cone']:.3f}, lit / area = {var['lit'] / var['area']:.3f}")
        out(f"  host form, whole call: lit {fmt(stimes['lit'])}, area {fmt(stimes['area'])}, cone {fmt(stimes['cone'])}")
        t_area, t_lit = ratios[book_light]
        out(f"  equal-time efficiency of cone (variance ratio x time ratio, the time ratio of the book frame lit by {book_light}: the 16 x 12 "
            f"frame is too small to time a kernel by):")
        for other, t in (("area", t_area), ("lit", t_lit)):
            eff = var[other] / var["cone"] * t
            out(f"    against {other}: {var[other] / var['cone']:.3f} x {t:.3f} = {eff:.3f}" + ("  -- cone LOSES at equal time" if eff < 1.0 else ""))


if __name__ == "__main__":
    main()
