#!/usr/bin/env python3
"""What choosing the light by its contribution at the hit point costs the lit path queue against the uniform choice, and what it buys
(profiles/weighted.txt).  Needs an MI355X.  The protocol of tools/paths_bench.py; a sibling of tools/cone_bench.py.

  (h) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, BEFORE this process opens the GPU (tools/paths_bench.py's own section (c)).
  The frame, 1200 x 675 x 16 spp on the book scene at night (a black sky), host clock around work that ends in a device synchronise, one
  warm-up, medians of --frame-reps, alternated in one process; (a) with the one small sphere of tools/cone_bench.py radiating
  (40, 32, 24) -- one light: the weighted frame is the cone frame bit for bit, so this is what the two walks cost when they can gain
  nothing --, (b) with eight small Lambertian spheres spread over the scene radiating the same:
  (d) rt_render_wavefront_lit_device -- the random walk;
  (g) rt_render_wavefront_nee_device with RT_DIRECT_CONE -- the yardstick;
  (w) ... with RT_DIRECT_WEIGHTED | RT_DIRECT_CONE.
  (v) the variance at equal samples per pixel on the eight-light 16 x 12 scene of tests/weighted_ref.py, 16 seeds, all three ways, over
      the pixels that see no light directly, and from it and the times of frame (b) the equal-time efficiency of weighted against cone
      and against lit.

usage: tools/weighted_bench.py [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
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

E_SMALL = (40.0, 32.0, 24.0)


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

    out(f"# tools/weighted_bench.py --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    dev = torch.device("cuda", 0)
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    os.environ.pop("RTIOW_WAVEFRONT_BATCH", None)
    os.environ.pop("RTIOW_PATHS_STEP_PARTS", None)
    lambertian_small = [k for k in range(len(flat)) if int(flat[k]["kind"]) == 0 and float(flat[k]["radius"]) < 0.5]
    # (a) tools/cone_bench.py's small light: the one nearest to the point (4, 0.2, 3), in front of the camera beside the large spheres
    small = min(lambertian_small, key=lambda k: float(np.linalg.norm(np.array(flat[k]["center"]) - np.array((4.0, 0.2, 3.0)))))
    # (b) eight of them spread over the scene: the list is built row by row over the ground, so evenly spaced entries are far apart
    eight = [lambertian_small[(2 * i + 1) * len(lambertian_small) // 16] for i in range(8)]
    cases = [("(d) lit", False, "area"), ("(g) NEE by cone", True, "cone"), ("(w) NEE weighted", True, "weighted")]
    med = statistics.median
    ratios = {}                                        # frame -> (t_cone / t_weighted, t_lit / t_weighted)

    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        out(f"book scene: {len(flat)} spheres; {W}x{H}, {SPP} samples per pixel: {W * H * SPP} paths; a black sky")
        p = rt.make_params(W, H, SPP, seed=1)
        cur = lambda: torch.cuda.current_stream().cuda_stream
        for frame, indices in (("(a) one small sphere", [small]), ("(b) eight small spheres", eight)):
            table = torch.zeros((len(flat), 3), dtype=torch.float64, device=dev)
            for index in indices:
                table[index] = torch.tensor(E_SMALL, dtype=torch.float64)
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
            where = "; ".join(f"{i} at ({flat[i]['center'][0]:.1f}, {flat[i]['center'][2]:.1f})" for i in indices)
            out(f"## the frame lit by {frame} (radius 0.2, e = {E_SMALL}; number and (x, z): {where}), {W}x{H}x{SPP}, host clock around work that "
                f"ends in a synchronise, alternated, medians of {a.frame_reps}")
            for k, (name, _, _) in enumerate(cases):
                out(f"  {name:20s} {fmt(times[k])}  ({int(rays[k].item())} rays, {int(shadow[k].item())} shadow rays)")
            for k in (1, 2):
                extra, n_shadow = med(times[k]) - med(times[0]), int(shadow[k].item())
                out(f"  {cases[k][0][:3]} - (d) = {extra:+.3f} ms ({100 * extra / med(times[0]):+.2f} %): {1e6 * extra / max(n_shadow, 1):.3f} ns per shadow ray")
            walks = med(times[2]) - med(times[1])
            out(f"  (w) - (g) = {walks:+.3f} ms ({100 * walks / med(times[1]):+.2f} % of the cone frame); (w) / (g) = {med(times[2]) / med(times[1]):.3f} in time, "
                f"{int(shadow[2].item()) / max(int(shadow[1].item()), 1):.3f} in shadow rays; all three trace the same path rays: "
                f"{int(rays[0].item()) == int(rays[1].item()) == int(rays[2].item())}")
            same = bool(torch.equal(fix[1], fix[2])) and int(shadow[1].item()) == int(shadow[2].item())
            out(f"  the weighted frame equals the cone frame bit for bit, sums and shadow rays: {same}" + ("" if len(indices) > 1 else " (one light: it must)"))
            lit_px = [np.count_nonzero(fix[k].cpu().numpy().any(axis=2)) for k in range(3)]
            out(f"  pixels that receive light: (d) {lit_px[0]}, (g) {lit_px[1]}, (w) {lit_px[2]} of {W * H}")
            ratios[frame] = (med(times[1]) / med(times[2]), med(times[0]) / med(times[2]))

    import nee_ref as nr
    import weighted_ref as wt
    sflat, slight = wt.many_light_scene()
    scam = nr.stat_camera()
    ways = (("weighted", True, "weighted"), ("cone", True, "cone"), ("lit", False, "area"))
    frames, stimes, nshadow, first = {w: [] for w, _, _ in ways}, {w: [] for w, _, _ in ways}, {w: 0 for w, _, _ in ways}, []
    with rt.Renderer(0) as r:
        r.upload_scene(sflat)
        SL = rt.Lighting(slight.sky_bottom, slight.sky_top, np.array(slight.emission))
        for rep in range(2):                                                     # (the first pass is the warm-up)
            for seed in wt.MANY_SEEDS:
                sp_ = rt.make_params(wt.MANY_W, wt.MANY_H, wt.MANY_SPP, max_depth=wt.MANY_DEPTH, seed=seed)
                for way, direct, sampling in ways:
                    t0 = time.perf_counter()
                    res = r.render_wavefront(scam, sp_, lighting=SL, direct=direct, sampling=sampling)
                    if rep:
                        stimes[way].append((time.perf_counter() - t0) * 1e3)
                        frames[way].append(res[0])
                        nshadow[way] += res[2]["shadow_rays"] if direct else 0
                if rep:
                    first.append(r.render_wavefront(scam, rt.make_params(wt.MANY_W, wt.MANY_H, wt.MANY_SPP, max_depth=1, seed=seed), lighting=SL)[0])
    mask = wt.indirect_pixels(first)
    out(f"## (v) the eight-light scene of tests/weighted_ref.py: {wt.MANY_W}x{wt.MANY_H}, {wt.MANY_SPP} spp, depth {wt.MANY_DEPTH}, {len(wt.MANY_SEEDS)} seeds; "
        f"{int(mask.sum())} of {mask.size} pixels see no light directly")
    var, var_all = {}, {}
    for other in ("lit", "cone"):
        mean, stderr, var["weighted"], var[other], var_all["weighted"], var_all[other] = wt.many_numbers(frames["weighted"], frames[other], mask)
        out(f"  energy on those pixels, weighted - {other}: mean {mean:+.4f}, standard error {stderr:.4f}: |mean| / stderr = {abs(mean) / stderr:.3f}")
    out(f"  per-pixel variance over the seeds, summed over those pixels: lit {var['lit']:.1f}, cone {var['cone']:.1f}, weighted {var['weighted']:.1f} "
        f"(the statement alone: 20504.9 / 19964.0 / 5294.1); over all {mask.size}: lit {var_all['lit']:.1f}, cone {var_all['cone']:.1f}, "
        f"weighted {var_all['weighted']:.1f}; shadow rays cone {nshadow['cone']}, weighted {nshadow['weighted']}")
    out(f"  at equal spp: cone / weighted = {var['cone'] / var['weighted']:.3f}, lit / weighted = {var['lit'] / var['weighted']:.3f}, lit / cone = {var['lit'] / var['cone']:.3f}")
    out(f"  host form, whole call: lit {fmt(stimes['lit'])}, cone {fmt(stimes['cone'])}, weighted {fmt(stimes['weighted'])}")
    t_cone, t_lit = ratios["(b) eight small spheres"]
    out("  equal-time efficiency of weighted (variance ratio x time ratio, the time ratio of the book frame (b): the 16 x 12 frame is too small to "
        "time a kernel by):")
    for other, t in (("cone", t_cone), ("lit", t_lit)):
        eff = var[other] / var["weighted"] * t
        out(f"    against {other}: {var[other] / var['weighted']:.3f} x {t:.3f} = {eff:.3f}" + ("  -- weighted LOSES at equal time" if eff < 1.0 else ""))


if __name__ == "__main__":
    main()
