#!/usr/bin/env python3
"""What the wavefront path steps cost (profiles/wavefront.txt).  Needs an MI355X.

Every kernel time is a pair of device events around ONE launch of the device form on a torch stream; three warm-ups, then REPS
repetitions with the kernels ALTERNATED within a repetition in one process; median, minimum, maximum and spread = (max - min) / median.
  (a) The three step kernels on the camera rays of a 1200 x 675 frame (16 samples per pixel: 12.96 M paths, pixel-major) and on their
      bounce-1 hits (rt_trace_rays of those rays on the book scene), each next to its own bytes per path at 6.3 TB/s (the rate DESIGN.md
      section 17 uses): the no-overlap streaming bound.  Bytes per path, every array once: camera 60 (8 in, 52 out); scatter 190 (89 in,
      8 event in and out, 97 out -- misses read 4 and write 1; the 80-byte material record of 530 spheres stays in cache and is not
      counted); accumulate 53 in plus 24 of atomic adds for a path that adds.  The accumulate kernel also runs without sky and select
      on every path, in pixel-major order (16 neighbouring lanes add to one pixel) and permuted.
  (b) The wavefront integrator's frame (rtiow_amd.render_wavefront_torch, batch 1 << 20) at 1200 x 675 x 16 spp next to rt_render_device
      for the same frame, alternated, host clock around work that ends in a device synchronise; then one instrumented pass of the same
      loop with a synchronise after every stage, to say where the time goes (trace, scatter, accumulate, camera rays, torch indexing).
      The two frames are compared bit for bit.
  (c) --parent-tree DIR: bench.py's headline from fresh processes of DIR (a built checkout of the parent commit) and of this tree,
      alternated, before this process opens the GPU.

usage: tools/shade_bench.py [--reps N] [--frame-reps N] [--parent-tree DIR] [--rounds N] [--out FILE]
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
BYTES = {"camera": 60, "scatter": 190, "accumulate": 53, "accumulate_add": 24}


def fmt(xs):
    med = statistics.median(xs)
    return f"{med:8.3f} ms (min {min(xs):.3f}, max {max(xs):.3f}, spread {100 * (max(xs) - min(xs)) / med:.1f} %)"


def headline(tree, steps, warmup):
    """One fresh process of bench.py in `tree` -> (Msamples/s, ms per step) of its JSON line."""
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

    # ---- (c) first: the child processes run while this one has not opened the GPU
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
    from rtiow_amd import _ffi

    out(f"# tools/shade_bench.py --reps {a.reps} --frame-reps {a.frame_reps}: {torch.cuda.get_device_name(0)}")
    stream = torch.cuda.Stream()
    dev = torch.device("cuda", 0)
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    seed = 1

    def timed(fn, before=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before:
            before()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        n = W * H * SPP
        out(f"book scene: {len(flat)} spheres; {W}x{H}, {SPP} samples per pixel: {n} paths, pixel-major")
        item = torch.arange(n, dtype=torch.int64, device=dev)
        pixel = torch.div(item, SPP, rounding_mode="floor").to(torch.int32)
        sample = (item % SPP).to(torch.int32)
        del item
        rays = rt.camera_rays_torch(r, cam, W, H, seed, pixel, sample)
        hit = rt.trace_rays_torch(r, rays["origin"], rays["dir"], want=("point", "normal", "front_face"))
        torch.cuda.synchronize()
        n_hit = int((hit["index"] >= 0).sum())
        miss = (hit["index"] < 0).to(torch.uint8)
        thr = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        event0 = rays["event"].clone()
        event = rays["event"].clone()
        o2, d2, att = (torch.empty((n, 3), dtype=torch.float64, device=dev) for _ in range(3))
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        fix = torch.zeros((H, W, 3), dtype=torch.int64, device=dev)
        out(f"  {n_hit} of the camera rays hit ({100 * n_hit / n:.1f} %): the scatter kernel's paths; the other {n - n_hit} are the accumulate kernel's")

        def k_camera():
            r.camera_rays_device(cam, W, H, seed, n, pixel.data_ptr(), sample.data_ptr(), rays["origin"].data_ptr(), rays["dir"].data_ptr(),
                                 rays["event"].data_ptr(), stream.cuda_stream)

        def k_scatter():
            r.scatter_device(seed, n, rays["dir"].data_ptr(), hit["index"].data_ptr(), hit["point"].data_ptr(), hit["normal"].data_ptr(),
                             hit["front_face"].data_ptr(), pixel.data_ptr(), sample.data_ptr(), event.data_ptr(), o2.data_ptr(), d2.data_ptr(),
                             att.data_ptr(), status.data_ptr(), stream.cuda_stream)

        def k_accumulate():
            r.accumulate_device(n, pixel.data_ptr(), thr.data_ptr(), fix.data_ptr(), W * H, rays["dir"].data_ptr(), miss.data_ptr(), stream.cuda_stream)

        def k_accumulate_all():
            r.accumulate_device(n, pixel.data_ptr(), thr.data_ptr(), fix.data_ptr(), W * H, 0, 0, stream.cuda_stream)

        # the same adds with the paths permuted: no run of 16 neighbouring lanes on one pixel's three words
        pixel_perm = pixel[torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(3))].contiguous()

        def k_accumulate_perm():
            r.accumulate_device(n, pixel_perm.data_ptr(), thr.data_ptr(), fix.data_ptr(), W * H, 0, 0, stream.cuda_stream)

        runs = {"camera": k_camera, "scatter": k_scatter, "accumulate": k_accumulate, "accumulate_all": k_accumulate_all,
                "accumulate_perm": k_accumulate_perm}
        times = {k: [] for k in runs}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for rep in range(3 + a.reps):
                for k, fn in runs.items():
                    # (every scatter launch starts from the same events: the copy runs on the stream, before the first event)
                    ms = timed(fn, before=(lambda: event.copy_(event0)) if k == "scatter" else None)
                    if rep >= 3:
                        times[k].append(ms)
        out("## (a) the step kernels, one launch each, beside their own bytes at 6.3 TB/s (the no-overlap streaming bound)")
        n_miss = n - n_hit
        # scatter: a miss reads its index and writes its status; accumulate: every path reads its select byte, a path that adds the rest
        bounds = {"camera": n * BYTES["camera"], "scatter": n_hit * BYTES["scatter"] + n_miss * 5,
                  "accumulate": n * 1 + n_miss * (BYTES["accumulate"] - 1 + BYTES["accumulate_add"]),
                  "accumulate_all": n * (4 + 24 + BYTES["accumulate_add"]), "accumulate_perm": n * (4 + 24 + BYTES["accumulate_add"])}
        label = {"camera": f"camera_rays_kernel   {n} paths", "scatter": f"scatter_kernel       {n_hit} hits + {n_miss} misses",
                 "accumulate": f"accumulate_kernel    sky, select: {n_miss} of {n} add", "accumulate_all": f"accumulate_kernel    no sky, no select: {n} add",
                 "accumulate_perm": f"accumulate_kernel    the same, paths permuted: {n} add"}
        for k in runs:
            b_ms = bounds[k] / HBM_RATE * 1e3
            m = statistics.median(times[k])
            out(f"  {label[k]:62s} {fmt(times[k])}; {bounds[k] / 1e6:.0f} MB = {b_ms:.3f} ms at 6.3 TB/s; time / bound = {m / b_ms:.2f}; "
                f"{bounds[k] / m / 1e9:.2f} TB/s")
        save()
        del rays, hit, thr, o2, d2, att, status, event, event0, miss, pixel, sample, pixel_perm

        # ---- (b) the frame
        p = rt.make_params(W, H, SPP, seed=seed)
        d_fix = torch.zeros((H, W, 3), dtype=torch.int64, device=dev)

        def dense():
            t0 = time.perf_counter()
            r.render_device(cam, p, d_fix.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def wavefront():
            t0 = time.perf_counter()
            f, nrays = rt.render_wavefront_torch(r, cam, p)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, f, nrays

        td, tw = [], []
        for rep in range(1 + a.frame_reps):
            ms_d = dense()
            ms_w, wf, nrays = wavefront()
            if rep >= 1:
                td.append(ms_d); tw.append(ms_w)
        st = r.last_stats()
        equal = bool(torch.equal(wf, d_fix))
        out(f"## (b) the frame, {W}x{H}x{SPP}, host clock around work that ends in a synchronise, alternated")
        out(f"  rt_render_device              {fmt(td)}  (kernel {st['kernel_ms']:.3f} ms, {st['rays_traced']} rays)")
        out(f"  render_wavefront_torch        {fmt(tw)}  ({nrays} rays, batch {1 << 20}); wavefront / megakernel = {statistics.median(tw) / statistics.median(td):.1f}")
        out(f"  the two frames are {'EQUAL bit for bit' if equal else 'DIFFERENT'}; ray counts {'equal' if nrays == st['rays_traced'] else 'DIFFER'}")
        save()

        # one instrumented pass of the same loop: a synchronise after every stage
        stage = {"camera rays": 0.0, "trace": 0.0, "accumulate": 0.0, "scatter": 0.0, "torch indexing": 0.0}
        launches = 0

        def staged(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            stage[name] += (time.perf_counter() - t0) * 1e3
            return res

        batch = 1 << 20
        t_all = time.perf_counter()
        for begin in range(0, n, batch):
            def start():
                it = torch.arange(begin, min(begin + batch, n), dtype=torch.int64, device=dev)
                return torch.div(it, SPP, rounding_mode="floor").to(torch.int32), (it % SPP).to(torch.int32)
            px, sm = staged("torch indexing", start)
            cr = staged("camera rays", lambda: rt.camera_rays_torch(r, cam, W, H, seed, px, sm))
            org, dr, ev = cr["origin"], cr["dir"], cr["event"]
            th = staged("torch indexing", lambda: torch.ones((px.shape[0], 3), dtype=torch.float64, device=dev))
            for _ in range(int(p.max_depth)):
                if px.shape[0] == 0:
                    break
                launches += 1
                ht = staged("trace", lambda: rt.trace_rays_torch(r, org, dr, t_min=float(p.t_min), want=("point", "normal", "front_face")))
                sel = staged("torch indexing", lambda: (ht["index"] < 0).to(torch.uint8))
                staged("accumulate", lambda: rt.accumulate_torch(r, d_fix, px, th, sky_dir=dr, select=sel))
                sc = staged("scatter", lambda: rt.scatter_torch(r, seed, dr, ht["index"], ht["point"], ht["normal"], ht["front_face"], px, sm, ev))

                def compact():
                    keep = torch.nonzero(sc["status"] == _ffi.RT_SCATTER_SCATTERED).squeeze(1)
                    return th[keep] * sc["attenuation"][keep], px[keep], sm[keep], ev[keep], sc["out_origin"][keep], sc["out_dir"][keep]
                th, px, sm, ev, org, dr = staged("torch indexing", compact)
        total = (time.perf_counter() - t_all) * 1e3
        out(f"  instrumented pass (a synchronise after every stage; {launches} bounce iterations): {total:.1f} ms in all")
        for k, v in stage.items():
            out(f"    {k:16s} {v:9.1f} ms  {100 * v / total:5.1f} %")
    save()


if __name__ == "__main__":
    main()
