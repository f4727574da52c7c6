#!/usr/bin/env python3
"""Host time per launch of two builds of the library, A against B, interleaved: (a) the `python bench.py` headline and (b) the wall
time of the tiny launch 400x225x10 through rt_render_rgba8.  Every sample is a fresh process that loads one library through
RTIOW_HIP_LIB; a pair is A then B or B then A, the order alternating from pair to pair.  Give the same build twice (a copy of the
file: two loads) for the spread of a build against itself.  A sample that fails or times out ends the run.
usage: python3 tools/launch_path_ab.py LIB_A LIB_B [PAIRS=6]       e.g. tools/var_parent.so rtiow_amd/librtiow_hip.so
       python3 tools/launch_path_ab.py --tiny                       (one sample of (b), the library from RTIOW_HIP_LIB)"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny():
    sys.path.insert(0, ROOT)
    import rtiow_amd as rt
    w, h, spp, n = 400, 225, 10, 600
    r = rt.Renderer(0)
    r.upload_scene(rt.random_scene(1).flatten())
    cam, p = rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=1)
    for _ in range(50):
        r.render_rgba8(cam, p)
    wall, kern = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        _, st = r.render_rgba8(cam, p)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(st["kernel_ms"])
    print(json.dumps({"wall_ms": statistics.median(wall), "kernel_ms": statistics.median(kern)}))


def sample(lib, cmd, limit):
    env = dict(os.environ, RTIOW_HIP_LIB=os.path.abspath(lib))
    run = subprocess.run([sys.executable, *cmd], env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if run.returncode != 0:
        sys.exit(f"{lib}: {' '.join(cmd)} ended with {run.returncode}\n{run.stderr[-1500:]}")
    return json.loads(run.stdout.strip().splitlines()[-1])


def main():
    lib_a, lib_b = sys.argv[1], sys.argv[2]
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    print(f"# A = {lib_a}, B = {lib_b}; {pairs} pairs, order alternating; every figure one fresh process")
    print("# (a) python bench.py --steps 20 --warmup 5: ms per step of 1200x675x500   (b) rt_render_rgba8 400x225x10: median wall ms of 600 calls (kernel ms)")
    rows = {"a": [], "b": []}
    for k in range(pairs):
        order = "AB" if k % 2 == 0 else "BA"
        got = {}
        for which in order:
            lib = lib_a if which == "A" else lib_b
            got[which] = (sample(lib, ["bench.py", "--steps", "20", "--warmup", "5"], 300)["ms_per_step"],
                          sample(lib, [os.path.join("tools", "launch_path_ab.py"), "--tiny"], 300))
        da = (got["B"][0] / got["A"][0] - 1) * 100
        db = (got["B"][1]["wall_ms"] / got["A"][1]["wall_ms"] - 1) * 100
        rows["a"].append(da)
        rows["b"].append(db)
        print(f"pair {k} {order}: (a) A {got['A'][0]:.4f} B {got['B'][0]:.4f} ms  B/A {da:+.2f} %   "
              f"(b) A {got['A'][1]['wall_ms']:.4f} ({got['A'][1]['kernel_ms']:.4f}) B {got['B'][1]['wall_ms']:.4f} ({got['B'][1]['kernel_ms']:.4f}) ms  B/A {db:+.2f} %", flush=True)
    for key in ("a", "b"):
        v = rows[key]
        print(f"({key}) B/A: median {statistics.median(v):+.2f} %, mean {statistics.mean(v):+.2f} %, range {min(v):+.2f} .. {max(v):+.2f} %")


if __name__ == "__main__":
    tiny() if sys.argv[1:] == ["--tiny"] else main()
