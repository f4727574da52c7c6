#!/usr/bin/env python3
"""A / A' / B timing of three builds of the library through bench.py, the method of profiles/scalar_trim*_ab.txt: A the parent's library, A' a second
build of the parent (the spread of a build against itself), B the new one; every figure a fresh process that loads one library through
RTIOW_HIP_LIB, the order rotating from round to round; every run under a time limit of its own, and the first failure ends the script.

usage: tools/bench_abc.py ROUNDS A.so A2.so B.so [bench.py arguments; default: --steps 10 --warmup 2 --no-other-configs]"""
import itertools, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rounds = int(sys.argv[1])
libs = dict(zip("ACB", sys.argv[2:5]))
bench_args = sys.argv[5:] or ["--steps", "10", "--warmup", "2", "--no-other-configs"]
orders = ["ACB", "BCA", "CBA", "BAC", "CAB", "ABC"]
print(f"# {libs}; bench.py --gpus 1 {' '.join(bench_args)}; {rounds} rounds, order rotating; kernel ms (HIP events, mean of the steps) / ms per step", flush=True)
res = {k: [] for k in libs}
for r, order in zip(range(rounds), itertools.cycle(orders)):
    got = {}
    for k in order:
        env = dict(os.environ, RTIOW_HIP_LIB=os.path.join(ROOT, libs[k]))
        p = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "bench.py", "--gpus", "1", *bench_args], cwd=ROOT, env=env, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"round {r} {k}: bench.py exit status {p.returncode}\n{p.stderr[-2000:]}")
            sys.exit(p.returncode)
        d = json.loads(p.stdout.strip().splitlines()[-1])
        kernel_ms = d.get("kernel_ms") or d.get("config", {}).get("kernel_ms") or d.get("roofline", {}).get("kernel_ms")
        got[k] = (kernel_ms if kernel_ms is not None else float("nan"), d["ms_per_step"], d["config"]["frame_crc32"])
        res[k].append(got[k])
    print(f"round {r} {order}: " + "  ".join(f"{'A_' if k == 'C' else k} {got[k][0]:.3f}/{got[k][1]:.3f}" for k in "ACB") +
          f"   B/A {100 * (got['B'][1] / got['A'][1] - 1):+.2f} %  A'/A {100 * (got['C'][1] / got['A'][1] - 1):+.2f} %  crc {got['A'][2]} {got['B'][2]}", flush=True)
for i, what in ((0, "kernel ms"), (1, "ms per step")):
    med = {k: statistics.median(v[i] for v in res[k]) for k in res}
    ba = [100 * (b[i] / a[i] - 1) for a, b in zip(res["A"], res["B"])]
    ca = [100 * (c[i] / a[i] - 1) for a, c in zip(res["A"], res["C"])]
    print(f"{what}: medians A {med['A']:.3f}  A' {med['C']:.3f}  B {med['B']:.3f}")
    print(f"   B/A: median {statistics.median(ba):+.2f} %, range {min(ba):+.2f} .. {max(ba):+.2f} %;   A'/A (the same build twice): median {statistics.median(ca):+.2f} %, "
          f"range {min(ca):+.2f} .. {max(ca):+.2f} %, spread {max(ca) - min(ca):.2f}")
