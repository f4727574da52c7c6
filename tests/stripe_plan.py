"""rt_host::plan_stripes (rt_launch.hpp) as a table: compiles tests/stripe_plan_table.cpp for the host only, runs it and parses its lines.
Shared by tests/test_stripe_plan_host.py (every line against a brute-force model) and tests/test_gpu_striped_sums.py (the sample counts at which
the number of replicas changes come from here, not from literals)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stripe_table(tmp_dir):
    """(block_items, spp, use_ring, striped kernel) -> (slots S, replicas R, mask)."""
    exe = os.path.join(str(tmp_dir), "stripe_plan_table")
    subprocess.run(["hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stripe_plan_table.cpp")],
                   check=True, cwd=ROOT, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60)
    table = {}
    for line in run.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        assert kind == "stripe", line
        key, val = rest.split(" -> ")
        table[tuple(int(x) for x in key.split())] = tuple(int(x) for x in val.split())
    return table


def first_spp(table, block_items, replicas):
    """The smallest sample count of the table from which a striped launch on block sums keeps at least `replicas` replicas on blocks of block_items."""
    spps = sorted(k[1] for k in table if k[0] == block_items and k[2] == 1 and k[3] == 1)
    first = min(s for s in spps if table[(block_items, s, 1, 1)][1] >= replicas)
    assert all(table[(block_items, s, 1, 1)][1] >= replicas for s in spps if s >= first)
    return first
