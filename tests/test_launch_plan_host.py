"""The launch plan without a GPU: rt_host::plan_launch (rt_launch.hpp) decides the work-block size, whether block sums are kept in
the LDS ring, and whether a launch takes blocks of 1 024 -- for the dense, the pixel-list and the frame-batch launches alike.  It is
a pure function of a few integers, so tests/launch_plan_table.cpp (host code only, its own main) prints it for a table of inputs and
every line is compared with a restatement that does not copy the formula: the pixels a block of `items` consecutive pixel-samples
touches, (o + items - 1) // spp + 1 for a block that starts at sample o of its first pixel, maximised over o by brute force."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE_ITEMS = 200_000_000


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_table")
    subprocess.run(["hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "launch_plan_table.cpp")],
                   check=True, cwd=ROOT, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60)
    plans, magics = {}, {}
    for line in run.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        key, val = rest.split(" -> ")
        if kind == "plan":
            plans[tuple(int(x) for x in key.split())] = tuple(int(x) for x in val.split())
        else:
            magics[int(key)] = int(val)
    return plans, magics


def _ring_block(spp, slots):
    """The largest of 256 / 192 / 128 / 64 pixel-samples that touches at most `slots` pixels wherever it starts; 0: none does."""
    if spp < 1:
        return 0
    for items in (256, 192, 128, 64):
        if max((o + items - 1) // spp + 1 for o in range(spp)) <= slots:
            return items
    return 0


def _model(spp, ring_min, shipped, small_grid, large_allowed, total, threshold):
    def large_on(slots):
        return bool(shipped and large_allowed and spp >= ring_min and _ring_block(spp, slots) == 256
                    and spp >= (69 if small_grid else 147) and total >= threshold)
    # 16 pixel slots on the shipped kernel -- but the large-grid kernel's blocks of 1 024 keep 8 --, 8 on every other kernel
    slots = 8 if not shipped or (not small_grid and large_on(8)) else 16
    block = _ring_block(spp, slots)
    use_ring = block != 0 and spp >= ring_min
    large = use_ring and large_on(slots)
    return (int(use_ring), 1024 if large else block if use_ring else 256, int(large))


def test_every_line_of_the_table_matches_the_brute_force_model(table):
    plans, _ = table
    spps = list(range(41)) + [68, 69, 146, 147, 500]
    want_keys = {(spp, rm, sh, sg, la, total, thr) for spp in spps for rm in (0, 20) for sh in (0, 1) for sg in (0, 1) for la in (0, 1)
                 for thr, total in ((0, 0), (LARGE_ITEMS, LARGE_ITEMS - 1), (LARGE_ITEMS, LARGE_ITEMS))}
    assert set(plans) == want_keys
    for key, got in plans.items():
        assert got == _model(*key), key


def _first_spp(plans, want, **fixed):
    """The smallest spp of the table's 0..40 from which on (up to 40) the plan is `want`, with ring_min_spp 0 and no large blocks in play."""
    key = lambda spp: (spp, 0, fixed["shipped"], fixed.get("small_grid", 0), 0, 0, 0)
    first = min(spp for spp in range(41) if plans[key(spp)] == want)
    assert all(plans[key(s)][1] >= want[1] and plans[key(s)][0] == 1 for s in range(first, 41))
    return first


def test_the_documented_thresholds(table):
    plans, _ = table
    # 8 slots (every kernel but the shipped one): ring from 9 spp; blocks of 64 / 128 / 192 / 256 from 9 / 19 / 28 / 37
    assert [_first_spp(plans, (1, b, 0), shipped=0) for b in (64, 128, 192, 256)] == [9, 19, 28, 37]
    assert plans[(8, 0, 0, 0, 0, 0, 0)] == (0, 256, 0)
    # 16 slots (the shipped kernel, either grid): ring from 5 spp; blocks of 64 / 128 / 192 / 256 from 5 / 9 / 13 / 17
    for sg in (0, 1):
        assert [_first_spp(plans, (1, b, 0), shipped=1, small_grid=sg) for b in (64, 128, 192, 256)] == [5, 9, 13, 17]
        assert plans[(4, 0, 1, sg, 0, 0, 0)] == (0, 256, 0)
    # blocks of 1 024 from 147 spp (69 on a small grid) at >= 2 x 10^8 pixel-samples ...
    assert plans[(147, 0, 1, 0, 1, LARGE_ITEMS, LARGE_ITEMS)] == (1, 1024, 1)
    assert plans[(146, 0, 1, 0, 1, LARGE_ITEMS, LARGE_ITEMS)] == (1, 256, 0)
    assert plans[(147, 0, 1, 0, 1, LARGE_ITEMS - 1, LARGE_ITEMS)] == (1, 256, 0)
    assert plans[(69, 0, 1, 1, 1, LARGE_ITEMS, LARGE_ITEMS)] == (1, 1024, 1)
    assert plans[(68, 0, 1, 1, 1, LARGE_ITEMS, LARGE_ITEMS)] == (1, 256, 0)
    assert plans[(69, 0, 1, 1, 1, LARGE_ITEMS - 1, LARGE_ITEMS)] == (1, 256, 0)
    assert plans[(69, 0, 1, 0, 1, LARGE_ITEMS, LARGE_ITEMS)] == (1, 256, 0)
    assert plans[(17, 0, 1, 1, 1, 0, 0)] == (1, 256, 0)                       # (a threshold of 0 items does not lower the samples per pixel)
    assert plans[(500, 0, 1, 1, 1, 0, 0)] == (1, 1024, 1)
    # ... on the shipped kernel only, and never when large blocks are not allowed (pixel lists, frame batches)
    assert not any(v[2] for k, v in plans.items() if not k[2] or not k[4])
    assert any(v[2] for k, v in plans.items())
    # spp 0: no ring, blocks of 256 -- whatever else is asked
    assert {v for k, v in plans.items() if k[0] == 0} == {(0, 256, 0)}
    # RTIOW_RING_MIN_SPP = 20: no block sums below 20 samples per pixel, the plan of the ring above
    assert plans[(19, 20, 1, 1, 0, 0, 0)] == (0, 256, 0) and plans[(20, 20, 1, 1, 0, 0, 0)] == (1, 256, 0)
    assert plans[(19, 20, 0, 0, 0, 0, 0)] == (0, 256, 0) and plans[(20, 20, 0, 0, 0, 0, 0)] == (1, 128, 0)


def test_the_divisor_constant(table):
    """udiv_small (rt_kernels.hpp): floor(x * M / 2^32) = x // d for every numerator the kernel forms, x < d + 1 024; 0 = divide for real."""
    _, magics = table
    assert set(magics) == {-1, 0, 1, 2, 3, 7, 10, 100, 500, 1200, 32767, 32768, 65535}
    for d, m in magics.items():
        if d <= 1 or d >= 32768:
            assert m == 0, d
        else:
            assert 0 < m < 2 ** 32 and all((x * m) >> 32 == x // d for x in range(d + 1024)), d
