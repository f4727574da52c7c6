"""The staging arena's layout without a GPU: a host-buffer entry point declares its device blocks on an rt_host::StageLayout
(rt_host.hpp) and gets their byte offsets in the context's one arena.  The layout is pure arithmetic, so tests/stage_layout_table.cpp
(host code only, its own main) prints it for a table of block-size lists, and every line is held to the rule as DESIGN.md states it --
every block on a 256-byte boundary, in declaration order, no two non-empty blocks overlapping, the total the end of the last block
rounded up to 256 -- without copying the code's formula.  Also here: the denoise input tests/test_gpu_staging.py uses must give different
results with and without its count buffer, or that test's "absent buffer after a present one" case would prove nothing."""
import os
import subprocess

import numpy as np
import pytest

import rtiow_amd as rt
import temporal_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENOISE_LEVELS = 2


def staging_inputs(w, h):
    """(fix u64 [h,w,3], count u32 [h,w] non-uniform, spp, feat u64 [h,w,8], feat_spp), (prev_fix, prev_len, prev_feat, prev_feat_spp):
    the synthetic frame and history tests/test_gpu_staging.py feeds rt_denoise, rt_temporal and the resolves at w x h."""
    return tr.synthetic_frame(w, h, 3), tr.synthetic_history(w, h, 3)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_layout") / "stage_layout_table")
    subprocess.run(["hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stage_layout_table.cpp")],
                   check=True, cwd=ROOT, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60)
    rows = {}
    for line in run.stdout.splitlines():
        kind, name, rest = line.split(" ", 2)
        assert kind == "layout" and name not in rows
        sizes, rest = rest[1:].split("->")
        offsets, total = rest.split("|")
        rows[name] = ([int(x) for x in sizes.split()], [int(x) for x in offsets.split()], int(total))
    return rows


def test_every_row_obeys_the_rule(table):
    assert len(table) >= 20
    for name, (sizes, offsets, total) in table.items():
        assert len(offsets) == len(sizes), name
        assert all(o % 256 == 0 for o in offsets) and total % 256 == 0, name
        assert offsets == sorted(offsets), name                                   # declaration order
        spans = [(o, o + s) for s, o in zip(sizes, offsets) if s > 0]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), name          # (sorted already: neighbours are enough)
        end = spans[-1][1] if spans else 0
        assert end <= total < end + 256, name                                     # the end of the last block, rounded up to 256
        # nothing is wasted either: a block starts on the first boundary at or after the end of the blocks before it
        before = 0
        for s, o in zip(sizes, offsets):
            assert before <= o < before + 256, name
            before = max(before, o + s)


def test_the_edge_sizes(table):
    assert table["none"] == ([], [], 0)
    assert {s: table[f"one_{s}"][2] for s in (0, 1, 255, 256, 257)} == {0: 0, 1: 256, 255: 256, 256: 256, 257: 512}
    assert all(table[f"one_{s}"][1] == [0] for s in (0, 1, 255, 256, 257))
    assert table["edges"] == ([0, 1, 255, 256, 257], [0, 0, 256, 512, 768], 1280)
    assert table["zero_between"] == ([100, 0, 100], [0, 256, 256], 512)           # a block of 0 bytes occupies nothing
    assert table["zeros"] == ([0, 0, 0], [0, 0, 0], 0)
    assert table["zero_last"] == ([512, 0], [0, 512], 512)


@pytest.mark.parametrize("size", [(7, 5), (33, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_real_lists_of_denoise_and_temporal(table, size):
    """The table's rows for rt_denoise and rt_temporal carry the sizes those calls' buffers have by the header's own statement: 3 and 8
    words of 8 bytes per pixel, 4 bytes per count or length, rt_denoise_workspace_bytes -- and an absent buffer nothing."""
    w, h = size
    npix = w * h
    fix, feat, words, work = npix * 24, npix * 64, npix * 4, rt.Renderer.denoise_workspace_bytes(w, h)
    for count in (0, 1):
        sizes, offsets, total = table[f"denoise_{w}x{h}_count{count}"]
        assert sizes == [fix, feat, fix, work, words * count]
        assert total >= sum(sizes) and total - sum(sizes) < 256 * len(sizes)
        for hist in (0, 1):
            sizes, offsets, total = table[f"temporal_{w}x{h}_count{count}_hist{hist}"]
            assert sizes == [fix, feat, words * count, fix * hist, feat * hist, words * hist, fix, words]
            assert total >= sum(sizes) and total - sum(sizes) < 256 * len(sizes)
    # with the optional buffers the arena is larger, and only by those buffers (each rounded up to 256)
    assert table[f"denoise_{w}x{h}_count1"][2] - table[f"denoise_{w}x{h}_count0"][2] == -(-words // 256) * 256
    assert table[f"temporal_{w}x{h}_count0_hist1"][2] - table[f"temporal_{w}x{h}_count0_hist0"][2] == sum(-(-b // 256) * 256 for b in (fix, feat, words))


def test_the_staging_tests_denoise_input_depends_on_its_counts():
    (fix, count, spp, feat, feat_spp), _ = staging_inputs(7, 5)
    assert len(np.unique(count)) > 1                                              # non-uniform
    dn = rt.make_denoise(levels=DENOISE_LEVELS)
    with_count = rt.denoise_host(fix, spp, feat, feat_spp, dn, count=count)
    without = rt.denoise_host(fix, spp, feat, feat_spp, dn)
    assert with_count.shape == without.shape == (5, 7, 3)
    assert not np.array_equal(with_count, without)
