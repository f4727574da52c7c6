"""The staging arena's layout without a GPU: a host-buffer entry point declares its device blocks on an rt_host::StageLayout
(rt_host.hpp) and gets their byte offsets in the context's one arena.  The layout is pure arithmetic, so tests/stage_layout_table.cpp
(host code only, its own main) prints it for a table of block-size lists, and every line is held to the rule as DESIGN.md states it --
every block on a 256-byte boundary, in declaration order, no two non-empty blocks overlapping, the total the end of the last block
rounded up to 256 -- without copying the code's formula.  Also here: the denoise input tests/test_gpu_staging.py uses must give different
results with and without its count buffer, or that test's "absent buffer after a present one" case would prove nothing.
On top of the layout a call DECLARES its buffers (rt_host::StagePlan): direction in / out / inout / scratch, the caller's pointer, bytes.
The same program prints what follows from a table of declared lists, and each line is held to the rule as rt_host.hpp and DESIGN.md
state it: a buffer whose pointer is NULL is a block of 0 bytes without a device pointer; the offsets are the layout's for those bytes; the
in and inout buffers the caller gave go up, the out and inout ones come down, in declaration order; at most 16 buffers, one more is
reported and writes nothing."""
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


CAPACITY = 16
SAN_FLAGS = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def build_and_run(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "stage_layout_table")
    subprocess.run(["hipcc", "--cuda-host-only", "-x", "hip", "-std=c++17", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stage_layout_table.cpp")],
                   check=True, cwd=ROOT, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    run = build_and_run(tmp_path_factory, "stage_layout", [])
    assert run.returncode == 0, run.stderr
    return run.stdout


@pytest.fixture(scope="module")
def table(output):
    rows = {}
    for line in output.splitlines():
        kind, name, rest = line.split(" ", 2)
        if kind == "plan":
            continue
        assert kind == "layout" and name not in rows
        sizes, rest = rest[1:].split("->")
        offsets, total = rest.split("|")
        rows[name] = ([int(x) for x in sizes.split()], [int(x) for x in offsets.split()], int(total))
    return rows


@pytest.fixture(scope="module")
def plans(output):
    """name -> (declared [(direction, given, bytes)], the program's fields by name: lists of ints, `after` a word)"""
    rows = {}
    for line in output.splitlines():
        kind, name, rest = line.split(" ", 2)
        if kind != "plan":
            continue
        assert name not in rows
        declared, rest = rest[1:].split("->")
        fields = {}
        for part in rest.split("|"):
            key, *values = part.split()
            fields[key] = values[0] if key == "after" else [int(x) for x in values]
        rows[name] = ([(d[0], d[1] == "1", int(d[3:])) for d in declared.split()], fields)
    return rows


def layout_by_the_rule(sizes):
    """every block on the first 256-byte boundary at or after the end of the blocks before it; the total likewise"""
    offsets, end = [], 0
    for s in sizes:
        offsets.append(-(-end // 256) * 256)
        end = offsets[-1] + s if s else end
    return offsets, -(-end // 256) * 256


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


def test_every_declared_list_obeys_the_rule(plans):
    assert len(plans) >= 18
    for name, (declared, f) in plans.items():
        kept = declared[:CAPACITY]
        assert f["ids"] == list(range(len(kept))) + [-1] * (len(declared) - len(kept)), name      # a declaration names its block, -1 past the capacity
        assert f["overflow"] == [1 if len(declared) > CAPACITY else 0] and f["after"] == "intact" and f["stray"] == [0], name
        has_pointer = [d == "s" or given for d, given, _ in kept]
        sizes = [b if d == "s" or given else 0 for d, given, b in kept]                           # a NULL buffer is a block of 0 bytes ...
        assert f["bytes"] == sizes, name
        assert (f["offsets"], f["total"]) == (layout_by_the_rule(sizes)[0], [layout_by_the_rule(sizes)[1]]), name
        assert f["ptr"] == [k for k, p in enumerate(has_pointer) if p], name                      # ... without a device pointer
        assert f["up"] == [k for k, (d, given, _) in enumerate(kept) if given and d in "ib"], name
        assert f["down"] == [k for k, (d, given, _) in enumerate(kept) if given and d in "ob"], name


def test_the_layout_rule_as_this_file_states_it_is_the_tables(table):
    """(layout_by_the_rule, which the declared lists are held to, against the rows test_every_row_obeys_the_rule checks property by property)"""
    for name, (sizes, offsets, total) in table.items():
        assert layout_by_the_rule(sizes) == (offsets, total), name


def test_the_declared_edge_cases(plans):
    def row(name):
        declared, f = plans[name]
        return f["offsets"], f["total"][0], f["ptr"], f["up"], f["down"]
    assert row("none") == ([], 0, [], [], [])
    assert row("null_middle") == ([0, 256, 256], 512, [0, 2], [0], [2])                        # the NULL buffer occupies nothing, copies nothing
    assert row("null_last") == ([0, 512], 512, [0], [0], [])
    assert row("null_each_direction") == ([0, 0, 0, 0], 256, [3], [], [])                       # (a scratch block has no caller's pointer to be NULL)
    assert row("inout") == ([0, 512, 768], 1024, [0, 1, 2], [0, 1], [1, 2])                     # an inout goes both ways
    assert row("scratch") == ([0, 256, 1280], 1536, [0, 1, 2], [0], [2])                        # a scratch block is there and is never copied
    # 0 elements behind a pointer the caller gave: 0 bytes, but PRESENT -- a device pointer, a copy of nothing
    assert row("zero_count_given") == ([0, 0, 0, 0, 0], 256, [0, 1, 2, 3, 4], [0, 1], [1, 2, 4])
    for extra in (0, 1, 2):
        declared, f = plans[f"capacity_plus_{extra}"]
        assert len(declared) == CAPACITY + extra and len(f["offsets"]) == CAPACITY and f["overflow"] == [int(extra > 0)]
        assert f["after"] == "intact"
    # what overflows changes nothing of what was declared before it
    assert all(plans[f"capacity_plus_{extra}"][1]["offsets"] == plans["capacity_plus_0"][1]["offsets"] for extra in (1, 2))


@pytest.mark.parametrize("n", [35, 2304])
def test_the_real_lists_of_scatter_and_trace_rays(plans, n):
    """The rows for rt_scatter and rt_trace_rays at the path counts of tests/test_gpu_staging.py's smallest and largest frame carry the sizes
    the header gives those buffers -- 3 doubles per direction, point, normal, origin and attenuation, 4 bytes per index, pixel, sample
    and event, 1 per front_face and status -- and the copies the header's in / out say: rt_scatter's outputs go up too (what the step
    leaves unwritten keeps the caller's bytes), all but the status; in place the directions are ONE block that goes up and comes down."""
    v3, w32 = n * 24, n * 4
    declared, f = plans[f"scatter_{n}"]
    assert [b for _, _, b in declared] == [v3, w32, v3, v3, n, w32, w32, w32, v3, v3, v3, n] == f["bytes"]
    assert f["up"] == list(range(11)) and f["down"] == [7, 8, 9, 10, 11] and f["ptr"] == list(range(12))
    declared, g = plans[f"scatter_in_place_{n}"]
    assert [b for _, _, b in declared] == [v3, w32, v3, v3, n, w32, w32, w32, v3, v3, n] == g["bytes"]
    assert g["up"] == list(range(10)) and g["down"] == [0, 7, 8, 9, 10]
    assert g["offsets"][:9] == f["offsets"][:9] and f["total"][0] - g["total"][0] == -(-v3 // 256) * 256      # one block of directions fewer
    declared, f = plans[f"trace_all_{n}"]
    assert [b for _, _, b in declared] == [v3, v3, n * 8, n * 4, n * 8, v3, v3, n] == f["bytes"]
    assert f["up"] == [0, 1, 2] and f["down"] == [3, 4, 5, 6, 7] and f["ptr"] == list(range(8))
    declared, g = plans[f"trace_index_{n}"]
    assert g["bytes"] == [v3, v3, 0, n * 4, 0, 0, 0, 0] and g["up"] == [0, 1] and g["down"] == [3] and g["ptr"] == [0, 1, 3]
    assert g["total"][0] == 2 * (-(-v3 // 256) * 256) + -(-n * 4 // 256) * 256


def test_the_table_program_is_clean_under_the_sanitizers(tmp_path_factory, output):
    """the same stand-alone program, host code only, under ASan + UBSan: a clean exit and the same lines -- the declaration one past the
    capacity included, which must write nothing"""
    run = build_and_run(tmp_path_factory, "stage_layout_san", SAN_FLAGS)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == output


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
