"""The lane-striped block sums' plan without a GPU: rt_host::plan_stripes (rt_launch.hpp) decides, from a launch's work-block size and its
samples per pixel, how many of the ring's 16 pixel slots a block can touch at all -- S, the smallest power of two that holds them, at least 4 --
and so how many replicas R = 16 / S of every live slot the capped dense kernels stripe over their lanes.  tests/stripe_plan_table.cpp prints it
for a table of inputs; every line is compared with a restatement that does not copy the formula: the pixels a block of `items` consecutive
pixel-samples touches, (o + items - 1) // spp + 1 for a block that starts at sample o of its first pixel, maximised over o by brute force."""
import pytest

import stripe_plan

BLOCKS = (64, 128, 192, 256, 1024)
SPPS = list(range(401)) + [500, 511, 512, 513, 1022, 1023, 1024, 1025, 2000, 32767]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return stripe_plan.stripe_table(tmp_path_factory.mktemp("stripe_plan"))


def _pixels_touched(items, spp):
    # (a block that starts at the LAST sample of a pixel touches the most: the maximum over every start o is reached there, and the brute force says so)
    return max((o + items - 1) // spp + 1 for o in (range(spp) if spp <= 2000 else (0, spp - 1)))


def _model(items, spp, use_ring, striped):
    if not use_ring or not striped or spp < 1:
        return (16, 1, 0)
    touched = _pixels_touched(items, spp)
    slots = next((s for s in (4, 8) if touched <= s), 16)
    if slots == 16:
        return (16, 1, 0)
    return (slots, 16 // slots, 15 & ~(slots - 1))


def test_every_line_of_the_table_matches_the_brute_force_model(table):
    assert set(table) == {(b, s, u, k) for b in BLOCKS for s in SPPS for u in (0, 1) for k in (0, 1)}
    for key, got in table.items():
        assert got == _model(*key), key


def test_one_replica_is_all_zeros(table):
    """R = 1 leaves a launch's addresses as they were: mask 0 -- on every kernel that is not striped, without block sums, and below the thresholds."""
    for key, (slots, replicas, mask) in table.items():
        assert replicas in (1, 2, 4) and slots * replicas == 16
        if replicas == 1:
            assert mask == 0, key
        else:
            assert key[2] == 1 and key[3] == 1 and mask == 15 & ~(slots - 1), key


def test_the_documented_thresholds(table):
    # blocks of 1 024: four replicas from 341 samples per pixel (ceil(1023 / 341) + 1 = 4 pixels), two from 147 (8 pixels)
    assert stripe_plan.first_spp(table, 1024, 4) == 341 and stripe_plan.first_spp(table, 1024, 2) == 147
    assert table[(1024, 340, 1, 1)][1] == 2 and table[(1024, 146, 1, 1)][1] == 1
    # blocks of 256: from 85 and from 37
    assert stripe_plan.first_spp(table, 256, 4) == 85 and stripe_plan.first_spp(table, 256, 2) == 37
    assert table[(256, 84, 1, 1)][1] == 2 and table[(256, 36, 1, 1)][1] == 1
    # the headline launch and the second configuration of the benchmark
    assert table[(1024, 500, 1, 1)] == (4, 4, 12) and table[(1024, 100, 1, 1)] == (16, 1, 0)
    # never more than four replicas, however few pixels a block touches
    assert table[(1024, 32767, 1, 1)] == (4, 4, 12) and table[(64, 400, 1, 1)] == (4, 4, 12)
