"""The round-key table of a launch without a GPU (rt_round_keys.hpp): tests/round_keys_main.cpp compiles the header
alone under ASan + UBSan and fills the table of 1 003 keys.  Per key: the run is clean, and dword 2 r / 2 r + 1 of the table is
k0 + r W0 / k1 + r W1 mod 2^32 for r = 0..9 -- the ten round keys Philox4x32-10 (Random123; rtiow_amd/philox.py) derives from the key,
which the capped dense kernels read from the device copy of this table instead of rebuilding them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rtiow_amd import philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W0, W1 = 0x9E3779B9, 0xBB67AE85
BENCH_SEED = 1                                     # bench.py renders make_params(..., seed=1): key (seed & 0xFFFFFFFF, seed >> 32)


def keys():
    rng = np.random.default_rng(20240607)
    rand = rng.integers(0, 2 ** 32, size=(1000, 2), dtype=np.uint64)
    return [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (BENCH_SEED & 0xFFFFFFFF, BENCH_SEED >> 32)] + [(int(a), int(b)) for a, b in rand]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    assert shutil.which("g++")
    src = open(os.path.join(ROOT, "rtiow_amd", "csrc", "rt_round_keys.hpp")).read()
    assert "#include <hip" not in src and not [l for l in src.splitlines() if l.startswith('#include "')]      # a pure header
    tmp = tmp_path_factory.mktemp("round_keys")
    exe = str(tmp / "round_keys_main")
    made = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "round_keys_main.cpp")],
                          capture_output=True, text=True, timeout=300)
    assert made.returncode == 0 and "warning" not in made.stderr, made.stderr
    path = str(tmp / "keys.txt")
    with open(path, "w") as f:
        f.writelines(f"{a:x} {b:x}\n" for a, b in keys())
    done = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and not done.stderr, done.stderr                        # clean under both sanitizers
    rows = [[int(w, 16) for w in line.split()] for line in done.stdout.splitlines()]
    assert len(rows) == len(keys())
    return rows


def test_the_table_is_k_plus_r_times_w(tables):
    for (k0, k1), row in zip(keys(), tables):
        assert len(row) == 20
        for r in range(10):
            assert row[2 * r] == (k0 + r * W0) % 2 ** 32 and row[2 * r + 1] == (k1 + r * W1) % 2 ** 32, (hex(k0), hex(k1), r)


def test_the_weyl_constants_are_the_python_philox_s():
    """... and W0, W1 are the constants of the package's own Philox (the oracle's stream contract)."""
    assert (int(philox.W0), int(philox.W1)) == (W0, W1)
