"""The scene's tables without a GPU (rt_scene_core.hpp): tests/scene_tables_main.cpp compiles the header alone
under ASan + UBSan and builds the tables of sixteen sphere lists.  Per list: the run is clean; the layout is the loaded library's
(rt_tile_layout_host); geo, mat, geo_slot and slot_orig are a numpy restatement's, bit for bit; every occupied column of btube has
the properties tests/test_host_filter_tables.py asks of one tile, with the scene's rho; every other column is the "never kept" one;
and the hash of each table's bytes is the one recorded from the commit before the header existed (tests/golden/scene_tables_hashes.json:
its rt_upload_scene, compiled for the host with stand-ins for the HIP calls, hashing what it would have uploaded)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtiow_amd as rt
from grid_model import scene_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
TABLES = ("geo", "mat", "filt", "btube", "geo_slot", "slot_orig")
SCALARS = ("n", "n_tiles", "n_global", "grid_dim", "grid", "scene_scale", "tube_rho", "n_always", "always_idx")


def inputs():
    """name -> (spheres, scan_mode, no_grid, grid_dim)"""
    cases = scene_cases()
    book = cases["book"]
    out = {name: (flat, 5, 0, 0) for name, flat in cases.items()}
    out["empty"] = (book[:0], 5, 0, 0)
    out["one"] = (book[1:2], 5, 0, 0)
    out["n33"] = (book[1:34], 5, 0, 0)                       # two tiles, no grid
    out["book_no_grid"] = (book, 5, 1, 0)
    out["book_grid7"] = (book, 5, 0, 7)
    out["book_mode1"] = (book, 1, 0, 0)
    return out


INPUTS = inputs()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++")
    src = open(os.path.join(ROOT, "rtiow_amd", "csrc", "rt_scene_core.hpp")).read()
    assert "#include <hip" not in src and "getenv" not in src and "rt_context" not in src
    assert [l for l in src.splitlines() if l.startswith('#include "')] == ['#include "rtiow_hip.h"']
    exe = str(tmp_path_factory.mktemp("scene_tables") / "scene_tables_main")
    made = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rtiow_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "scene_tables_main.cpp")], capture_output=True, text=True, timeout=300)
    assert made.returncode == 0 and "warning" not in made.stderr, made.stderr          # the header compiles with -Wall -Wextra as it stands
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "scene_tables_hashes.json")) as f:
        return json.load(f)


def run(program, tmp_path, name):
    """-> (scalars and hashes as printed, slot_of, the tables)"""
    flat, mode, no_grid, grid_dim = INPUTS[name]
    path = str(tmp_path / f"{name}.bin")
    np.ascontiguousarray(flat, dtype=rt.SPHERE_DTYPE).tofile(path)
    done = subprocess.run([program, path, str(mode), str(no_grid), str(grid_dim), "--dump"], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and not done.stderr, done.stderr                        # clean under both sanitizers
    printed, tables, slot_of = {}, {}, None
    for line in done.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "hash":
            printed[rest.split()[0]] = rest.split()[1]
        elif key == "dump":
            t, _, words = rest.partition(" ")
            tables[t] = np.array([int(w, 16) for w in words.split()], dtype=np.uint64 if t in ("geo", "mat", "geo_slot") else np.uint32)
        elif key == "slot_of":
            slot_of = np.array(rest.split(), dtype=np.int64)
        else:
            printed[key] = rest
    return printed, slot_of, tables


def bf16_to_f64(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def exact_records(flat):
    """geo [n][4] and mat [n][10] of rt_upload_scene, in numpy's f64 (one rounding per operation, as in the header)."""
    n = len(flat)
    geo = np.zeros((max(n, 1), 4))
    mat = np.zeros((max(n, 1), 10))
    if n:
        r, p = flat["radius"], flat["param"]
        geo[:, :3], geo[:, 3] = flat["center"], r * r
        mat[:, 0], mat[:, 1], mat[:, 2:5], mat[:, 5] = 1.0 / r, p, flat["albedo"], flat["kind"]
        d = flat["kind"] == 2
        with np.errstate(all="ignore"):
            front = 1.0 / p
            r0f, r0b = (1.0 - front) / (1.0 + front), (1.0 - p) / (1.0 + p)
        mat[d, 6], mat[d, 7], mat[d, 8] = front[d], (r0f * r0f)[d], (r0b * r0b)[d]
        mat[d, 2:5] = 1.0
    return geo, mat


@pytest.mark.parametrize("name", list(INPUTS))
def test_the_tables_of_a_list(program, golden, tmp_path, monkeypatch, name):
    flat, mode, no_grid, grid_dim = INPUTS[name]
    flat = np.ascontiguousarray(flat, dtype=rt.SPHERE_DTYPE)
    n = len(flat)
    printed, slot_of, tables = run(program, tmp_path, name)
    assert int(printed["n"]) == n

    geo, mat = exact_records(flat)
    assert np.array_equal(tables["geo"], geo.view(np.uint64).ravel()) and np.array_equal(tables["mat"], mat.view(np.uint64).ravel())

    if mode == 5:
        # the layout is the loaded library's (RTIOW_HIP_LIB: another build's)
        if no_grid:
            monkeypatch.setenv("RTIOW_NO_GRID", str(no_grid))
        if grid_dim:
            monkeypatch.setenv("RTIOW_GRID_DIM", str(grid_dim))
        (lib_g, lib_ng), lib_grid, lib_slot = rt.tile_layout_host(flat)
        assert (int(printed["grid_dim"]), int(printed["n_global"])) == (lib_g, lib_ng)
        assert [int(w, 16) for w in printed["grid"].split()] == list(lib_grid.view(np.uint32))
        assert np.array_equal(slot_of, lib_slot)
        if name in ("n33", "book_no_grid"):
            assert lib_g == 0 and len(slot_of) == {"n33": 64, "book_no_grid": 32 * ((n + 31) // 32)}[name]
        if name == "book_grid7":
            assert lib_g == 7
        assert "filt" not in tables and printed["filt"] == "-"
        assert int(printed["n_tiles"]) == 2 * (len(slot_of) // 32)

        # geo_slot, slot_orig: one tile longer than slot_of; a padding column is a zero record that names no sphere
        slots = len(slot_of) + 32
        col = np.concatenate([slot_of, np.full(32, -1, dtype=np.int64)])
        used = col >= 0
        want_geo = np.zeros((slots, 4))
        want_geo[used] = geo[col[used]]
        want_orig = np.where(used, col, 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(tables["geo_slot"], want_geo.view(np.uint64).ravel()) and np.array_equal(tables["slot_orig"], want_orig)
        # what has no column is the always-exact list
        always = [int(v) for v in printed["always_idx"].split()][:int(printed["n_always"])]
        assert sorted(np.setdiff1d(np.arange(n), col[used])) == sorted(always)

        # btube [tile][64][4]: K-slots 0..7 of column c in entry c, 8..15 in entry 32 + c
        b = tables["btube"].reshape(slots // 32, 64, 4)
        k0, k1 = b[:, :32].reshape(slots, 4), b[:, 32:].reshape(slots, 4)
        assert not k0[~used].any() and not k1[~used][:, :3].any() and np.all(k1[~used][:, 3] == 0x40800000)      # never kept
        rho = np.array([int(printed["tube_rho"], 16)], dtype=np.uint32).view(np.float32)[0]
        if used.any():
            sp = flat[col[used]]
            r, c = np.abs(sp["radius"]), sp["center"]
            quart = np.sort(r[(r > 1e-15) & (r < 1e15)])
            assert rho == np.float32(quart[len(quart) // 4])                    # lower quartile of the filtered radii
            need = np.maximum(r * (1.0 + 64 * U) + 640 * U * np.linalg.norm(c, axis=1), float(rho))
            inside = (r * r > 1e-30) & ((c * c).sum(1) + r * r < 1e30)
            assert inside.all()
            w0, w1 = k0[used], k1[used]
            sg = w1[:, 2] & 0xFFFF
            sigma = bf16_to_f64(sg)
            # sigma = 2 (1 - 2^-6) / bound rounded DOWN to 8 significant bits, bound in [need, need (1 + 2^-22)]
            target = 2.0 * (1.0 - 2.0 ** -6) / need
            assert np.all(sigma <= target * (1.0 + 2.0 ** -23)) and np.all(sigma >= target / (1.0 + 2.0 ** -22) * (1.0 - 2.0 ** -7))
            assert np.array_equal(w1[:, 2], sg | (sg << 16)) and np.array_equal(w1[:, 3], sg)
            for i, (wa, wb) in enumerate([(w0[:, 0], w0[:, 1]), (w0[:, 2], w0[:, 3]), (w1[:, 0], w1[:, 1])]):
                assert np.array_equal(wa, wb)                                   # (y1, y2, y1, y2)
                ci = c[:, i] * sigma
                assert np.all(np.abs(ci - (bf16_to_f64(wa & 0xFFFF) + bf16_to_f64(wa >> 16))) <= 2.0 ** -16 * np.abs(ci))
        else:
            assert rho == np.float32(1.0)
    else:
        # scan mode 1: the f32 filter records and nothing of the shipped mode's
        assert slot_of is not None and len(slot_of) == 0 and int(printed["grid_dim"]) == 0 and int(printed["n_tiles"]) == 2 * ((n + 31) // 32)
        assert all(printed[t] == "-" for t in ("btube", "geo_slot", "slot_orig"))
        filt = tables["filt"].view(np.float32).reshape(n, 4)
        assert np.array_equal(filt[:, :3], flat["center"].astype(np.float32))
        r2, c2 = flat["radius"] ** 2, (flat["center"] ** 2).sum(1)
        kappa = 2.0 ** -17 / (1.0 - 2.0 ** -17)
        exact = c2 * (1.0 - kappa) - r2 * (1.0 + 2.0 * kappa)
        kp = filt[:, 3].astype(np.float64)
        assert np.all(kp <= exact) and np.all(kp >= exact - np.abs(exact) * 2.0 ** -22)           # K' rounded DOWN, and tight

    # the recorded hashes: first the input's, so that a drift of the scene generator is not taken for a change of the tables
    want = golden[name]
    assert want["knobs"] == {"scan_mode": mode, "no_grid": no_grid, "grid_dim": grid_dim}
    assert printed["input"] == want["input"], "the scene generator drifted: this list is not the one the hashes were recorded for"
    for key in SCALARS + TABLES:
        assert printed[key] == want[key], key
