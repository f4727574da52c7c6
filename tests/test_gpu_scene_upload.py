"""rt_upload_scene on one context, scene after scene: a large-grid scene, the empty list, small-grid scenes,
a single cell, overflowing cells, one sphere, a scene without a grid, and the large one again -- chosen so that a table of the wrong
size, a table left over from the scene before, or a missing spare tile shows in the next render.  After every upload a 32 x 18 x 4 spp
frame equals Oracle B bit for bit.  Then the book scene on a context of the VALU cross-check filter (RTIOW_SCAN_MODE=1), whose tables
are the f32 filter records."""
import os

import numpy as np
import pytest

import rtiow_amd as rt
from grid_model import scene_cases

pytestmark = pytest.mark.gpu

W, H, SPP = 32, 18, 4


@pytest.fixture(scope="module")
def lists():
    cases = scene_cases()
    book = cases["book"]
    out = {name: cases[name] for name in ("tenk", "book", "same", "clusters", "small")}
    out["empty"] = book[:0]
    out["one"] = book[1:2]
    return {name: np.ascontiguousarray(flat, dtype=rt.SPHERE_DTYPE) for name, flat in out.items()}


@pytest.fixture(scope="module")
def wanted(oracle_mod, lists):
    """Oracle B's frame of every list, rendered once."""
    cam = oracle_mod.camera_from_host(rt.book1_camera(W, H))
    return {name: oracle_mod.render_b(cam, flat, oracle_mod.make_params(W, H, SPP, seed=1)) for name, flat in lists.items()}


def check(r, name, lists, wanted):
    r.upload_scene(lists[name])
    sums, fix, st = r.render(rt.book1_camera(W, H), rt.make_params(W, H, SPP, seed=1))
    want_fix, want_sum, ost = wanted[name]
    assert np.array_equal(fix, want_fix), f"{name}: {int((fix != want_fix).any(axis=-1).sum())} pixels differ from the oracle"
    assert np.array_equal(sums, want_sum)
    assert st["rays_traced"] == ost["rays_traced"] and st["samples"] == W * H * SPP and st["n_spheres"] == len(lists[name])
    return st


def test_a_sequence_of_uploads_on_one_context(lists, wanted):
    (g, n_global), _, slot_of = rt.tile_layout_host(lists["tenk"])
    assert n_global + g * g > 64 and len(slot_of) // 32 > 64                # the large-grid kernel, more than 64 tiles
    # the empty list's frame is the sky: one ray per sample, none of them scattered
    assert wanted["empty"][2]["rays_traced"] == W * H * SPP
    with rt.Renderer(0) as r:
        for name in ("tenk", "empty", "book", "same", "clusters", "one", "small", "tenk"):
            st = check(r, name, lists, wanted)
            if st["scan_mode"] == 5:
                (g, n_global), _, _ = rt.tile_layout_host(lists[name])
                assert st["kernel_variant"] & 1 == (1 if g > 0 and n_global + g * g <= 64 else 0), name


def test_the_book_scene_on_a_context_of_scan_mode_1(lists, wanted):
    old = os.environ.get("RTIOW_SCAN_MODE")
    os.environ["RTIOW_SCAN_MODE"] = "1"
    try:
        r = rt.Renderer(0)
    finally:
        if old is None:
            os.environ.pop("RTIOW_SCAN_MODE")
        else:
            os.environ["RTIOW_SCAN_MODE"] = old
    with r:
        assert check(r, "book", lists, wanted)["scan_mode"] == 1
