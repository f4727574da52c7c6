"""The shipped filter tiles its spheres by position and a wave scans only the tiles its rays can reach (DESIGN.md
section 5.2).  CPU tests of the two halves of that:

  * the host half, through the real library (rt_tile_layout_host, no device needed): every sphere that goes through the
    filter sits in exactly one column, and what the kernel assumes of a cell's tile holds (centre in the cell, radius
    within the pad, extent in y within the slab);
  * the device half (rt_device.hpp, grid_cells) as a numpy.float32 model with the hardware's approximate reciprocals
    perturbed by an ulp either way, run against those tables: whenever the reference's own f64 arithmetic finds a root
    with t >= t_min for a sphere of a cell tile, that cell is in the ray's footprint -- with the kernel's margins reduced
    to a QUARTER, so the shipped ones have room to spare.
"""
import ctypes as C

import numpy as np
import pytest

import rtiow_amd as rt
from rtiow_amd import _ffi
from grid_model import model_grid_cells, rays_for, reference_hits, scene_cases


def layout(flat):
    (g, ng), grid, slot = rt.tile_layout_host(flat)
    return g, ng, grid, slot


CASES = scene_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_every_filtered_sphere_has_one_column_and_cells_hold_what_the_kernel_assumes(name):
    flat = CASES[name]
    G, n_global, g, slot_of = layout(flat)
    n = len(flat)
    assert len(slot_of) % 32 == 0 and len(slot_of) <= 65536
    used = slot_of[slot_of >= 0]
    assert len(np.unique(used)) == len(used) and used.max() < n
    # what is in no column is the always-exact list: at most 8 spheres, each more than 8x the median radius
    missing = np.setdiff1d(np.arange(n), used)
    r = np.abs(flat["radius"])
    assert len(missing) <= 8 and np.all(r[missing] > 8 * np.median(r))
    if name in ("small", "wide"):
        assert G == 0
    if name == "same":
        assert G == 1
    if G == 0:
        assert np.array_equal(used, np.sort(used)) and np.all(slot_of[used] == used)      # columns in list order
        return
    assert name in ("same", "line", "huge_x") or G > 1        # (a 1-D distribution of spheres: one cell can be the cheapest grid)
    assert len(slot_of) == 32 * (n_global + G * G) and 0 <= n_global <= 48
    x0, z0, inv, x1, z1, ylo, yhi, pad = [float(v) for v in g]
    for t in range(n_global, n_global + G * G):
        idx = slot_of[32 * t:32 * t + 32]
        idx = idx[idx >= 0]
        if len(idx) == 0:
            continue
        ix, iz = (t - n_global) % G, (t - n_global) // G
        c, rr = flat["center"][idx], np.abs(flat["radius"][idx])
        fx, fz = (c[:, 0] - x0) * inv, (c[:, 2] - z0) * inv
        # (the host clamps a centre beyond the last cell into it; the kernel clamps the same way)
        assert np.all(fx >= ix - 1e-4) and np.all((fx <= ix + 1 + 1e-4) | (ix == G - 1))
        assert np.all(fz >= iz - 1e-4) and np.all((fz <= iz + 1 + 1e-4) | (iz == G - 1))
        assert np.all(rr <= pad) and np.all(c[:, 1] - rr >= ylo) and np.all(c[:, 1] + rr <= yhi)
        assert np.all(c[:, 0] <= x1) and np.all(c[:, 2] <= z1) and np.all(c[:, 0] >= x0) and np.all(c[:, 2] >= z0)


@pytest.mark.parametrize("name", ["book", "tenk", "cloud", "clusters", "line"])
def test_a_sphere_the_reference_can_hit_lies_in_a_cell_of_the_rays_footprint(name):
    flat = CASES[name]
    G, n_global, g, slot_of = layout(flat)
    assert G > 0
    rng = np.random.default_rng(5)
    # the kernel's scale is at least the grid box's own (rt_api.hip); use exactly that: the smallest margins
    scale = max(abs(g[0]), abs(g[3])) + max(abs(g[5]), abs(g[6])) + max(abs(g[1]), abs(g[4])) + 2 * g[7]
    cell_slots = np.arange(32 * n_global, len(slot_of))
    cell_slots = cell_slots[slot_of[cell_slots] >= 0]
    idx = slot_of[cell_slots]
    cell = cell_slots // 32 - n_global
    six, siz = cell % G, cell // G
    c, r = flat["center"][idx], np.abs(flat["radius"][idx])
    n_rays, checked, rect_cells, line_cells = 6000, 0, [], []
    for lo in range(0, n_rays, 500):
        o, d = rays_for(flat, g, rng, 500)
        ix0, ix1, iz0, iz1, kind = model_grid_cells(o, d, g, G, scale, rng)
        hits = reference_hits(o, d, c, r)
        inside = (six[None, :] >= ix0[:, None]) & (six[None, :] <= ix1[:, None]) & (siz[None, :] >= iz0[:, None]) & (siz[None, :] <= iz1[:, None])
        n_cells = (ix1 - ix0 + 1) * (iz1 - iz0 + 1)
        if n_global + G * G > 64:
            # the kernel instantiation for large grids marks the cells row by row: the sphere's column must lie in the run
            # of the sphere's row (and the rows are those of the rectangle)
            rlo, rhi = model_grid_cells.row_runs
            ray = np.arange(len(o))[:, None]
            inside &= (six[None, :] >= rlo[ray, siz[None, :]]) & (six[None, :] <= rhi[ray, siz[None, :]])
            rowsel = (np.arange(G)[None, :] >= iz0[:, None]) & (np.arange(G)[None, :] <= iz1[:, None])
            n_row_cells = np.where(rowsel, rhi - rlo + 1, 0).sum(1)
            assert np.all(n_row_cells[kind == 1] <= n_cells[kind == 1])         # never more than the rectangle
            line_cells.append(np.where(kind == 1, n_row_cells, 0))
            n_cells = n_row_cells
        ok = (kind[:, None] == -1) | ((kind[:, None] == 1) & inside)
        bad = hits & ~ok
        assert not bad.any(), (name, np.argwhere(bad)[:5], o[np.argwhere(bad)[0][0]], d[np.argwhere(bad)[0][0]])
        checked += int(hits.sum())
        rect_cells.append(np.where(kind == 1, n_cells, 0))
    assert checked > 2000                                    # the statement was tested on real hits
    # and the footprints are not trivially "everything": the typical ray marks a small part of the grid
    rc = np.concatenate(rect_cells)
    assert np.median(rc[rc > 0]) <= max(4, G * G // 4)
    if line_cells:
        print(name, "cells per footprint: mean", np.concatenate(line_cells)[rc > 0].mean())


def test_the_model_can_fail():
    """With the pad removed a sphere straddling a cell border is missed: the check above has teeth."""
    flat = CASES["book"]
    G, n_global, g, slot_of = layout(flat)
    rng = np.random.default_rng(5)
    g0 = g.copy()
    g0[7] = -0.15                                            # shrink instead of grow
    cell_slots = np.arange(32 * n_global, len(slot_of))
    cell_slots = cell_slots[slot_of[cell_slots] >= 0]
    idx = slot_of[cell_slots]
    cell = cell_slots // 32 - n_global
    six, siz = cell % G, cell // G
    c, r = flat["center"][idx], np.abs(flat["radius"][idx])
    o, d = rays_for(flat, g, rng, 3000)
    ix0, ix1, iz0, iz1, kind = model_grid_cells(o, d, g0, G, 40.0, rng)
    hits = reference_hits(o, d, c, r)
    inside = (six[None, :] >= ix0[:, None]) & (six[None, :] <= ix1[:, None]) & (siz[None, :] >= iz0[:, None]) & (siz[None, :] <= iz1[:, None])
    ok = (kind[:, None] == -1) | ((kind[:, None] == 1) & inside)
    assert (hits & ~ok).any()
