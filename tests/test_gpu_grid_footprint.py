"""The tile grid's footprint (rt_device.hpp, grid_cells and grid_row_run) as the DEVICE computes it, through the
cross-check build's hook rt_grid_cells_device (the functions themselves, compiled for gfx950; the product ABI does not
carry the hook).  test_grid_layout.py checks a numpy model of the same arithmetic; here the compiled code is held to

  * soundness with the shipped margins: every cell sphere the reference's f64 hit test (sphere.rs) can hit lies in the
    ray's rectangle AND in the run of its row, on >= 50 000 rays per layout (a verdict of -1 is always allowed);
  * culling: on sane rays "cannot tell" is rare and the median footprint small;
  * the model: with the model's margins unshrunk and exact-rounded reciprocals, the same verdict on every ray and the
    same bounds on nearly every ray (never more than one cell apart);
  * an edge catalogue whose answers are derived in f64 (zero, tiny and huge direction components, vertical rays, corners,
    NaN and inf, footprints beyond the int range) at grid_dim 1 .. 63.

Every test skips unless the loaded library is the cross-check build: test_gpu_crosscheck_modes.py's
test_crosscheck_build_in_a_subprocess runs this file against it."""
import numpy as np
import pytest

import rtiow_amd as rt
from rtiow_amd import _ffi
from grid_model import cell_spheres, line_passes_near, minimal_scale, model_grid_cells, rays_for, reference_hits_pairs, scene_cases

pytestmark = pytest.mark.gpu
f32 = np.float32
LAYOUTS = ["book", "tenk", "cloud", "clusters", "line", "huge_x", "huge_xz"]
_CASES = {}


def needs_xcheck():
    if not _ffi.has_crosscheck_modes():
        pytest.skip("product library loaded: rt_grid_cells_device lives in tools/librtiow_hip_xcheck.so")


def case(name):
    if not _CASES:
        _CASES.update(scene_cases())
    flat = _CASES[name]
    (G, n_global), g, slot_of = rt.tile_layout_host(flat)
    assert G > 0, name
    return flat, G, n_global, g, slot_of


# ---- f64 expectations ------------------------------------------------------------------------------------

def exact_piece(o, d, g):
    """The ray o + t d, t >= 0, clipped in f64 to the box the cells' spheres live in: [g0 - g7, g3 + g7] x [g5, g6] x
    [g1 - g7, g4 + g7] -> (end a, end b) or None."""
    lo = (float(g[0]) - float(g[7]), float(g[5]), float(g[1]) - float(g[7]))
    hi = (float(g[3]) + float(g[7]), float(g[6]), float(g[4]) + float(g[7]))
    t0, t1 = 0.0, np.inf
    for a in range(3):
        if d[a] == 0.0:
            if not lo[a] <= o[a] <= hi[a]:
                return None
            continue
        ta, tb = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    if t1 < t0:
        return None
    return o + t0 * d, o + t1 * d


def cells_of(lo, hi, origin, inv, G):
    return (int(np.clip(np.floor((lo - float(origin)) * float(inv)), 0, G - 1)),
            int(np.clip(np.floor((hi - float(origin)) * float(inv)), 0, G - 1)))


def exact_footprint(o, d, g, G):
    """-> None (no cell), or ((ix0, ix1, iz0, iz1), {row: (first, last column)}): the cells whose spheres (radius <= g7,
    centre in the cell, inside the slab) the ray can reach, and per row the columns of the part of the piece in the row's
    band, both grown by g7."""
    p = exact_piece(np.asarray(o, float), np.asarray(d, float), g)
    if p is None:
        return None
    (xa, _, za), (xb, _, zb) = p
    pad = float(g[7])
    ix0, ix1 = cells_of(min(xa, xb) - pad, max(xa, xb) + pad, g[0], g[2], G)
    iz0, iz1 = cells_of(min(za, zb) - pad, max(za, zb) + pad, g[1], g[2], G)
    runs = {}
    for iz in range(iz0, iz1 + 1):
        b0, b1 = float(g[1]) + iz / float(g[2]) - pad, float(g[1]) + (iz + 1) / float(g[2]) + pad
        if zb == za:
            if not b0 <= za <= b1:
                continue
            s0, s1 = 0.0, 1.0
        else:
            s0, s1 = sorted(((b0 - za) / (zb - za), (b1 - za) / (zb - za)))
            s0, s1 = max(s0, 0.0), min(s1, 1.0)
            if s1 < s0:
                continue
        x0, x1 = sorted((xa + s0 * (xb - xa), xa + s1 * (xb - xa)))
        runs[iz] = cells_of(x0 - pad, x1 + pad, g[0], g[2], G)
    return (ix0, ix1, iz0, iz1), runs


def grid_at(g, G_from, G):
    """The layout's grid box at G cells per side, as the host builds it (rt_api.hip tile_layout: 1/cell as an f32, the far
    edges rounded up)."""
    cell = (G_from / float(g[2])) / G
    out = g.copy()
    out[2] = f32(1.0 / cell)
    for k, origin in ((3, g[0]), (4, g[1])):
        v = float(origin) + G * cell
        out[k] = f32(v) if float(f32(v)) >= v else np.nextafter(f32(v), f32(np.inf))
    return out


def away_from_borders(pad_cells):
    """A fraction f of a cell such that f, f - pad and f + pad lie >= 0.05 cells from every cell border."""
    for f in np.linspace(0.5, 0.95, 46):
        if all(abs(v - np.round(v)) >= 0.05 for v in (f - pad_cells, f + pad_cells, f)):
            return float(f)
    raise AssertionError("no position away from the borders")


def edge_catalogue(g, G):
    """[(what, o, d, expect)]; expect: "cannot" (-1), "none" (0), "rect" (contains the f64 footprint), "tight" (contains
    it, at most one cell more each way), "exact" (equals it) -- "+whole": every row's run spans the rectangle's columns."""
    inv, pad = float(g[2]), float(g[7])
    cell = 1.0 / inv
    f = away_from_borders(pad * inv)
    ylo, yhi = float(g[5]), float(g[6])
    ym = 0.5 * (ylo + yhi)
    X = lambda i: float(g[0]) + (i + f) * cell
    Z = lambda i: float(g[1]) + (i + f) * cell
    mid = np.array((X(G // 2), ym, Z(G // 3)))
    out = []
    add = lambda what, o, d, e: out.append((what, np.array(o, float), np.array(d, float), e))
    # direction components exactly 0, below the dmin cut (1e-30), just above it, tiny relative to the others
    add("dy = 0", (X(0) - 3, ym, Z(0)), (1.0, 0.0, 0.3), "cannot")
    add("vertical, dx = dz = 0", (X(0), yhi + 2, Z(0)), (0.0, -1.0, 0.0), "cannot")
    add("dx = dz = 1e-31", (X(G - 1), yhi + 2, Z(G - 1)), (1e-31, -1.0, -1e-31), "cannot")
    add("dz = -1e-31", (X(0) - 3, ym, Z(0)), (1.0, -1e-3, -1e-31), "cannot")
    add("dz = 1e-29", (X(0) - 3, ym, Z(G // 2)), (1.0, -1e-3, 1e-29), "tight+whole")
    add("dz = 1e-20 |d|", (X(0) - 3, ym, Z(G // 2)), (1.0, -2e-3, 1e-20), "tight+whole")
    add("dx = 1e-8 |d|", (X(G // 3), ym, Z(0) - 2), (1e-8, 1e-3, 1.0), "tight+whole")
    add("dy = 1e-20 |d|", (X(0) - 3, ym, Z(0) - 3), (1.0, 1e-20, 0.7), "tight")
    # |d|_1 and the origin's 1-norm either side of 1e15
    dd = np.array((0.6, -0.01, 0.8))
    add("|d|_1 = 0.99e15", (X(0) - 3, ym, Z(0) - 4), dd * (0.99e15 / 1.41), "tight")
    add("|d|_1 = 1.01e15", (X(0) - 3, ym, Z(0) - 4), dd * (1.01e15 / 1.41), "cannot")
    far = np.array((4.9e14, ym + 0.01, 4.9e14))
    add("|o|_1 = 0.98e15, toward the grid", far, mid - far, "rect")
    add("|o|_1 = 0.98e15, away from it", far, far - mid, "none")
    far2 = np.array((5.1e14, ym + 0.01, 5.1e14))
    add("|o|_1 = 1.02e15", far2, mid - far2, "cannot")
    # ... whose unclamped cell coordinates leave the int range once the margins (1e-6 |o|_1 ~ 1e9 units) are added: the
    # conversions must saturate (a float -> int conversion of an out-of-range value is undefined in C++)
    add("|o|_1 = 0.98e15, diagonal", (4.9e14 + mid[0], ym, 4.9e14 + mid[2]), (-1.0, -1e-18, -1.0), "rect")
    add("|o|_1 = 0.98e15, from -x", (-9.8e14, ym, Z(G // 2)), (1.0, 1e-19, 1e-17), "rect")
    # vertical rays inside a cell, away from its borders: exactly that cell, widened by the pad
    for ix, iz in ((0, 0), (G - 1, G - 1), (G // 2, G // 3), (G - 1, 0)):
        add(f"vertical in cell ({ix}, {iz})", (X(ix), yhi + 2, Z(iz)), (1e-20, -1.0, -1e-20), "exact+whole")
        add(f"vertical up in cell ({ix}, {iz})", (X(ix), ylo - 2, Z(iz)), (-1e-20, 1.0, 1e-20), "exact+whole")
    # above the slab going up, below it going down, outside the box going away: nothing to reach
    add("above the slab, up", (X(G // 2), yhi + 0.5, Z(G // 2)), (0.3, 1.0, -0.2), "none")
    add("above the slab, up, flat", (X(0) - 1, yhi + 1e-2, Z(0)), (1.0, 1e-6, 1.0), "none")
    add("below the slab, down", (X(G // 2), ylo - 0.5, Z(G // 2)), (0.1, -1.0, 0.1), "none")
    add("outside the box, away", (float(g[3]) + 5, ym, Z(0)), (1.0, 1e-4, 0.5), "none")
    # flat pieces: a z extent below 1e-2 cells takes the whole run; slopes of 0.9e6 and 1.1e6 (on a grid of <= 63 cells a
    # clipped piece is at most ~64 cells long, so a slope near the 1e6 cut always comes with a z extent below 1e-2 cells)
    length = (float(g[3]) - float(g[0])) + 2 * pad + 2.0
    x_in, x_out = float(g[0]) - pad - 1.0, float(g[3]) + pad + 1.0
    for dzc in (0.5e-2, 0.9e-2):
        add(f"dz = {dzc} cells", (x_in, ym, Z(G // 2)), (1.0, 1e-7, dzc * cell / length), "tight+whole")
    add("dz = 3e-2 cells", (x_in, ym, Z(G // 2)), (1.0, 1e-7, 3e-2 * cell / length), "tight")
    for sl in (0.9e6, 1.1e6):
        add(f"slope {sl:g}", (x_in, ym, Z(G // 2)), (1.0, 1e-7, 1.0 / sl), "tight+whole")
        add(f"slope -{sl:g}", (x_out, ym, Z(G // 2)), (-1.0, -1e-7, 1.0 / sl), "tight+whole")
    # through a cell corner: straight down on it, and diagonally across it both ways
    for ix, iz in ((1, 1), (G // 2, G // 2), (G - 1, 1)):
        cx, cz = float(g[0]) + ix * cell, float(g[1]) + iz * cell
        add(f"down on corner ({ix}, {iz})", (cx, yhi + 1, cz), (1e-12, -1.0, 1e-12), "tight+whole")
        add(f"across corner ({ix}, {iz})", (cx - 3 * cell, ym, cz - 3 * cell), (1.0, 1e-4, 1.0), "tight")
        add(f"across corner ({ix}, {iz}), other diagonal", (cx - 3 * cell, ym, cz + 3 * cell), (1.0, -1e-4, -1.0), "tight")
    # NaN and inf: never 0, never a rectangle -- whatever the other components would make of the ray
    nan, inf = float("nan"), float("inf")
    add("NaN in dx", mid, (nan, -1.0, 0.2), "cannot")
    add("NaN in dx, the rest leaves the slab", (X(0), yhi + 1, Z(0)), (nan, 1.0, 0.2), "cannot")
    add("NaN in dy, the rest crosses the grid", (X(0) - 3, ym, Z(0)), (1.0, nan, 0.5), "cannot")
    add("NaN in dz", (X(0) - 3, ym, Z(0)), (1.0, -1e-3, nan), "cannot")
    add("NaN in o", (nan, ym, 0.0), (1.0, -0.1, 0.2), "cannot")
    add("inf in d", mid, (inf, -1.0, 0.2), "cannot")
    add("-inf in o", (0.0, -inf, 0.0), (0.1, 1.0, 0.2), "cannot")
    add("d all NaN", mid, (nan, nan, nan), "cannot")
    return out


def check_catalogue(rect, runs, cat, g, G):
    bad = []
    for k, (what, o, d, expect) in enumerate(cat):
        v, ix0, nx, iz0, nz = (int(x) for x in rect[k])
        kind = expect.split("+")[0]
        if kind in ("cannot", "none"):
            if v != (-1 if kind == "cannot" else 0):
                bad.append((what, expect, tuple(rect[k])))
            continue
        ex = exact_footprint(o, d, g, G)
        assert ex is not None, what
        (ex0, ex1, ez0, ez1), eruns = ex
        ix1, iz1 = ix0 + nx - 1, iz0 + nz - 1
        if v <= 0 or v != nx * nz or not (ix0 <= ex0 and ix1 >= ex1 and iz0 <= ez0 and iz1 >= ez1):
            bad.append((what, expect, tuple(rect[k]), (ex0, ex1, ez0, ez1)))
            continue
        if kind == "tight" and not (ix0 >= ex0 - 1 and ix1 <= ex1 + 1 and iz0 >= ez0 - 1 and iz1 <= ez1 + 1):
            bad.append((what, "tight", tuple(rect[k]), (ex0, ex1, ez0, ez1)))
        if kind == "exact" and (ix0, ix1, iz0, iz1) != (ex0, ex1, ez0, ez1):
            bad.append((what, "exact", tuple(rect[k]), (ex0, ex1, ez0, ez1)))
        for iz, (c0, c1) in eruns.items():
            rx0, rnx = (int(x) for x in runs[k, iz - iz0])
            if not (rx0 <= c0 and rx0 + rnx - 1 >= c1):
                bad.append((what, f"row {iz}", (rx0, rnx), (c0, c1)))
        if expect.endswith("+whole"):
            for j in range(nz):
                if tuple(runs[k, j]) != (ix0, nx):
                    bad.append((what, f"whole run of row {iz0 + j}", tuple(runs[k, j]), (ix0, nx)))
    assert not bad, (G, bad[:6])


@pytest.mark.parametrize("G", [1, 2, 8, 9, 32, 33, 63])
def test_edge_catalogue_follows_the_f64_derivation(renderer, G):
    needs_xcheck()
    flat, G0, _, g0, _ = case("book")
    g = grid_at(g0, G0, G)
    cat = edge_catalogue(g, G)
    o = np.array([c[1] for c in cat]); d = np.array([c[2] for c in cat])
    rect, runs = renderer.grid_cells(o, d, g, G, minimal_scale(g))
    check_catalogue(rect, runs, cat, g, G)
    if G >= 32:       # (the far rays' margins alone, ~5e9 units, put their unclamped cell coordinates beyond the int range)
        assert 5e-6 * 0.98e15 * float(g[2]) > 2.0 ** 31


# ---- soundness on many rays ----------------------------------------------------------------------------------

def unsound_pairs(o, d, rect, runs, c, r, six, siz):
    """-> (number of reference hits, [(ray, sphere)] hit but outside the device's rectangle or its row's run)."""
    ray, sph = np.nonzero(line_passes_near(o, d, c, r))     # (reference_hits on every pair, but only where it can be true)
    hit = reference_hits_pairs(o[ray], d[ray], c[sph], r[sph])
    ray, sph = ray[hit], sph[hit]
    v, ix0, nx, iz0, nz = (rect[ray, k] for k in range(5))
    sx, sz = six[sph], siz[sph]
    k = np.clip(sz - iz0, 0, 62)
    rx0, rnx = runs[ray, k, 0], runs[ray, k, 1]
    inside = (sx >= ix0) & (sx < ix0 + nx) & (sz >= iz0) & (sz < iz0 + nz) & (sx >= rx0) & (sx < rx0 + rnx)
    ok = (v == -1) | ((v > 0) & inside)
    return len(ray), np.stack([ray[~ok], sph[~ok]], 1)


def soundness(renderer, name, g, n_rays, seed, stop_at_first=False):
    flat, G, n_global, g_layout, slot_of = case(name)
    idx, six, siz = cell_spheres(flat, G, n_global, slot_of)
    c, r = flat["center"][idx], np.abs(flat["radius"][idx])
    o, d = rays_for(flat, g_layout, np.random.default_rng(seed), n_rays)
    cat = edge_catalogue(g_layout, G)
    o = np.concatenate([o, [x[1] for x in cat]]); d = np.concatenate([d, [x[2] for x in cat]])
    rect, runs = renderer.grid_cells(o, d, g, G, minimal_scale(g_layout))
    hits, misses = 0, []
    chunk = max(100, 2_000_000 // max(1, len(idx)))
    for lo in range(0, len(o), chunk):
        h, m = unsound_pairs(o[lo:lo + chunk], d[lo:lo + chunk], rect[lo:lo + chunk], runs[lo:lo + chunk], c, r, six, siz)
        hits += h
        misses += [(lo + a, b) for a, b in m[:4]]
        if misses and stop_at_first:
            break
    return o, d, rect, runs, hits, misses


@pytest.mark.parametrize("name", LAYOUTS)
def test_every_sphere_the_reference_hits_lies_in_the_devices_footprint(renderer, name):
    needs_xcheck()
    flat, G, n_global, g, _ = case(name)
    n_rays = 50_000
    o, d, rect, runs, hits, misses = soundness(renderer, name, g, n_rays, seed=17)
    assert not misses, (name, [(o[a], d[a], tuple(rect[a])) for a, _ in misses[:3]])
    assert hits > 5000                                        # the statement was tested on real hits
    # the rows' runs are never empty and never leave the rectangle
    v, ix0, nx, iz0, nz = (rect[:, k] for k in range(5))
    rows = np.arange(63)[None, :] < np.where(v > 0, nz, 0)[:, None]
    rx0, rnx = runs[:, :, 0], runs[:, :, 1]
    assert np.all(~rows | ((rnx >= 1) & (rx0 >= ix0[:, None]) & (rx0 + rnx <= (ix0 + nx)[:, None])))
    assert np.all(v[v > 0] == (nx * nz)[v > 0]) and np.all(nz[v > 0] <= G) and np.all(nx[v > 0] <= G)
    # the footprints really cull: on the sane rays -- rays_for's rays that the render kernel gives to grid_cells at all
    # (make_tube's TubeRay::sane: |d|^2 within (1e-20, 1e20), |o|_1 < 1e15) -- "cannot tell" is rare and the typical ray marks
    # a small part of the grid: its rectangle on small grids, its rows' runs where the kernel uses them (more than 64 cells)
    of, df = o[:n_rays].astype(f32), d[:n_rays].astype(f32)
    a = (df.astype(np.float64) ** 2).sum(1)
    sane = (a > 1e-20) & (a < 1e20) & (np.abs(of).astype(np.float64).sum(1) < 1e15)
    assert sane.sum() > 10_000
    vs = v[:n_rays][sane]
    assert np.mean(vs == -1) < 0.01, (name, np.mean(vs == -1))
    cells = (np.where(rows, rnx, 0).sum(1) if n_global + G * G > 64 else nx * nz)[:n_rays][sane]
    assert np.median(cells[vs > 0]) <= max(4, G * G // 4), (name, np.median(cells[vs > 0]))
    print(f"{name}: G={G}, {hits} hits checked, cannot tell {np.mean(vs == -1):.4f}, median cells {np.median(cells[vs > 0])}")


def test_the_device_check_can_fail(renderer):
    """With the pad shrunk instead of grown (g7 = -0.15) a sphere straddling a cell border is missed: the check has teeth."""
    needs_xcheck()
    flat, G, n_global, g, _ = case("book")
    g0 = g.copy()
    g0[7] = -0.15
    misses = soundness(renderer, "book", g0, 5000, seed=5, stop_at_first=True)[-1]
    assert misses


# ---- the model against the compiled code ---------------------------------------------------------------------

@pytest.mark.parametrize("name", LAYOUTS)
def test_the_numpy_model_matches_the_device(renderer, name):
    """grid_model.model_grid_cells (test_grid_layout.py's model) with the margins unshrunk and exact-rounded reciprocals:
    the verdict identical on every ray; each bound of the rectangle and of the rows' runs identical on >= 99.9 % of the
    rays and never more than one cell off (v_rcp_f32 is within 1 ulp; the model rounds 1/x exactly)."""
    needs_xcheck()
    flat, G, n_global, g, _ = case(name)
    o, d = rays_for(flat, g, np.random.default_rng(23), 20_000)
    cat = edge_catalogue(g, G)
    o = np.concatenate([o, [x[1] for x in cat]]); d = np.concatenate([d, [x[2] for x in cat]])
    scale = minimal_scale(g)
    rect, runs = renderer.grid_cells(o, d, g, G, scale)
    ix0, ix1, iz0, iz1, kind = model_grid_cells(o, d, g, G, scale, None, shrink=1.0)
    rlo, rhi = model_grid_cells.row_runs
    v = rect[:, 0]
    mv = np.where(kind == 1, (ix1 - ix0 + 1) * (iz1 - iz0 + 1), kind)
    assert np.array_equal(v, mv), (name, np.flatnonzero(v != mv)[:5], rect[v != mv][:5], mv[v != mv][:5])
    sel = v > 0
    dev = np.stack([rect[:, 1], rect[:, 1] + rect[:, 2] - 1, rect[:, 3], rect[:, 3] + rect[:, 4] - 1], 1)[sel]
    mod = np.stack([ix0, ix1, iz0, iz1], 1)[sel]
    diff = np.abs(dev - mod)
    assert diff.max(initial=0) <= 1 and np.all(np.mean(diff == 0, axis=0) >= 0.999), (name, np.mean(diff == 0, axis=0))
    # the rows' runs, row by row (k < nz), as [first, last] column
    ray, k = np.nonzero(np.arange(63)[None, :] < np.where(sel, rect[:, 4], 0)[:, None])
    row = rect[ray, 3] + k
    d0 = runs[ray, k, 0]
    d1 = d0 + runs[ray, k, 1] - 1
    m0, m1 = rlo[ray, row], np.maximum(rhi[ray, row], rlo[ray, row])     # (the device's run is never empty: nx >= 1 by construction)
    rd = np.abs(np.stack([d0 - m0, d1 - m1], 1))
    assert rd.max(initial=0) <= 1, (name, np.argwhere(rd > 1)[:3])
    differs = np.zeros(len(o), bool)
    np.logical_or.at(differs, ray, (rd != 0).any(1))
    assert np.mean(differs[sel]) <= 0.001, (name, np.mean(differs[sel]))
    print(f"{name}: {sel.sum()} rectangles; bounds differing {np.mean(diff != 0, axis=0)}, rays with a differing run {np.mean(differs[sel]):.5f}")
