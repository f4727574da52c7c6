"""End-to-end parity from viewpoints the other parity tests never take.  Which tiles a wave scans (rt_kernels.hpp: the
small grid's 64-bit cell mask, the large grid's LDS row words of 32 and 64 bits, the 16-ray group bits, the fall-back to
the whole table past kListCap) has no known-answer hook: it is reached here through Renderer.render, against Oracle B bit
for bit (sums and rays_traced), from cameras whose footprints are long (several 14-tile segments, more than kListCap
cells), vertical, axis-parallel or degenerate, inside spheres and below the ground.  test_the_hard_cases_are_hard (no GPU)
proves with the grid_model helpers that the cameras still make those footprints, so that an edit of a camera cannot
quietly turn a case into an easy one."""
import ctypes as C
import functools

import numpy as np
import pytest

import rtiow_amd as rt
from rtiow_amd import _ffi
from grid_model import minimal_scale, model_grid_cells

K_LIST_CAP = 126           # rt_params.hpp kListCap: the longest tile list a wave scans by list
K_SEG_TILES = 14           # tiles per segment of the tile loop (kSegTilesTube / 2)


def _mat(rng):
    k = rng.integers(0, 3)
    return (rt.Lambertian(rng.uniform(0.05, 0.95, 3)) if k == 0 else
            rt.Metal(rng.uniform(0.5, 1.0, 3), float(rng.uniform(0.0, 0.5))) if k == 1 else rt.Dialectric(1.5))


def _boulders():
    """~200 overlapping spheres of radius 1.5-3 within 5 units, plus the ground: every one is too large for a cell even
    at one cell (r > cell / 4), so no cell holds a sphere and rays scan only tiles every ray scans."""
    rng = np.random.default_rng(7)
    w = rt.HittableList()
    w.push(rt.Sphere(rt.Point3(0, -1000, 0), 1000, rt.Lambertian(rt.Color(0.5, 0.5, 0.5))))
    for _ in range(200):
        r = float(rng.uniform(1.5, 3.0))
        w.push(rt.Sphere(np.array([rng.uniform(-2.4, 2.4), r * rng.uniform(0.5, 1.0), rng.uniform(-2.4, 2.4)]), r, _mat(rng)))
    return w.flatten()


def _giants():
    """The book's small spheres on a 13 x 13 lattice plus 11 giants (radius 2.5-4, > 8x the median 0.2): the always-exact
    list holds the 8 largest, the other 3 go through the filter."""
    rng = np.random.default_rng(8)
    w = rt.random_scene(3, grid=(-6, 6))
    for k in range(11):
        r = 2.5 + 0.15 * k
        w.push(rt.Sphere(np.array([rng.uniform(-20, 20), r, rng.uniform(-20, 20)]), r, _mat(rng)))
    return w.flatten()


# name -> (scene, RTIOW_GRID_DIM)
SCENES = {"book": ("book", None), "big": ("big", None), "big42": ("big", "42"), "big63": ("big", "63"),
          "boulders": ("boulders", None), "giants": ("giants", None)}


@functools.lru_cache(None)
def flat_scene(which):
    return {"book": lambda: rt.random_scene(1).flatten(),
            "big": lambda: rt.random_scene(1, grid=(-27, 27)).flatten(),       # ~3 000 spheres: the large-grid kernel
            "boulders": _boulders, "giants": _giants}[which]()


def layout(monkeypatch, name):
    which, gd = SCENES[name]
    if gd:
        monkeypatch.setenv("RTIOW_GRID_DIM", gd)
    else:
        monkeypatch.delenv("RTIOW_GRID_DIM", raising=False)
    flat = flat_scene(which)
    (G, n_global), g, slot_of = rt.tile_layout_host(flat)
    return flat, G, n_global, g, slot_of


def look(frm, at, vup=(0, 1, 0), fov=20.0, aperture=0.0, focus=None):
    def make(w, h):
        f = focus if focus is not None else float(np.linalg.norm(np.subtract(frm, at)))
        return rt.Camera(np.array(frm, float), np.array(at, float), np.array(vup, float), fov, w / h, aperture, f)
    return make


def flat_camera(dz):
    """Hand-built (like test_gpu_oracle_holes.degenerate_camera): every camera ray has d.z = dz EXACTLY (origin.z = 0,
    horizontal.z = vertical.z = 0, lower_left_corner.z = dz, no lens); the rays graze along -x through the slab at z = 0."""
    def make(w, h):
        c = _ffi.rt_camera()
        c.origin = (C.c_double * 3)(30.0, 0.35, 0.0)
        c.lower_left_corner = (C.c_double * 3)(29.0, 0.34, dz)
        c.horizontal = (C.c_double * 3)(0.02, 0.0, 0.0)
        c.vertical = (C.c_double * 3)(0.0, 0.02, 0.0)
        c.u = (C.c_double * 3)(0.0, 0.0, 1.0)
        c.v = (C.c_double * 3)(0.0, 1.0, 0.0)
        c.lens_radius = 0.0
        return c
    return make


CAMERAS = {
    # at ground level, looking along +x, +z and the grid's diagonal (a slight downward tilt: the centre ray is not flat)
    "ground_x_20": look((-30, 0.3, 0.45), (30, 0.25, 0.45), fov=20), "ground_x_90": look((-30, 0.3, 0.45), (30, 0.25, 0.45), fov=90),
    "ground_z_20": look((0.45, 0.3, -30), (0.45, 0.25, 30), fov=20), "ground_z_90": look((0.45, 0.3, -30), (0.45, 0.25, 30), fov=90),
    "ground_diag_20": look((-30, 0.3, -30), (30, 0.2, 30), fov=20), "ground_diag_90": look((-30, 0.3, -30), (30, 0.2, 30), fov=90),
    # straight down (vup along -z), the same rolled, straight up from inside the grid
    "down": look((0.3, 30, 0.2), (0.3, 0, 0.2), vup=(0, 0, -1), fov=40),
    "down_rolled": look((0.3, 30, 0.2), (0.3, 0, 0.2), vup=(0.6, 0, -0.8), fov=40),
    "up_inside": look((1.5, 0.25, 1.5), (1.5, 10, 1.5), vup=(0, 0, 1), fov=60),
    # inside the book's glass sphere and its metal sphere; below the ground plane
    "in_glass": look((0, 1, 0), (3, 1.2, 1), fov=60), "in_metal": look((4, 1.1, 0.1), (0, 0.5, 2), fov=60),
    "below_ground": look((2, -3, 1), (0, 0.5, 0), fov=60),
    # a telephoto ~500 away grazing the grid from outside its box, along the diagonal
    "telephoto": look((-350, 0.3, -350), (0, 0.2, 0), fov=1.0),
    "fov170": look((13, 2, 3), (0, 0, 0), fov=170), "lens2": look((13, 2, 3), (0, 0, 0), fov=30, aperture=4.0, focus=10.0),
    "dz_0": flat_camera(0.0), "dz_1e-31": flat_camera(1e-31), "dz_1e-12": flat_camera(1e-12),
}
GRAZING = ["ground_diag_20", "ground_diag_90", "telephoto"]
# vertical, or parallel to x: a z extent of ~0 cells takes the whole run (or a zero component "cannot tell"); a ray parallel
# to z has the slope 0 and needs no special branch
AXIAL = ["ground_x_20", "ground_x_90", "down", "down_rolled", "up_inside", "dz_0", "dz_1e-31", "dz_1e-12"]


def rt_cam(cam):
    return cam if isinstance(cam, _ffi.rt_camera) else cam.to_rt_camera()


def oracle_camera(oracle_mod, cam):
    oc = oracle_mod.camera()
    rc = rt_cam(cam)
    for name, _ in _ffi.rt_camera._fields_:
        setattr(oc, name, getattr(rc, name))
    return oc


def centre_footprint(flat, G, n_global, g, cam):
    """The footprint of the camera's centre ray (grid_model, margins unshrunk): (verdict, cells marked, whole run)."""
    rc = rt_cam(cam)
    o = np.array(rc.origin[:])
    d = np.array(rc.lower_left_corner[:]) + 0.5 * np.array(rc.horizontal[:]) + 0.5 * np.array(rc.vertical[:]) - o
    ix0, ix1, iz0, iz1, kind = model_grid_cells(o[None], d[None], g, G, minimal_scale(g), None, shrink=1.0)
    rlo, rhi = model_grid_cells.row_runs
    if n_global + G * G > 64:
        cells = int(sum(rhi[0, z] - rlo[0, z] + 1 for z in range(iz0[0], iz1[0] + 1)))
    else:
        cells = int((ix1[0] - ix0[0] + 1) * (iz1[0] - iz0[0] + 1))
    return int(kind[0]), cells, bool(model_grid_cells.whole[0])


def test_the_hard_cases_are_hard(monkeypatch):
    """No GPU: what the scenes' layouts and the cameras' centre rays make of the tile list."""
    W, H = 16, 10
    shapes = {}
    for name in SCENES:
        flat, G, n_global, g, slot_of = layout(monkeypatch, name)
        shapes[name] = (G, n_global)
        if name in ("book", "big", "big42", "big63"):
            for cam in GRAZING:          # one ray alone fills more than one 14-tile segment
                kind, cells, _ = centre_footprint(flat, G, n_global, g, CAMERAS[cam](W, H))
                assert kind == 1 and n_global + cells > K_SEG_TILES, (name, cam, kind, cells)
            for cam in AXIAL:            # vertical and axis-parallel: the whole run, or "cannot tell"
                kind, cells, whole = centre_footprint(flat, G, n_global, g, CAMERAS[cam](W, H))
                assert kind == -1 or (kind == 1 and whole), (name, cam, kind, whole)
        if name == "big63":              # one ray alone marks more cells than the list holds: the fall-back is certain
            for cam in ("ground_diag_20", "ground_diag_90", "telephoto"):
                kind, cells, _ = centre_footprint(flat, G, n_global, g, CAMERAS[cam](W, H))
                assert kind == 1 and cells > K_LIST_CAP - n_global, (cam, cells, n_global)
        if name == "boulders":           # no cell holds a sphere
            assert G == 0 or np.all(slot_of[32 * n_global:] < 0)
        if name == "giants":             # the always-exact list is full; three giants go through the filter (global tiles)
            r = np.abs(flat["radius"])
            used = slot_of[slot_of >= 0]
            missing = np.setdiff1d(np.arange(len(flat)), used)
            big = np.flatnonzero(r > 8 * np.median(r))
            assert len(big) == 12 and len(missing) == 8 and len(np.intersect1d(big, used)) == 4   # (the ground and 3 giants)
            assert np.all(np.isin(big[np.isin(big, used)], slot_of[:32 * n_global]))
    # the kernels the scenes take: the small-grid one (64-bit cell mask) for the book, the large-grid one with 32-bit row
    # words (G <= 32) for the 3 000-sphere scene, 64-bit words under G = 42 and 63
    assert shapes["book"][0] > 0 and shapes["book"][1] + shapes["book"][0] ** 2 <= 64
    assert 8 < shapes["big"][0] <= 32 and shapes["big42"][0] == 42 and shapes["big63"][0] == 63


def small_grid(G, n_global):
    return G > 0 and n_global + G * G <= 64


def check(renderer, oracle_mod, flat, cam, w, h, spp, seed, flags=0, what=None):
    sm, fix, st = renderer.render(cam, rt.make_params(w, h, spp, seed=seed, flags=flags))
    fb, sb, stb = oracle_mod.render_b(oracle_camera(oracle_mod, cam), flat,
                                      oracle_mod.make_params(w, h, spp, seed=seed, nthreads=16,
                                                             uniform53=bool(flags & rt.RT_FLAG_UNIFORM53)))
    assert np.array_equal(fix, fb), (what, int(np.count_nonzero((fix != fb).any(2))))
    assert np.array_equal(sm.view(np.uint32), sb.view(np.uint32)), what
    assert st["rays_traced"] == stb["rays_traced"], what
    assert st["samples"] == w * h * spp
    return fix, st


@pytest.mark.gpu
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_viewpoint_matches_oracle_b(renderer, oracle_mod, monkeypatch, scene, camera):
    """3 samples per pixel (every sample written to the frame buffer directly); on the book and G = 63 scenes the grazing
    and axis cameras also without the filter (RT_FLAG_NO_FILTER), which must give the same bits."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    renderer.upload_scene(flat)
    cam = CAMERAS[camera](16, 10)
    seed = 1000 + 17 * list(CAMERAS).index(camera) + list(SCENES).index(scene)
    fix, st = check(renderer, oracle_mod, flat, cam, 16, 10, 3, seed, what=(scene, camera))
    assert st["kernel_variant"] == (1 if small_grid(G, n_global) else 0) and st["direct_samples"] == st["samples"]
    if scene in ("book", "big63") and camera in GRAZING + AXIAL + ["ground_z_20"]:
        fix0, st0 = check(renderer, oracle_mod, flat, cam, 16, 10, 3, seed, flags=rt.RT_FLAG_NO_FILTER, what=(scene, camera, "no filter"))
        assert np.array_equal(fix0, fix) and st0["rays_traced"] == st["rays_traced"]
        assert st0["kernel_variant"] == 0 and st0["scan_mode"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene,camera,w,h,spp,flags,large", [
    ("book", "ground_diag_90", 10, 6, 40, 0, False),            # block sums in LDS
    ("big", "telephoto", 10, 6, 40, 0, False),
    ("big63", "ground_diag_20", 10, 6, 40, 0, False),
    ("giants", "down_rolled", 10, 6, 40, 0, False),
    ("book", "telephoto", 6, 4, 150, 0, True),                  # work blocks of 1 024 pixel-samples, small-grid kernel
    ("big", "ground_diag_90", 6, 4, 150, 0, True),              # ... and the large-grid kernel
    ("big42", "dz_1e-12", 8, 5, 37, rt.RT_FLAG_UNIFORM53, False),
])
def test_launch_shapes_from_hard_viewpoints(renderer, oracle_mod, monkeypatch, scene, camera, w, h, spp, flags, large):
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    if large:
        monkeypatch.setenv("RTIOW_LARGE_BLOCK_MIN_ITEMS", "0")
    renderer.upload_scene(flat)
    _, st = check(renderer, oracle_mod, flat, CAMERAS[camera](w, h), w, h, spp, seed=77 + spp, flags=flags, what=(scene, camera, spp))
    want = (1 if small_grid(G, n_global) else 0) | (2 if flags & rt.RT_FLAG_UNIFORM53 else 0) | (4 if large else 0)
    assert st["kernel_variant"] == want, (st["kernel_variant"], want)
    assert st["direct_samples"] < st["samples"]
