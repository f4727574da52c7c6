"""The first-hit feature kernel (rt_features.hip) from the viewpoints of test_gpu_viewpoints.py.  The kernel has
a tile selection of its own -- one wave per 8 x 8 pixel tile, the wave-wide bounding rectangle of its lanes' grid_cells rectangles plus
the global tiles, every tile when a lane "cannot tell" or the scene has no grid -- which the book camera's coherent footprints do not
strain.  Here it is reached through Renderer.render_features against tests/features_ref.py, all eight words and the ids bit for bit,
from cameras along the ground, straight down, axis-parallel, inside spheres, below the ground, through a telephoto and at fov 170, on
the small grid, the large grid (G <= 32, 42, 63), a scene with no sphere in any cell and one with a full always-exact list.
test_the_feature_waves_are_hard (no GPU) proves with the grid_model helpers that these frames hold the waves the selection rule can go
wrong on, so that an edit of a camera or a frame size cannot quietly turn the suite into an easy one."""
import ctypes as C
import functools

import numpy as np
import pytest

import features_ref as fr
import rtiow_amd as rt
from features_ref import same
from grid_model import minimal_scale, model_grid_cells
from test_gpu_viewpoints import AXIAL, CAMERAS, GRAZING, SCENES, flat_camera, flat_scene, layout, rt_cam

W, H, SPP, BEGIN = 20, 18, 2, 11        # 3 x 3 wave tiles of 8 x 8 pixels, ragged on both sides; samples 11 and 12
TILE = 8


def straddling_camera(w, h):
    """test_gpu_viewpoints.flat_camera with d.z = 2e-30 u: left of the frame's middle |d.z| <= 1e-30 and grid_cells "cannot tell", right
    of it the ray has a rectangle -- the waves on the middle columns hold lanes of both kinds (no camera of the render suite makes one)."""
    c = flat_camera(0.0)(w, h)
    c.horizontal = (C.c_double * 3)(0.02, 0.0, 2e-30)
    return c


VIEWS = {**CAMERAS, "dz_straddle": straddling_camera}          # the render suite's 18 cameras, in their order, and this file's own

# The reference shows at least one hit in every case but these (at most 2 of the render suite's 108 may be listed):
ALL_SKY = {
    ("book", "up_inside"),              # 0 of 720 samples hit: straight up from the ground between the book's small spheres
}


def case_seed(scene, camera):
    """As the render suite derives it."""
    return 1000 + 17 * list(VIEWS).index(camera) + list(SCENES).index(scene)


@functools.lru_cache(None)
def reference(scene, camera):
    """features_ref's frame of the case, computed once and left unchanged (it depends on the spheres, not on the grid's layout)."""
    flat = flat_scene(SCENES[scene][0])
    feat, ids = fr.render_features(fr.camera_from_rt(rt_cam(VIEWS[camera](W, H))), flat, W, H, SPP, sample_begin=BEGIN,
                                   seed=case_seed(scene, camera))
    feat.setflags(write=False); ids.setflags(write=False)
    return feat, ids


@pytest.mark.gpu
@pytest.mark.parametrize("camera", list(VIEWS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_feature_viewpoint_matches_reference(renderer, oracle_mod, monkeypatch, scene, camera):
    flat, _, _, _, _ = layout(monkeypatch, scene)
    want = reference(scene, camera)
    hits = int(want[0][..., 7].sum())
    assert (hits == 0) == ((scene, camera) in ALL_SKY) and len(ALL_SKY) <= 2, (scene, camera, hits)
    renderer.upload_scene(flat)                                         # RTIOW_GRID_DIM is read here
    got = renderer.render_features(VIEWS[camera](W, H), rt.make_params(W, H, SPP, sample_begin=BEGIN, seed=case_seed(scene, camera)))
    same(got, want)


# ---- what the kernel's selection rule makes of these frames (no GPU) ----------------------------------------------------------------

def wave_footprints(scene, camera, G, g):
    """The model's grid_cells of every camera ray of the case, grouped as the kernel groups them: one entry per (8 x 8 wave tile,
    sample) -> dict(kind [lanes], cells [lanes], union (cells of the bounding rectangle of the lanes with a rectangle), pixels)."""
    ocam = fr.camera_from_rt(rt_cam(VIEWS[camera](W, H)))
    seed = case_seed(scene, camera)
    out = []
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            pix = [(i, j) for j in range(ty, min(ty + TILE, H)) for i in range(tx, min(tx + TILE, W))]      # (lanes past an edge keep nothing)
            for s in range(BEGIN, BEGIN + SPP):
                rays = [fr.camera_ray(ocam, W, H, seed, i, j, s) for i, j in pix]
                o = np.array([r[0][:] for r in rays]); d = np.array([r[1][:] for r in rays])
                ix0, ix1, iz0, iz1, kind = model_grid_cells(o, d, g, G, minimal_scale(g), None, shrink=1.0)
                has = kind == 1
                cells = np.where(has, (ix1 - ix0 + 1) * (iz1 - iz0 + 1), 0)
                union = int((ix1[has].max() - ix0[has].min() + 1) * (iz1[has].max() - iz0[has].min() + 1)) if has.any() else 0
                out.append(dict(kind=kind, cells=cells, union=union, pixels=pix))
    return out


def tile_of(flat, n_global, slot_of):
    """Where rt_tile_layout_host puts the spheres: (the always-exact list -- in no column --, those in the global tiles)."""
    used = slot_of[slot_of >= 0]
    head = slot_of[:32 * n_global]
    return set(range(len(flat))) - set(used.tolist()), set(head[head >= 0].tolist())


MIXED = [(scene, "dz_straddle") for scene in ("book", "big", "big42", "big63", "giants")]
UNION_LARGER = [(scene, camera) for scene in ("book", "big", "big42", "big63") for camera in ("down", "down_rolled")]
WHOLE_GRID = [("book", camera) for camera in GRAZING] + [("big", "ground_diag_20"), ("giants", "telephoto")]
NO_FOOTPRINT = [("book", "in_glass", "global"), ("big63", "in_metal", "global"),          # inside a large sphere, looking over the grid's box
                ("giants", "telephoto", "global"), ("giants", "telephoto", "always"),   # giants above the box, from outside it
                ("book", "ground_x_90", "always")]                                       # the ground beside the box


def test_the_feature_waves_are_hard(monkeypatch):
    """No GPU: what the 8 x 8 waves of the frames above hand to the kernel's selection rule, by the grid_model restatement of grid_cells on
    features_ref's camera rays.  (The boulders scene has no grid at all -- G = 0, the `all_tiles` start value -- and from below_ground every
    wave has a footprint: the waves without one are found elsewhere.)"""
    assert set(GRAZING + AXIAL) <= set(CAMERAS) and {"down", "down_rolled"} <= set(AXIAL)
    grid = {}
    for scene in SCENES:
        flat, G, n_global, g, slot_of = layout(monkeypatch, scene)
        grid[scene] = (flat, G, n_global, g, slot_of)
    assert grid["boulders"][1] == 0 and all(grid[s][1] > 0 for s in SCENES if s != "boulders")

    @functools.lru_cache(None)
    def waves(scene, camera):
        _, G, _, g, _ = grid[scene]
        return wave_footprints(scene, camera, G, g)

    # lanes that "cannot tell" beside lanes with a rectangle: the __ballot(verdict < 0) branch must win over the union
    for scene, camera in MIXED:
        assert any((w["kind"] == -1).any() and (w["kind"] == 1).any() for w in waves(scene, camera)), (scene, camera)
        assert any(not (w["kind"] == -1).any() for w in waves(scene, camera)), (scene, camera)        # ... and the frame has waves without
    # the union is strictly larger than every lane's own rectangle, and it is what the wave scans (no lane "cannot tell")
    for scene, camera in UNION_LARGER:
        assert any(not (w["kind"] == -1).any() and w["union"] > w["cells"].max() > 0 for w in waves(scene, camera)), (scene, camera)
    # the union is the whole grid although every lane can tell
    for scene, camera in WHOLE_GRID:
        G = grid[scene][1]
        assert any(not (w["kind"] == -1).any() and w["union"] == G * G for w in waves(scene, camera)), (scene, camera)
    # no lane of a wave has a footprint in either sample, and the reference still reports hits there: on a sphere of the global
    # tiles, or of the always-exact list
    for scene, camera, where in NO_FOOTPRINT:
        flat, _, n_global, _, slot_of = grid[scene]
        always, in_global = tile_of(flat, n_global, slot_of)
        feat, ids = reference(scene, camera)
        ws = waves(scene, camera)
        found = False
        for k in range(0, len(ws), SPP):                                   # the SPP entries of one wave tile
            if all((w["kind"] == 0).all() for w in ws[k:k + SPP]):
                hit = {int(ids[j, i]) for i, j in ws[k]["pixels"]} - {-1}
                found = found or bool(hit & (in_global if where == "global" else always))
        assert found, (scene, camera, where)
    assert len(tile_of(*[grid["giants"][k] for k in (0, 2, 4)])[0]) == 8          # the giants' always-exact list is full


# ---- seed, sample_begin and t_min away from their usual values ------------------------------------------------------------------------

SEED_HI = 0x123456789ABCDEF0                # k1 = seed >> 32 is not 0
LAST_BEGIN = 2 ** 31 - 1 - SPP              # the last samples rt_params admits


@functools.lru_cache(None)
def reference_params(scene, camera, t_min):
    flat = flat_scene(SCENES[scene][0])
    feat, ids = fr.render_features(fr.camera_from_rt(rt_cam(CAMERAS[camera](W, H))), flat, W, H, SPP, sample_begin=LAST_BEGIN, seed=SEED_HI, t_min=t_min)
    feat.setflags(write=False); ids.setflags(write=False)
    return feat, ids


@pytest.mark.gpu
@pytest.mark.parametrize("camera", ["in_glass", "in_metal", "up_inside"])
@pytest.mark.parametrize("scene", ["book", "giants"])
def test_feature_params_off_the_beaten_path(renderer, oracle_mod, book1_flat, monkeypatch, scene, camera):
    """A seed with a high word, the last sample numbers, and t_min beyond the near sphere: from inside the book's glass sphere (radius 1,
    |d| ~ 3.2: its far root is ~0.32) t_min = 0.5 skips both roots of the enclosing sphere and the ray sees what lies behind it."""
    flat, _, _, _, _ = layout(monkeypatch, scene)
    if scene == "book":
        assert np.array_equal(flat, book1_flat)                           # (the committed scene is the generated one)
    renderer.upload_scene(flat)
    for t_min in (1e-4, 0.5, 2.5):
        want = reference_params(scene, camera, t_min)
        got = renderer.render_features(CAMERAS[camera](W, H), rt.make_params(W, H, SPP, sample_begin=LAST_BEGIN, seed=SEED_HI, t_min=t_min))
        same(got, want)
    if camera == "in_glass":
        near, past = reference_params(scene, camera, 1e-4)[1], reference_params(scene, camera, 0.5)[1]
        assert (near != past).any() and len(np.unique(near)) == 1 and len(np.unique(past)) > 1
