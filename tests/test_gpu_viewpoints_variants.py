"""The pixel-list and the frame-batch variants of the render kernel (kernel_variant bits 8 and 16; rt_kernels.hpp, rt_frames.hip) from the
viewpoints and scene layouts of test_gpu_viewpoints.py, and rt_render_adaptive -- which runs on pixel lists after its first round -- from
one of them.  Both variants are instantiations of their own, and they hand the tile selection waves no dense render forms: a shuffled
list puts unrelated pixels into the four 16-lane groups of a wave (the group bits of the list entries, the readlane(16 g + 15) of the row
ORs and the per-group row words then matter, and a union of short footprints alone can pass kListCap), a frame batch puts rays of unlike
cameras into one wave, and frames of fewer than 64 pixel-samples make one pass of PHASE 1 take several blocks, so that the camera loop
runs two, three or four times.  None of this has a known-answer hook: everything is compared with Oracle B, np.array_equal on the u64
sums, no tolerances.  (Tried on broken builds: a camera loop that stops after its first frame fails the tests of frames below 64
pixel-samples here and no dense test; a wrong group bit in the list entries fails most tests here -- and many dense ones, whose
waves' groups differ often enough.)  test_the_variant_cases_are_hard (no GPU) proves with the grid_model helpers that the lists, seeds and frame sizes
used here still make those waves."""
import functools

import numpy as np
import pytest

import features_ref as fr
import rtiow_amd as rt
from grid_model import minimal_scale, model_grid_cells
from test_gpu_adaptive import adaptive_model
from test_gpu_viewpoints import AXIAL, CAMERAS, GRAZING, K_LIST_CAP, SCENES, flat_scene, layout, oracle_camera, rt_cam, small_grid
from test_launch_plan_host import _model as plan_model

W, H, SPP = 16, 10, 3                   # 160 pixels, 480 pixel-samples: a block of 256 and one of 224, 8 first fills of a wave
PERM_SEED = 11
FRAME_SEED = 31                         # one seed per batch: the layouts big, big42 and big63 share their oracle frames


def case_seed(scene, camera):
    """Derived as the dense suite derives it, from another base.  With the dense suite's own 1000 the case (big63, down) gets the seed
    1105, under which two waves of the ASCENDING list already pass kListCap through their union alone: test_the_variant_cases_are_hard
    asks that none does (the shuffled list is to be what brings that about), and no choice of the permutation changes an ascending list.
    From 4000 every statement of that test holds."""
    return 4000 + 17 * list(CAMERAS).index(camera) + list(SCENES).index(scene)


def permutation(npix):
    return np.random.default_rng(PERM_SEED).permutation(npix).astype(np.uint32)


def pixel_lists(npix):
    """name -> list: shuffled; shuffled with a quarter of its entries again (they land at the list's end, most in the last, partial
    block); every third pixel in ascending order (the shape of an adaptive list with holes)."""
    perm = permutation(npix)
    return {"shuffled": perm, "shuffled, duplicates": np.concatenate([perm, perm[:npix // 4]]), "every third": np.arange(0, npix, 3, dtype=np.uint32)}


def interleaved_cameras():
    """All 18 cameras, neighbours unlike: the axis-parallel ones alternate with the others, the grazing ones spread among those."""
    rest = [c for c in CAMERAS if c not in GRAZING + AXIAL]
    others = []
    for k, c in enumerate(rest):
        others.append(c)
        if k < len(GRAZING):
            others.append(GRAZING[k])
    order = []
    for k in range(max(len(AXIAL), len(others))):
        order += AXIAL[k:k + 1] + others[k:k + 1]
    return order


@functools.lru_cache(None)
def oracle_frame(spheres, camera, w, h, spp, begin, seed):
    """(Oracle-B sums u64 [h,w,3], rays traced) of one dense render, computed once and left unchanged.  `spheres` names the scene's
    spheres (SCENES[layout][0]): the oracle does not depend on RTIOW_GRID_DIM."""
    import oracle
    oracle.load()
    fix, _, st = oracle.render_b(oracle_camera(oracle, CAMERAS[camera](w, h)), flat_scene(spheres),
                                 oracle.make_params(w, h, spp, sample_begin=begin, seed=seed, nthreads=16))
    fix.setflags(write=False)
    return fix, int(st["rays_traced"])


# ---- 1. pixel lists ---------------------------------------------------------------------------------------------------------------------

def check_lists(renderer, scene, camera, G, n_global, w, h, spp, seed, ring):
    cam = CAMERAS[camera](w, h)
    want, rays = oracle_frame(SCENES[scene][0], camera, w, h, spp, 0, seed)
    dense = want.reshape(-1, 3)
    for name, px in pixel_lists(w * h).items():
        got, st = renderer.render_pixels(cam, rt.make_params(w, h, spp, seed=seed), px)
        assert np.array_equal(got, dense[px]), (scene, camera, spp, name, int(np.count_nonzero((got != dense[px]).any(1))))
        assert st["samples"] == len(px) * spp, (scene, camera, spp, name)
        assert st["kernel_variant"] == 8 | small_grid(G, n_global) and st["scan_mode"] == 5, (st["kernel_variant"], st["scan_mode"])
        if ring:
            assert st["direct_samples"] < st["samples"], (scene, camera, spp, name)
        else:
            assert st["direct_samples"] == st["samples"], (scene, camera, spp, name)
        if name == "shuffled":                               # every pixel once: the rays of the dense render
            assert st["rays_traced"] == rays and st["samples"] == w * h * spp, (scene, camera, spp)


@pytest.mark.gpu
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_pixel_lists_match_oracle_b_from_every_viewpoint(renderer, oracle_mod, monkeypatch, scene, camera):
    """3 samples per pixel: every sample is added to the output directly."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    renderer.upload_scene(flat)
    assert W * H * SPP == 480
    check_lists(renderer, scene, camera, G, n_global, W, H, SPP, case_seed(scene, camera), ring=False)


LIST_SHAPES = [("book", "ground_diag_90"), ("big", "telephoto"), ("big63", "down"), ("big63", "lens2"), ("giants", "down_rolled"),
               ("boulders", "in_glass")]


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [8, 40])
@pytest.mark.parametrize("scene,camera", LIST_SHAPES)
def test_pixel_list_block_shapes_from_hard_viewpoints(renderer, oracle_mod, monkeypatch, scene, camera, spp):
    """Block sums in LDS: 8 samples per pixel (blocks shorter than 256), 40 (blocks of 256, which straddle list entries)."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    renderer.upload_scene(flat)
    use_ring, block, _ = plan_model(spp, 0, 1, 0, 0, 0, 0)            # the pixel-list plan: the shipped kernel's 16 slots, no blocks of 1 024
    assert use_ring and (block < 256 if spp == 8 else block == 256 and 256 % spp)
    check_lists(renderer, scene, camera, G, n_global, 10, 6, spp, 77 + spp, ring=True)


# ---- 2. frame batches -------------------------------------------------------------------------------------------------------------------

def check_batch(renderer, scene, G, n_global, order, w, h, spp, begin=0, stride=0, seed=FRAME_SEED):
    want = [oracle_frame(SCENES[scene][0], c, w, h, spp, begin + f * stride, seed) for f, c in enumerate(order)]
    cams = [CAMERAS[c](w, h) for c in order]                 # (Camera objects and hand-built rt_camera structs alike)
    fix, st = renderer.render_frames(cams, rt.make_params(w, h, spp, sample_begin=begin, seed=seed), sample_stride=stride)
    assert fix.shape == (len(order), h, w, 3)
    for f, c in enumerate(order):
        assert np.array_equal(fix[f], want[f][0]), (scene, w, h, spp, stride, f, c, int(np.count_nonzero((fix[f] != want[f][0]).any(2))))
    assert st["samples"] == len(order) * w * h * spp
    assert st["rays_traced"] == sum(r for _, r in want), (scene, w, h, spp, stride)
    assert st["kernel_variant"] == 16 | small_grid(G, n_global) and st["scan_mode"] == 5, (st["kernel_variant"], st["scan_mode"])
    if plan_model(spp, 0, 1, 0, 0, 0, 0)[0]:                 # the frame-batch plan gives block sums in LDS
        assert st["direct_samples"] < st["samples"], (scene, w, h, spp)
    else:
        assert st["direct_samples"] == st["samples"], (scene, w, h, spp)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_eighteen_unlike_frames_in_one_launch(renderer, oracle_mod, monkeypatch, scene):
    """All 18 cameras as one batch, neighbours unlike, forwards and backwards (other frames meet in a wave), every frame the same
    samples; then frame f the samples [5 + 1000 f, ...)."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    renderer.upload_scene(flat)
    order = interleaved_cameras()
    st = check_batch(renderer, scene, G, n_global, order, W, H, SPP)
    assert st["samples"] == 18 * 480
    check_batch(renderer, scene, G, n_global, order[::-1], W, H, SPP)
    check_batch(renderer, scene, G, n_global, order, W, H, SPP, begin=5, stride=1000)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_two_frames_share_every_first_fill(renderer, oracle_mod, monkeypatch, scene):
    """4 x 4 pixels at 3 samples: one block of 48 items per frame, so a wave's first pass takes two blocks and its camera loop two turns."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    renderer.upload_scene(flat)
    check_batch(renderer, scene, G, n_global, interleaved_cameras(), 4, 4, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_three_and_four_frames_in_one_pass(renderer, oracle_mod, monkeypatch, scene):
    """2 x 2 pixels, a frame is one block.  At 9 samples (36 items) a first fill takes 36 + 28; the 8 left over, the next frame's 36 and
    the head of the one after it then meet in a later pass as soon as 45 lanes want work.  At 7 samples (28 items) every first fill
    certainly holds three frames, 28 + 28 + 8.  At 8 samples (32 items) the fills fall on frame pairs, and here the frames' sample ranges
    follow one another.  All three keep their block sums in LDS.  At 4 samples (16 items; no block sums below 5 samples per pixel) a
    fill holds four frames."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    renderer.upload_scene(flat)
    order = interleaved_cameras()
    assert all(plan_model(spp, 0, 1, 0, 0, 0, 0)[0] for spp in (9, 7, 8)) and not plan_model(4, 0, 1, 0, 0, 0, 0)[0]
    check_batch(renderer, scene, G, n_global, order, 2, 2, 9)
    check_batch(renderer, scene, G, n_global, order, 2, 2, 7)
    check_batch(renderer, scene, G, n_global, order, 2, 2, 8, stride=8)
    check_batch(renderer, scene, G, n_global, order, 2, 2, 4)


RING_CAMERAS = ["ground_diag_90", "telephoto", "down_rolled", "in_glass", "dz_1e-12", "fov170"]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["book", "big63", "giants"])
def test_blocks_that_end_inside_a_frame_with_block_sums(renderer, oracle_mod, monkeypatch, scene):
    """10 x 6 at 40 samples: 2 400 items per frame, 9 blocks of 256 and one of 96; at 8 samples 480 items in blocks shorter than 256."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    renderer.upload_scene(flat)
    assert plan_model(40, 0, 1, 0, 0, 0, 0) == (1, 256, 0) and (10 * 6 * 40) % 256 == 96
    block8 = plan_model(8, 0, 1, 0, 0, 0, 0)[1]
    assert plan_model(8, 0, 1, 0, 0, 0, 0)[0] and block8 < 256 and (10 * 6 * 8) % block8
    check_batch(renderer, scene, G, n_global, RING_CAMERAS, 10, 6, 40)
    check_batch(renderer, scene, G, n_global, RING_CAMERAS, 10, 6, 8)


# ---- 3. adaptive sampling ---------------------------------------------------------------------------------------------------------------

AW, AH, ASTEP, ACAP, AFLOOR, ASEED, ACAMERA = 24, 14, 4, 32, 0.01, 3, "ground_diag_90"
ATHRESHOLD = {"book": 0.02, "big": 0.02}          # chosen on the CPU from the model alone: about half the pixels stop at 2 * step, 24 % and
                                                  # 40 % go to the cap, four distinct counts (the shares are asserted below)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(ATHRESHOLD))
def test_render_adaptive_from_a_hard_viewpoint(renderer, oracle_mod, monkeypatch, scene):
    """rt_render_adaptive against the loop run in numpy on Oracle-B passes: count, fix and half bit for bit.  After round 1 every launch
    is a pixel list in ascending order with holes, from a camera whose rays cross the whole grid."""
    flat, G, n_global, _, _ = layout(monkeypatch, scene)
    passes = [oracle_frame(SCENES[scene][0], ACAMERA, AW, AH, ASTEP, k * ASTEP, ASEED)[0] for k in range(ACAP // ASTEP)]
    mf, mh, mc, rounds = adaptive_model(passes, ASTEP, ACAP, ATHRESHOLD[scene], AFLOOR)
    share_min, share_cap = (mc == 2 * ASTEP).mean(), (mc == ACAP).mean()
    print(f"model: mean {mc.mean():.1f} spp, {100 * share_min:.1f} % at {2 * ASTEP}, {100 * share_cap:.1f} % at {ACAP}, active per round {rounds}")
    assert share_min >= 0.10 and share_cap >= 0.10                   # (the model's result: no vacuous pass)
    renderer.upload_scene(flat)
    fix, half, count, st = renderer.render_adaptive(CAMERAS[ACAMERA](AW, AH), rt.make_params(AW, AH, ACAP, seed=ASEED),
                                                    rt.make_adaptive(ASTEP, ATHRESHOLD[scene], AFLOOR))
    assert np.array_equal(count, mc)
    assert np.array_equal(fix, mf)
    assert np.array_equal(half, mh)
    assert st["samples"] == int(mc.sum(dtype=np.uint64))


# ---- 4. what the tile selection makes of these lists and frames (no GPU) ----------------------------------------------------------------

def first_fill_waves(scene, camera, G, n_global, g, px, w=W, h=H, spp=SPP, block_items=256):
    """The bounce-0 footprints of the list's items, grouped as the kernel groups a first fill: item t is sample t % spp of pixel
    px[t // spp]; blocks of block_items; waves of 64 items within a block; groups of 16.  One entry per wave:
    dict(union (set of cells), groups (the sets of its groups of 16), most (the most cells one of its rays marks), listed (the wave scans
    a list whose entries carry group bits: always on a small grid; on a large one unless a ray "cannot tell" or the list would pass
    kListCap -- then every group scans the whole table)).  A cell is (ix, iz): the rectangle on a small grid, the row runs on a large one; a
    ray that "cannot tell" marks every cell."""
    ocam = fr.camera_from_rt(rt_cam(CAMERAS[camera](w, h)))
    seed = case_seed(scene, camera)
    items = [(int(px[t // spp]), t % spp) for t in range(len(px) * spp)]
    rays = [fr.camera_ray(ocam, w, h, seed, p % w, p // w, s) for p, s in items]
    o = np.array([r[0][:] for r in rays]); d = np.array([r[1][:] for r in rays])
    ix0, ix1, iz0, iz1, kind = model_grid_cells(o, d, g, G, minimal_scale(g), None, shrink=1.0)
    rlo, rhi = model_grid_cells.row_runs
    every = {(x, z) for x in range(G) for z in range(G)}

    def cells(k):
        if kind[k] < 0:
            return every
        if kind[k] == 0:
            return set()
        if small_grid(G, n_global):
            return {(x, z) for z in range(iz0[k], iz1[k] + 1) for x in range(ix0[k], ix1[k] + 1)}
        return {(x, z) for z in range(iz0[k], iz1[k] + 1) for x in range(rlo[k, z], rhi[k, z] + 1)}

    per_ray = [cells(k) for k in range(len(items))]
    out = []
    for b0 in range(0, len(items), block_items):
        for w0 in range(b0, min(b0 + block_items, len(items)), 64):
            lanes = range(w0, min(w0 + 64, b0 + block_items, len(items)))
            groups = [set().union(*[per_ray[k] for k in lanes[q:q + 16]]) for q in range(0, len(lanes), 16)]
            union = set().union(*groups)
            listed = small_grid(G, n_global) or (all(kind[k] >= 0 for k in lanes) and n_global + len(union) <= K_LIST_CAP)
            out.append(dict(union=union, groups=groups, most=max(len(per_ray[k]) for k in lanes), listed=listed))
    return out


GROUPS_DIFFER = [("book", "ground_x_20"), ("big", "ground_x_90"), ("big42", "in_glass"), ("big63", "ground_x_90")]


def test_the_variant_cases_are_hard(monkeypatch):
    """No GPU: the waves the lists of test 1 hand to the tile selection, and the frame sizes and the frame order of test 2."""
    ascending, shuffled = np.arange(W * H, dtype=np.uint32), permutation(W * H)
    assert sorted(shuffled.tolist()) == ascending.tolist()

    def waves(scene, camera, px):
        _, G, n_global, g, _ = layout(monkeypatch, scene)
        ws = first_fill_waves(scene, camera, G, n_global, g, px)
        assert len(ws) == 8
        return ws, n_global

    # a group of 16 whose cells are a proper subset of the wave's: its bits in the list entries are not all set.  Nearly every wave of
    # a shuffled list has one, hardly any of an ascending list (which is what a dense render forms)
    subset = lambda ws: sum(wv["listed"] and any(gr < wv["union"] for gr in wv["groups"]) for wv in ws)
    for scene, camera in GROUPS_DIFFER:
        assert subset(waves(scene, camera, shuffled)[0]) >= 6, (scene, camera)
        assert subset(waves(scene, camera, ascending)[0]) <= 2, (scene, camera)
    # G = 63 from above: no ray marks more than 8 cells, and the union of a shuffled wave alone passes kListCap (the fall-back to the
    # whole table); no wave of the ascending list does
    ws, n_global = waves("big63", "down", shuffled)
    assert any(n_global + len(wv["union"]) > K_LIST_CAP and wv["most"] <= 8 for wv in ws)
    ws, n_global = waves("big63", "down", ascending)
    assert not any(n_global + len(wv["union"]) > K_LIST_CAP for wv in ws)
    # ... and through a wide lens every wave of the shuffled list passes it
    ws, n_global = waves("big63", "lens2", shuffled)
    assert all(n_global + len(wv["union"]) > K_LIST_CAP for wv in ws)
    # frames of fewer than 64 pixel-samples.  4 x 4 x 3: two share every first fill.  2 x 2 x 9: a pass can hold the tail of one frame,
    # a whole one and the head of a third.  2 x 2 x 7: every first fill holds two whole frames and the head of a third.  2 x 2 x 4: four
    assert 4 * 4 * 3 < 64 < 2 * 4 * 4 * 3 and 1 + 2 * 2 * 9 + 1 <= 64 and 2 * 2 * 7 + 2 * 2 * 7 < 64 < 3 * 2 * 2 * 7 and 4 * 2 * 2 * 4 == 64
    # the batch's order: all 18 cameras, no two neighbours both grazing or both axis-parallel -- forwards, hence backwards too
    order = interleaved_cameras()
    assert sorted(order) == sorted(CAMERAS) and len(order) == 18
    for a, b in zip(order, order[1:]):
        assert not (a in GRAZING and b in GRAZING) and not (a in AXIAL and b in AXIAL), (a, b)
    assert set(RING_CAMERAS) <= set(CAMERAS) and {c for _, c in LIST_SHAPES + GROUPS_DIFFER} <= set(CAMERAS)
