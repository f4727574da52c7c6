"""The dense capped kernels after the third cut of their scalar stream (rt_kernels.hpp behind `if constexpr (CAPPED)`; DESIGN.md section 6,
"the scalar port"): the small-grid pair walks a segment's candidate bitmaps in an inline-asm block (`kAsmWalk`: v_cmpx narrows exec to the lanes
that have a candidate, the refill of a used-up word runs under a second v_cmpx, the pooled rounds stay C++ and run when the block leaves with 64
pairs waiting) and takes the pooled minimum without a lane-level region.  The ring must hold the same pairs in the same order: every frame must
stay what it was.

As in test_gpu_scalar_trim_segments.py every case is rendered through Renderer.render_device in a child process of its own per body
(RTIOW_DENSE_BODY=capped / classic is in the environment before the library loads) at 64 x 48 x 8 spp, depth 8, which runs the instantiation
for blocks of 256, and -- the launch plan gives blocks of 1 024 to the small-grid kernel from 69 samples per pixel on (rt_launch.hpp), so 8 spp
cannot reach them -- again at 32 x 24 x 70 spp with RTIOW_LARGE_BLOCK_MIN_ITEMS=0 for the instantiation on blocks of 1 024, as
test_gpu_scalar_trim_segments.py reaches it; every frame is compared sum for sum (u64) body against body and with Oracle B; rays_traced, samples, candidates and exact_roots of rt_stats must be equal, and rt_last_dense_body says the capped body ran.  Each
child also renders every scene once at 64 x 48 x 8 with RT_FLAG_DIAG_STATS (the classic kernel whatever the body: the capped one has no counters), whose
candidate count is what the pile's precondition is checked against on the device.

Scenes where the walk can go wrong, each with its precondition asserted from the host layout (rt_tile_layout_host) and f64 geometry before
anything is rendered:

* tiles_14 / tiles_15 / tiles_29: 448, 449 and 900 spheres of radius 1.5 ... 2.5 over 12 x 12 -- one grid cell whose tile holds 32 of them and
  13, 14 and 28 global tiles: a wave whose rays reach the cell scans 14 (one full segment), 15 (a second segment of one word) and 29 tiles
  (14 + 14 + 1), a wave whose rays all miss the grid's box 13, 14 and 28.  The ring persists across the segments.
* pile: 144 spheres of radius 0.3 with their centres within 0.06 of the corner that the four cells of a 2 x 2 grid share, 36 in each quadrant,
  so that each cell's tile is full (slots 0 ... 31) and 16 of them overflow into the one global tile, seen head-on from 3 away.  The rays of a
  pixel all leave one point (no aperture), and the (u, v) whose ray hits a sphere form a convex set: when the rays through the four corners of
  a pixel's jitter square hit a sphere, every ray the kernel can draw for that pixel does, and what a ray can hit the filter keeps.  So such a
  pixel's lanes own, for certain, candidates in five words of one segment (>= 3 asked), 32 bits of a cell's word with bit 0 and bit 31 among
  them (>= 16 asked), and 144 pairs each: one lane alone pushes more than the ring's 128 entries in one walk, the ring index wraps and pooled
  rounds fire between the walk's trips.  The classic kernel's candidate counter must show at least those pairs.
* pile_sky: the same pile seen at 120 degrees, where it is three pixels wide, centred on pixel column 31, and well over half of the image is sky.  A ray further than
  three radii from every centre has no candidate (the filter keeps a sphere only while both components of the offset, i.e. at least the distance
  / sqrt 2, stay below 1.02 bounds, and the bound is the radius here), and some run of eight pixels that a wave starts together (64 items of
  8 spp) holds such a pixel beside one whose rays own two or more bits of one word: lanes without a candidate and lanes in the middle of a word
  in the same trip (asserted for the 8 spp shape; at 70 spp a wave starts inside one or two pixels)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEPTH, SEED = 8, 1
SIZES = {False: (64, 48, 8), True: (32, 24, 70)}            # blocks of 1 024 -> (width, height, spp)
SCENES = ("tiles_14", "tiles_15", "tiles_29", "pile", "pile_sky")
# name -> (scene, RTIOW_LARGE_BLOCK_MIN_ITEMS=0 in the child for this render: the instantiation for blocks of 1 024)
SHAPES = [(f"{s}_{'1024' if large else '256'}", s, large) for s in SCENES for large in (False, True)]
# scene -> (grid cells per side, global tiles) of the host layout
LAYOUTS = {"tiles_14": (1, 13), "tiles_15": (1, 14), "tiles_29": (1, 28), "pile": (2, 1), "pile_sky": (2, 1)}
PILE_AT = np.array([0.0, 0.3, 0.0])
PILE_R, PILE_PER_CELL = 0.3, 36


def camera(scene, w, h):
    import rtiow_amd as rt
    if scene == "pile":
        return rt.Camera(PILE_AT + (0.35, 0.25, 3.0), PILE_AT, (0.0, 1.0, 0.0), 19.0, float(w) / float(h), 0.0, 3.0)
    if scene == "pile_sky":
        return rt.Camera(PILE_AT + (0.35, 0.25, 3.0), PILE_AT, (0.0, 1.0, 0.0), 120.0, float(w) / float(h), 0.0, 3.0)
    return rt.book1_camera(w, h)


def scenes():
    import rtiow_amd as rt
    rng = np.random.default_rng(53)

    def make(centers, radii):
        n = len(radii)
        flat = np.zeros(n, dtype=rt.SPHERE_DTYPE)
        flat["center"], flat["radius"] = centers, radii
        kind = np.arange(n) % 3                                 # Lambertian, Metal, Dialectric in turn
        flat["kind"] = kind
        flat["albedo"] = rng.uniform(0.3, 0.9, (n, 3))
        flat["param"] = np.where(kind == 1, 0.3, np.where(kind == 2, 1.5, 0.0))
        return flat

    def tiles(n):
        radii = rng.uniform(1.5, 2.5, n)
        c = rng.uniform(-6, 6, (n, 3)) * (1, 0, 1)
        c[:, 1] = radii
        return make(c, radii)

    # the pile: quadrant by quadrant around the corner (0, 0) of the 2 x 2 grid that four far markers span; the markers come LAST in the list, so
    # the first 32 spheres of each quadrant fill its cell's tile and the quadrant's other four and its marker go to the global tile
    quads = [(sx, sz) for sz in (-1.0, 1.0) for sx in (-1.0, 1.0)]
    c = np.concatenate([PILE_AT + rng.uniform(0.01, 0.06, (PILE_PER_CELL, 3)) * (sx, 0.3, sz) for sx, sz in quads] +
                       [np.array([[12.0 * sx, 0.3, 12.0 * sz] for sx, sz in quads])])
    pile = make(c, np.full(len(c), PILE_R))
    return {"tiles_14": tiles(448), "tiles_15": tiles(449), "tiles_29": tiles(900), "pile": pile, "pile_sky": pile}


def child(in_path, out_path):
    """Renders every shape with the body the environment names, and every scene once with RT_FLAG_DIAG_STATS; the sums, the statistics and which
    body ran go to out_path."""
    import torch
    import rtiow_amd as rt
    data = np.load(in_path, allow_pickle=False)
    out = {}

    def render(r, scene, large, flags):
        w, h, spp = SIZES[large]
        d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        r.render_device(camera(scene, w, h), rt.make_params(w, h, spp, max_depth=DEPTH, seed=SEED, flags=flags), d_fix.data_ptr())
        torch.cuda.synchronize()
        st = r.last_stats()
        return d_fix.cpu().numpy().view(np.uint64), np.array([st["rays_traced"], st["samples"], st["candidates"], st["exact_roots"], st["kernel_variant"],
                                                              st["scan_mode"], r._lib.rt_last_dense_body(r._h)], dtype=np.int64)

    with rt.Renderer(0) as r:
        for scene in SCENES:
            r.upload_scene(np.ascontiguousarray(data[scene].view(rt.SPHERE_DTYPE).reshape(-1)))
            for name, s, large in SHAPES:
                if s != scene:
                    continue
                if large:
                    os.environ["RTIOW_LARGE_BLOCK_MIN_ITEMS"] = "0"         # (read per launch)
                else:
                    os.environ.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
                out[name], out[name + "_stats"] = render(r, scene, large, 0)
            os.environ.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
            out[scene + "_diag"], out[scene + "_diag_stats"] = render(r, scene, False, rt.RT_FLAG_DIAG_STATS)
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child(sys.argv[1], sys.argv[2])
    sys.exit(0)

pytestmark = pytest.mark.gpu


def corner_rays(cam, W, H):
    """-> origin (3,), directions [H, W, 4, 3]: camera.rs:47-54 without a lens for the four corners of every pixel's jitter square,
    u in [i, i + 1] / (W - 1), v in [j, j + 1] / (H - 1) (main.rs:131-132)."""
    u = (np.arange(W)[None, :, None] + np.array([0.0, 1.0, 0.0, 1.0])[None, None, :]) / (W - 1.0)
    v = (np.arange(H)[:, None, None] + np.array([0.0, 0.0, 1.0, 1.0])[None, None, :]) / (H - 1.0)
    d = (cam.lower_left_corner[None, None, None, :] + u[..., None] * cam.horizontal + v[..., None] * cam.vertical) - cam.origin
    return cam.origin, np.broadcast_to(d, (H, W, 4, 3))


def pile_pixels(flat, scene, W, H):
    """Per pixel, from f64 geometry: hits [H, W, n] -- every ray of the pixel hits sphere k (all four corner rays do: the set is convex);
    sky [H, W] -- every corner ray and hence, the pixel being far smaller than a radius, every ray stays further than 3 radii from every centre."""
    from grid_model import reference_hits
    o, d = corner_rays(camera(scene, W, H), W, H)
    c, r = flat["center"].astype(np.float64), np.abs(flat["radius"]).astype(np.float64)
    dd = d.reshape(-1, 3)
    hit = reference_hits(np.broadcast_to(o, dd.shape), dd, c, r, t_min=1e-4).reshape(H, W, 4, len(flat)).all(2)
    oc = c[None, :, :] - o[None, None, :]
    dn = dd / np.linalg.norm(dd, axis=1)[:, None]
    dist = np.linalg.norm(np.cross(oc, dn[:, None, :]), axis=2).reshape(H, W, 4, len(flat))
    sky = (dist > 3.0 * PILE_R + 0.3).all((2, 3))                      # (+ 0.3: a pixel of the 8 spp shapes is at most 0.22 wide at the pile)
    return hit, sky


def checked_scenes():
    """The scenes, with every precondition above asserted on the host; "_deep": (scene, blocks of 1 024) -> (pixels whose every ray owns more
    than 128 candidates, the pairs of one sample of each of them)."""
    import rtiow_amd as rt
    made = scenes()
    info = {}
    for scene, (grid_dim, n_global) in LAYOUTS.items():
        (G, ng), _, slot_of = rt.tile_layout_host(made[scene])
        assert (G, ng) == (grid_dim, n_global), (scene, G, ng)
        assert len(slot_of) == 32 * (ng + G * G), (scene, len(slot_of))
        info[scene] = np.asarray(slot_of)
    # ---- the pile's preconditions, before anything is rendered ----
    flat, slot_of = made["pile"], info["pile"]
    n = len(flat)
    assert n == 4 * PILE_PER_CELL + 4 and np.ptp(np.abs(flat["radius"])) == 0.0
    word_of = np.full(n, -1)
    bit_of = np.full(n, -1)
    for s, k in enumerate(slot_of):
        if k >= 0:
            word_of[k], bit_of[k] = s // 32, s % 32
    assert (word_of >= 0).all()
    assert all((slot_of[32 * wd:32 * wd + 32] >= 0).all() for wd in range(1, 5)), "each cell's tile is full: bits 0 ... 31"
    assert word_of.max() == 4                                           # the global tile and the four cells: five words, one segment
    deep = {}
    for scene, large in (("pile", False), ("pile", True), ("pile_sky", False)):
        W, H, _ = SIZES[large]
        hit, sky = pile_pixels(flat, scene, W, H)
        per_word = np.stack([(hit & (word_of == wd)[None, None, :]).sum(2) for wd in range(5)], 2)            # [H, W, word]
        ends = np.stack([hit[:, :, slot_of[32 * wd]] & hit[:, :, slot_of[32 * wd + 31]] for wd in range(1, 5)], 2)
        is_deep = (hit.sum(2) > 128) & ((per_word > 0).sum(2) >= 3) & ((per_word[:, :, 1:] >= 16) & ends).any(2)
        assert is_deep.sum() >= (4 if scene == "pile" else 0), (scene, int(is_deep.sum()))
        deep[(scene, large)] = (int(is_deep.sum()), int(hit.sum(2)[is_deep].sum()))
        if scene == "pile_sky":
            assert sky.mean() > 0.5, float(sky.mean())
            mid_word = (per_word >= 2).any(2)
            runs_sky, runs_mid = sky.reshape(H, W // 8, 8).any(2), mid_word.reshape(H, W // 8, 8).any(2)
            assert (runs_sky & runs_mid).any(), "no run of eight pixels holds a sky pixel beside one in the middle of a word"
    made["_deep"] = deep
    return made


@pytest.fixture(scope="module")
def all_scenes():
    return checked_scenes()


@pytest.fixture(scope="module")
def rendered(all_scenes, tmp_path_factory):
    """body -> the child's arrays."""
    tmp = tmp_path_factory.mktemp("scalar_trim_walk")
    in_path = str(tmp / "scenes.npz")
    np.savez(in_path, **{k: np.ascontiguousarray(v).view(np.uint8) for k, v in all_scenes.items() if not k.startswith("_")})
    got = {}
    for body in ("capped", "classic"):
        out_path = str(tmp / f"{body}.npz")
        env = dict(os.environ, RTIOW_DENSE_BODY=body)
        env.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), in_path, out_path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-3000:]
        got[body] = dict(np.load(out_path, allow_pickle=False))
    return got


@pytest.fixture(scope="module")
def wanted(all_scenes, oracle_mod):
    """name -> (Oracle B's sums, its statistics), computed once."""
    out = {}
    for name, scene, large in SHAPES:
        w, h, spp = SIZES[large]
        p = oracle_mod.make_params(w, h, spp, max_depth=DEPTH, nthreads=8, seed=SEED)
        out[name] = oracle_mod.render_b(oracle_mod.camera_from_host(camera(scene, w, h)), all_scenes[scene], p)[::2]
    return out


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_both_bodies_give_the_oracles_sums(rendered, wanted, name):
    _, scene, large = next(s for s in SHAPES if s[0] == name)
    want_fix, ost = wanted[name]
    W, H, SPP = SIZES[large]
    capped, classic = rendered["capped"], rendered["classic"]
    rays, samples, cands, roots, variant, mode, body = (int(v) for v in capped[name + "_stats"])
    rays_c, samples_c, cands_c, roots_c, variant_c, mode_c, body_c = (int(v) for v in classic[name + "_stats"])
    assert mode == 5 and body == 1 and body_c == 0
    assert np.array_equal(classic[name], capped[name]), "the two bodies differ"
    assert np.array_equal(capped[name], want_fix), "the capped body's sums differ from Oracle B's"
    assert rays == ost["rays_traced"] == rays_c and samples == W * H * SPP == samples_c
    assert (cands, roots) == (cands_c, roots_c)
    assert variant == variant_c
    assert bool(variant & 1), variant                                   # the small-grid kernel
    assert bool(variant & 4) == large, variant                          # blocks of 1 024


@pytest.mark.parametrize("scene", SCENES)
def test_the_counted_launch_agrees_and_shows_the_piles_pairs(rendered, all_scenes, scene):
    capped, classic = rendered["capped"], rendered["classic"]
    assert np.array_equal(classic[scene + "_diag"], capped[scene + "_256"]), "the counted launch gives another frame"
    assert np.array_equal(classic[scene + "_diag_stats"][:4], capped[scene + "_diag_stats"][:4])
    rays, samples, cands, roots = (int(v) for v in classic[scene + "_diag_stats"][:4])
    assert rays == int(capped[scene + "_256_stats"][0]) and cands >= roots > 0
    SPP = SIZES[False][2]
    if (scene, False) in all_scenes["_deep"]:
        n_deep, pairs = all_scenes["_deep"][(scene, False)]
        print(f"{scene}: {n_deep} pixels whose every ray owns > 128 candidates ({pairs} pairs per sample of them); counted {cands} candidates for {rays} rays")
        assert cands >= SPP * pairs, (cands, SPP * pairs)                   # the camera rays of those pixels alone
