"""The dense capped kernels after the second cut of their scalar stream (rt_kernels.hpp behind `if constexpr (CAPPED)`; DESIGN.md section 6,
"the scalar port"): a segment zeroes all fourteen bitmap rows without a loop, the summary reads them two at a time, and the bookkeeping of
finished samples runs on wave masks.  Every frame must stay what it was.

As in test_gpu_scalar_trim.py every case is rendered through Renderer.render_device twice, each time in a child process of its own whose
environment names the body (RTIOW_DENSE_BODY=capped / classic is there before the library loads), and compared sum for sum (u64) with Oracle B
and body against body; rays_traced and samples are the oracle's; rt_last_dense_body says that the capped body ran.

* the headline instantiation itself at a small shape: the book scene, seed 1, 96 x 54 x 70 with RTIOW_LARGE_BLOCK_MIN_ITEMS=0 (kernel_variant
  bits 0 and 2: small grid, blocks of 1 024), and the same frame without that variable (blocks of 256: the second small-grid capped instantiation);
* segment boundaries -- stale bits in rows a segment does not use are what unconditional zeroing and a paired summary could get wrong.  448, 449
  and 900 spheres of radius 1.5 ... 2.5 over 12 x 12: too large for a cell of any grid finer than 1 x 1, so the host takes the grid of ONE cell,
  whose tile holds 32 of them, and makes global tiles of the rest: 13, 14 and 28 global tiles (the host caps them at 48) plus the cell tile.  A wave
  whose rays reach the cell scans 14 tiles (one full segment), 15 (a second segment of one word behind 14 used rows) and 29 (14 + 14 + 1); a wave
  of rays that all miss the grid's box scans 13, 14 and 28 (an odd count, a full segment, two full segments).  The counts are asserted on the host
  layout before anything is rendered;
* one word: ten spheres, nine of them in one spot (no grid: one tile that every group scans; the large-grid kernel on blocks of 256) -- also at
  70 spp with RTIOW_LARGE_BLOCK_MIN_ITEMS=0, the shape the issue names, which stays on blocks of 256 (the large-grid kernel takes blocks of
  1 024 from 147 spp on), and at 147 spp, which does reach the large-grid capped instantiation on blocks of 1 024 (kernel_variant bit 2);
* list entries with one group: the three clusters of test_gpu_scalar_trim.py;
* a walk with long per-lane lists: 60 spheres of radius 0.12 within ~0.3 of one point (a ray through the heap passes within a radius of a
  dozen of them), twelve more far out so that the scene has a grid, seen from 1.7 away at 64 x 36 x 20: the 64 rays of a wave carry several
  hundred candidates together, so pooled rounds fire inside the walk's trips and the ring of 128 pairs wraps within one pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (scene, camera, width, height, spp, seed, RTIOW_LARGE_BLOCK_MIN_ITEMS=0 in the child for this render)
SHAPES = [("headline_1024", "book", "book", 96, 54, 70, 1, True), ("headline_256", "book", "book", 96, 54, 70, 1, False),
          ("tiles_14", "tiles_14", "book", 64, 36, 8, 1, False), ("tiles_15", "tiles_15", "book", 64, 36, 8, 1, False),
          ("tiles_29", "tiles_29", "book", 64, 36, 8, 1, False),
          ("ten_20", "ten", "book", 64, 36, 20, 1, False), ("ten_70", "ten", "book", 64, 36, 70, 1, True), ("ten_147", "ten", "book", 32, 18, 147, 1, True),
          ("clusters", "clusters", "book", 64, 36, 20, 1, False),
          ("heap", "heap", "close", 64, 36, 20, 1, False)]
# scene -> (grid cells per side, global tiles) of the host layout
LAYOUTS = {"tiles_14": (1, 13), "tiles_15": (1, 14), "tiles_29": (1, 28), "ten": (0, 0), "heap": (1, 2)}
HEAP_AT = (2.0, 0.3, 2.0)


def camera(name, w, h):
    import rtiow_amd as rt
    if name == "book":
        return rt.book1_camera(w, h)
    at = np.array(HEAP_AT)
    return rt.Camera(at + (1.2, 0.2, 1.2), at, (0.0, 1.0, 0.0), 40.0, float(w) / float(h), 0.0, 1.7)


def scenes(book):
    import rtiow_amd as rt
    rng = np.random.default_rng(47)

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

    ten = make(np.concatenate([rng.uniform(-0.6, 0.6, (9, 3)) * (1, 0, 1) + (0, 0.3, 0), [[3.0, 0.3, -2.0]]]), np.full(10, 0.3))
    corners = [(-3.0, 0.2, -3.0), (3.0, 0.2, -3.0), (-3.0, 0.2, 3.0)]
    c = np.concatenate([rng.normal(p, 0.4, (22, 3)) * (1, 0, 1) + (0, 0.2, 0) for p in corners] + [[[2.9, 0.2, 2.9], [0.1, 0.2, -0.1]]])
    clusters = make(c, np.full(len(c), 0.2))
    far = np.array([(x, 0.12, z) for x in (-4.0, -1.0, 4.0) for z in (-4.0, -1.5, 1.0, 4.0)])
    heap = make(np.concatenate([rng.normal(HEAP_AT, 0.15, (60, 3)), far]), np.full(72, 0.12))
    return {"book": book, "tiles_14": tiles(448), "tiles_15": tiles(449), "tiles_29": tiles(900), "ten": ten, "clusters": clusters, "heap": heap}


def child(in_path, out_path):
    """Renders every shape with the body the environment names; the sums, the statistics and which body ran go to out_path."""
    import torch
    import rtiow_amd as rt
    data = np.load(in_path, allow_pickle=False)
    out = {}
    with rt.Renderer(0) as r:
        loaded = None
        for name, scene, cam, w, h, spp, seed, large in SHAPES:
            if loaded != scene:
                r.upload_scene(np.ascontiguousarray(data[scene].view(rt.SPHERE_DTYPE).reshape(-1)))
                loaded = scene
            if large:
                os.environ["RTIOW_LARGE_BLOCK_MIN_ITEMS"] = "0"         # (read per launch)
            else:
                os.environ.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
            d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            r.render_device(camera(cam, w, h), rt.make_params(w, h, spp, seed=seed), d_fix.data_ptr())
            torch.cuda.synchronize()
            st = r.last_stats()
            out[name] = d_fix.cpu().numpy().view(np.uint64)
            out[name + "_stats"] = np.array([st["rays_traced"], st["samples"], st["kernel_variant"], st["scan_mode"],
                                             r._lib.rt_last_dense_body(r._h)], dtype=np.int64)
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child(sys.argv[1], sys.argv[2])
    sys.exit(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def all_scenes(book1_flat):
    import rtiow_amd as rt
    made = scenes(book1_flat)
    # the tile counts the cases rely on, from the host layout (tests/test_grid_layout.py), before anything is rendered
    for scene, (grid_dim, n_global) in LAYOUTS.items():
        (G, ng), _, slot_of = rt.tile_layout_host(made[scene])
        assert (G, ng) == (grid_dim, n_global), (scene, G, ng)
        assert len(slot_of) == (32 * (ng + G * G) if G else 32 * ((len(made[scene]) + 31) // 32)), (scene, len(slot_of))
    return made


@pytest.fixture(scope="module")
def rendered(all_scenes, tmp_path_factory):
    """body -> the child's arrays."""
    tmp = tmp_path_factory.mktemp("scalar_trim_segments")
    in_path = str(tmp / "scenes.npz")
    np.savez(in_path, **{k: np.ascontiguousarray(v).view(np.uint8) for k, v in all_scenes.items()})
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
    """name -> (Oracle B's sums, its statistics), computed once (the two headline shapes are one frame: one oracle render)."""
    out, by_frame = {}, {}
    for name, scene, cam, w, h, spp, seed, _ in SHAPES:
        key = (scene, cam, w, h, spp, seed)
        if key not in by_frame:
            fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(camera(cam, w, h)), all_scenes[scene],
                                              oracle_mod.make_params(w, h, spp, nthreads=8, seed=seed))
            by_frame[key] = (fix, ost)
        out[name] = by_frame[key]
    return out


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_both_bodies_give_the_oracles_sums(rendered, wanted, name):
    _, scene, cam, w, h, spp, seed, large = next(s for s in SHAPES if s[0] == name)
    want_fix, ost = wanted[name]
    capped, classic = rendered["capped"], rendered["classic"]
    rays, samples, variant, mode, body = (int(v) for v in capped[name + "_stats"])
    rays_c, samples_c, variant_c, mode_c, body_c = (int(v) for v in classic[name + "_stats"])
    assert body == (1 if mode == 5 else 0) and body_c == 0                    # (a context under RTIOW_SCAN_MODE=1 has no capped body)
    assert np.array_equal(capped[name], want_fix), "the capped body's sums differ from Oracle B's"
    assert np.array_equal(classic[name], capped[name]), "the two bodies differ"
    assert rays == ost["rays_traced"] == rays_c and samples == w * h * spp == samples_c
    assert variant == variant_c
    if mode == 5:
        small_grid = scene != "ten"                                               # (ten spheres: no tile grid, the large-grid kernel scans every tile)
        assert bool(variant & 1) == small_grid, variant
        assert bool(variant & 4) == (name in ("headline_1024", "ten_147")), variant   # blocks of 1 024


def test_the_two_headline_shapes_are_one_frame(rendered):
    assert np.array_equal(rendered["capped"]["headline_1024"], rendered["capped"]["headline_256"])
