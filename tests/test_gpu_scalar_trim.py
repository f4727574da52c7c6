"""The dense kernels with the trimmed scalar stream (rt_dense.hip; DESIGN.md section 6, "the scalar port"): the capped body reads its Philox
round keys from a device table instead of rebuilding them, and every frame must stay what it was.

Every case is rendered through Renderer.render_device twice, each time in a child process of its own whose environment names the body
(RTIOW_DENSE_BODY=capped / classic is there before the library loads), and compared sum for sum (u64) with Oracle B -- the oracle of
the parity tests -- and body against body; rays_traced and samples are the oracle's.

* the book scene, seed 1, 96 x 54 at 70, 20 and 5 samples per pixel, depth 50: the small-grid kernel (kernel_variant bit 0) on blocks of
  256 with the ring of 2 x 16 pixel sums, then smaller blocks; 5 spp is the ring's lower edge.  Tiles with one to four reachable groups,
  glass, metal and parked lanes all occur;
* three further keys at 64 x 36 x 20 -- seeds 7, 123 456 789 and one with a high word, so that k1 and its Weyl sequence are not those
  of 0: a wrong round key or a wrong table shows as a different frame; the last launch returns to the first key, so the table of a
  launch slot is rewritten for a new key and again for an old one;
* ten spheres, nine of them in one spot (no tile grid: one tile that every group scans), twelve spheres of radius >= 1.5 (as the
  book scene's global tiles: nothing but 0xF entries), and 68 small spheres in three clusters at three corners of a 2 x 2 grid with
  one cell empty (a 16-ray group mostly reaches one cell: list entries with one group)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIGH_SEED = 0x9E3779B97F4A7C15

# name -> (scene, width, height, spp, seed)
SHAPES = [("book_70", "book", 96, 54, 70, 1), ("book_20", "book", 96, 54, 20, 1), ("book_5", "book", 96, 54, 5, 1),
          ("seed_7", "book", 64, 36, 20, 7), ("seed_123456789", "book", 64, 36, 20, 123456789), ("seed_high", "book", 64, 36, 20, HIGH_SEED),
          ("seed_1_again", "book", 64, 36, 20, 1),
          ("ten", "ten", 64, 36, 20, 1), ("globals", "globals", 64, 36, 20, 1), ("clusters", "clusters", 64, 36, 20, 1)]


def scenes(book):
    import rtiow_amd as rt
    rng = np.random.default_rng(31)

    def make(centers, radii):
        n = len(radii)
        flat = np.zeros(n, dtype=rt.SPHERE_DTYPE)
        flat["center"], flat["radius"] = centers, radii
        kind = np.arange(n) % 3                                 # Lambertian, Metal, Dialectric in turn
        flat["kind"] = kind
        flat["albedo"] = rng.uniform(0.3, 0.9, (n, 3))
        flat["param"] = np.where(kind == 1, 0.3, np.where(kind == 2, 1.5, 0.0))
        return flat

    ten = make(np.concatenate([rng.uniform(-0.6, 0.6, (9, 3)) * (1, 0, 1) + (0, 0.3, 0), [[3.0, 0.3, -2.0]]]), np.full(10, 0.3))
    globs = make(rng.uniform(-6, 6, (12, 3)) * (1, 0, 1) + (0, 1.5, 0), rng.uniform(1.5, 2.5, 12))
    corners = [(-3.0, 0.2, -3.0), (3.0, 0.2, -3.0), (-3.0, 0.2, 3.0)]
    c = np.concatenate([rng.normal(p, 0.4, (22, 3)) * (1, 0, 1) + (0, 0.2, 0) for p in corners] + [[[2.9, 0.2, 2.9], [0.1, 0.2, -0.1]]])
    clusters = make(c, np.full(len(c), 0.2))
    return {"book": book, "ten": ten, "globals": globs, "clusters": clusters}


def child(in_path, out_path):
    """Renders every shape with the body the environment names; the sums, the statistics and which body ran go to out_path."""
    import torch
    import rtiow_amd as rt
    data = np.load(in_path, allow_pickle=False)
    out = {}
    with rt.Renderer(0) as r:
        loaded = None
        for name, scene, w, h, spp, seed in SHAPES:
            if loaded != scene:
                r.upload_scene(np.ascontiguousarray(data[scene].view(rt.SPHERE_DTYPE).reshape(-1)))
                loaded = scene
            d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            r.render_device(rt.book1_camera(w, h), rt.make_params(w, h, spp, seed=seed), d_fix.data_ptr())
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
    return scenes(book1_flat)


@pytest.fixture(scope="module")
def rendered(all_scenes, tmp_path_factory):
    """body -> the child's arrays."""
    tmp = tmp_path_factory.mktemp("scalar_trim")
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
    """name -> (Oracle B's sums, its statistics), computed once."""
    import rtiow_amd as rt
    out = {}
    for name, scene, w, h, spp, seed in SHAPES:
        fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(rt.book1_camera(w, h)), all_scenes[scene],
                                          oracle_mod.make_params(w, h, spp, nthreads=8, seed=seed))
        out[name] = (fix, ost)
    return out


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_both_bodies_give_the_oracles_sums(rendered, wanted, name):
    _, scene, w, h, spp, seed = next(s for s in SHAPES if s[0] == name)
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
        if scene == "book":
            assert variant & 1, variant                                           # the small-grid kernel
            assert not variant & 4                                                # ... on blocks of 256 or less
        if scene in ("ten", "globals"):
            assert not variant & 1, variant                                       # no tile grid: the large-grid kernel scans every tile
