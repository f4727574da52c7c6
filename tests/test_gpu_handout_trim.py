"""The dense capped kernels after the hand-out's cut (rt_kernels.hpp behind `if constexpr (kMaskHandout)`; DESIGN.md section 6, "the top of
the pass"): lanes without a path take the queue's entries on wave masks -- a first take of what the queue holds, then refill-and-take trips --
no lane is marked dead any more (a wave whose counter says "no block left" skips the hand-out), and the lanes that start a camera ray are the
takers' mask.  Which lane takes which entry decides the pixel, the sample and the Philox counters of every path, so every frame must stay what it was.

As in test_gpu_scalar_trim_segments.py every case is rendered through Renderer.render_device twice, each time in a child process of its own
whose environment names the body (RTIOW_DENSE_BODY=capped / classic is there before the library loads), and compared sum for sum (u64) with
Oracle B and body against body; rays_traced and samples are the oracle's; rt_last_dense_body says that the capped body ran.  All cases are the
book scene, seed 1 (the small-grid pair of kernels: the two instantiations that hand out on masks in every launch):

* the headline instantiation at a small shape: 96 x 54 x 70 with RTIOW_LARGE_BLOCK_MIN_ITEMS=0 (blocks of 1 024), and without it (blocks of 256);
* a short last block: 7 x 5 x 70 = 2 450 items -- two blocks of 1 024 and one of 402, whose last refill brings 18 entries: more takers than
  entries, most of the grid's waves get no block at all, and lanes run out of work while their neighbours go on -- and the same on blocks of 256;
* one lone wave: 3 x 2 x 9 = 54 items, fewer than a wave has lanes: the first refill cannot serve every taker;
* low sample counts, 64 x 36 at 1, 3 and 17 samples per pixel: a block spans many pixels; 1 and 3 add every sample to the frame buffer directly,
  17 keeps block sums in LDS;
* depth 1, 64 x 36 x 20: every lane finishes in every pass, so every pass takes 64 entries: the queue drains exactly and the next pass starts on
  an empty queue (the first take is skipped, the refill trip serves everybody);
* sky only: the camera looks up from above the scene; no ray hits anything, every lane finishes in every pass at full depth;
* cameras: aperture 0 (every lens sample maps to the origin), a wide aperture, a tilted vup."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (camera, width, height, spp, max_depth, RTIOW_LARGE_BLOCK_MIN_ITEMS=0 in the child for this render)
SHAPES = [("headline_1024", "book", 96, 54, 70, 50, True), ("headline_256", "book", 96, 54, 70, 50, False),
          ("short_last_1024", "book", 7, 5, 70, 50, True), ("short_last_256", "book", 7, 5, 70, 50, False),
          ("lone_wave", "book", 3, 2, 9, 50, False),
          ("spp_1", "book", 64, 36, 1, 50, False), ("spp_3", "book", 64, 36, 3, 50, False), ("spp_17", "book", 64, 36, 17, 50, False),
          ("depth_1", "book", 64, 36, 20, 1, False),
          ("sky_only", "up", 64, 36, 20, 50, False),
          ("aperture_0", "pinhole", 64, 36, 20, 50, False), ("aperture_wide", "wide", 64, 36, 20, 50, False),
          ("tilted_vup", "tilted", 64, 36, 20, 50, False)]
SEED = 1


def camera(name, w, h):
    import rtiow_amd as rt
    aspect = float(w) / float(h)
    if name == "book":
        return rt.book1_camera(w, h)
    if name == "up":                        # from above the spheres straight up: sky in every pixel
        return rt.Camera((0.0, 30.0, 0.0), (0.0, 60.0, 0.0), (0.0, 0.0, 1.0), 40.0, aspect, 0.1, 10.0)
    if name == "pinhole":
        return rt.Camera((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, aspect, 0.0, 10.0)
    if name == "wide":
        return rt.Camera((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, aspect, 2.0, 10.0)
    assert name == "tilted"
    return rt.Camera((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.3, 1.0, 0.2), 20.0, aspect, 0.1, 10.0)


def child(in_path, out_path):
    """Renders every shape with the body the environment names; the sums, the statistics and which body ran go to out_path."""
    import torch
    import rtiow_amd as rt
    flat = np.ascontiguousarray(np.load(in_path, allow_pickle=False).view(rt.SPHERE_DTYPE).reshape(-1))
    out = {}
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        for name, cam, w, h, spp, depth, large in SHAPES:
            if large:
                os.environ["RTIOW_LARGE_BLOCK_MIN_ITEMS"] = "0"         # (read per launch)
            else:
                os.environ.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
            d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            r.render_device(camera(cam, w, h), rt.make_params(w, h, spp, seed=SEED, max_depth=depth), d_fix.data_ptr())
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
def rendered(book1_flat, tmp_path_factory):
    """body -> the child's arrays."""
    tmp = tmp_path_factory.mktemp("handout_trim")
    in_path = str(tmp / "scene.npy")
    np.save(in_path, np.ascontiguousarray(book1_flat).view(np.uint8))
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
def wanted(book1_flat, oracle_mod):
    """name -> (Oracle B's sums, its statistics), computed once (shapes that differ in the block size only are one frame: one oracle render)."""
    out, by_frame = {}, {}
    for name, cam, w, h, spp, depth, _ in SHAPES:
        key = (cam, w, h, spp, depth)
        if key not in by_frame:
            fix, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(camera(cam, w, h)), book1_flat,
                                              oracle_mod.make_params(w, h, spp, nthreads=8, seed=SEED, max_depth=depth))
            by_frame[key] = (fix, ost)
        out[name] = by_frame[key]
    return out


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_both_bodies_give_the_oracles_sums(rendered, wanted, name):
    _, cam, w, h, spp, depth, large = next(s for s in SHAPES if s[0] == name)
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
        assert variant & 1, variant                                           # the book scene: the small-grid kernels
        assert bool(variant & 4) == large, variant                            # blocks of 1 024


def test_the_block_size_does_not_change_the_frame(rendered):
    assert np.array_equal(rendered["capped"]["headline_1024"], rendered["capped"]["headline_256"])
    assert np.array_equal(rendered["capped"]["short_last_1024"], rendered["capped"]["short_last_256"])


def test_sky_only_traces_one_ray_per_sample(rendered):
    rays, samples = (int(v) for v in rendered["capped"]["sky_only_stats"][:2])
    assert rays == samples == 64 * 36 * 20
