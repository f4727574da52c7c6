"""The dense capped kernels with lane-striped block sums (rt_kernels.hpp behind `if constexpr (kStriped)`): at many samples per
pixel a work block touches at most S <= 8 of the ring's 16 pixel slots, the refill gives every sample one of R = 16 / S replicas of its pixel's slot,
the per-pass adds go to the replica and the block's write-out folds the replicas into the pixel.  The sums are integer sums, so every frame must stay
what it was -- at every number of replicas, at the sample counts where that number changes, and where it is 1 and no address may move.

As in test_gpu_handout_trim.py every case is rendered through Renderer.render_device twice, each time in a child process of its own whose environment
names the body (RTIOW_DENSE_BODY=capped / classic is there before the library loads), and compared sum for sum (u64) with Oracle B and body against
body; rays_traced and samples are the oracle's; rt_last_dense_body says that the capped body ran.  All cases are the book scene, seed 1.  The sample
counts at which the number of replicas changes are read from the plan's own table (tests/stripe_plan.py: rt_host::plan_stripes, compiled for the host):

* blocks of 1 024 (RTIOW_LARGE_BLOCK_MIN_ITEMS=0), 8 x 4: the smallest spp with four replicas, one less (two), the smallest with two, one less (one);
* blocks of 256, 8 x 4: the same four boundaries;
* 7 x 5 x 500 on blocks of 1 024: a short last block, and blocks that straddle two and three pixels beside refills inside one pixel;
* depth 1 with four replicas: every lane finishes in every pass -- the worst contention -- and the queue drains exactly;
* sky only with four replicas;
* a sharded launch (shard 1 of 3, tiles of 2 rows) with four replicas: the shard's rows are not the image's;
* 96 x 54 x 70 on blocks of 1 024, the headline-shaped case of the earlier cuts: one replica, nothing moves."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1


def shapes(table):
    """name -> (camera, width, height, spp, max_depth, blocks of 1 024, (shard_index, shard_count, tile_rows) or None, replicas the plan gives)."""
    import stripe_plan
    out = {}
    for items, large in ((1024, True), (256, False)):
        r4, r2 = stripe_plan.first_spp(table, items, 4), stripe_plan.first_spp(table, items, 2)
        for tag, spp in (("r4_first", r4), ("r4_below", r4 - 1), ("r2_first", r2), ("r2_below", r2 - 1)):
            out[f"{tag}_{items}"] = ("book", 8, 4, spp, 50, large, None, table[(items, spp, 1, 1)][1])
    r4 = stripe_plan.first_spp(table, 1024, 4)
    out["short_last_500"] = ("book", 7, 5, 500, 50, True, None, table[(1024, 500, 1, 1)][1])
    out["depth_1_r4"] = ("book", 8, 4, r4, 1, True, None, 4)
    out["sky_only_r4"] = ("up", 8, 4, r4, 50, True, None, 4)
    out["sharded_r4"] = ("book", 8, 12, r4, 50, True, (1, 3, 2), 4)
    out["headline_1024"] = ("book", 96, 54, 70, 50, True, None, table[(1024, 70, 1, 1)][1])
    return out


def camera(name, w, h):
    import rtiow_amd as rt
    if name == "book":
        return rt.book1_camera(w, h)
    assert name == "up"                     # from above the spheres straight up: sky in every pixel
    return rt.Camera((0.0, 30.0, 0.0), (0.0, 60.0, 0.0), (0.0, 0.0, 1.0), 40.0, float(w) / float(h), 0.1, 10.0)


def shard_image_rows(h, shard):
    """Image rows of a shard's compact rows, in order (tiles of tile_rows rows dealt round robin)."""
    if shard is None:
        return list(range(h))
    index, count, tile_rows = shard
    return [j for j in range(h) if (j // tile_rows) % count == index]


def child(in_path, out_path):
    """Renders every shape with the body the environment names; the sums, the statistics and which body ran go to out_path."""
    import torch
    import rtiow_amd as rt
    import stripe_plan
    flat = np.ascontiguousarray(np.load(in_path, allow_pickle=False).view(rt.SPHERE_DTYPE).reshape(-1))
    with tempfile.TemporaryDirectory() as tmp:
        cases = shapes(stripe_plan.stripe_table(tmp))
    out = {}
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        for name, (cam, w, h, spp, depth, large, shard, _) in cases.items():
            if large:
                os.environ["RTIOW_LARGE_BLOCK_MIN_ITEMS"] = "0"         # (read per launch)
            else:
                os.environ.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
            rows = len(shard_image_rows(h, shard))
            d_fix = torch.zeros((rows, w, 3), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            kw = {} if shard is None else dict(shard_index=shard[0], shard_count=shard[1], tile_rows=shard[2])
            r.render_device(camera(cam, w, h), rt.make_params(w, h, spp, seed=SEED, max_depth=depth, **kw), d_fix.data_ptr())
            torch.cuda.synchronize()
            st = r.last_stats()
            out[name] = d_fix.cpu().numpy().view(np.uint64)
            out[name + "_stats"] = np.array([st["rays_traced"], st["samples"], st["kernel_variant"], st["scan_mode"],
                                             r._lib.rt_last_dense_body(r._h)], dtype=np.int64)
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    child(sys.argv[1], sys.argv[2])
    sys.exit(0)

import stripe_plan  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = [f"{tag}_{items}" for items in (1024, 256) for tag in ("r4_first", "r4_below", "r2_first", "r2_below")] + [
    "short_last_500", "depth_1_r4", "sky_only_r4", "sharded_r4", "headline_1024"]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    got = shapes(stripe_plan.stripe_table(tmp_path_factory.mktemp("stripe_plan")))
    assert list(got) == NAMES
    return got


@pytest.fixture(scope="module")
def rendered(book1_flat, tmp_path_factory):
    """body -> the child's arrays."""
    tmp = tmp_path_factory.mktemp("striped_sums")
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
def wanted(cases, book1_flat, oracle_mod):
    """name -> (Oracle B's sums for the rows the launch renders, its statistics or None for a shard), one oracle render per frame."""
    out, by_frame = {}, {}
    for name, (cam, w, h, spp, depth, _, shard, _) in cases.items():
        key = (cam, w, h, spp, depth)
        if key not in by_frame:
            by_frame[key] = oracle_mod.render_b(oracle_mod.camera_from_host(camera(cam, w, h)), book1_flat,
                                                oracle_mod.make_params(w, h, spp, nthreads=8, seed=SEED, max_depth=depth))
        fix, _, ost = by_frame[key]
        out[name] = (np.asarray(fix)[shard_image_rows(h, shard)], ost if shard is None else None)
    return out


def test_the_cases_sit_on_the_plans_boundaries(cases):
    """The table's thresholds are what the cases were built from: 4 / 2 / 2 / 1 replicas round each pair of boundaries, 4 in the high-spp cases, 1 at 70 spp."""
    for items in (1024, 256):
        assert [cases[f"{tag}_{items}"][7] for tag in ("r4_first", "r4_below", "r2_first", "r2_below")] == [4, 2, 2, 1]
    assert cases["short_last_500"][7] == 4 and cases["headline_1024"][7] == 1


@pytest.mark.parametrize("name", NAMES)
def test_both_bodies_give_the_oracles_sums(cases, rendered, wanted, name):
    cam, w, h, spp, depth, large, shard, _ = cases[name]
    want_fix, ost = wanted[name]
    capped, classic = rendered["capped"], rendered["classic"]
    rays, samples, variant, mode, body = (int(v) for v in capped[name + "_stats"])
    rays_c, samples_c, variant_c, mode_c, body_c = (int(v) for v in classic[name + "_stats"])
    assert body == (1 if mode == 5 else 0) and body_c == 0                    # (a context under RTIOW_SCAN_MODE=1 has no capped body)
    assert np.array_equal(capped[name], want_fix), "the capped body's sums differ from Oracle B's"
    assert np.array_equal(classic[name], capped[name]), "the two bodies differ"
    assert rays == rays_c and samples == want_fix.shape[0] * w * spp == samples_c
    if ost is not None:
        assert rays == ost["rays_traced"]
    assert variant == variant_c
    if mode == 5:
        assert variant & 1, variant                                           # the book scene: the small-grid kernels
        assert bool(variant & 4) == large, variant                            # blocks of 1 024


def test_depth_1_and_sky_only_trace_one_ray_per_sample(cases, rendered):
    for name in ("depth_1_r4", "sky_only_r4"):
        _, w, h, spp = cases[name][:4]
        rays, samples = (int(v) for v in rendered["capped"][name + "_stats"][:2])
        assert rays == samples == w * h * spp
