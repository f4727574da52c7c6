"""The dense capped kernels after the cut of their shading's register copies and dead selects (rt_kernels.hpp behind `if constexpr (CAPPED)`;
DESIGN.md section 6, "the vector side"): a lane without a hit takes no default for the hit record's variables, the hit point is computed in the
origin's registers after the tries and under the mask of the lanes that scatter, the materials run for those lanes only and write the next
direction in place, the sky's colour is written into the pass's radiance, the recording path forms its bit from the lane id, and the pooled
round has no constants for the lanes without a root.  None of it may change a frame.

As in test_gpu_scalar_trim_walk.py every shape is rendered through Renderer.render_device in a child process of its own per body
(RTIOW_DENSE_BODY=capped / classic is in the environment before the library loads): at 64 x 48 x 8 spp, which runs the instantiation for blocks
of 256, and at 32 x 24 x 70 spp with RTIOW_LARGE_BLOCK_MIN_ITEMS=0, which runs the one for blocks of 1 024 (the headline's).  Depth 8 but for
lambert_deep (2 and 50).  Every frame is compared sum for sum (u64) body against body and with Oracle B; rays_traced, samples, candidates and
exact_roots of rt_stats must be equal, and rt_last_dense_body says the capped body ran.

The scenes are where the edited joins can go wrong.  Each precondition is asserted on the CPU before anything is rendered: from f64 geometry, or
from the CPU statement of a path (tests/wavefront_ref.py: camera_path, trace_ref.fast_hit, scatter_path and unit_sphere_run, the loop of
wavefront_ref.render with its events written down), walked for some pixels of the very frame that is rendered and checked against Oracle B's sums
of those pixels, so that the walk is the statement the frame follows.

* sky_only: every sphere lies behind the camera's plane, so no ray has a hit: every lane takes the path that reads none of the removed defaults.
* half_sky: a pile of spheres (materials in turn) under a sky.  Without a lens the rays of a pixel leave one point, and the (u, v) whose ray hits a
  sphere form a convex set: when the rays through the four corners of a pixel's jitter square hit one sphere, every ray of the pixel hits; when
  all four stay further from every centre than the radius plus the pixel's width at the pile, none does.  Some run of eight pixels that a wave
  starts together (64 items of 8 spp) holds a pixel of each class: hit and no-hit lanes in one wave (asserted for the 8 spp shapes; at 70 spp a
  wave starts inside one or two pixels).
* inside_glass: the camera sits inside a Dialectric sphere of ir 1.5, 0.3 from its surface: back-face hits (front == false: the flip of the
  normal), total internal reflection, reflection and refraction -- each at least once among the walked paths of each shape.
* metal_graze: Metal spheres of fuzz 1.0 in a row, seen along their tangent: scatters that are absorbed (dot(ndir, nrm) <= 0) beside kept ones.
* lambert_deep: Lambertian only, a bowl of spheres, at max_depth 2 and 50: depth exhaustion in the pass of a scatter, and parked lanes -- a
  scatter parks when its first four tries fail (0.4764^4, about 5 %): among the walked paths one scatter fails four tries and one fails eight
  (two parks in a row).
* mixed: materials in turn (arange(n) % 3) on the book camera, and the book scene itself: all three material masks live in one wave.

Every scene has more than 64 spheres, from which on the host layout builds a grid: only a scene with a grid of at most 64 tiles runs the small-grid
kernels (asserted from rt_tile_layout_host).  mixed_few, the first 30 spheres of mixed, has none and runs the large-grid capped pair, whose
shading the same cuts changed."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 1
SIZES = {False: (64, 48, 8), True: (32, 24, 70)}            # blocks of 1 024 -> (width, height, spp)
# scene -> max_depth
SCENES = {"sky_only": 8, "half_sky": 8, "inside_glass": 8, "metal_graze": 8, "lambert_deep_2": 2, "lambert_deep_50": 50, "mixed": 8, "mixed_few": 8, "book": 8}
SHAPES = [(f"{s}_{'1024' if large else '256'}", s, large) for s in SCENES for large in (False, True)]
PILE_R = 0.35
GLASS_R, GLASS_FROM = 2.0, (0.0, 0.2, 1.69)


def camera(scene, w, h):
    import rtiow_amd as rt
    a = float(w) / float(h)
    if scene == "sky_only":
        return rt.Camera((0.0, 1.0, 0.0), (0.0, 1.0, -1.0), (0.0, 1.0, 0.0), 60.0, a, 0.1, 1.0)
    if scene == "half_sky":
        return rt.Camera((0.0, 0.0, 7.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, a, 0.0, 7.0)
    if scene == "inside_glass":
        return rt.Camera(GLASS_FROM, (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), 100.0, a, 0.02, 2.0)
    if scene == "metal_graze":
        return rt.Camera((-7.0, 0.52, 0.0), (6.0, 0.45, 0.0), (0.0, 1.0, 0.0), 25.0, a, 0.0, 7.0)
    if scene.startswith("lambert_deep"):
        return rt.Camera((0.0, 2.5, 5.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 35.0, a, 0.05, 5.0)
    return rt.book1_camera(w, h)


def scenes():
    import rtiow_amd as rt
    rng = np.random.default_rng(71)

    def make(centers, radii, kind, fuzz=0.3):
        n = len(radii)
        flat = np.zeros(n, dtype=rt.SPHERE_DTYPE)
        flat["center"], flat["radius"] = centers, radii
        kind = np.asarray(kind)
        flat["kind"] = kind
        flat["albedo"] = rng.uniform(0.3, 0.9, (n, 3))
        flat["param"] = np.where(kind == 1, fuzz, np.where(kind == 2, 1.5, 0.0))
        return flat

    def fillers(n, lo, hi, keep_out=0.0, y=0.15, r=0.15):
        """n small spheres on a plane, further than keep_out from the y axis: the layout builds its grid from 65 spheres on, and only a scene with a
        grid runs the small-grid kernels."""
        c = np.zeros((0, 3))
        while len(c) < n:
            q = np.stack([rng.uniform(lo, hi, 4 * n), np.full(4 * n, y), rng.uniform(lo, hi, 4 * n)], 1)
            c = np.concatenate([c, q[np.hypot(q[:, 0], q[:, 2]) > keep_out]])[:n]
        return c, np.full(n, r)

    out = {}
    # behind the camera's plane (the camera looks down -z from (0, 1, 0))
    n = 72
    c = rng.uniform(-3.0, 3.0, (n, 3)) + (0.0, 1.0, 9.0)
    out["sky_only"] = make(c, np.full(n, 0.8), np.arange(n) % 3)
    # the pile: the lower half of the frame
    n = 100
    c = np.stack([rng.uniform(-4.0, 4.0, n), rng.uniform(-2.6, -0.3, n), rng.uniform(-0.8, 0.8, n)], 1)
    out["half_sky"] = make(c, np.full(n, PILE_R), np.arange(n) % 3)
    # the glass sphere round the camera, a ground, a Metal and a Lambertian sphere outside
    c = np.array([[0.0, 0.0, 0.0], [0.0, -103.0, 0.0], [3.5, 0.0, -3.5], [-3.5, 0.0, -3.5], [0.0, 0.5, -5.0]])
    fc, fr = fillers(70, -8.0, 8.0, keep_out=2.6, y=-2.7, r=0.3)          # on the ground round the glass sphere, clear of it
    out["inside_glass"] = make(np.concatenate([c, fc]), np.concatenate([[GLASS_R, 100.0, 1.0, 1.0, 1.2], fr]), [2, 0, 1, 0, 1] + [0, 1] * 35, fuzz=0.2)
    # Metal of fuzz 1.0 in a row along x, the camera looks along their tops; a Lambertian ground
    n = 12
    c = np.concatenate([np.stack([np.arange(n) - 4.0, np.zeros(n), rng.uniform(-0.05, 0.05, n)], 1), [[0.0, -100.5, 0.0]]])
    fc, fr = fillers(70, -9.0, 9.0, keep_out=1.5, y=-0.35, r=0.15)       # Metal too, on the ground beside the row
    out["metal_graze"] = make(np.concatenate([c, fc]), np.concatenate([np.full(n, 0.5), [100.0], fr]), [1] * n + [0] + [1] * 70, fuzz=1.0)
    # Lambertian only: a ground and a ring of spheres round a centre one (paths bounce between them)
    ang = np.arange(8) * (2.0 * math.pi / 8.0)
    c = np.concatenate([[[0.0, -100.0, 0.0], [0.0, 0.6, 0.0]], np.stack([1.5 * np.cos(ang), np.full(8, 0.5), 1.5 * np.sin(ang)], 1)])
    fc, fr = fillers(70, -4.0, 4.0, keep_out=2.2)
    deep = make(np.concatenate([c, fc]), np.concatenate([[100.0, 0.6], np.full(8, 0.5), fr]), np.zeros(80, dtype=np.int64))
    out["lambert_deep_2"] = out["lambert_deep_50"] = deep
    # materials in turn under the book camera (it looks from (13, 2, 3) at the origin)
    n = 90
    r = rng.uniform(0.3, 0.7, n)
    c = np.stack([rng.uniform(-3.0, 5.0, n), r, rng.uniform(-3.0, 3.0, n)], 1)
    c[0], r[0] = (0.0, -1000.0, 0.0), 1000.0                    # sphere 0: the ground, Lambertian
    out["mixed"] = make(c, r, np.arange(n) % 3)
    out["mixed_few"] = out["mixed"][:30].copy()                 # no grid below 65 spheres: the LARGE-grid capped pair, which the cuts changed too
    out["book"] = rt.random_scene(1).flatten()
    return out


def child(in_path, out_path):
    """Renders every shape with the body the environment names; the sums, the statistics and which body ran go to out_path."""
    import torch
    import rtiow_amd as rt
    data = np.load(in_path, allow_pickle=False)
    out = {}
    with rt.Renderer(0) as r:
        for scene, depth in SCENES.items():
            r.upload_scene(np.ascontiguousarray(data[scene].view(rt.SPHERE_DTYPE).reshape(-1)))
            for name, s, large in SHAPES:
                if s != scene:
                    continue
                if large:
                    os.environ["RTIOW_LARGE_BLOCK_MIN_ITEMS"] = "0"         # (read per launch)
                else:
                    os.environ.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
                w, h, spp = SIZES[large]
                d_fix = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                r.render_device(camera(scene, w, h), rt.make_params(w, h, spp, max_depth=depth, seed=SEED), d_fix.data_ptr())
                torch.cuda.synchronize()
                st = r.last_stats()
                out[name] = d_fix.cpu().numpy().view(np.uint64)
                out[name + "_stats"] = np.array([st["rays_traced"], st["samples"], st["candidates"], st["exact_roots"], st["kernel_variant"],
                                                 st["scan_mode"], r._lib.rt_last_dense_body(r._h)], dtype=np.int64)
            os.environ.pop("RTIOW_LARGE_BLOCK_MIN_ITEMS", None)
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child(sys.argv[1], sys.argv[2])
    sys.exit(0)

pytestmark = pytest.mark.gpu


# ---- the CPU statement of a path, with its events written down ------------------------------------------------------------------------------

def walk(flat, ocam, W, H, spp, depth, pixels, oracle_mod):
    """The loop of wavefront_ref.render for the given pixels -> (events, {pixel: [3] sums}).  events counts: sky (a ray without a hit), back (a
    hit from inside), tir / refract / reflect (the Dialectric's three ways), absorbed / kept (Metal), exhausted (max_depth rays traced and the
    last one scattered), failed4 / failed8 (a Lambertian or Metal scatter whose first four / eight tries fail: one park / two in a row)."""
    import wavefront_ref as ref
    from trace_ref import Scene, fast_hit
    lib = oracle_mod.load()
    scene = Scene(flat)
    ev = dict.fromkeys(("sky", "back", "tir", "refract", "reflect", "absorbed", "kept", "exhausted", "failed4", "failed8", "scatters"), 0)
    sums = {}
    for pixel in pixels:
        acc = [0, 0, 0]
        for s in range(spp):
            o, d, event, _ = ref.camera_path(ocam, W, H, SEED, pixel, s)
            thr = [1.0, 1.0, 1.0]
            for bounce in range(depth):
                idx, _, p, nrm, front = fast_hit(scene, o, d, 1e-4)
                if idx < 0:
                    ev["sky"] += 1
                    v = ref.sky_sample(thr, d)
                    for c in range(3):
                        acc[c] += int(lib.oracle_b_quantize(float(v[c])))
                    break
                ev["back"] += 0 if front else 1
                r = ref.scatter_path(scene.flat[idx], SEED, d, p, nrm, front, pixel, s, event)
                ev["scatters"] += 1
                kind = int(scene.flat[idx]["kind"])
                if kind == ref.DIALECTRIC:
                    ev[r["mode"]] += 1
                else:
                    ev["failed4"] += r["tries"] > 4
                    ev["failed8"] += r["tries"] > 8
                if kind == ref.METAL:
                    ev["absorbed" if r["status"] != ref.SCATTERED else "kept"] += 1
                if r["status"] != ref.SCATTERED:
                    break
                thr = [thr[c] * r["attenuation"][c] for c in range(3)]
                o, d, event = p, r["out_dir"], r["event"]
                ev["exhausted"] += bounce == depth - 1
        sums[pixel] = [a & ref.MASK64 for a in acc]
    return ev, sums


def corner_rays(cam, W, H):
    """-> origin (3,), directions [H, W, 4, 3]: camera.rs:47-54 without a lens for the four corners of every pixel's jitter square."""
    u = (np.arange(W)[None, :, None] + np.array([0.0, 1.0, 0.0, 1.0])[None, None, :]) / (W - 1.0)
    v = (np.arange(H)[:, None, None] + np.array([0.0, 0.0, 1.0, 1.0])[None, None, :]) / (H - 1.0)
    d = (cam.lower_left_corner[None, None, None, :] + u[..., None] * cam.horizontal + v[..., None] * cam.vertical) - cam.origin
    return cam.origin, np.broadcast_to(d, (H, W, 4, 3))


def pile_pixels(flat, cam, W, H):
    """-> (hit [H, W]: the four corner rays hit one and the same sphere, hence every ray of the pixel does; sky [H, W]: every corner ray stays
    further from every centre than the radius plus the pixel's width at the far side of the pile, hence no ray of the pixel has a hit)."""
    o, d = corner_rays(cam, W, H)
    c, r = flat["center"].astype(np.float64), np.abs(flat["radius"]).astype(np.float64)
    dn = d / np.linalg.norm(d, axis=-1)[..., None]
    oc = c[None, None, None, :, :] - o                                                              # [1, 1, 1, n, 3]
    along = (oc * dn[:, :, :, None, :]).sum(-1)                                                     # [H, W, 4, n]
    dist = np.sqrt(np.maximum((oc * oc).sum(-1) - along * along, 0.0))
    hits = (dist < r * (1.0 - 1e-9)) & (along > 0.0)
    hit = hits.all(2).any(2)
    far = float(np.linalg.norm(c - o, axis=1).max() + r.max())
    width = far * float(np.linalg.norm(cam.horizontal / (W - 1.0) + cam.vertical / (H - 1.0)) / np.linalg.norm(d, axis=-1).min())
    sky = (dist > r + width).all((2, 3))
    return hit, sky


# which pixels of a frame the statement is walked for (rows through the middle of the picture), and how many samples of each
def walked_pixels(W, H, rows, step=1):
    return [j * W + i for j in rows for i in range(0, W, step)]


def checked_scenes(oracle_mod):
    """The scenes with every precondition asserted; "_walks": name -> (the pixels walked, their sums by the statement)."""
    import rtiow_amd as rt
    made = scenes()
    walks = {}
    # ---- every scene has a grid of at most 64 tiles with its global ones: the small-grid kernels run it (rt_launch.hpp, small_grid_scene)
    for scene, flat in made.items():
        (G, ng), _, _ = rt.tile_layout_host(flat)
        assert (G == 0) if scene == "mixed_few" else (G > 0 and ng + G * G <= 64), (scene, G, ng)
    # ---- sky_only: behind the camera's plane, radius and all (a ray leaves the lens towards -w; the lens is 0.05 wide, the margin 3)
    for large in (False, True):
        W, H, _ = SIZES[large]
        cam = camera("sky_only", W, H)
        f = made["sky_only"]
        assert ((f["center"] - cam.origin) @ (-cam.w) + np.abs(f["radius"]) < -3.0).all()
    # ---- half_sky
    for large in (False, True):
        W, H, _ = SIZES[large]
        hit, sky = pile_pixels(made["half_sky"], camera("half_sky", W, H), W, H)
        assert sky.mean() > 0.4 and hit.mean() > 0.1, (float(sky.mean()), float(hit.mean()))
        if not large:
            runs_hit, runs_sky = hit.reshape(H, W // 8, 8).any(2), sky.reshape(H, W // 8, 8).any(2)
            assert (runs_hit & runs_sky).sum() >= 4, "no run of eight pixels holds a pixel that always hits beside one that never does"
    # ---- the walked statements
    plan = {  # scene -> (rows as fractions of the height, pixel step, samples at 8 spp / at 70 spp, what must have occurred)
        "inside_glass": ((0.5,), 2, (8, 4), ("back", "tir", "refract", "reflect")),
        "metal_graze": ((0.4, 0.5), 2, (8, 4), ("absorbed", "kept")),
        "lambert_deep_2": ((0.3, 0.5, 0.7), 1, (8, 16), ("failed4", "failed8", "exhausted")),
        "lambert_deep_50": ((0.4,), 2, (8, 8), ("failed4", "failed8", "sky")),
        "mixed": ((0.45,), 4, (8, 4), ("refract", "kept", "failed4", "sky")),
    }
    for scene, (rows, step, nsamp, needs) in plan.items():
        for large in (False, True):
            W, H, spp = SIZES[large]
            ocam = oracle_mod.camera_from_host(camera(scene, W, H))
            pixels = walked_pixels(W, H, [int(f * H) for f in rows], step)
            n = min(spp, nsamp[large])
            ev, sums = walk(made[scene], ocam, W, H, n, SCENES[scene], pixels, oracle_mod)
            print(f"{scene} {W}x{H}: {len(pixels)} pixels x {n} samples walked: {ev}")
            for what in needs:
                assert ev[what] >= 1, (scene, W, H, what, ev)
            walks[(scene, large)] = (pixels, n, sums)
    made["_walks"] = walks
    return made


@pytest.fixture(scope="module")
def all_scenes(oracle_mod):
    return checked_scenes(oracle_mod)


@pytest.fixture(scope="module")
def rendered(all_scenes, tmp_path_factory):
    """body -> the child's arrays."""
    tmp = tmp_path_factory.mktemp("vector_trim")
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
        p = oracle_mod.make_params(w, h, spp, max_depth=SCENES[scene], nthreads=8, seed=SEED)
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
    assert bool(variant & 1) == (scene != "mixed_few"), variant         # the small-grid kernel
    if scene != "mixed_few":                                            # (without a grid the launch plan keeps blocks of 256 at these sizes)
        assert bool(variant & 4) == large, variant                      # blocks of 1 024
    if scene == "sky_only":
        assert rays == W * H * SPP                                      # one ray per sample: nothing was hit


@pytest.mark.parametrize("scene", ["inside_glass", "metal_graze", "lambert_deep_2", "lambert_deep_50", "mixed"])
def test_the_walked_statement_is_the_frames(all_scenes, oracle_mod, scene):
    """The paths whose events the preconditions count are paths of the rendered frame: Oracle B, restricted to the walked samples, gives the walk's sums."""
    for large in (False, True):
        W, H, _ = SIZES[large]
        pixels, n, sums = all_scenes["_walks"][(scene, large)]
        p = oracle_mod.make_params(W, H, n, max_depth=SCENES[scene], nthreads=8, seed=SEED)
        fix = oracle_mod.render_b(oracle_mod.camera_from_host(camera(scene, W, H)), all_scenes[scene], p)[0].reshape(-1, 3)
        for px in pixels:
            assert [int(v) for v in fix[px]] == [int(v) for v in sums[px]], (scene, W, H, px)
