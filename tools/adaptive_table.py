"""What adaptive sampling buys: 1200x675 on the book scene, cap 512, step 16, for three thresholds -- samples rendered, wall time of
rt_render_adaptive (host clock; the call ends in a synchronise) against one dense 512-spp launch, the share of that time outside the
render kernels (selection, add-back, the one-word read-backs, the copies out), and the RMSE of the resolved frame against a dense
4096-spp frame, beside the RMSE of dense frames of 64 / 128 / 256 / 512 spp against the same: which uniform sample count each
threshold matches, and what it cost.  RMSE over the 8-bit R, G, B of Color::to_rgba, in units of one byte step.
usage: python tools/adaptive_table.py [--step N] [threshold ...]      (default: step 16, thresholds 0.02 0.01 0.005)"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rtiow_amd as rt

ARGS = sys.argv[1:]
STEP = int(ARGS.pop(ARGS.index("--step") + 1)) if "--step" in ARGS else 16
THRESHOLDS = [float(a) for a in ARGS if a != "--step"] or [0.02, 0.01, 0.005]
W, H, CAP, FLOOR, REF_SPP = 1200, 675, 512, 0.01, 4096
r = rt.Renderer(0)
r.upload_scene(rt.random_scene(1).flatten())
cam = rt.book1_camera(W, H)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


ref_fix = np.zeros((H, W, 3), dtype=np.uint64)
for k in range(REF_SPP // 512):                                   # other samples than the frames under test use: sample_begin from 100 000
    ref_fix += r.render(cam, rt.make_params(W, H, 512, sample_begin=100000 + 512 * k, seed=1))[1]
ref = r.resolve_rgba8(ref_fix, REF_SPP)
print(f"{W}x{H}, book scene, cap {CAP}, step {STEP}, dark_floor {FLOOR}; reference: dense {REF_SPP} spp (other samples)")
dense_wall = {}
for spp in (64, 128, 256, 512):
    p = rt.make_params(W, H, spp, seed=1)
    r.render(cam, p)
    walls, kms = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        _, fix, st = r.render(cam, p)
        walls.append((time.perf_counter() - t0) * 1e3)
        kms.append(st["kernel_ms"])
    dense_wall[spp] = statistics.median(walls)
    print(f"dense {spp:4d} spp: {W * H * spp / 1e6:8.1f} Msamples  wall {dense_wall[spp]:8.2f} ms (kernel {statistics.median(kms):8.2f})  "
          f"RMSE {rmse(r.resolve_rgba8(fix, spp), ref):6.3f}")
for thr in THRESHOLDS:
    a = rt.make_adaptive(STEP, thr, FLOOR)
    p = rt.make_params(W, H, CAP, seed=1)
    r.render_adaptive(cam, p, a, want_half=False)
    walls, kms = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        fix, _, count, st = r.render_adaptive(cam, p, a, want_half=False)
        walls.append((time.perf_counter() - t0) * 1e3)
        kms.append(st["kernel_ms"])
    wall, km = statistics.median(walls), statistics.median(kms)
    img = r.resolve_rgba8_counts(fix, count)
    print(f"adaptive threshold {thr:g}: {st['samples'] / 1e6:8.1f} Msamples ({count.mean():6.1f} per pixel, {100 * (count == CAP).mean():4.1f} % at the cap, "
          f"{100 * (count == 2 * STEP).mean():4.1f} % at {2 * STEP})  wall {wall:8.2f} ms = {wall / dense_wall[512]:5.3f} x dense 512  "
          f"outside render kernels {100 * (wall - km) / wall:4.1f} %  RMSE {rmse(img, ref):6.3f}")
