"""What a pixel list costs: 1200x675x100 on the book scene through rt_render_pixels_device -- the identity list, every second pixel, a
random 10 % in ascending order and the same 10 % shuffled (coherence lost on purpose) -- against the dense rt_render_device of the same
library.  Kernel time from the library's HIP events (rt_last_stats), warmed, N launches each, alternated; medians.
usage: python tools/pixel_list_cost.py [launches]"""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import rtiow_amd as rt

N = int(sys.argv[1]) if len(sys.argv) > 1 else 12
W, H, SPP = 1200, 675, 100
r = rt.Renderer(0)
r.upload_scene(rt.random_scene(1).flatten())
cam = rt.book1_camera(W, H)
p = rt.make_params(W, H, SPP, seed=1)
rng = np.random.default_rng(1)
tenth = np.sort(rng.choice(W * H, size=W * H // 10, replace=False)).astype(np.uint32)
lists = {"identity list": np.arange(W * H, dtype=np.uint32), "every second pixel": np.arange(0, W * H, 2, dtype=np.uint32),
         "random 10 %, ascending": tenth, "random 10 %, shuffled": rng.permutation(tenth).astype(np.uint32)}
d_lists = {k: torch.from_numpy(v.view(np.int32).copy()).cuda() for k, v in lists.items()}
d_fix = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda")
stream = torch.cuda.current_stream().cuda_stream


def run(name):
    if name == "dense rt_render_device":
        r.render_device(cam, p, d_fix.data_ptr(), stream)
    else:
        r.render_pixels_device(cam, p, d_lists[name].data_ptr(), len(lists[name]), d_fix.data_ptr(), stream)
    st = r.last_stats()
    return st["kernel_ms"], st["samples"]


names = ["dense rt_render_device"] + list(lists)
times, samples = {k: [] for k in names}, {}
r.render_device(cam, p, d_fix.data_ptr(), stream)
torch.cuda.synchronize()
dense_fix = d_fix.cpu().numpy().copy()
for k in names:                                                   # warm-up, and the lists' sums are the dense frame's
    run(k)
    torch.cuda.synchronize()
    if k in lists:
        assert np.array_equal(d_fix.cpu().numpy().reshape(-1, 3)[:len(lists[k])], dense_fix.reshape(-1, 3)[lists[k]]), k
for _ in range(N):
    for k in names:
        ms, n = run(k)
        times[k].append(ms)
        samples[k] = n
base = statistics.median(times[names[0]]) / samples[names[0]]
print(f"{W}x{H}x{SPP}, book scene, {N} launches each, alternated; kernel ms from HIP events")
for k in names:
    med = statistics.median(times[k])
    print(f"{k:26s} {samples[k]:>10d} samples  median {med:8.3f} ms  min {min(times[k]):8.3f}  {samples[k] / med / 1e6:7.3f} Gsample/s  "
          f"time per sample = {med / samples[k] / base:6.4f} x dense")
