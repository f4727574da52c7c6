#!/usr/bin/env python3
"""The sweep behind make_denoise_var's default sigma_color: RMSE of the variance-guided denoiser against a
1024-spp reference on two frames at 240 x 135, one parameter at a time, with the library's CPU statement of the filter
(rt_denoise_var_host) on sums the GPU rendered; beside it the noisy frame and rt_denoise at its default.

  (a) the daylight frame of tools/denoise_sweep.py: random_scene(1), book1_camera, depth 50, 8 spp (seed 1) rendered as 2 x 4;
  (b) the same scene at night: a black sky, sphere 528 radiating (4, 3.2, 2.4), weighted direct lighting through the device path queue,
      depth 16, 16 spp (seed 1) rendered as 2 x 8.
Both: features at 8 spp (seed 1); the reference 1024 spp with seed 7 at the frame's own depth and lighting.
Metric: sqrt(mean((clip(x, 0, 1) - clip(ref, 0, 1))^2)) over all channels of the linear means.  The shipped default is the swept
sigma_color with the lowest SUM of the two frames' ratios to noisy.

  tools/denoise_var_sweep.py --save-inputs FILE.npz     renders the inputs (needs an MI355X) and stores their exact sums
  tools/denoise_var_sweep.py --inputs FILE.npz          the sweep, on the CPU
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rtiow_amd as rt  # noqa: E402

W, H, REF_SPP, FEAT_SPP = 240, 135, 1024, 8
SPP = {"a": 8, "b": 16}
LIGHT, EMISSION, NIGHT_DEPTH = 528, (4, 3.2, 2.4), 16
SIGMAS = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 1e6)


def value(q):
    q = np.asarray(q, dtype=np.uint64)
    return ((q >> np.uint64(32)).astype(np.float64) * 4294967296.0 + (q & np.uint64(0xFFFFFFFF)).astype(np.float64)) * (1.0 / 4294967296.0)


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(x, 0.0, 1.0) - np.clip(ref, 0.0, 1.0)) ** 2)))


def render_inputs():
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    z = {}
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        z["feat"] = r.render_features(cam, rt.make_params(W, H, FEAT_SPP, seed=1), want_ids=False)[0]
        n = SPP["a"]
        z["a_half"] = r.render(cam, rt.make_params(W, H, n // 2, seed=1, max_depth=50))[1]
        z["a_fix"] = z["a_half"] + r.render(cam, rt.make_params(W, H, n // 2, seed=1, max_depth=50, sample_begin=n // 2))[1]
        assert np.array_equal(z["a_fix"], r.render(cam, rt.make_params(W, H, n, seed=1, max_depth=50))[1])
        z["a_ref"] = r.render(cam, rt.make_params(W, H, REF_SPP, seed=7, max_depth=50))[1]
        kw = dict(lighting=rt.Lighting((0, 0, 0), (0, 0, 0), {LIGHT: EMISSION}), direct=True, sampling="weighted")
        n = SPP["b"]
        z["b_half"] = r.render_wavefront_pixels(cam, rt.make_params(W, H, n // 2, seed=1, max_depth=NIGHT_DEPTH), **kw)[0]
        z["b_fix"] = r.render_wavefront_pixels(cam, rt.make_params(W, H, n // 2, seed=1, max_depth=NIGHT_DEPTH, sample_begin=n // 2), into=z["b_half"], **kw)[0]
        z["b_ref"] = r.render_wavefront(cam, rt.make_params(W, H, REF_SPP, seed=7, max_depth=NIGHT_DEPTH), **kw)[0]
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save-inputs", default=None)
    ap.add_argument("--inputs", default=None)
    a = ap.parse_args()
    if a.save_inputs:
        np.savez_compressed(a.save_inputs, **render_inputs())
        print(f"{W}x{H}: frames (a) and (b), features of {FEAT_SPP} spp, references of {REF_SPP} spp -> {a.save_inputs}")
        return
    z = np.load(a.inputs, allow_pickle=False) if a.inputs else render_inputs()
    feat = z["feat"]
    frames = {}
    for k in ("a", "b"):
        ref = value(z[k + "_ref"]) / REF_SPP
        frames[k] = (z[k + "_fix"], z[k + "_half"], SPP[k], ref, rmse(value(z[k + "_fix"]) / SPP[k], ref))

    def run(k, levels, sc, sn, sd, demodulate=True):
        fix, half, spp, ref, noisy = frames[k]
        out = rt.denoise_var_host(fix, half, spp, feat, FEAT_SPP, rt.make_denoise_var(levels, sc, sn, sd, demodulate))
        return rmse(value(out), ref) / noisy

    print(f"# {W}x{H} against {REF_SPP} spp; (a) daylight {SPP['a']} spp as 2 x {SPP['a'] // 2}, (b) night {SPP['b']} spp as 2 x {SPP['b'] // 2}")
    for k in ("a", "b"):
        fix, half, spp, ref, noisy = frames[k]
        plain = rmse(value(rt.denoise_host(fix, spp, feat, FEAT_SPP, rt.make_denoise())), ref)
        print(f"# ({k}) noisy {noisy:.5f}   rt_denoise at its default {plain:.5f} (ratio to noisy {plain / noisy:.3f})")
    print("# rt_denoise_var, ratios to noisy:  levels sigma_color sigma_normal sigma_depth demodulate   (a)     (b)     sum")
    rows = [(4, sc, 1.0, 0.2, True) for sc in SIGMAS]
    best = None
    for lv, sc, sn, sd, dm in rows:
        ra, rb = run("a", lv, sc, sn, sd, dm), run("b", lv, sc, sn, sd, dm)
        best = (ra + rb, sc) if best is None or ra + rb < best[0] else best
        print(f"  {lv}      {sc:<10g} {sn:<12g} {sd:<11g} {str(dm):<10}  {ra:.3f}   {rb:.3f}   {ra + rb:.3f}", flush=True)
    sc = best[1]
    print(f"# lowest sum of ratios: sigma_color = {sc:g}; around it, one parameter at a time")
    rows = [(lv, sc, 1.0, 0.2, True) for lv in (1, 2, 3, 5, 6)]
    rows += [(4, sc, sn, 0.2, True) for sn in (0.5, 2.0, 1e6)]
    rows += [(4, sc, 1.0, sd, True) for sd in (0.1, 0.4, 1e6)]
    rows += [(4, sc, 1.0, 0.2, False)]
    for lv, s, sn, sd, dm in rows:
        ra, rb = run("a", lv, s, sn, sd, dm), run("b", lv, s, sn, sd, dm)
        print(f"  {lv}      {s:<10g} {sn:<12g} {sd:<11g} {str(dm):<10}  {ra:.3f}   {rb:.3f}   {ra + rb:.3f}", flush=True)


if __name__ == "__main__":
    main()
