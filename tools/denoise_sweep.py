#!/usr/bin/env python3
"""The parameter sweep behind make_denoise's defaults: RMSE of the denoised 8-spp book frame against a
1024-spp reference, over levels and the three sigmas, with the library's CPU statement of the filter (rt_denoise_host).

The case: random_scene(1), book1_camera(240, 135), depth 50; 8 spp with seed 1; features at 8 spp with seed 1; reference 1024 spp
with seed 7.  Metric: sqrt(mean((clip(x, 0, 1) - clip(ref, 0, 1))^2)) over all channels of the linear means.

  tools/denoise_sweep.py --save-inputs FILE.npz     renders the three inputs (needs an MI355X) and stores their exact sums
  tools/denoise_sweep.py --inputs FILE.npz          the sweep, on the CPU
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rtiow_amd as rt  # noqa: E402

W, H, SPP, REF_SPP = 240, 135, 8, 1024


def value(q):
    q = np.asarray(q, dtype=np.uint64)
    return ((q >> np.uint64(32)).astype(np.float64) * 4294967296.0 + (q & np.uint64(0xFFFFFFFF)).astype(np.float64)) * (1.0 / 4294967296.0)


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(x, 0.0, 1.0) - np.clip(ref, 0.0, 1.0)) ** 2)))


def render_inputs():
    flat = rt.random_scene(1).flatten()
    cam = rt.book1_camera(W, H)
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        _, fix, _ = r.render(cam, rt.make_params(W, H, SPP, seed=1, max_depth=50))
        feat, _, _ = r.render_features(cam, rt.make_params(W, H, SPP, seed=1), want_ids=False)
        _, ref, _ = r.render(cam, rt.make_params(W, H, REF_SPP, seed=7, max_depth=50))
    return fix, feat, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save-inputs", default=None)
    ap.add_argument("--inputs", default=None)
    a = ap.parse_args()
    if a.save_inputs:
        fix, feat, ref = render_inputs()
        np.savez_compressed(a.save_inputs, fix=fix, feat=feat, ref=ref)
        print(f"{W}x{H}: sums of {SPP} spp, features of {SPP} spp, reference of {REF_SPP} spp -> {a.save_inputs}")
        return
    if a.inputs:
        z = np.load(a.inputs, allow_pickle=False)
        fix, feat, ref = z["fix"], z["feat"], z["ref"]
    else:
        fix, feat, ref = render_inputs()
    ref_mean = value(ref) / REF_SPP
    noisy = rmse(value(fix) / SPP, ref_mean)
    print(f"# {W}x{H}, {SPP} spp against {REF_SPP} spp: noisy {noisy:.5f}")

    def run(levels, sc, sn, sd, demodulate=True):
        out = rt.denoise_host(fix, SPP, feat, SPP, rt.make_denoise(levels, sc, sn, sd, demodulate))
        return rmse(value(out), ref_mean)

    print("# levels sigma_color sigma_normal sigma_depth demodulate   rmse    rmse / noisy")
    rows = [(4, 0.35, 1.0, 0.2, True)]
    rows += [(lv, 0.35, 1.0, 0.2, True) for lv in (1, 2, 3, 5, 6)]
    rows += [(4, sc, 1.0, 0.2, True) for sc in (0.1, 0.2, 0.25, 0.5, 0.7, 1.0, 1e6)]
    rows += [(4, 0.35, sn, 0.2, True) for sn in (0.25, 0.5, 2.0, 1e6)]
    rows += [(4, 0.35, 1.0, sd, True) for sd in (0.05, 0.1, 0.4, 1.0, 1e6)]
    rows += [(4, 0.35, 1.0, 0.2, False), (3, 1e6, 1.0, 0.2, True), (5, 1e6, 1.0, 0.2, True)]
    for lv, sc, sn, sd, dm in rows:
        e = run(lv, sc, sn, sd, dm)
        print(f"  {lv}      {sc:<10g} {sn:<12g} {sd:<11g} {str(dm):<10}  {e:.5f}  {e / noisy:.3f}", flush=True)


if __name__ == "__main__":
    main()
