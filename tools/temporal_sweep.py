#!/usr/bin/env python3
"""The parameter sweep behind make_temporal's defaults: RMSE of the LAST frame of a short turntable after temporal
accumulation against a high-spp reference of that frame, one parameter varied at a time around the defaults, with the library's CPU
statement of the filter (rt_temporal_host).

The case: random_scene(1), the first 6 cameras of orbit_cameras(N, 96, 54) (default N = 180: 2 degrees per step), depth 50; 4 spp per
frame, sample_stride 4 (every frame a random stream of its own), seed 1; features at 4 spp with each frame's sample_begin; reference
512 spp of the last camera with seed 7.  Metric: sqrt(mean((clip(x, 0, 1) - clip(ref, 0, 1))^2)) over all channels of the linear means.

  tools/temporal_sweep.py --save-inputs FILE.npz [--oracle]   renders the inputs and stores their exact sums: on an MI355X, or with
                                                              --oracle from Oracle B and the CPU feature reference (minutes, no GPU)
  tools/temporal_sweep.py --inputs FILE.npz                   the sweep, on the CPU
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rtiow_amd as rt  # noqa: E402

W, H, SPP, FRAMES, REF_SPP = 96, 54, 4, 6, 512


def value(q):
    q = np.asarray(q, dtype=np.uint64)
    return ((q >> np.uint64(32)).astype(np.float64) * 4294967296.0 + (q & np.uint64(0xFFFFFFFF)).astype(np.float64)) * (1.0 / 4294967296.0)


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(x, 0.0, 1.0) - np.clip(ref, 0.0, 1.0)) ** 2)))


def render_inputs(n_orbit):
    flat = rt.random_scene(1).flatten()
    cams = rt.orbit_cameras(n_orbit, W, H)[:FRAMES]
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        fix, _ = r.render_frames(cams, rt.make_params(W, H, SPP, seed=1, max_depth=50), SPP)
        feat = np.stack([r.render_features(cams[f], rt.make_params(W, H, SPP, sample_begin=f * SPP, seed=1), want_ids=False)[0] for f in range(FRAMES)])
        _, ref, _ = r.render(cams[-1], rt.make_params(W, H, REF_SPP, seed=7, max_depth=50))
    return fix, feat, ref


def oracle_inputs(n_orbit):
    """The same sums from the CPU oracle (tests/features_ref.py restates the feature kernel; the parity tests hold the GPU to both)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import features_ref as fr
    import oracle
    flat = rt.random_scene(1).flatten()
    cams = rt.orbit_cameras(n_orbit, W, H)[:FRAMES]
    fix, feat = [], []
    for f, cam in enumerate(cams):
        ocam = oracle.camera_from_host(cam)
        fix.append(oracle.render_b(ocam, flat, oracle.make_params(W, H, SPP, sample_begin=f * SPP, seed=1, max_depth=50))[0])
        feat.append(fr.render_features(ocam, flat, W, H, SPP, sample_begin=f * SPP, seed=1)[0])
    ref = oracle.render_b(oracle.camera_from_host(cams[-1]), flat, oracle.make_params(W, H, REF_SPP, seed=7, max_depth=50))[0]
    return np.stack(fix), np.stack(feat), ref


def chain(fix, feat, cams, tp):
    """-> (the last accumulated frame, per step the share of hit pixels that found valid history)"""
    history, found = None, []
    for f in range(len(cams)):
        acc, length = rt.temporal_host(fix[f], SPP, feat[f], SPP, cams[f], history, tp)
        history = (acc, length, feat[f], SPP, cams[f])
        if f:
            hit = feat[f][..., 7] != 0
            found.append(float((length[hit] >= 2).mean()))
    return acc, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save-inputs", default=None)
    ap.add_argument("--inputs", default=None)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--orbit", type=int, default=180, help="cameras per turn: the step is 360 / N degrees")
    a = ap.parse_args()
    if a.inputs:
        z = np.load(a.inputs, allow_pickle=False)
        fix, feat, ref, n_orbit = z["fix"], z["feat"], z["ref"], int(z["orbit"])
    else:
        n_orbit = a.orbit
        fix, feat, ref = oracle_inputs(n_orbit) if a.oracle else render_inputs(n_orbit)
    if a.save_inputs:
        np.savez_compressed(a.save_inputs, fix=fix, feat=feat, ref=ref, orbit=n_orbit)
        print(f"{W}x{H}: {FRAMES} frames of {SPP} spp, step {360.0 / n_orbit:g} degrees, features of {SPP} spp, reference of {REF_SPP} spp -> {a.save_inputs}")
        return
    cams = rt.orbit_cameras(n_orbit, W, H)[:FRAMES]
    ref_mean = value(ref) / REF_SPP
    noisy = rmse(value(fix[-1]) / SPP, ref_mean)
    print(f"# {W}x{H}, frame {FRAMES - 1} of an orbit of {360.0 / n_orbit:g} degrees per step, {SPP} spp against {REF_SPP} spp: noisy {noisy:.5f}")
    print("# alpha_min sigma_normal sigma_depth clamp clamp_scale   rmse    rmse / noisy   hit pixels with history, per step")
    base = dict(alpha_min=0.1, sigma_normal=0.5, sigma_depth=0.1, clamp=True, clamp_scale=1.0)
    rows = [dict(base)]
    rows += [dict(base, alpha_min=x) for x in (0.05, 0.2, 0.3, 0.5, 1.0)]
    rows += [dict(base, sigma_normal=x) for x in (0.1, 0.25, 1.0, 1e6)]
    rows += [dict(base, sigma_depth=x) for x in (0.01, 0.03, 0.3, 1e6)]
    rows += [dict(base, clamp=False)] + [dict(base, clamp_scale=x) for x in (0.0, 0.5, 0.75, 1.5, 2.0, 4.0)]
    for o in rows:
        acc, found = chain(fix, feat, cams, rt.make_temporal(**o))
        e = rmse(value(acc), ref_mean)
        print(f"  {o['alpha_min']:<9g} {o['sigma_normal']:<12g} {o['sigma_depth']:<11g} {str(o['clamp']):<5} {o['clamp_scale']:<11g}  {e:.5f}  {e / noisy:.3f}"
              f"          {' '.join(f'{100 * x:.0f}%' for x in found)}", flush=True)


if __name__ == "__main__":
    main()
