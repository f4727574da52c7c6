#!/usr/bin/env python3
"""The sweep behind render_sequence_var's default sigma_color: RMSE of the last frame of a night sequence against a
1024-spp reference, with the library's CPU statements (rt_temporal_var_host, rt_denoise_var_given_host) on sums the GPU rendered.

  The scene is section 25's night scene: random_scene(1), a black sky, sphere 528 radiating (4, 3.2, 2.4), weighted direct lighting through
  the device path queue, depth 16.  The geometry is section 16's: 96 x 54, the first 6 cameras of orbit_cameras(180) (2 degrees per step).
  Every frame has 8 spp with sample_stride 8 (seed 1) and guides at 8 spp with the frame's sample_begin; the last frame is also kept as 2 x 4
  (its half sums).  The reference is 1024 spp of the last camera with seed 7.
Metric: sqrt(mean((clip(x, 0, 1) - clip(ref, 0, 1))^2)) over all channels of the linear means.  Four figures -- noisy, accumulated only
(rt_temporal_var's out_fix), the last frame alone through rt_denoise_var, accumulated then rt_denoise_var_given -- and the last one per
swept sigma_color.  The shipped default is the swept sigma_color with the lowest final-frame RMSE.

  tools/temporal_var_sweep.py --save-inputs FILE.npz     renders the inputs (needs an MI355X) and stores their exact sums
  tools/temporal_var_sweep.py --inputs FILE.npz          the sweep, on the CPU
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rtiow_amd as rt  # noqa: E402

W, H, FRAMES, SPP, FEAT_SPP, REF_SPP = 96, 54, 6, 8, 8, 1024
LIGHT, EMISSION, DEPTH = 528, (4, 3.2, 2.4), 16
SIGMAS = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 1e6)


def value(q):
    q = np.asarray(q, dtype=np.uint64)
    return ((q >> np.uint64(32)).astype(np.float64) * 4294967296.0 + (q & np.uint64(0xFFFFFFFF)).astype(np.float64)) * (1.0 / 4294967296.0)


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(x, 0.0, 1.0) - np.clip(ref, 0.0, 1.0)) ** 2)))


def render_inputs():
    flat = rt.random_scene(1).flatten()
    cams = rt.orbit_cameras(180, W, H)[:FRAMES]
    kw = dict(lighting=rt.Lighting((0, 0, 0), (0, 0, 0), {LIGHT: EMISSION}), direct=True, sampling="weighted")
    z = {}
    with rt.Renderer(0) as r:
        r.upload_scene(flat)
        for f, cam in enumerate(cams):
            z[f"fix{f}"] = r.render_wavefront(cam, rt.make_params(W, H, SPP, sample_begin=f * SPP, seed=1, max_depth=DEPTH), **kw)[0]
            z[f"feat{f}"] = r.render_features(cam, rt.make_params(W, H, FEAT_SPP, sample_begin=f * SPP, seed=1), want_ids=False)[0]
        begin = (FRAMES - 1) * SPP
        z["half"] = r.render_wavefront_pixels(cams[-1], rt.make_params(W, H, SPP // 2, sample_begin=begin, seed=1, max_depth=DEPTH), **kw)[0]
        both = r.render_wavefront_pixels(cams[-1], rt.make_params(W, H, SPP // 2, sample_begin=begin + SPP // 2, seed=1, max_depth=DEPTH),
                                         into=z["half"].copy(), **kw)[0]
        assert np.array_equal(both, z[f"fix{FRAMES - 1}"])                  # two accumulated passes are the frame's one pass
        z["ref"] = r.render_wavefront(cams[-1], rt.make_params(W, H, REF_SPP, seed=7, max_depth=DEPTH), **kw)[0]
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save-inputs", default=None)
    ap.add_argument("--inputs", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.save_inputs:
        np.savez_compressed(a.save_inputs, **render_inputs())
        print(f"{W}x{H}: {FRAMES} night frames of {SPP} spp, features of {FEAT_SPP} spp, a reference of {REF_SPP} spp -> {a.save_inputs}")
        return
    z = np.load(a.inputs, allow_pickle=False) if a.inputs else render_inputs()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    cams = rt.orbit_cameras(180, W, H)[:FRAMES]
    ref = value(z["ref"]) / REF_SPP
    history = None
    for f, cam in enumerate(cams):
        acc, length, m2, var = rt.temporal_var_host(z[f"fix{f}"], SPP, z[f"feat{f}"], FEAT_SPP, cam, history)
        history = (acc, length, z[f"feat{f}"], FEAT_SPP, cam, m2)
    last, feat = z[f"fix{FRAMES - 1}"], z[f"feat{FRAMES - 1}"]
    noisy, accumulated = rmse(value(last) / SPP, ref), rmse(value(acc), ref)
    single = rmse(value(rt.denoise_var_host(last, z["half"], SPP, feat, FEAT_SPP, rt.make_denoise_var())), ref)
    absolute = rmse(value(rt.denoise_host(acc, 1, feat, FEAT_SPP, rt.make_denoise())), ref)
    hit = feat[..., 7] != 0
    out(f"# {W}x{H}, {FRAMES} night frames of {SPP} spp, 2 degrees per step, against {REF_SPP} spp; default rt_temporal options")
    out(f"# last frame: {100 * float((length[hit] >= 2).mean()):.1f} % of the hit pixels with history, {100 * float((length[hit] >= 4).mean()):.1f} % "
        f"at length >= {rt.RT_TEMPORAL_VAR_MIN_LEN} (the temporal variance)")
    out(f"# noisy {noisy:.5f}   accumulated only {accumulated:.5f} (ratio to noisy {accumulated / noisy:.4f})")
    out(f"# the last frame alone through rt_denoise_var (2 x {SPP // 2}, its default) {single:.5f} (ratio to noisy {single / noisy:.4f})")
    out(f"# accumulated then rt_denoise at its default (--temporal --denoise) {absolute:.5f} (ratio to accumulated {absolute / accumulated:.4f})")
    out("# accumulated then rt_denoise_var_given, 4 levels, sigma_normal 1, sigma_depth 0.2, demodulated:")
    out("#   sigma_color   RMSE      / accumulated   / noisy   / single frame")
    best = None
    for sc in SIGMAS:
        e = rmse(value(rt.denoise_var_given_host(acc, var, 1, feat, FEAT_SPP, rt.make_denoise_var(4, sc))), ref)
        best = (e, sc) if best is None or e < best[0] else best
        out(f"    {sc:<12g} {e:.5f}   {e / accumulated:.4f}          {e / noisy:.4f}    {e / single:.4f}")
    out(f"# lowest final-frame RMSE: sigma_color = {best[1]:g} ({best[0]:.5f}, {best[0] / accumulated:.4f} of accumulated only)")
    sc = best[1]
    out("# around it, one parameter at a time:  levels sigma_normal sigma_depth demodulate   RMSE   / accumulated")
    rows = [(lv, 1.0, 0.2, True) for lv in (1, 2, 3, 5)] + [(4, sn, 0.2, True) for sn in (0.5, 2.0)] + [(4, 1.0, sd, True) for sd in (0.1, 0.4)]
    rows += [(4, 1.0, 0.2, False)]
    for lv, sn, sd, dm in rows:
        e = rmse(value(rt.denoise_var_given_host(acc, var, 1, feat, FEAT_SPP, rt.make_denoise_var(lv, sc, sn, sd, dm))), ref)
        out(f"    {lv}      {sn:<12g} {sd:<11g} {str(dm):<10}  {e:.5f}  {e / accumulated:.4f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
