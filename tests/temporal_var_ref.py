"""The contract of temporal accumulation with second moments and of the variance-guided denoiser fed by a given variance
(include/rtiow_hip.h "temporal accumulation with second moments") in numpy -- a test helper, written from the text of
the contract and not from the C++.  What the contract takes over word for word (the constants, the guides, the colour, quantize, the
levels of the filter) is temporal_ref's, denoise_ref's and denoise_var_ref's; steps 3-7 are stated here once more because the moments ride
through them, and the test holds out_fix and out_len to rt_temporal's own arrays.

Every step is an elementwise numpy operation on float64 arrays (numpy does not fuse a product into a sum; no np.dot, no sum): the four
taps are gathered and added one after the other in the stated order, and the 3 x 3 walk visits its pixels dy outer, dx inner.
"""
import numpy as np

import denoise_ref as dr
import denoise_var_ref as vr
import features_ref as fr
import temporal_ref as tr

MIN_LEN = 4                                                           # RT_TEMPORAL_VAR_MIN_LEN
SIGMA_COLOR = 1.5                                                     # the shipped default of the sequence (rtiow_amd.render.TEMPORAL_VAR_SIGMA_COLOR)


def clip0(x):
    return np.where(x > 0.0, x, 0.0)


def neighbourhood(c):
    """The 3 x 3 walk of the current frame, dy outer, dx inner, the centre in its place -> (lo, hi, vs): the clamp's box (from the centre's
    colour; the centre's own visit changes nothing) and the spatial variance."""
    h_, w_ = c.shape[0], c.shape[1]
    lo, hi = c.copy(), c.copy()
    a1, a2 = np.zeros_like(c), np.zeros_like(c)
    cnt = np.zeros((h_, w_, 1), dtype=np.float64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if abs(dy) >= h_ or abs(dx) >= w_:
                continue
            dst_j, src_j = slice(max(0, -dy), min(h_, h_ - dy)), slice(max(0, dy), min(h_, h_ + dy))
            dst_i, src_i = slice(max(0, -dx), min(w_, w_ - dx)), slice(max(0, dx), min(w_, w_ + dx))
            cq = c[src_j, src_i]
            a1[dst_j, dst_i] = a1[dst_j, dst_i] + cq
            a2[dst_j, dst_i] = a2[dst_j, dst_i] + cq * cq
            cnt[dst_j, dst_i] = cnt[dst_j, dst_i] + 1.0
            lo[dst_j, dst_i] = np.where(cq < lo[dst_j, dst_i], cq, lo[dst_j, dst_i])
            hi[dst_j, dst_i] = np.where(cq > hi[dst_j, dst_i], cq, hi[dst_j, dst_i])
    mu = a1 / cnt
    return lo, hi, clip0(a2 / cnt - mu * mu)


def accumulate(fix, spp, feat, feat_spp, cam, history=None, *, alpha_min=0.1, sigma_normal=0.5, sigma_depth=0.1, clamp=True, clamp_scale=1.0,
               count=None):
    """-> (out_fix u64 [H,W,3], out_len u32 [H,W], out_m2 f64 [H,W,3], out_var f64 [H,W,3]).
    history: None or (prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam, prev_m2)."""
    with np.errstate(all="ignore"):
        c = tr.colour(fix, spp, count)
        h_, w_ = c.shape[0], c.shape[1]
        hits, n, z = tr.guides(feat, feat_spp)
        lo, hi, vs = neighbourhood(c)
        s2 = c * c
        # no history: m2 = s2, at = 1.0, len = 1 (< MIN_LEN: the spatial estimate)
        out0, len0, m20, var0 = tr.quantize(c), np.ones((h_, w_), dtype=np.uint32), s2, vs * 1.0
        if history is None:
            return out0, len0, m20, var0
        prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam, prev_m2 = history
        prev_len = np.asarray(prev_len, dtype=np.uint32)
        prev_m2 = np.asarray(prev_m2, dtype=np.float64)
        co, cl, ch_, cv = tr.cam_vectors(cam)
        po, pl, Hh, Vv = tr.cam_vectors(prev_cam)
        L = tuple(pl[k] - po[k] for k in range(3))
        nrm = tr.cross(Hh, Vv)
        iLn = np.float64(1.0) / np.float64(tr.dot(L, nrm))
        LH, LV = tr.dot(L, Hh), tr.dot(L, Vv)
        iHH, iVV = np.float64(1.0) / np.float64(tr.dot(Hh, Hh)), np.float64(1.0) / np.float64(tr.dot(Vv, Vv))
        wm1, hm1 = float(w_ - 1), float(h_ - 1)
        sz2 = float(sigma_depth) * float(sigma_depth)
        inn = 1.0 / (float(sigma_normal) * float(sigma_normal))
        # 3. the world point
        jj, ii = np.mgrid[0:h_, 0:w_]
        u = (ii.astype(np.float64) + 0.5) / wm1
        v = (jj.astype(np.float64) + 0.5) / hm1
        e = []
        for k in range(3):
            d = ((cl[k] + u * ch_[k]) + v * cv[k]) - co[k]
            P = co[k] + z * d
            e.append(P - po[k])
        # 4. into the previous image
        s = tr.dot(e, nrm) * iLn
        have = (hits != 0) & (s > 0.0)
        inv_s = 1.0 / s
        up = (tr.dot(e, Hh) * inv_s - LH) * iHH
        vp = (tr.dot(e, Vv) * inv_s - LV) * iVV
        fx = up * wm1 - 0.5
        fy = vp * hm1 - 0.5
        have &= (fx >= -1.0) & (fx < float(w_)) & (fy >= -1.0) & (fy < float(h_))
        i0, j0 = tr._floor(fx), tr._floor(fy)
        a = fx - i0.astype(np.float64)
        b = fy - j0.astype(np.float64)
        # 5. the four taps, the second moment beside the colour
        phits, pn, pz = tr.guides(prev_feat, prev_feat_spp)
        pc = fr.fix_to_f64(np.asarray(prev_fix, dtype=np.uint64))
        lim = sz2 * (s * s) + 1e-12
        acc = np.zeros((h_, w_, 3), dtype=np.float64)
        acc2 = np.zeros((h_, w_, 3), dtype=np.float64)
        ws = np.zeros((h_, w_), dtype=np.float64)
        N = np.full((h_, w_), 0xFFFFFFFF, dtype=np.int64)
        for (di, dj, kw) in ((0, 0, (1.0 - a) * (1.0 - b)), (1, 0, a * (1.0 - b)), (0, 1, (1.0 - a) * b), (1, 1, a * b)):
            ti, tj = i0 + di, j0 + dj
            keep = have & (ti >= 0) & (ti < w_) & (tj >= 0) & (tj < h_) & (kw > 0.0)
            qi, qj = np.clip(ti, 0, w_ - 1), np.clip(tj, 0, h_ - 1)                 # (a rejected tap's values are not used)
            keep &= (prev_len[qj, qi] != 0) & (phits[qj, qi] != 0)
            dz = pz[qj, qi] - s
            keep &= (dz * dz) < lim
            dn = n - pn[qj, qi]
            keep &= ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) * inn < 1.0
            acc = np.where(keep[..., None], acc + kw[..., None] * pc[qj, qi], acc)
            acc2 = np.where(keep[..., None], acc2 + kw[..., None] * prev_m2[qj, qi], acc2)
            ws = np.where(keep, ws + kw, ws)
            N = np.where(keep, np.minimum(N, prev_len[qj, qi].astype(np.int64)), N)
        have &= ws > 0.0
        hcol = acc / ws[..., None]
        h2 = acc2 / ws[..., None]
        # 6. the clamp moves the history's mean and keeps its central variance
        if clamp:
            hb = hcol
            mid = (lo + hi) * 0.5
            ext = ((hi - lo) * 0.5) * float(clamp_scale)
            hcol = np.where(hcol < mid - ext, mid - ext, hcol)
            hcol = np.where(hcol > mid + ext, mid + ext, hcol)
            h2 = (h2 - hb * hb) + hcol * hcol
        # 7. the blend, the moment, the variance of the frame mean; then the variance of the accumulated value
        at = 1.0 / (N + 1).astype(np.float64)
        at = np.where(at < float(alpha_min), float(alpha_min), at)[..., None]
        o = hcol + at * (c - hcol)
        m2 = h2 + at * (s2 - h2)
        vt = clip0(m2 - o * o)
        length = np.where(have, np.minimum(N + 1, tr.MAX_LEN), 1).astype(np.uint32)
        vf = np.where((length < MIN_LEN)[..., None], vs, vt)
        hv = have[..., None]
        return np.where(hv, tr.quantize(o), out0), length, np.where(hv, m2, m20), np.where(hv, vf * at, var0)


def chain(frames, **options):
    """frames: [(fix, spp, feat, feat_spp, cam)] -> [(out_fix, out_len, out_m2, out_var)] with ping-pong history."""
    results, history = [], None
    for fix, spp, feat, feat_spp, cam in frames:
        r = accumulate(fix, spp, feat, feat_spp, cam, history, **options)
        results.append(r)
        history = (r[0], r[1], feat, feat_spp, cam, r[2])
    return results


def prepare_var_given(var, m):
    """x = (var / m) / m, a NaN and a negative count 0, (x_r + x_g) + x_b"""
    x = clip0((np.asarray(var, dtype=np.float64) / m) / m)
    return (x[..., 0] + x[..., 1]) + x[..., 2]


def denoise_var_given(fix, var, spp, feat, feat_spp, *, levels=4, sigma_color=vr.SIGMA_COLOR, sigma_normal=1.0, sigma_depth=0.2, demodulate=True,
                      count=None):
    """-> the denoised one-sample frame, u64 [H,W,3]: denoise_var_ref's filter behind the one new rule of Prepare."""
    with np.errstate(all="ignore"):
        c, m, n, z = dr.prepare(fix, count, spp, feat, feat_spp, demodulate)
        v = prepare_var_given(var, m)
        for l in range(levels):
            c, v = vr.level(c, v, n, z, l, float(sigma_color), float(sigma_normal), float(sigma_depth))
        return dr.quantize(c * m)


def synthetic_m2(prev_fix, seed):
    """prev_m2 f64 [h,w,3] for a synthetic history, mixing pixel by pixel: h^2 + a positive variance (consistent with the history colour),
    values below h^2 (the clip at 0 decides), 0, a NaN, 1e12."""
    hcol = fr.fix_to_f64(np.asarray(prev_fix, dtype=np.uint64))
    rng = np.random.default_rng(seed + 4242 + 1000 * hcol.shape[1] + hcol.shape[0])
    kind = rng.integers(0, 10, size=hcol.shape[:2])
    first = min(5, kind.size)                                          # every special kind is there at every size (2 x 2 has four pixels: kinds 5-8)
    kind.flat[:first] = (np.arange(5) + 5)[:first]
    m2 = hcol * hcol + 0.3 * rng.random(hcol.shape)
    k = lambda v: (kind == v)[..., None]
    m2 = np.where(k(5), hcol * hcol * 0.5, m2)
    m2 = np.where(k(6), 0.0, m2)
    m2 = np.where(k(7), np.nan, m2)
    m2 = np.where(k(8), 1e12, m2)
    return m2


def synthetic_var(fix, count, spp, seed):
    """var f64 [h,w,3] for the filter's synthetic cases: mostly the order of the squared mean over the samples, with 0, negatives, a NaN,
    1e-300 and 1e12 among them (no infinity: one would spread as NaN through the levels and leave a frame of zeros to compare)."""
    c = dr.mean_of(fix, spp, count)
    rng = np.random.default_rng(seed + 99 + 1000 * c.shape[1] + c.shape[0])
    var = (c * c) * rng.random(c.shape) * 0.25
    kind = rng.integers(0, 16, size=c.shape[:2])
    k = lambda v: (kind == v)[..., None]
    var = np.where(k(0), 0.0, var)
    var = np.where(k(1), -var, var)
    var = np.where(k(2), np.nan, var)
    var = np.where(k(3), 1e12, var)
    var = np.where(k(4), 1e-300, var)
    return var


def bits(a):
    """doubles as u64, so that NaN and -0 count"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def checksum(*arrays):
    """FNV-1a, 64 bits, over the little-endian bytes of the arrays in turn: what tests/temporal_var_san_main.cpp prints."""
    hsh = 0xCBF29CE484222325
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            hsh = ((hsh ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return hsh
