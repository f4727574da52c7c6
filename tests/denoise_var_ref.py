"""The variance-guided denoiser's contract (include/rtiow_hip.h "variance-guided denoiser") in numpy -- a test
helper, written from the text of the contract and not from the C++.  What the contract takes over from the denoiser's word for word
(prepare, the 3x3 box mean, quantize) is denoise_ref's; what it states itself (the variance of the half means, its 3x3 Gaussian, the level
with the colour stop in standard deviations and the variance propagated with the squared weights) is stated here.

Every step is an elementwise numpy operation on float64 arrays (numpy does not fuse a product into a sum), and the taps are added as
shifted slices in the stated order, dy outer and dx inner, so every pixel sees its in-frame taps in exactly that order.
"""
import numpy as np

import denoise_ref as dr
import features_ref as fr

SIGMA_COLOR = 1.0                                                     # the shipped default (rtiow_amd.make_denoise_var)
KK = ((1.0 / 16.0, 2.0 / 16.0, 1.0 / 16.0), (2.0 / 16.0, 4.0 / 16.0, 2.0 / 16.0), (1.0 / 16.0, 2.0 / 16.0, 1.0 / 16.0))
Q1 = dr.Q1


def prepare_var(fix, half, count, spp, m):
    """-> var [H,W]: d = |2 half - fix| (wrapping u64, two's complement), e = (v(d) / samples) / m, (e_r e_r + e_g e_g) + e_b e_b"""
    fix = np.asarray(fix, dtype=np.uint64)
    half = np.asarray(half, dtype=np.uint64)
    samples = np.float64(spp) if count is None else np.asarray(count, dtype=np.uint32).astype(np.float64)[..., None]
    d = half * np.uint64(2) - fix                                       # (arrays of uint64 wrap)
    neg = d.view(np.int64) < 0
    d = np.where(neg, (~d) + np.uint64(1), d)
    e = (fr.fix_to_f64(d) / samples) / m
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def gauss_var(var):
    h, w = var.shape
    sv = np.zeros((h, w), dtype=np.float64)
    sk = np.zeros((h, w), dtype=np.float64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if abs(dy) >= h or abs(dx) >= w:
                continue
            (dj, sj), (di, si) = dr._shift(h, dy), dr._shift(w, dx)
            kk = KK[dy + 1][dx + 1]
            sv[dj, di] = sv[dj, di] + kk * var[sj, si]
            sk[dj, di] = sk[dj, di] + kk
    return sv / sk


def level(c, var, n, z, l, sigma_color, sigma_normal, sigma_depth):
    """-> (c', var')"""
    h, w = c.shape[0], c.shape[1]
    s = 1 << l
    sc2 = sigma_color * sigma_color
    inn = 1.0 / (sigma_normal * sigma_normal)
    sz2 = sigma_depth * sigma_depth
    g = dr.box_mean(c)
    gv = gauss_var(var)
    izp = 1.0 / (sz2 * (z * z) + 1e-12)
    icv = 1.0 / (sc2 * gv + 1e-12)
    stop = lambda x: np.where(x < 1.0, 1.0 - x, 0.0)
    acc = np.zeros(c.shape, dtype=np.float64)
    ws = np.zeros((h, w), dtype=np.float64)
    va = np.zeros((h, w), dtype=np.float64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if abs(s * dy) >= h or abs(s * dx) >= w:
                continue
            (dj, sj), (di, si) = dr._shift(h, s * dy), dr._shift(w, s * dx)
            k = dr.H5[dy + 2] * dr.H5[dx + 2]
            d = g[dj, di] - g[sj, si]
            xc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * icv[dj, di]
            e = n[dj, di] - n[sj, si]
            xn = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * inn
            f = z[dj, di] - z[sj, si]
            xz = (f * f) * izp[dj, di]
            tc, tn, tz = stop(xc), stop(xn), stop(xz)
            wgt = ((k * (tc * tc)) * (tn * tn)) * (tz * tz)
            acc[dj, di] = acc[dj, di] + wgt[..., None] * c[sj, si]
            ws[dj, di] = ws[dj, di] + wgt
            va[dj, di] = va[dj, di] + (wgt * wgt) * var[sj, si]
    return acc / ws[..., None], va / (ws * ws)


def denoise_var(fix, half, spp, feat, feat_spp, *, levels=4, sigma_color=SIGMA_COLOR, sigma_normal=1.0, sigma_depth=0.2, demodulate=True,
                count=None):
    """-> the denoised one-sample frame, u64 [H,W,3]."""
    with np.errstate(all="ignore"):
        c, m, n, z = dr.prepare(fix, count, spp, feat, feat_spp, demodulate)
        var = prepare_var(fix, half, count, spp, m)
        for l in range(levels):
            c, var = level(c, var, n, z, l, float(sigma_color), float(sigma_normal), float(sigma_depth))
        return dr.quantize(c * m)


def synthetic_case(w, h, seed=11):
    """(fix u64 [h,w,3], half u64 [h,w,3], count u32 [h,w] even, spp (even), feat u64 [h,w,8], feat_spp): denoise_ref.synthetic_case
    (itself built on features_ref.synthetic_sums) with even counts 2..40 and a `half` that mixes, pixel by pixel: 2 half == fix (zero
    variance; fix made even there), half = 0, half = fix, half > fix, a half whose double wraps past 2^64, and -- every second pixel -- a
    plausible half, a fraction 0.3 .. 0.7 of fix drawn per channel.  The last pixel carries sums above 2^53 in fix, half and their
    difference."""
    fix, count, spp, feat, feat_spp = dr.synthetic_case(w, h, seed)
    rng = np.random.default_rng(seed + 77 + 1000 * h + w)
    fix = fix.copy()
    count = (2 * rng.integers(1, 21, size=(h, w))).astype(np.uint32)
    kind = rng.integers(0, 10, size=(h, w))
    fix[kind == 0] &= ~np.uint64(1)
    frac = rng.random((h, w, 3)) * 0.4 + 0.3
    half = np.floor(fix.astype(np.float64) * frac).astype(np.uint64)
    k = lambda v: (kind == v)[..., None]
    half = np.where(k(0), fix >> np.uint64(1), half)
    half = np.where(k(1), np.uint64(0), half)
    half = np.where(k(2), fix, half)
    half = np.where(k(3), fix + fix // np.uint64(3) + np.uint64(1), half)
    half = np.where(k(4), np.uint64((1 << 63) + 5) + fix, half)
    fix[h - 1, w - 1] = np.array([(1 << 54) + 12345, (1 << 54) + 2, 3 * Q1], dtype=np.uint64)
    half[h - 1, w - 1] = np.array([0, (1 << 53) + 1 + (1 << 20), 3 * Q1], dtype=np.uint64)
    count[h - 1, w - 1] = 40
    return fix, half, count, spp, feat, feat_spp
