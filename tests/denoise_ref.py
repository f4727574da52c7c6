"""The denoiser's contract (include/rtiow_hip.h "denoiser") in numpy -- a test helper, written from the text of
the contract and not from the C++.

Every step is an elementwise numpy operation on float64 arrays (numpy does not fuse a product into a sum), and the taps of a level are
added as shifted slices in the stated order, dy outer and dx inner, so every pixel sees its in-frame taps in exactly that order.
"""
import numpy as np

import features_ref as fr

ALBEDO_FLOOR = 0.015625
H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
Q1 = 1 << 32


def quantize(x):
    """Contract C5 on an array: floor(min(x, 65536) * 2^32) for x >= 0, 0 for negatives and NaN."""
    x = np.where(x > 0.0, x, 0.0)
    x = np.where(x < 65536.0, x, 65536.0)
    return np.floor(x * 4294967296.0).astype(np.uint64)         # (the product is exact, <= 2^48)


def _shift(n, o):
    """Slices (dst, src) of an axis of length n for the tap at offset o: the p with 0 <= p + o < n, and p + o."""
    return slice(max(0, -o), min(n, n - o)), slice(max(0, o), min(n, n + o))


def prepare(fix, count, spp, feat, feat_spp, demodulate):
    """-> (c0 [H,W,3], m [H,W,3], n [H,W,3], z [H,W])"""
    fix = np.asarray(fix, dtype=np.uint64)
    feat = np.asarray(feat, dtype=np.uint64)
    samples = np.float64(spp) if count is None else np.asarray(count, dtype=np.uint32).astype(np.float64)[..., None]
    fs = np.float64(feat_spp)
    c = fr.fix_to_f64(fix) / samples
    alb = fr.fix_to_f64(feat[..., 0:3]) / fs
    nq = feat[..., 3:6]
    neg = nq.view(np.int64) < 0
    v = fr.fix_to_f64(np.where(neg, (~nq) + np.uint64(1), nq))
    n = np.where(neg, -v, v) / fs
    hits = feat[..., 7]
    hf = hits.astype(np.float64)
    z = np.where(hits != 0, fr.fix_to_f64(feat[..., 6]) / np.where(hits != 0, hf, 1.0), 0.0)
    alpha = hf / fs
    if demodulate:
        m = alb + (1.0 - alpha)[..., None]
        m = np.where(m < ALBEDO_FLOOR, ALBEDO_FLOOR, m)
    else:
        m = np.ones(c.shape, dtype=np.float64)
    return c / m, m, n, z


def box_mean(c):
    h, w = c.shape[0], c.shape[1]
    total = np.zeros(c.shape, dtype=np.float64)
    number = np.zeros((h, w), dtype=np.float64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if abs(dy) >= h or abs(dx) >= w:
                continue
            (dj, sj), (di, si) = _shift(h, dy), _shift(w, dx)
            total[dj, di] = total[dj, di] + c[sj, si]
            number[dj, di] = number[dj, di] + 1.0
    return total / number[..., None]


def level(c, n, z, l, sigma_color, sigma_normal, sigma_depth):
    h, w = c.shape[0], c.shape[1]
    s = 1 << l
    scl = sigma_color * 0.5 ** l
    ic = 1.0 / (scl * scl)
    inn = 1.0 / (sigma_normal * sigma_normal)
    sz2 = sigma_depth * sigma_depth
    g = box_mean(c)
    izp = 1.0 / (sz2 * (z * z) + 1e-12)
    stop = lambda x: np.where(x < 1.0, 1.0 - x, 0.0)
    acc = np.zeros(c.shape, dtype=np.float64)
    ws = np.zeros((h, w), dtype=np.float64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if abs(s * dy) >= h or abs(s * dx) >= w:
                continue
            (dj, sj), (di, si) = _shift(h, s * dy), _shift(w, s * dx)
            k = H5[dy + 2] * H5[dx + 2]
            d = g[dj, di] - g[sj, si]
            xc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * ic
            e = n[dj, di] - n[sj, si]
            xn = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * inn
            f = z[dj, di] - z[sj, si]
            xz = (f * f) * izp[dj, di]
            tc, tn, tz = stop(xc), stop(xn), stop(xz)
            wgt = ((k * (tc * tc)) * (tn * tn)) * (tz * tz)
            acc[dj, di] = acc[dj, di] + wgt[..., None] * c[sj, si]
            ws[dj, di] = ws[dj, di] + wgt
    return acc / ws[..., None]


def denoise(fix, spp, feat, feat_spp, *, levels=4, sigma_color=0.35, sigma_normal=1.0, sigma_depth=0.2, demodulate=True, count=None):
    """-> the denoised one-sample frame, u64 [H,W,3]."""
    with np.errstate(all="ignore"):
        c, m, n, z = prepare(fix, count, spp, feat, feat_spp, demodulate)
        for l in range(levels):
            c = level(c, n, z, l, float(sigma_color), float(sigma_normal), float(sigma_depth))
        return quantize(c * m)


def mean_of(fix, spp=1, count=None):
    """The linear mean radiance of a frame of sums (the quality metric's input)."""
    samples = np.float64(spp) if count is None else np.asarray(count).astype(np.float64)[..., None]
    return fr.fix_to_f64(fix) / samples


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(x, 0.0, 1.0) - np.clip(ref, 0.0, 1.0)) ** 2)))


def synthetic_case(w, h, seed=11):
    """(fix u64 [h,w,3], count u32 [h,w], spp, feat u64 [h,w,8], feat_spp): features_ref.synthetic_sums in the corner (as much of it as
    fits; feat_spp is its 3), around it random frames made of patches of 6 x 5 pixels -- sky (no hit), partly covered and fully covered
    ones with a patch-wise normal, depth and albedo plus per-pixel scatter, so that every edge-stop takes values inside (0, 1) as well as
    0 and 1 --, radiance sums of 8 samples (count: 1..40 samples, mixed), and one sum above 2^53."""
    q, feat_spp = fr.synthetic_sums()
    rng = np.random.default_rng(seed + 1000 * w + h)
    jj, ii = np.mgrid[0:h, 0:w]
    patch = (ii // 6) * 7 + (jj // 5) * 3
    kind = patch % 4                                                    # 0: sky
    prng = np.random.default_rng(seed)
    table = prng.random((int(patch.max()) + 1, 8))
    t = table[patch]
    hits = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(0, feat_spp + 1, size=(h, w)), feat_spp)).astype(np.uint64)
    feat = np.zeros((h, w, 8), dtype=np.uint64)
    hitsf = hits.astype(np.float64)
    for ch in range(3):
        feat[..., ch] = np.floor(t[..., ch] * hitsf * Q1).astype(np.uint64)
        nrm = (2.0 * t[..., 3 + ch] - 1.0 + 0.2 * (rng.random((h, w)) - 0.5)) * hitsf
        feat[..., 3 + ch] = np.floor(nrm * Q1).astype(np.int64).view(np.uint64)
    feat[..., 6] = np.floor((1.0 + 20.0 * t[..., 6]) * (1.0 + 0.1 * rng.random((h, w))) * hitsf * Q1).astype(np.uint64)
    feat[..., 7] = hits
    count = rng.integers(1, 41, size=(h, w)).astype(np.uint32)
    spp = 8
    base = np.where((kind == 0)[..., None], 0.7, t[..., 0:3] * t[..., 7:8])
    noise = rng.random((h, w, 3)) * 1.5 + 0.25
    fix = np.floor(base * noise * 8.0 * Q1).astype(np.uint64)
    qh, qw = min(h, q.shape[0]), min(w, q.shape[1])
    src = q[0:qh, q.shape[1] - qw:]                                     # (a 1 x 1 frame takes the pixel with the depth sum above 2^53)
    feat[0:qh, 0:qw] = src
    fix[h - 1, w - 1] = np.array([(1 << 54) + 12345, (1 << 53) + 1, 3 * Q1], dtype=np.uint64)
    count[h - 1, w - 1] = 40
    return fix, count, spp, feat, feat_spp


def checksum(out):
    """FNV-1a, 64 bits, over the little-endian bytes of a u64 array: what tests/denoise_san_main.cpp prints."""
    hsh = 0xCBF29CE484222325
    for b in np.ascontiguousarray(out, dtype="<u8").tobytes():
        hsh = ((hsh ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return hsh
