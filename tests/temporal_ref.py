"""The contract of temporal accumulation (include/rtiow_hip.h "temporal accumulation") in numpy -- a test helper,
written from the text of the contract and not from the C++.

Every step is an elementwise numpy operation on float64 arrays (numpy does not fuse a product into a sum; no np.dot, no sum): dot and
cross are spelled out in the header's order, the four taps are gathered and added one after the other in the stated order, and the 3 x 3
box of the clamp visits its neighbours dy outer, dx inner.  The case builders the CPU and the GPU tests share live here too.
"""
import math

import numpy as np

import features_ref as fr

Q1 = 1 << 32
MAX_LEN = 65535
SIZES = [(2, 2), (5, 3), (37, 19), (70, 45)]
DEFAULTS = dict(alpha_min=0.1, sigma_normal=0.5, sigma_depth=0.1, clamp=True, clamp_scale=1.0)


def quantize(x):
    """Contract C5 on an array: floor(min(x, 65536) * 2^32) for x >= 0, 0 for negatives and NaN."""
    x = np.where(x > 0.0, x, 0.0)
    x = np.where(x < 65536.0, x, 65536.0)
    return np.floor(x * 4294967296.0).astype(np.uint64)         # (the product is exact, <= 2^48)


def cam_vectors(cam):
    """(origin, lower_left_corner, horizontal, vertical) of an rt_camera / host Camera as tuples of Python floats."""
    c = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
    return tuple(tuple(float(x) for x in getattr(c, name)) for name in ("origin", "lower_left_corner", "horizontal", "vertical"))


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def guides(feat, feat_spp):
    """-> (hits u64 [H,W], n [H,W,3], z [H,W])"""
    feat = np.asarray(feat, dtype=np.uint64)
    fs = np.float64(feat_spp)
    nq = feat[..., 3:6]
    neg = nq.view(np.int64) < 0
    v = fr.fix_to_f64(np.where(neg, (~nq) + np.uint64(1), nq))
    n = np.where(neg, -v, v) / fs
    hits = feat[..., 7]
    hf = hits.astype(np.float64)
    z = np.where(hits != 0, fr.fix_to_f64(feat[..., 6]) / np.where(hits != 0, hf, 1.0), 0.0)
    return hits, n, z


def colour(fix, spp, count):
    samples = np.float64(spp) if count is None else np.asarray(count, dtype=np.uint32).astype(np.float64)[..., None]
    return fr.fix_to_f64(np.asarray(fix, dtype=np.uint64)) / samples


def _floor(x):
    """floor by cast and correction (x is finite and small wherever the result is used)"""
    k = np.where(np.isfinite(x), x, 0.0).astype(np.int64)
    return np.where(k.astype(np.float64) > x, k - 1, k)


def accumulate(fix, spp, feat, feat_spp, cam, history=None, *, alpha_min=0.1, sigma_normal=0.5, sigma_depth=0.1, clamp=True, clamp_scale=1.0,
               count=None):
    """-> (out_fix u64 [H,W,3], out_len u32 [H,W]).  history: None or (prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam)."""
    with np.errstate(all="ignore"):
        c = colour(fix, spp, count)
        h_, w_ = c.shape[0], c.shape[1]
        hits, n, z = guides(feat, feat_spp)
        out = quantize(c)
        length = np.ones((h_, w_), dtype=np.uint32)
        if history is None:
            return out, length
        prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam = history
        prev_len = np.asarray(prev_len, dtype=np.uint32)
        co, cl, ch_, cv = cam_vectors(cam)
        po, pl, Hh, Vv = cam_vectors(prev_cam)
        # the constants
        L = tuple(pl[k] - po[k] for k in range(3))
        nrm = cross(Hh, Vv)
        iLn = np.float64(1.0) / np.float64(dot(L, nrm))
        LH, LV = dot(L, Hh), dot(L, Vv)
        iHH, iVV = np.float64(1.0) / np.float64(dot(Hh, Hh)), np.float64(1.0) / np.float64(dot(Vv, Vv))
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
        s = dot(e, nrm) * iLn
        have = (hits != 0) & (s > 0.0)
        inv_s = 1.0 / s
        up = (dot(e, Hh) * inv_s - LH) * iHH
        vp = (dot(e, Vv) * inv_s - LV) * iVV
        fx = up * wm1 - 0.5
        fy = vp * hm1 - 0.5
        have &= (fx >= -1.0) & (fx < float(w_)) & (fy >= -1.0) & (fy < float(h_))
        i0, j0 = _floor(fx), _floor(fy)
        a = fx - i0.astype(np.float64)
        b = fy - j0.astype(np.float64)
        # 5. the four taps
        phits, pn, pz = guides(prev_feat, prev_feat_spp)
        pc = fr.fix_to_f64(np.asarray(prev_fix, dtype=np.uint64))
        lim = sz2 * (s * s) + 1e-12
        acc = np.zeros((h_, w_, 3), dtype=np.float64)
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
            ws = np.where(keep, ws + kw, ws)
            N = np.where(keep, np.minimum(N, prev_len[qj, qi].astype(np.int64)), N)
        have &= ws > 0.0
        hcol = acc / ws[..., None]
        # 6. the clamp
        if clamp:
            lo, hi = c.copy(), c.copy()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dx == 0 and dy == 0) or abs(dy) >= h_ or abs(dx) >= w_:
                        continue
                    dst_j, src_j = slice(max(0, -dy), min(h_, h_ - dy)), slice(max(0, dy), min(h_, h_ + dy))
                    dst_i, src_i = slice(max(0, -dx), min(w_, w_ - dx)), slice(max(0, dx), min(w_, w_ + dx))
                    cq = c[src_j, src_i]
                    lo[dst_j, dst_i] = np.where(cq < lo[dst_j, dst_i], cq, lo[dst_j, dst_i])
                    hi[dst_j, dst_i] = np.where(cq > hi[dst_j, dst_i], cq, hi[dst_j, dst_i])
            mid = (lo + hi) * 0.5
            ext = ((hi - lo) * 0.5) * float(clamp_scale)
            hcol = np.where(hcol < mid - ext, mid - ext, hcol)
            hcol = np.where(hcol > mid + ext, mid + ext, hcol)
        # 7. the blend
        at = 1.0 / (N + 1).astype(np.float64)
        at = np.where(at < float(alpha_min), float(alpha_min), at)
        blended = quantize(hcol + at[..., None] * (c - hcol))
        out = np.where(have[..., None], blended, out)
        length = np.where(have, np.minimum(N + 1, MAX_LEN), 1).astype(np.uint32)
        return out, length


def chain(frames, **options):
    """frames: [(fix, spp, feat, feat_spp, cam)] -> [(out_fix, out_len)] with ping-pong history."""
    results, history = [], None
    for fix, spp, feat, feat_spp, cam in frames:
        out, length = accumulate(fix, spp, feat, feat_spp, cam, history, **options)
        results.append((out, length))
        history = (out, length, feat, feat_spp, cam)
    return results


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(x, 0.0, 1.0) - np.clip(ref, 0.0, 1.0)) ** 2)))


def checksum(out_fix, out_len):
    """FNV-1a, 64 bits, over the little-endian bytes of out_fix then out_len: what tests/temporal_san_main.cpp prints."""
    hsh = 0xCBF29CE484222325
    for b in np.ascontiguousarray(out_fix, dtype="<u8").tobytes() + np.ascontiguousarray(out_len, dtype="<u4").tobytes():
        hsh = ((hsh ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return hsh


# ---- case builders ----------------------------------------------------------------------------------------------------------------

def _tile(a, h, w):
    reps = (-(-h // a.shape[0]), -(-w // a.shape[1]), 1)
    return np.ascontiguousarray(np.tile(a, reps)[:h, :w])


def synthetic_frame(w, h, seed):
    """(fix u64 [h,w,3], count u32 [h,w], spp, feat u64 [h,w,8], feat_spp): features_ref.synthetic_sums tiled over the frame -- zero-hit
    pixels, negative normal sums, sums above 2^53 -- with the depth sums of most pixels replaced by depths near the focus plane (so that
    reprojection lands in the frame and the depth test has both outcomes), random radiance sums of 8 samples and random counts."""
    q, feat_spp = fr.synthetic_sums()
    rng = np.random.default_rng(seed + 1000 * w + h)
    feat = _tile(q, h, w).copy()
    hits = feat[..., 7].astype(np.float64)
    near = rng.random((h, w)) < 0.85
    depth = (0.9 + 0.2 * rng.random((h, w))) * hits
    feat[..., 6] = np.where(near, np.floor(depth * Q1).astype(np.uint64), feat[..., 6])
    smooth = rng.random((h, w)) < 0.6                               # pixels whose normal is that of the synthetic frame's pixel (0, 2)
    for ch in range(3):
        base = q[0, 2, 3 + ch].view(np.int64).astype(np.float64) / 3.0
        feat[..., 3 + ch] = np.where(smooth & (feat[..., 7] != 0), np.floor(base * hits * (1.0 + 0.05 * rng.random((h, w)))).astype(np.int64).view(np.uint64),
                                     feat[..., 3 + ch])
    fix = np.floor(rng.random((h, w, 3)) * 1.5 * 8.0 * Q1).astype(np.uint64)
    fix[h - 1, w - 1] = np.array([(1 << 54) + 12345, (1 << 53) + 1, 3 * Q1], dtype=np.uint64)
    count = rng.integers(1, 41, size=(h, w)).astype(np.uint32)
    return fix, count, 8, feat, feat_spp


def synthetic_history(w, h, seed):
    """(prev_fix u64 [h,w,3] random colours, prev_len u32 [h,w] with 0, 1 and 65535 among them, prev_feat, prev_feat_spp)"""
    rng = np.random.default_rng(seed + 77)
    _, _, _, feat, feat_spp = synthetic_frame(w, h, seed + 5)
    prev_fix = np.floor(rng.random((h, w, 3)) * 1.25 * Q1).astype(np.uint64)
    prev_len = rng.choice(np.array([0, 1, 2, 3, 9, 10, 200, 65534, 65535, 70000], dtype=np.uint32), size=(h, w))
    return prev_fix, prev_len, feat, feat_spp


def camera(w, h, look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0), v_up=(0.0, 1.0, 0.0), fov=20.0, aperture=0.1, focus=10.0):
    import rtiow_amd as rt
    return rt.Camera(rt.Point3(*look_from), rt.Point3(*look_at), rt.Vec3(*v_up), fov, float(w) / float(h), aperture, focus)


def camera_pairs(w, h):
    """name -> (current camera, previous camera), real host Cameras."""
    import rtiow_amd as rt
    base = camera(w, h)
    # one pixel of the image plane at the focus distance is viewport_width / (w - 1) wide
    px = 2.0 * math.tan(math.radians(20.0) / 2.0) * (float(w) / float(h)) * 10.0 / float(max(w - 1, 1))
    right = np.asarray(base.u, dtype=np.float64)
    shift = lambda d: (tuple(np.array([13.0, 2.0, 3.0]) + d * right), tuple(np.array([0.0, 0.0, 0.0]) + d * right))
    sub = shift(0.37 * px)
    wide = ((13.0, 2.0, 3.0), tuple(3.0 * w * px * right))            # a pan about the eye: three frame widths, whatever the depth
    nan_cam = camera(w, h).to_rt_camera()
    nan_cam.horizontal[1] = float("nan")
    return {
        "identical": (base, camera(w, h)),
        "subpixel_pan": (base, camera(w, h, look_from=sub[0], look_at=sub[1])),
        "wide_pan": (base, camera(w, h, look_from=wide[0], look_at=wide[1])),
        "facing_away": (base, camera(w, h, look_from=(13.0, 2.0, 3.0), look_at=(26.0, 4.0, 6.0))),
        "roll_90": (base, camera(w, h, v_up=(3.0, 0.0, -13.0))),
        "fov": (base, camera(w, h, fov=23.0)),
        "nan_prev": (base, nan_cam),
        "lens_radius": (camera(w, h, aperture=0.0), camera(w, h, look_from=sub[0], look_at=sub[1], aperture=2.0)),
        "orbit_step": tuple(rt.orbit_cameras(180, w, h)[1::-1]),
    }


OPTION_SETS = [dict(DEFAULTS), dict(DEFAULTS, clamp=False), dict(DEFAULTS, clamp_scale=0.0),
               dict(alpha_min=1.0, sigma_normal=5.0, sigma_depth=5.0, clamp=True, clamp_scale=0.5),
               dict(alpha_min=1e-6, sigma_normal=0.05, sigma_depth=0.01, clamp=False, clamp_scale=1.0)]


def make_options(**kw):
    import rtiow_amd as rt
    o = dict(DEFAULTS)
    o.update(kw)
    return rt.make_temporal(o["alpha_min"], o["sigma_normal"], o["sigma_depth"], o["clamp"], o["clamp_scale"])


# ---- the rejections every form makes before it touches anything --------------------------------------------------------------------

BAD = [
    (dict(tp=None), "options are NULL"), (dict(fix=None), "a buffer is NULL"), (dict(feat=None), "a buffer is NULL"), (dict(cam=None), "a buffer is NULL"),
    (dict(out=None), "a buffer is NULL"), (dict(olen=None), "a buffer is NULL"),
    (dict(pfix=None), "partial history"), (dict(plen=None), "partial history"), (dict(pfeat=None), "partial history"), (dict(pcam=None), "partial history"),
    (dict(pfix=None, plen=None, pfeat=None), "partial history"),
    (dict(flags=2), "unknown flags"), (dict(flags=0x80000001), "unknown flags"),
    (dict(alpha_min=0.0), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"), (dict(alpha_min=math.nan), "alpha_min"),
    (dict(sigma_normal=0.0), "sigma"), (dict(sigma_depth=-1.0), "sigma"), (dict(sigma_depth=math.inf), "sigma"), (dict(sigma_normal=math.nan), "sigma"),
    (dict(clamp_scale=-0.5), "clamp_scale"), (dict(clamp_scale=math.inf), "clamp_scale"), (dict(clamp_scale=math.nan), "clamp_scale"),
    (dict(width=1), "must be >= 2"), (dict(height=1), "must be >= 2"), (dict(height=-3), "must be >= 2"), (dict(width=65536, height=32769), "<= 2^31"),
    (dict(spp=0), "spp >= 1 without a count"), (dict(feat_spp=0), "feat_spp >= 1"), (dict(pspp=0), "prev_feat_spp >= 1"),
]


BAD_IDS = ["-".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in BAD]


def rejection_arrays(w=4, h=3):
    """name -> array: valid arguments of a 4 x 3 call, the outputs filled with a pattern a rejected call must leave alone"""
    return dict(fix=np.full((h, w, 3), 1 << 32, dtype=np.uint64), feat=np.zeros((h, w, 8), dtype=np.uint64),
                pfix=np.zeros((h, w, 3), dtype=np.uint64), plen=np.ones((h, w), dtype=np.uint32), pfeat=np.zeros((h, w, 8), dtype=np.uint64),
                out=np.full((h, w, 3), 0xABCD, dtype=np.uint64), olen=np.full((h, w), 0xABCD, dtype=np.uint32))


def call_form(lib, form, kw, bufs, ctx=None, stream=None):
    """One call of rt_temporal_host / rt_temporal / rt_temporal_device on the buffers `bufs` (name -> address) with the arguments `kw`
    knocks out or replaces."""
    import ctypes as C
    import rtiow_amd as rt
    tp = rt.make_temporal()
    for k in ("flags", "alpha_min", "sigma_normal", "sigma_depth", "clamp_scale"):
        if k in kw:
            setattr(tp, k, kw[k])
    cam, pcam = rt.book1_camera(4, 3).to_rt_camera(), rt.book1_camera(4, 3).to_rt_camera()
    ptr = lambda name: None if name in kw else C.c_void_p(bufs[name])
    args = [ptr("fix"), None, kw.get("spp", 8), ptr("feat"), kw.get("feat_spp", 8), None if "cam" in kw else C.byref(cam),
            ptr("pfix"), ptr("plen"), ptr("pfeat"), kw.get("pspp", 8), None if "pcam" in kw else C.byref(pcam),
            kw.get("width", 4), kw.get("height", 3), None if "tp" in kw else C.byref(tp), ptr("out"), ptr("olen")]
    if form == "host":
        return lib.rt_temporal_host(*args)
    if form == "buffers":
        return lib.rt_temporal(ctx, *args, None)
    return lib.rt_temporal_device(ctx, *args, stream)
