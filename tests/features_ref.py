"""CPU reference of the first-hit feature buffers (include/rtiow_hip.h "feature buffers") -- a test helper.

Composed only from what oracle/ already exports: oracle.philox for the words, the camera run of oracle/oracle_f64.c's sample_ray
restated in Python floats (IEEE binary64, no fused multiply-add), oracle_get_ray for the ray, trace_ref.fast_hit (oracle_world_hit for
(index, t), oracle_sphere_hit on the winner for the normal), and Python integers for quantize / qs (oracle_b_quantize pins quantize).
"""
import ctypes as C
import math

import numpy as np

import oracle
from trace_ref import Scene, fast_hit

FEATURE_WORDS = 8
MASK64 = (1 << 64) - 1
KIND_DIALECTRIC = 2


def quantize(x):
    """Contract C5: floor(min(x, 65536) * 2^32) for x >= 0, 0 for negatives and NaN (exact integer arithmetic)."""
    if x != x or x <= 0.0:
        return 0
    return math.floor(min(x, 65536.0) * 4294967296.0)


def qs(x):
    """A normal's component: 0 for a NaN, else floor(clamp(x, -65536, 65536) * 2^32) as a two's-complement 64-bit integer."""
    if x != x:
        return 0
    return math.floor(max(-65536.0, min(x, 65536.0)) * 4294967296.0) & MASK64


def camera_sample(width, height, seed, i, j, s):
    """The camera run of sample s of pixel (i, j): (u, v, lens x, lens y) and the number of Philox blocks it took."""
    g = j * width + i
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = list(oracle.philox((g, s & 0xFFFFFFFF, 0, 0), key))
    blocks = 1
    u = (float(i) + words[0] * (1.0 / 4294967296.0)) / float(width - 1)       # main.rs:131
    v = (float(j) + words[1] * (1.0 / 4294967296.0)) / float(height - 1)      # main.rs:132
    sym = lambda w: float(w - (1 << 32) if w & 0x80000000 else w) * (1.0 / 2147483648.0)
    k = 2
    while True:                                                               # vec3.rs:59-68
        if k >= len(words):
            words += list(oracle.philox((g, s & 0xFFFFFFFF, blocks, 0), key))
            blocks += 1
        lx, ly = sym(words[k]), sym(words[k + 1])
        k += 2
        if (lx * lx + ly * ly) + 0.0 * 0.0 < 1.0:
            return u, v, lx, ly, blocks


def camera_ray(ocam, width, height, seed, i, j, s):
    u, v, lx, ly, _ = camera_sample(width, height, seed, i, j, s)
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    oracle.load().oracle_get_ray(C.byref(ocam), u, v, lx, ly, o, d)
    return o, d


def render_features(ocam, flat, width, height, spp, *, sample_begin=0, seed=1, t_min=1e-4):
    """-> (feat u64 [H,W,8], ids i32 [H,W]): the eight exact sums of every pixel over the samples [sample_begin, sample_begin + spp)
    and the list index the first of them hits (-1: a miss)."""
    scene = Scene(flat)
    feat = np.zeros((height, width, FEATURE_WORDS), dtype=np.uint64)
    ids = np.full((height, width), -1, dtype=np.int32)
    for j in range(height):
        for i in range(width):
            sums = [0] * FEATURE_WORDS
            for s in range(sample_begin, sample_begin + spp):
                o, d = camera_ray(ocam, width, height, seed, i, j, s)
                idx, t, _, nrm, _ = fast_hit(scene, o, d, t_min)
                if s == sample_begin:
                    ids[j, i] = idx
                if idx < 0:
                    continue
                rec = scene.flat[idx]
                albedo = (1.0, 1.0, 1.0) if int(rec["kind"]) == KIND_DIALECTRIC else tuple(float(x) for x in rec["albedo"])
                for c in range(3):
                    sums[c] += quantize(albedo[c])
                    sums[3 + c] += qs(nrm[c])
                sums[6] += quantize(t)
                sums[7] += 1
            feat[j, i] = np.array([x & MASK64 for x in sums], dtype=np.uint64)
    return feat, ids


def same(got, want):
    """(feat, ids, ...) of a kernel against the reference's (feat, ids): all eight words and the ids, bit for bit."""
    feat, ids = got[0], got[1]
    assert feat.dtype == np.uint64 and ids.dtype == np.int32
    assert np.array_equal(ids, want[1]), f"{int((ids != want[1]).sum())} ids differ"
    assert np.array_equal(feat, want[0]), f"{int((feat != want[0]).any(axis=-1).sum())} pixels differ"


def fix_to_f64(q):
    """rt_api.hip fix_to_f64 on a u64 array: ((f64)(q >> 32) * 2^32 + (f64)(u32)q) * 2^-32."""
    q = np.asarray(q, dtype=np.uint64)
    return ((q >> np.uint64(32)).astype(np.float64) * 4294967296.0 + (q & np.uint64(0xFFFFFFFF)).astype(np.float64)) * (1.0 / 4294967296.0)


def features_to_f32(feat, spp):
    """The rule of rt_features_to_f32, restated in numpy (IEEE binary64 throughout, one rounding to f32 at the end)."""
    feat = np.asarray(feat, dtype=np.uint64)
    out = np.zeros(feat.shape, dtype=np.float32)
    sppf = np.float64(spp)
    out[..., 0:3] = (fix_to_f64(feat[..., 0:3]) / sppf).astype(np.float32)
    nq = feat[..., 3:6]
    neg = nq.view(np.int64) < 0
    mag = np.where(neg, (~nq) + np.uint64(1), nq)                              # |q| of a two's-complement integer
    v = fix_to_f64(mag)
    out[..., 3:6] = (np.where(neg, -v, v) / sppf).astype(np.float32)
    hits = feat[..., 7]
    hf = hits.astype(np.float64)
    depth = np.divide(fix_to_f64(feat[..., 6]), hf, out=np.zeros(hf.shape, dtype=np.float64), where=hits != 0)
    out[..., 6] = np.where(hits != 0, depth, 0.0).astype(np.float32)
    out[..., 7] = (hf / sppf).astype(np.float32)
    return out


def synthetic_sums():
    """[3, 4, 8] sums of spp = 3 samples: no hit, one hit, three hits, negative normal sums, values above 2^53 / 2^32."""
    Q1 = 1 << 32
    q = np.zeros((3, 4, 8), dtype=np.uint64)
    neg = lambda x: (1 << 64) - x
    row = lambda *v: np.array(v, dtype=np.uint64)                                           # (Python integers: exact)
    q[0, 1] = row(Q1 // 2, Q1 // 4, Q1, neg(Q1), Q1 // 3, neg(1), 5 * Q1 + 12345, 1)
    q[0, 2] = row(3 * Q1, 3 * Q1 - 1, 1, neg(3 * Q1), 3 * Q1, neg(Q1 // 7), 3 * 65536 * Q1, 3)
    q[0, 3] = row(Q1 + 1, 2 * Q1 + 3, 0, 0, neg(2 * Q1 + 1), 2 * Q1 + 1, (1 << 55) + 12345678901, 2)
    rng = np.random.default_rng(7)
    q[1:, :, 0:3] = rng.integers(0, 3 * Q1, size=(2, 4, 3), dtype=np.uint64)
    q[1:, :, 3:6] = rng.integers(-3 * Q1, 3 * Q1, size=(2, 4, 3), dtype=np.int64).view(np.uint64)
    q[1:, :, 7] = rng.integers(0, 4, size=(2, 4), dtype=np.uint64)
    q[1:, :, 6] = rng.integers(0, 1 << 40, size=(2, 4), dtype=np.uint64) * q[1:, :, 7]
    return q, 3


def camera_from_rt(rt_cam):
    """rtiow_amd._ffi.rt_camera -> oracle camera struct, field by field (no arithmetic)."""
    oc = oracle.camera()
    for name, _ in oracle.camera._fields_:
        setattr(oc, name, getattr(rt_cam, name))
    return oc


# ---- hand scenes with analytic answers (pinhole cameras), shared by the CPU and the GPU tests -----------------------------------

def hand_scenes():
    """name -> (flat scene, host-mirror Camera for a 16 x 16 frame).  Every camera is a pinhole (aperture 0)."""
    import rtiow_amd as rt
    L, M, D = rt.Lambertian, rt.Metal, rt.Dialectric
    S, P = rt.Sphere, rt.Point3
    cam = lambda frm, at: rt.Camera(P(*frm), P(*at), rt.Vec3(0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    out = {}
    w = rt.HittableList(); w.push(S(P(0, 0, -5), 1.0, L(rt.Color(0.25, 0.5, 0.75))))
    out["one_sphere"] = (w.flatten(), cam((0, 0, 0), (0, 0, -5)))
    w = rt.HittableList(); w.push(S(P(0, 0, 0), 4.0, M(rt.Color(0.5, 0.25, 0.125), 0.0)))
    out["inside"] = (w.flatten(), cam((0, 0, 1), (0, 0, -1)))
    w = rt.HittableList()
    w.push(S(P(0, 0, -5), 1.0, L(rt.Color(0.25, 0.5, 0.75)))); w.push(S(P(0, 0, -5), 1.0, M(rt.Color(0.75, 0.5, 0.25), 0.5)))
    out["coincident"] = (w.flatten(), cam((0, 0, 0), (0, 0, -5)))
    w = rt.HittableList(); w.push(S(P(0, 0, -5), 1.0, D(1.5)))
    glass = w.flatten()
    glass[0]["albedo"] = (0.3, 0.6, 0.9)              # (a producer that fills the field: it must not be read)
    out["glass"] = (glass, cam((0, 0, 0), (0, 0, -5)))
    w = rt.HittableList(); w.push(S(P(0, 0, -5), -1.0, L(rt.Color(0.25, 0.5, 0.75))))
    out["negative_radius"] = (w.flatten(), cam((0, 0, 0), (0, 0, -5)))
    return out
