"""CPU statement of the wavefront path steps (include/rtiow_hip.h "wavefront path steps") -- a test helper.

Composed only from what oracle/ already exports: oracle.philox for the words of a path's stream (key = seed, counter = (pixel, sample,
event, 0)); the camera run and the unit-sphere run restated in Python floats (IEEE binary64, no fused multiply-add), left to right as
length_squared writes them; oracle_get_ray for the camera ray; oracle_scatter with an explicit draw list holding exactly the words the
accepted run consumed (a symmetric draw of word w goes in as the uniform (w ^ 0x80000000) * 2^-32, for which the oracle's 2u - 1 is
exactly (int32)w * 2^-31; the Dialectric's draw as w * 2^-32; *used gives the words consumed and from it the event advance);
oracle_b_quantize for the sums; trace_ref.fast_hit for closest hits.  A NaN is written as the quiet NaN 0x7FF8000000000000.
"""
import ctypes as C
import functools

import numpy as np

import oracle
from trace_ref import Scene, canonical, fast_hit

ABSORBED, SCATTERED, MISS, BAD_INDEX = 0, 1, 2, 3
LAMBERTIAN, METAL, DIALECTRIC = 0, 1, 2
D3 = C.c_double * 3
MASK64 = (1 << 64) - 1
F64_SENTINEL, U8_SENTINEL = -777.25, 0xEE          # what the GPU tests prefill outputs with


def key_of(seed):
    return (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


class Words:
    """The words of the blocks event, event + 1, ... of (pixel, sample), fetched as they are asked for."""

    def __init__(self, seed, pixel, sample, event):
        self.key, self.pixel, self.sample, self.event = key_of(seed), int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF, int(event)
        self.words = []

    def __getitem__(self, k):
        while k >= len(self.words):
            e = (self.event + len(self.words) // 4) & 0xFFFFFFFF
            self.words += list(oracle.philox((self.pixel, self.sample, e, 0), self.key))
        return self.words[k]


def u01(w):
    return w * (1.0 / 4294967296.0)


def u11(w):
    return float(w - (1 << 32) if w & 0x80000000 else w) * (1.0 / 2147483648.0)


def as_symmetric_uniform(w):
    """The uniform u with 2u - 1 == u11(w), exactly."""
    return (w ^ 0x80000000) * (1.0 / 4294967296.0)


# ---- rt_camera_rays ----------------------------------------------------------------------------------------------------------------------

def camera_path(ocam, width, height, seed, pixel, sample):
    """sample_ray (main.rs:131-134, camera.rs:47-54) -> (origin, dir, event, lens tries)."""
    w = Words(seed, pixel, sample, 0)
    i, j = pixel % width, pixel // width
    u = (float(i) + u01(w[0])) / float(width - 1)                             # main.rs:131
    v = (float(j) + u01(w[1])) / float(height - 1)                            # main.rs:132
    tries = 0
    while True:                                                               # vec3.rs:59-68
        lx, ly = u11(w[2 + 2 * tries]), u11(w[3 + 2 * tries])
        tries += 1
        if (lx * lx + ly * ly) + 0.0 * 0.0 < 1.0:
            break
    o, d = D3(), D3()
    oracle.load().oracle_get_ray(C.byref(ocam), u, v, lx, ly, o, d)
    return tuple(o), tuple(d), 1 + tries // 2, tries                          # 1 + ceil((tries - 1) / 2)


def camera_rays(ocam, width, height, seed, pixel, sample):
    n = len(pixel)
    out = dict(origin=np.zeros((n, 3)), dir=np.zeros((n, 3)), event=np.zeros(n, dtype=np.uint32), tries=np.zeros(n, dtype=np.int32))
    for k in range(n):
        out["origin"][k], out["dir"][k], out["event"][k], out["tries"][k] = camera_path(ocam, width, height, seed, int(pixel[k]), int(sample[k]))
    out["origin"], out["dir"] = canonical(out["origin"]), canonical(out["dir"])
    return out


# ---- rt_scatter ----------------------------------------------------------------------------------------------------------------------------

def unit_sphere_run(seed, pixel, sample, event):
    """vec3.rs:37-45 on the stream: the tries of three consecutive words from block `event` on -> (tries, the 3 * tries words)."""
    w = Words(seed, pixel, sample, event)
    tries = 0
    while True:
        x, y, z = u11(w[3 * tries]), u11(w[3 * tries + 1]), u11(w[3 * tries + 2])
        tries += 1
        if x * x + y * y + z * z < 1.0:
            return tries, [w[k] for k in range(3 * tries)]


def scatter_path(rec, seed, d_in, point, normal, front, pixel, sample, event):
    """Scatter::scatter of the flat sphere record `rec` -> dict(status, attenuation, out_dir, event, tries, mode).  mode: for a Dialectric
    "tir" (no draw), "refract" or "reflect"; else ""."""
    lib = oracle.load()
    kind = int(rec["kind"])
    tries = 0
    if kind == DIALECTRIC:
        draws = [u01(Words(seed, pixel, sample, event)[0])]
    else:
        tries, run = unit_sphere_run(seed, pixel, sample, event)
        draws = [as_symmetric_uniform(x) for x in run]
    one = np.ascontiguousarray(rec).reshape(1)
    used = C.c_int(0)
    att, d_out = D3(), D3()
    n_arr = D3(*normal)
    ok = lib.oracle_scatter(one.ctypes.data_as(C.POINTER(oracle.sphere)), D3(*d_in), D3(*point), n_arr, int(front),
                            (C.c_double * len(draws))(*draws), len(draws), C.byref(used), att, d_out)
    if kind == DIALECTRIC:
        assert used.value in (0, 1)
    else:
        assert used.value == 3 * tries, (used.value, tries)                    # the oracle's own rejection loop agrees with the restated one
    mode = ""
    if kind == DIALECTRIC:
        if used.value == 0:
            mode = "tir"
        else:
            # which branch the draw chose: materials.rs:96, `reflectance(cos_theta, ratio) > u` reflects
            ratio = 1.0 / float(rec["param"]) if front else float(rec["param"])
            with np.errstate(all="ignore"):
                d = np.array(d_in, dtype=np.float64)
                ud = d * (np.float64(1.0) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
                dt = -(ud[0] * normal[0] + ud[1] * normal[1] + ud[2] * normal[2])
                cos_theta = float(dt) if dt < 1.0 else 1.0
            mode = "reflect" if lib.oracle_reflectance(cos_theta, ratio) > draws[0] else "refract"
    return dict(status=SCATTERED if ok else ABSORBED, attenuation=tuple(att), out_dir=tuple(d_out),
                event=(int(event) + (used.value + 3) // 4) & 0xFFFFFFFF, tries=tries, mode=mode)


def scatter(flat, seed, dirs, index, point, normal, front_face, pixel, sample, event, out=None):
    """rt_scatter as the header defines it.  out: dict of arrays the outputs are written INTO (prefilled by the caller; default: the
    sentinels), so that what the contract leaves unwritten keeps its bytes.  Returns out plus "event" (advanced copy), "tries", "mode"."""
    n = len(index)
    res = dict(out_origin=np.full((n, 3), F64_SENTINEL), out_dir=np.full((n, 3), F64_SENTINEL), attenuation=np.full((n, 3), F64_SENTINEL),
               status=np.full(n, U8_SENTINEL, dtype=np.uint8))
    res.update({k: np.array(v, copy=True) for k, v in (out or {}).items()})
    res["event"] = np.array(event, dtype=np.uint32, copy=True)
    res["tries"], res["mode"] = np.zeros(n, dtype=np.int32), [""] * n
    for k in range(n):
        idx = int(index[k])
        if idx == -1:
            res["status"][k] = MISS
            continue
        if idx < -1 or idx >= len(flat):
            res["status"][k] = BAD_INDEX
            continue
        # (everything of path k is read before anything of it is written: out_dir may be dirs)
        r = scatter_path(flat[idx], seed, dirs[k].tolist(), point[k].tolist(), normal[k].tolist(), int(front_face[k]), int(pixel[k]),
                         int(sample[k]), int(event[k]))
        res["status"][k], res["event"][k], res["tries"][k], res["mode"][k] = r["status"], r["event"], r["tries"], r["mode"]
        res["attenuation"][k] = r["attenuation"]
        if r["status"] == SCATTERED:
            res["out_origin"][k], res["out_dir"][k] = point[k], r["out_dir"]
    for name in ("out_origin", "out_dir", "attenuation"):
        res[name] = canonical(res[name])
    return res


# ---- rt_accumulate -------------------------------------------------------------------------------------------------------------------------

def sky_sample(weight, sky_dir):
    """weight * sky(sky_dir) per channel: main.rs:54-56 in the reference's operation order, then Oracle B's mulv(thr, sky)."""
    with np.errstate(all="ignore"):
        w = [np.float64(x) for x in weight]
        if sky_dir is None:
            return w
        d = [np.float64(x) for x in sky_dir]
        inv = np.float64(1.0) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])      # unit_vector: v * (1 / length)
        t = np.float64(0.5) * (d[1] * inv + np.float64(1.0))
        sky = [np.float64(1.0) * (np.float64(1.0) - t) + np.float64(c) * t for c in (0.5, 0.7, 1.0)]
        return [w[c] * sky[c] for c in range(3)]


def accumulate(fix, pixel, weight, sky_dir=None, select=None):
    """rt_accumulate on a COPY of fix (u64 [..., 3]); returns it."""
    lib = oracle.load()
    out = np.array(fix, dtype=np.uint64, copy=True)
    flat = out.reshape(-1, 3)
    npix = flat.shape[0]
    for k in range(len(pixel)):
        if select is not None and select[k] == 0:
            continue
        if int(pixel[k]) >= npix:
            continue
        v = sky_sample(weight[k], None if sky_dir is None else sky_dir[k])
        for c in range(3):
            flat[int(pixel[k]), c] = np.uint64((int(flat[int(pixel[k]), c]) + int(lib.oracle_b_quantize(float(v[c])))) & MASK64)
    return out


# ---- the whole frame: the reference loop ---------------------------------------------------------------------------------------------------

def render(flat, ocam, width, height, spp, *, max_depth=50, seed=1, t_min=1e-4, sample_begin=0):
    """The wavefront loop path by path -> (fix u64 [H, W, 3], rays traced): camera ray, then up to max_depth times { closest hit; a miss
    adds quantize(throughput * sky) and ends the path; scatter; absorbed ends it; throughput *= attenuation }."""
    lib = oracle.load()
    scene = Scene(flat)
    fix = np.zeros((height, width, 3), dtype=np.uint64)
    rays = 0
    for pixel in range(width * height):
        acc = [0, 0, 0]
        for s in range(sample_begin, sample_begin + spp):
            o, d, event, _ = camera_path(ocam, width, height, seed, pixel, s)
            thr = [1.0, 1.0, 1.0]
            for _ in range(max_depth):
                rays += 1
                idx, _, p, nrm, front = fast_hit(scene, o, d, t_min)
                if idx < 0:
                    v = sky_sample(thr, d)
                    for c in range(3):
                        acc[c] += int(lib.oracle_b_quantize(float(v[c])))
                    break
                r = scatter_path(scene.flat[idx], seed, d, p, nrm, front, pixel, s, event)
                if r["status"] != SCATTERED:
                    break
                thr = [thr[c] * r["attenuation"][c] for c in range(3)]
                o, d, event = p, r["out_dir"], r["event"]
        fix[pixel // width, pixel % width] = [a & MASK64 for a in acc]
    return fix, rays


# ---- the step inputs the GPU tests use: hard by construction, checked by tests/test_wavefront_host.py ------------------------------------

SEED = 0x9E3779B97F4A7C15                 # both halves of the key in use
CW, CH = 37, 19                           # the frame of the camera cases
N_CASES = 257


def step_scene():
    """Five spheres, one per material variant: 0 Lambertian, 1 Metal fuzz 0.3, 2 Metal fuzz 0, 3 Dialectric ir 1.5, 4 Metal fuzz 1."""
    import rtiow_amd as rt
    flat = np.zeros(5, dtype=rt.SPHERE_DTYPE)
    for k, (kind, albedo, param) in enumerate([(LAMBERTIAN, (0.8, 0.3, 0.1), 0.0), (METAL, (0.7, 0.6, 0.5), 0.3), (METAL, (0.9, 0.9, 0.2), 0.0),
                                                (DIALECTRIC, (0.25, 0.5, 0.75), 1.5), (METAL, (0.4, 0.5, 0.6), 1.0)]):
        flat[k]["center"], flat[k]["radius"] = (3.0 * k - 6.0, 1.0, 0.0), 1.0
        flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = albedo, param, kind
    return flat


def _search(predicate, what):
    for pixel in range(1, 4000):
        if predicate(pixel):
            return pixel
    raise AssertionError(f"no pixel below 4000 gives {what}")


@functools.lru_cache(None)
def scatter_cases():
    """N_CASES scatter inputs over step_scene() and the reference's answer (computed once, read-only).  The first 14 are built to be each
    of the hard kinds; the rest are seeded random hits of every material, misses and bad indices among them."""
    flat = step_scene()
    rng = np.random.default_rng(18)
    n = N_CASES
    index = rng.integers(0, 5, n).astype(np.int32)
    dirs = rng.normal(size=(n, 3)) * rng.choice([1.0, 1e-3, 40.0], n)[:, None]
    normal = rng.normal(size=(n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    point = rng.uniform(-10.0, 10.0, (n, 3))
    front = rng.integers(0, 2, n).astype(np.uint8)
    pixel = rng.integers(0, 1 << 20, n).astype(np.uint32)
    sample = rng.integers(0, 64, n).astype(np.uint32)
    event = rng.integers(1, 40, n).astype(np.uint32)
    index[20::16] = -1                                                          # misses ...
    index[25::32] = np.array([-2, 5, -(2 ** 31), 2 ** 31 - 1, 6, -3, 100, -100], dtype=np.int64)[:len(index[25::32])].astype(np.int32)
    up, s5, e5 = (0.0, 1.0, 0.0), 5, 7
    path = lambda idx, d, nrm, fr, px, ev=e5: scatter_path(flat[idx], SEED, d, (1.0, 2.0, 3.0), nrm, fr, px, s5, ev)

    def put(k, idx, d, nrm, fr, px, ev=e5):
        index[k], dirs[k], normal[k], front[k], pixel[k], sample[k], event[k], point[k] = idx, d, nrm, fr, px, s5, ev, (1.0, 2.0, 3.0)

    down = (0.3, -1.0, 0.2)
    put(0, 0, down, up, 1, 11)                                                   # Lambertian, ordinary
    # Lambertian near zero: normal = minus the drawn unit vector, in the oracle's own arithmetic (v * (1 / sqrt(v.v)))
    tries, run = unit_sphere_run(SEED, 12, s5, e5)
    sp = np.array([u11(x) for x in run[-3:]], dtype=np.float64)
    uv = sp * (np.float64(1.0) / np.sqrt(sp[0] * sp[0] + sp[1] * sp[1] + sp[2] * sp[2]))
    put(1, 0, down, tuple(-uv), 1, 12)
    put(2, 1, down, up, 1, _search(lambda px: path(1, down, up, 1, px)["status"] == SCATTERED, "a scattering Metal"))
    graze = (1.0, -0.01, 0.0)
    put(3, 4, graze, up, 1, _search(lambda px: path(4, graze, up, 1, px)["status"] == ABSORBED, "an absorbing Metal"))
    put(4, 2, down, up, 1, 13)                                                   # Metal, fuzz 0
    put(5, 3, (0.05, -1.0, 0.02), up, 1, _search(lambda px: path(3, (0.05, -1.0, 0.02), up, 1, px)["mode"] == "refract", "a refraction"))
    shallow = (1.0, -0.05, 0.0)
    put(6, 3, shallow, up, 1, _search(lambda px: path(3, shallow, up, 1, px)["mode"] == "reflect", "a reflection by the draw"))
    put(7, 3, (1.0, -0.5, 0.0), up, 0, 14)                                       # back face, 63 degrees: total internal reflection
    px5 = _search(lambda px: unit_sphere_run(SEED, px, s5, e5)[0] >= 5, "five unit-sphere tries")
    put(8, 0, down, up, 1, px5)
    put(9, 1, down, up, 1, px5)
    index[10], index[11], index[12], index[13] = -1, -2, 5, 4
    want = scatter(flat, SEED, dirs, index, point, normal, front, pixel, sample, event)
    inputs = dict(dirs=dirs, index=index, point=point, normal=normal, front_face=front, pixel=pixel, sample=sample, event=event)
    for a in list(inputs.values()) + [v for v in want.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return flat, inputs, want


@functools.lru_cache(None)
def camera_cases():
    """N_CASES (pixel, sample) pairs of a CW x CH frame with a wide lens and the reference's rays: every pixel of the first rows, then
    seeded ones; sample indices up to 2^31."""
    import rtiow_amd as rt
    from rtiow_amd.scene import Camera
    cam = Camera((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, CW / CH, 0.5, 10.0)
    rng = np.random.default_rng(19)
    pixel = np.concatenate([np.arange(100), rng.integers(0, CW * CH, N_CASES - 100)]).astype(np.uint32)
    sample = np.concatenate([np.zeros(50), rng.integers(0, 1 << 31, N_CASES - 50)]).astype(np.uint32)
    pixel[0], pixel[1], pixel[2] = 0, CW * CH - 1, CW - 1                         # the corners
    want = camera_rays(oracle.camera_from_host(cam), CW, CH, SEED, pixel, sample)
    for a in [pixel, sample] + list(want.values()):
        a.setflags(write=False)
    return cam, pixel, sample, want
