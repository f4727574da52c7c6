"""CPU statement of the environment cube map in the lit path queue (include/rtiow_hip.h "environment") -- a test helper.

Composed from tests/lights_ref.py (bounce_lit: which sphere is a light, what a path adds there and that it ends; through it
tests/paths_ref.py: what a path that scatters does, and the queue) and tests/trace_ref.py (fast_hit: the closest hit, of the path's ray and
of the shadow ray) and restating none of them: here is only what the environment adds -- the lookup of a direction, the table of running
sums, the sample at a Lambertian hit and the shadow ray that decides it, and the DIRECT bit of the event word.  The arithmetic is IEEE
binary64 without fused multiply-add, left to right as dot writes it.  An environment is (texels f64 [6, N, N, 3], cdf f64 [6 N N] or None).
"""
import functools
import math

import numpy as np

import lights_ref as lr
import oracle
import paths_ref as pr
import wavefront_ref as wr
from trace_ref import Scene, fast_hit

DIRECT = 0x80000000                                # RT_PATH_EVENT_DIRECT
NO_DIRECT = 1                                      # RT_STEP_NO_DIRECT
OUTSIDE = 0xFFFFFFFF                               # a pixel outside every frame: such a path adds nothing
MASK64 = lr.MASK64
F = np.float64
PI = float(np.array([0x400921FB54442D18], dtype=np.uint64).view(np.float64)[0])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _row(c, size):
    x = ((c + F(1.0)) * F(0.5)) * F(size)
    return size - 1 if x >= size else (int(x) if x >= 0.0 else 0)          # a NaN fails both comparisons


def env_lookup(d, size):
    """The texel index a direction names, for any d, not normalised."""
    d = [F(x) for x in d]
    ax, m = 0, abs(d[0])
    if abs(d[1]) > m:
        ax, m = 1, abs(d[1])
    if abs(d[2]) > m:
        ax, m = 2, abs(d[2])
    f = 2 * ax + (1 if d[ax] < 0.0 else 0)
    with np.errstate(all="ignore"):
        a, b = [d[k] / m for k in range(3) if k != ax]
        return (f * size + _row(a, size)) * size + _row(b, size)


def texel_of(k, size):
    return k // (size * size), (k // size) % size, k % size


def environment_cdf(texels, size):
    """rt_environment_cdf: the running sums of mx / r^3 in index order."""
    t = np.asarray(texels, dtype=np.float64).reshape(-1, 3)
    assert len(t) == 6 * size * size
    s = F(2.0) / F(size)
    out = np.zeros(len(t), dtype=np.float64)
    run = F(0.0)
    with np.errstate(all="ignore"):
        for k in range(len(t)):
            _, i, j = texel_of(k, size)
            ac = (F(i) + F(0.5)) * s - F(1.0)
            bc = (F(j) + F(0.5)) * s - F(1.0)
            r2 = (F(1.0) + ac * ac) + bc * bc
            mx = F(0.0)
            for c in range(3):
                if t[k, c] > mx:                                                # NaN and negative channels count as 0
                    mx = t[k, c]
            run = run + mx / (r2 * np.sqrt(r2))
            out[k] = run
    return out


def samples(texels, cdf):
    """Whether a step samples this environment, and then its total: tot > 0.0 and tot < inf."""
    if cdf is None:
        return False, 0.0
    tot = float(cdf[-1])
    return (tot > 0.0 and tot < math.inf), tot


def sample_words(texels, cdf, size, words, n, weight):
    """Steps 2 .. 9 of the contract from the three words (x, y, z) of the sample's block -> dict(k, P, dv, ns, c: what the path adds
    per channel if the shadow ray is visible, shadow: a shadow ray is traced)."""
    t = np.asarray(texels, dtype=np.float64).reshape(-1, 3)
    tot = F(cdf[-1])
    x = F(wr.u01(int(words[0]))) * tot
    lo, hi = 0, len(cdf) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if cdf[mid] > x:
            hi = mid
        else:
            lo = mid + 1
    k = lo
    with np.errstate(all="ignore"):
        P = (F(cdf[k]) - (F(cdf[k - 1]) if k else F(0.0))) / tot
    out = dict(k=k, P=float(P), dv=None, ns=None, c=None, shadow=False)
    if not P > 0.0:
        return out
    f, i, j = texel_of(k, size)
    s = F(2.0) / F(size)
    a = (F(i) + F(wr.u01(int(words[1])))) * s - F(1.0)
    b = (F(j) + F(wr.u01(int(words[2])))) * s - F(1.0)
    dv = [a, b]
    dv.insert(f >> 1, F(-1.0) if f & 1 else F(1.0))
    with np.errstate(all="ignore"):
        ns = dot([F(v) for v in n], dv)
        dd = dot(dv, dv)
        out["dv"], out["ns"] = [float(v) for v in dv], float(ns)
        if not ns > 0.0:
            return out
        w = (ns * (s * s)) / ((F(PI) * P) * (dd * dd))
        out["c"] = [float((F(weight[c]) * t[k, c]) * w) for c in range(3)]
    out["shadow"] = True
    return out


def sample_env(scene, seed, env, size, pixel, sample, ev_in, p, n, weight, t_min=1e-4):
    """Steps 1 .. 10 for one Lambertian hit: sample_words on the block (pixel, sample, ev_in, 1), and `visible`: the closest-hit scan of
    the shadow ray (p, dv) finds no sphere."""
    texels, cdf = env
    b = oracle.philox((int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF, int(ev_in) & 0xFFFFFFFF, 1), wr.key_of(seed))
    out = sample_words(texels, cdf, size, b[:3], n, weight)
    out["visible"] = out["shadow"] and fast_hit(scene, [float(a) for a in p], out["dv"], t_min)[0] < 0
    return out


def sample_many(texels, cdf, size, words, n, weight=(1.0, 1.0, 1.0)):
    """sample_words for an array of words u32 [m, 3], in numpy (a table without NaNs) -> (k [m], c [m, 3] with 0 where nothing follows)."""
    t = np.asarray(texels, dtype=np.float64).reshape(-1, 3)
    cdf = np.asarray(cdf, dtype=np.float64)
    w = np.asarray(words, dtype=np.float64) * (1.0 / 4294967296.0)
    tot = cdf[-1]
    k = np.minimum(np.searchsorted(cdf, w[:, 0] * tot, side="right"), len(cdf) - 1)      # the first entry above x
    P = (cdf[k] - np.where(k > 0, cdf[k - 1], 0.0)) / tot
    f, i, j = k // (size * size), (k // size) % size, k % size
    s = F(2.0) / F(size)
    a, b = (i + w[:, 1]) * s - 1.0, (j + w[:, 2]) * s - 1.0
    on = np.where(f & 1, -1.0, 1.0)
    ax = f >> 1
    dv = np.stack([np.where(ax == 0, on, a), np.where(ax == 1, on, np.where(ax == 0, a, b)), np.where(ax == 2, on, b)], axis=1)
    ns = n[0] * dv[:, 0] + n[1] * dv[:, 1] + n[2] * dv[:, 2]
    dd = dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2]
    ok = (P > 0.0) & (ns > 0.0)
    with np.errstate(all="ignore"):
        wgt = (ns * (s * s)) / ((PI * P) * (dd * dd))
    c = (np.asarray(weight, dtype=np.float64)[None, :] * t[k]) * wgt[:, None]
    c[~ok] = 0.0
    return k, c


def quadrature(texels, size, n, sub=16):
    """The integral of L cos(theta) / pi over the sphere of directions at an unoccluded point with normal n, by the midpoint rule on
    sub x sub cells per texel: a direction (.., a, b, ..) of a face has d omega = da db / r^3 and cos(theta) = dot(n, dv) / r."""
    t = np.asarray(texels, dtype=np.float64).reshape(6, size, size, 3)
    h = 2.0 / (size * sub)
    centre = (np.arange(size * sub) + 0.5) * h - 1.0
    a, b = np.meshgrid(centre, centre, indexing="ij")
    total = np.zeros(3)
    for f in range(6):
        on = np.full_like(a, -1.0 if f & 1 else 1.0)
        dv = {0: (on, a, b), 1: (a, on, b), 2: (a, b, on)}[f >> 1]
        ns = np.maximum(n[0] * dv[0] + n[1] * dv[1] + n[2] * dv[2], 0.0)
        r2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]
        g = ns / (math.pi * r2 * r2) * (h * h)
        total += (np.repeat(np.repeat(t[f], sub, axis=0), sub, axis=1) * g[..., None]).sum(axis=(0, 1))
    return total


def bounce_env(scene, queue, seed, npix, light, env, size, no_direct=False, t_min=1e-4):
    """One environment bounce of every path of `queue` -> (the new state per INPUT slot, the fate of each -- lights_ref.bounce_lit's --,
    the additions u64 [npix, 3], per slot the environment sample or None)."""
    if not isinstance(scene, Scene):
        scene = Scene(scene)
    texels, cdf = env
    flat_texels = np.asarray(texels, dtype=np.float64).reshape(-1, 3)
    lib = oracle.load()
    n = len(queue["pixel"])
    was_direct = (queue["event"] & np.uint32(DIRECT)) != 0
    masked = {f: np.array(queue[f], copy=True) for f in pr.FIELDS}
    masked["event"] &= np.uint32(DIRECT ^ 0xFFFFFFFF)                             # masked off before any Philox use
    hits = [fast_hit(scene, queue["origin"][k].tolist(), queue["dir"][k].tolist(), t_min) for k in range(n)]
    missed = [k for k in range(n) if hits[k][0] < 0]
    for k in missed:
        masked["pixel"][k] = OUTSIDE                                              # the sky of `light` is not used: the miss is added below
    new, fates, adds = lr.bounce_lit(scene, masked, seed, npix, light, t_min)

    def add(pixel, v):
        for c in range(3):
            adds[pixel, c] = np.uint64((int(adds[pixel, c]) + int(lib.oracle_b_quantize(float(v[c])))) & MASK64)

    for k in missed:
        assert fates[k] == "miss"
        pixel = int(queue["pixel"][k])
        if pixel < npix and not was_direct[k]:                                    # (DIRECT: the previous hit's shadow ray counted the environment)
            e = flat_texels[env_lookup(queue["dir"][k].tolist(), size)]
            with np.errstate(all="ignore"):
                add(pixel, [F(queue["throughput"][k][c]) * e[c] for c in range(3)])
    got = [None] * n
    if samples(texels, cdf)[0] and not no_direct:
        for k in range(n):
            if fates[k] != "lambertian":
                continue
            idx, _, p, nrm, _ = hits[k]
            pixel = int(queue["pixel"][k])
            s = sample_env(scene, seed, env, size, pixel, int(queue["sample"][k]), int(masked["event"][k]), p, nrm, new["throughput"][k].tolist(), t_min)
            got[k] = s
            new["event"][k] |= np.uint32(DIRECT)                                  # decided before sampling
            if s["visible"] and pixel < npix:
                add(pixel, s["c"])
    return new, fates, adds, got


def step_env(scene, queue, seed, npix, light, env, size, no_direct=False, t_min=1e-4):
    """rt_paths_step_env_device -> (the out queue, the additions u64 [npix, 3], the live count of `queue`, the shadow rays traced)."""
    new, fates, adds, got = bounce_env(scene, queue, seed, npix, light, env, size, no_direct, t_min)
    return pr.compact(new, fates, adds) + (sum(1 for s in got if s is not None and s["shadow"]),)


def render_env(flat, ocam, width, height, spp, light, env, size, *, max_depth=50, seed=1, t_min=1e-4, sample_begin=0, batch=1 << 20):
    """rt_render_wavefront_env: paths_ref.frame with step_env, the LAST step of each batch with NO_DIRECT -> (fix u64 [H, W, 3], rays
    traced, shadow rays traced)."""
    scene, npix = Scene(flat), width * height
    fix, rays, shadow = pr.frame(lambda first, n: pr.begin(ocam, width, height, seed, spp, sample_begin, first, n),
                                 lambda q, last: step_env(scene, q, seed, npix, light, env, size, last, t_min), npix, npix * spp, max_depth, batch)
    return fix.reshape(height, width, 3), rays, shadow


# ---- the hand-built environment queue of the GPU tests: hard by construction, checked by tests/test_env_host.py -------------------------------

SEED, HAND_N, HAND_NPIX = lr.SEED, lr.HAND_N, lr.HAND_NPIX
NAN = float("nan")
# one more sphere over lights_ref.hand_queue()'s fourteen: an occluder straight above the Lambertian sphere 0 and above every ray's origin
EXTRA = [((-6.0, 7.0, 0.0), 1.0, wr.METAL, (0.9, 0.9, 0.9), 0.0)]
SUN = (2, 6, 5)                                    # the texel of 400 of the size-8 map: face +y, seen from sphere 0 past the occluder
# slot -> what it was rebuilt to do (test_env_host.py checks each with the statement); every slot below 63
CASES = {1: "visible", 19: "occluded", 25: "below_horizon", 31: "outside_frame", 37: "sun", 43: "nan_channel"}
DIRECT_SLOTS = {6: "light", 18: "miss", 2: "metal", 3: "glass", 17: "lambertian"}          # these carry the DIRECT bit on entry
PLAIN_MISS = 24                                    # a miss without the bit, inside the frame
ALL_WAVE = range(320, 384)                         # every lane a shadow ray
NAN_TEXEL = (2, 2, 2)                              # (NaN, 0.5, -1): chosen by its green channel; the other two add 0
ZERO_TEXELS = ((0, 3, 3), (2, 1, 6), (5, 7, 6))    # weight 0 between positive ones: never chosen


@functools.lru_cache(None)
def hand_env(size):
    """(texels [6, size, size, 3], cdf) of the hand queue's map at `size`: seeded texels in [0, 1); at size 8 the sun, the NaN texel and
    the zero texels above.  Read-only."""
    rng = np.random.default_rng(31 + size)
    texels = rng.uniform(0.0, 1.0, (6, size, size, 3))
    if size == 8:
        texels[SUN] = (400.0, 300.0, 200.0)
        texels[NAN_TEXEL] = (NAN, 0.5, -1.0)
        for z in ZERO_TEXELS:
            texels[z] = (0.0, -0.0, 0.0)
    cdf = environment_cdf(texels, size)
    texels.setflags(write=False)
    cdf.setflags(write=False)
    return texels, cdf


def special_envs(size=8):
    """Environments that sample at an edge or not at all: name -> (texels, cdf)."""
    n = 6 * size * size
    first, last, zero = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    first[0], last[-1] = (0.5, 2.0, 1.0), (1.0, 0.25, 3.0)
    shape = (6, size, size, 3)
    out = {"first": (first.reshape(shape), environment_cdf(first, size)), "last": (last.reshape(shape), environment_cdf(last, size)),
           "zero": (zero.reshape(shape), environment_cdf(zero, size)),
           "nan_table": (np.array(hand_env(size)[0]), np.full(n, NAN)), "inf_table": (np.array(hand_env(size)[0]), np.full(n, math.inf))}
    return out


def _matches(what, s):
    if what in ("visible", "outside_frame"):
        return s["visible"] and s["k"] != (SUN[0] * 8 + SUN[1]) * 8 + SUN[2]
    if what == "occluded":
        return s["shadow"] and not s["visible"]
    if what == "below_horizon":
        return s["ns"] is not None and s["ns"] <= 0.0
    if what == "sun":
        return s["visible"] and s["k"] == (SUN[0] * 8 + SUN[1]) * 8 + SUN[2]
    if what == "nan_channel":
        return s["visible"] and s["k"] == (NAN_TEXEL[0] * 8 + NAN_TEXEL[1]) * 8 + NAN_TEXEL[2]
    if what == "shadow":
        return s["shadow"]
    raise KeyError(what)


@functools.lru_cache(None)
def hand_queue():
    """(flat, queue, light): lights_ref.hand_queue()'s scene with EXTRA above it (no path of the original comes near: its rays start at
    y = 5 and below, or leave upwards around x = 0), its 513 paths with the slots of CASES, DIRECT_SLOTS and one wave of the second
    workgroup rebuilt.  Every rebuilt Lambertian path is the original's ray onto sphere 0 with the sample searched -- with the statement
    alone, under hand_env(8) -- so that its environment sample is the named case.  Read-only."""
    import rtiow_amd as rt
    base_flat, base_q, light = lr.hand_queue()
    flat = np.zeros(len(base_flat) + len(EXTRA), dtype=rt.SPHERE_DTYPE)
    flat[:len(base_flat)] = base_flat
    for k, (centre, radius, kind, albedo, param) in enumerate(EXTRA, start=len(base_flat)):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = centre, radius, albedo, param, kind
    emission = np.concatenate([light.emission, np.zeros((len(EXTRA), 3))])
    light = lr.Light(light.sky_bottom, light.sky_top, emission)
    scene = Scene(flat)
    env = hand_env(8)
    q = {f: np.array(base_q[f], copy=True) for f in pr.FIELDS}
    rng = np.random.default_rng(37)
    jit = lambda: rng.uniform(-0.2, 0.2)

    def lambertian(k, what, pixel=None):
        """Slot k: a ray down onto sphere 0 whose environment sample is `what`, by search over samples."""
        q["origin"][k], q["dir"][k] = (-6.0 + jit(), 5.0, jit()), (0.1 * jit(), -1.0, 0.1 * jit())
        q["pixel"][k] = k % HAND_NPIX if pixel is None else pixel
        probe = {f: q[f][[k]].copy() for f in pr.FIELDS}
        for sample in range(20000):
            probe["sample"][0] = sample
            _, fates, _, got = bounce_env(scene, probe, SEED, HAND_NPIX, light, env, 8)
            assert fates[0] == "lambertian"
            if _matches(what, got[0]):
                q["sample"][k] = sample
                return
        raise AssertionError(f"no sample below 20000 makes slot {k} the case {what}")

    for k, what in CASES.items():
        lambertian(k, what, HAND_NPIX + 5 if what == "outside_frame" else None)
    for k in ALL_WAVE:
        lambertian(k, "occluded" if k % 8 == 0 else "shadow")
    q["pixel"][PLAIN_MISS], q["pixel"][18] = 21, 22                                     # (inside the frame whatever the draw was)
    for k in DIRECT_SLOTS:
        q["event"][k] |= np.uint32(DIRECT)
    for a in list(q.values()) + [emission]:
        a.setflags(write=False)
    return flat, q, light


@functools.lru_cache(None)
def hand_step(count, size=8, sampled=True, no_direct=False):
    """The statement's answer for the first `count` paths of hand_queue() under hand_env(size) (computed once per setting, read-only)."""
    flat, q, light = hand_queue()
    texels, cdf = hand_env(size)
    out, adds, live, shadow = step_env(flat, pr.prefix(q, count), SEED, HAND_NPIX, light, (texels, cdf if sampled else None), size, no_direct)
    for a in list(out.values()) + [adds]:
        a.setflags(write=False)
    return out, adds, live, shadow


def degenerate_queue():
    """(queue, the directions' names): paths that all miss (origins far above the scene) whose directions have equal components, +-0,
    zero, infinite and NaN entries."""
    inf = math.inf
    dirs = [(1.0, 1.0, 1.0), (-1.0, -1.0, -1.0), (1.0, -1.0, 1.0), (0.0, 2.0, 2.0), (2.0, 0.0, -2.0), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0),
            (0.0, -0.0, 1.0), (inf, 1.0, 1.0), (-inf, inf, 0.0), (1.0, inf, -inf), (inf, inf, inf), (NAN, 1.0, 0.5), (1.0, NAN, 0.5), (0.5, 1.0, NAN),
            (NAN, NAN, NAN), (0.0, NAN, 0.0), (-1.0, 1.0, 0.0), (0.0, -3.0, 3.0), (1e-300, 1e300, 0.0), (1e300, 1e300, 1e-300), (-2.0, 1.0, -2.0)]
    q = pr.empty(len(dirs))
    q["pixel"][:] = np.arange(len(dirs))
    q["sample"][:] = 3
    q["event"][:] = 5
    q["origin"][:] = (0.0, 5000.0, 0.0)
    q["dir"][:] = dirs
    q["throughput"][:] = (0.5, 0.25, 1.0)
    return q, dirs


# ---- the small scene of the expectation and variance tests ---------------------------------------------------------------------------------

STAT_W, STAT_H, STAT_SPP, STAT_DEPTH = 16, 12, 64, 8
STAT_SEEDS = tuple(range(1, 17))
STAT_ENV_SIZE = 8


def stat_scene():
    """(flat, light): a Lambertian ground, a Metal, a Dialectric and a Lambertian occluder; no sphere emits."""
    import rtiow_amd as rt
    spheres = [((0.0, -1000.0, 0.0), 1000.0, wr.LAMBERTIAN, (0.6, 0.6, 0.6), 0.0),
               ((-1.5, 0.5, 0.0), 0.5, wr.METAL, (0.8, 0.8, 0.8), 0.0),
               ((1.5, 0.5, 0.0), 0.5, wr.DIALECTRIC, (1.0, 1.0, 1.0), 1.5),
               ((0.3, 1.4, 0.2), 0.35, wr.LAMBERTIAN, (0.7, 0.3, 0.3), 0.0)]
    flat = np.zeros(len(spheres), dtype=rt.SPHERE_DTYPE)
    for k, (centre, radius, kind, albedo, param) in enumerate(spheres):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = centre, radius, albedo, param, kind
    return flat, lr.Light((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None)


def stat_environment():
    """rtiow_amd.Environment.sun_sky at STAT_ENV_SIZE: a dim sky and a sun high behind the camera, out of its view."""
    import rtiow_amd as rt
    return rt.Environment.sun_sky(STAT_ENV_SIZE, sun_dir=(0.3, 0.8, 0.6), sun_radiance=(400.0, 360.0, 300.0), cos_radius=0.99,
                                  bottom=(0.05, 0.05, 0.05), top=(0.02, 0.03, 0.06))


def stat_camera():
    from rtiow_amd.scene import Camera
    return Camera((0.0, 2.0, 6.0), (0.0, 0.7, 0.0), (0.0, 1.0, 0.0), 40.0, STAT_W / STAT_H, 0.0, 6.0)


def stat_numbers(frames_sampled, frames_plain):
    """From the 16 sampled and the 16 unsampled frames (u64 [H, W, 3], one per seed of STAT_SEEDS) -> (the mean of the per-seed
    differences of the frame-total energy, its standard error, the per-pixel variance over the seeds summed over the frame for the
    sampled and for the unsampled frames)."""
    a = np.array([f.astype(np.float64) for f in frames_sampled]) / 4294967296.0
    b = np.array([f.astype(np.float64) for f in frames_plain]) / 4294967296.0
    diff = a.sum(axis=(1, 2, 3)) - b.sum(axis=(1, 2, 3))
    stderr = float(diff.std(ddof=1) / math.sqrt(len(diff)))
    return float(diff.mean()), stderr, float(a.var(axis=0, ddof=1).sum()), float(b.var(axis=0, ddof=1).sum())


@functools.lru_cache(None)
def stat_reference():
    """The statement's 16 sampled and 16 unsampled frames of the stat scene (a minute of CPU) -> (frames sampled, frames unsampled)."""
    flat, light = stat_scene()
    ocam = oracle.camera_from_host(stat_camera())
    texels = stat_environment().table()
    cdf = environment_cdf(texels, STAT_ENV_SIZE)
    frames = {True: [], False: []}
    for seed in STAT_SEEDS:
        for sampled in (True, False):
            fix, _, _ = render_env(flat, ocam, STAT_W, STAT_H, STAT_SPP, light, (texels, cdf if sampled else None), STAT_ENV_SIZE,
                                   max_depth=STAT_DEPTH, seed=seed)
            frames[sampled].append(fix)
    return frames[True], frames[False]


# stat_numbers(*stat_reference()), recorded: what the GPU's 32 frames, equal to the statement's bit for bit, must give again
STAT_EXPECTED = (227.40128127003845, 2164.3861135720113, 934785.0282896878, 14769010.702740405)
