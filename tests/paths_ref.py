"""CPU statement of the device path queue (include/rtiow_hip.h "path queue") -- a test helper.

Composed from tests/wavefront_ref.py (camera_path, scatter_path, sky_sample) and tests/trace_ref.py (fast_hit: HittableList::hit with
t_max = +inf and the winner's record) and restating neither: here is only the queue -- which item a slot holds, what a bounce does with a
path, and that the survivors keep their order.  A queue is a dict of numpy arrays: pixel, sample, event u32 [n], origin, dir, throughput
f64 [n, 3]; its length is the live count.
"""
import functools

import numpy as np

import oracle
import wavefront_ref as wr
from trace_ref import Scene, canonical, fast_hit

FIELDS = ("pixel", "sample", "event", "origin", "dir", "throughput")
MASK64 = (1 << 64) - 1
FATES = ("miss", "absorbed", "lambertian", "metal", "refract", "reflect", "tir")
SURVIVES = FATES[2:]                               # the fates of a path that goes on: every step keeps these and no other


def empty(n):
    q = {f: np.zeros(n, dtype=np.uint32) for f in ("pixel", "sample", "event")}
    q.update({f: np.zeros((n, 3)) for f in ("origin", "dir", "throughput")})
    return q


def begin(ocam, width, height, seed, spp, sample_begin, first_item, n):
    """rt_paths_begin_device: slot k holds item first_item + k, pixel-major."""
    q = empty(n)
    for k in range(n):
        item = first_item + k
        pixel, sample = item // spp, sample_begin + item % spp
        o, d, event, _ = wr.camera_path(ocam, width, height, seed, pixel, sample)
        q["pixel"][k], q["sample"][k], q["event"][k], q["origin"][k], q["dir"][k], q["throughput"][k] = pixel, sample, event, o, d, (1.0, 1.0, 1.0)
    q["origin"], q["dir"] = canonical(q["origin"]), canonical(q["dir"])
    return q


def bounce(scene, queue, seed, npix, t_min=1e-4):
    """One bounce of every path of `queue` -> (the new state per INPUT slot, the fate of each, the additions u64 [npix, 3])."""
    lib = oracle.load()
    if not isinstance(scene, Scene):
        scene = Scene(scene)
    n = len(queue["pixel"])
    new, fates = empty(n), []
    adds = np.zeros((npix, 3), dtype=np.uint64)
    for k in range(n):
        o, d, thr = queue["origin"][k].tolist(), queue["dir"][k].tolist(), queue["throughput"][k].tolist()
        pixel, sample, event = int(queue["pixel"][k]), int(queue["sample"][k]), int(queue["event"][k])
        idx, _, p, nrm, front = fast_hit(scene, o, d, t_min)
        if idx < 0:
            if pixel < npix:
                v = wr.sky_sample(thr, d)
                for c in range(3):
                    adds[pixel, c] = np.uint64((int(adds[pixel, c]) + int(lib.oracle_b_quantize(float(v[c])))) & MASK64)
            fates.append("miss")
            continue
        r = wr.scatter_path(scene.flat[idx], seed, d, p, nrm, front, pixel, sample, event)
        if r["status"] != wr.SCATTERED:
            fates.append("absorbed")
            continue
        kind = int(scene.flat[idx]["kind"])
        fates.append(r["mode"] if kind == wr.DIALECTRIC else ("lambertian" if kind == wr.LAMBERTIAN else "metal"))
        with np.errstate(all="ignore"):
            new["throughput"][k] = [np.float64(thr[c]) * np.float64(r["attenuation"][c]) for c in range(3)]     # one multiply per channel
        new["pixel"][k], new["sample"][k], new["event"][k], new["origin"][k], new["dir"][k] = pixel, sample, r["event"], p, r["out_dir"]
    return new, fates, adds


def compact(new, fates, adds):
    """The tail of every step, from a bounce's answer: the survivors in the order they had -> (the out queue, the additions u64 [npix, 3],
    the live count of the queue that went in)."""
    keep = np.array([f in SURVIVES for f in fates], dtype=bool)
    out = {f: new[f][keep] for f in FIELDS}
    for f in ("origin", "dir", "throughput"):
        out[f] = canonical(out[f])
    return out, adds, len(fates)


def step(scene, queue, seed, npix, t_min=1e-4):
    """rt_paths_step_device -> compact's three."""
    return compact(*bounce(scene, queue, seed, npix, t_min))


def prefix(queue, n):
    return {f: queue[f][:n] for f in FIELDS}


def frame(begin, step, npix, total, max_depth, batch):
    """The loop of every frame form over `total` items: batches of `batch`, per batch q = begin(first_item, n) and then max_depth times
    step(q, last: this is the batch's last step), which answers (the out queue, the additions, the live count[, the shadow rays traced])
    -> (fix u64 [npix, 3], rays traced, shadow rays traced)."""
    fix = np.zeros((npix, 3), dtype=np.uint64)
    rays = shadow = 0
    for first in range(0, total, batch):
        q = begin(first, min(batch, total - first))
        for depth in range(max_depth):
            q, adds, live, *sh = step(q, depth + 1 == max_depth)
            fix += adds                                                         # (u64: wraps as the device's adds do)
            rays += live
            shadow += sum(sh)
    return fix, rays, shadow


def render(flat, ocam, width, height, spp, *, max_depth=50, seed=1, t_min=1e-4, sample_begin=0, batch=1 << 20):
    """rt_render_wavefront: frame() over begin and step -> (fix u64 [H, W, 3], rays traced)."""
    scene, npix = Scene(flat), width * height
    fix, rays, _ = frame(lambda first, n: begin(ocam, width, height, seed, spp, sample_begin, first, n),
                         lambda q, last: step(scene, q, seed, npix, t_min), npix, npix * spp, max_depth, batch)
    return fix.reshape(height, width, 3), rays


# ---- the hand-built step queue of the GPU tests: hard by construction, checked by tests/test_paths_host.py -------------------------------

SEED = wr.SEED
HAND_N = 513                              # two workgroups of 256 slots and one slot
HAND_NPIX = 1000
SENTINEL_F64, SENTINEL_U32 = wr.F64_SENTINEL, 0xEEEEEEEE


@functools.lru_cache(None)
def hand_queue():
    """(flat, queue of HAND_N paths over wavefront_ref.step_scene(), the fates the reference gives them).  By waves of 64 slots: wave 0
    holds one path of every fate with a survivor in its last slot, wave 1 (its first slot a survivor) only survivors, wave 2 none, wave 3
    a seeded mix, slots 256 .. 511 -- the second workgroup -- only misses, slot 512 a survivor.  Read-only."""
    flat = wr.step_scene()
    scene = Scene(flat)
    rng = np.random.default_rng(19)
    q = empty(HAND_N)
    q["pixel"][:] = rng.integers(0, HAND_NPIX, HAND_N)
    q["sample"][:] = rng.integers(0, 64, HAND_N)
    q["event"][:] = rng.integers(1, 40, HAND_N)
    q["throughput"][:] = rng.uniform(0.05, 1.0, (HAND_N, 3))
    jit = lambda: rng.uniform(-0.2, 0.2)
    # the rays by what they are built to do (sphere k of step_scene() sits at x = 3 k - 6, y = 1, radius 1)
    down = lambda x: ((x + jit(), 5.0, jit()), (0.1 * jit(), -1.0, 0.1 * jit()))
    kinds = {
        "miss": lambda: ((jit(), 5.0, jit()), (jit(), 1.0, jit())),                     # upwards, above every sphere
        "lambertian": lambda: down(-6.0),
        "metal0": lambda: down(0.0),                                                    # fuzz 0: always scatters
        "glass": lambda: down(3.0),                                                     # front face: refracts or reflects by the draw
        "tir": lambda: ((3.9, 1.0, 0.0), (0.0, 1.0, 0.0)),                              # from inside, 64 degrees: no draw
    }

    def put(k, kind):
        q["origin"][k], q["dir"][k] = kinds[kind]()

    survivors = ("lambertian", "metal0", "glass", "tir")
    for k in range(HAND_N):
        if k < 64:
            put(k, ("miss", "lambertian", "metal0", "glass", "tir", "lambertian")[k % 6])
        elif k < 128:
            put(k, survivors[k % 4])
        elif k < 192 or 256 <= k < 512:
            put(k, "miss")
        elif k < 256:
            put(k, ("miss", "lambertian", "miss", "glass", "metal0", "miss")[int(rng.integers(0, 6))])
        else:
            put(k, "lambertian")
    put(63, "glass")
    put(64, "metal0")
    # paths that a fuzzy Metal absorbs (sphere 4, fuzz 1, at x = 6): a grazing ray; the pixel is searched so that the drawn vector points inwards
    graze_o, graze_d = (4.5, 1.0 + 0.995, 0.0), (1.0, 0.0, 0.0)
    for k in (5, 130, 140):
        q["origin"][k], q["dir"][k] = graze_o, graze_d
    # a miss outside the frame adds nothing
    q["pixel"][0], q["pixel"][128] = HAND_NPIX + 7, 0xFFFFFFF0
    probe = {f: q[f][[5]].copy() for f in FIELDS}
    for pixel in range(1, 4000):
        probe["pixel"][0] = pixel
        if bounce(scene, probe, SEED, HAND_NPIX)[1][0] == "absorbed":
            for k in (5, 130, 140):
                q["pixel"][k], q["sample"][k], q["event"][k] = pixel, q["sample"][5], q["event"][5]
            break
    else:
        raise AssertionError("no pixel below 4000 makes the grazing Metal ray absorb")
    _, fates, _ = bounce(scene, q, SEED, HAND_NPIX)
    for a in q.values():
        a.setflags(write=False)
    return flat, q, tuple(fates)


@functools.lru_cache(None)
def hand_step(count):
    """The reference's answer for the first `count` paths of hand_queue() (computed once per count, read-only)."""
    flat, q, _ = hand_queue()
    out, adds, live = step(flat, prefix(q, count), SEED, HAND_NPIX)
    for a in list(out.values()) + [adds]:
        a.setflags(write=False)
    return out, adds, live
