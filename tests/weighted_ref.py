"""CPU statement of direct lighting with a weighted choice of the light in the lit path queue (include/rtiow_hip.h "direct lighting with a
weighted choice of the light") -- a test helper.

Composed from tests/cone_ref.py (steps 2 .. 9 and 11 of the cone sample: sample_light_cone on the one-entry list of the chosen light) and
tests/nee_ref.py (the DIRECT bit, the face a path that carries it does not count again, which paths sample), restating neither: here are
only the two walks that choose the light -- steps 1a, 1b and 1c --, the weight of step 10', and nee_ref's loop with that sampler.  The
arithmetic is IEEE binary64 without fused multiply-add, in exactly the order the contract writes.
"""
import functools

import numpy as np

import cone_ref as cr
import lights_ref as lr
import nee_ref as nr
import oracle
import paths_ref as pr
import wavefront_ref as wr
from trace_ref import Scene, fast_hit

CONE = cr.CONE                                     # RT_DIRECT_CONE
WEIGHTED = 8                                       # RT_DIRECT_WEIGHTED
FLAGS = WEIGHTED | CONE                            # the one legal value that carries it: 10
DIRECT, MASK64 = nr.DIRECT, nr.MASK64
F = np.float64


def choice_draw(word):
    """The draw of step 1c from word x of block 0 (a function of its own so that a test can force the draw no word gives: 1.0)."""
    return wr.u01(word)


def max2(a, b):
    """a > b ? a : b: a NaN in `a` is dropped, a NaN in `b` is taken."""
    return a if a > b else b


def importance(scene, light, s, p):
    """Step 1a for the list entry that names sphere s, at the hit point p -> imp (np.float64)."""
    s = int(s)
    if s < 0 or s >= scene.n or light.emission is None or s >= len(light.emission):
        return F(0.0)
    with np.errstate(all="ignore"):
        c, radius = scene.flat[s]["center"], F(scene.flat[s]["radius"])
        r2 = radius * radius                                                          # as the upload builds the geometry table
        wv = [F(c[k]) - F(p[k]) for k in range(3)]
        d2 = (wv[0] * wv[0] + wv[1] * wv[1]) + wv[2] * wv[2]
        e = [F(x) for x in light.emission[s]]
        em = max2(max2(e[0], e[1]), e[2])
        v = (r2 / d2) * em
        return v if (d2 > r2 and v > 0.0) else F(0.0)                                 # a NaN fails either test


def choose_light(scene, light, lights, p, word):
    """Steps 1a .. 1c -> (j or None when !(tot > 0), tot, the list of imp_i, fallback: no i qualified).  The second walk recomputes imp_i
    with the same expressions on the same operands, so it reads the first walk's values."""
    imps = [importance(scene, light, s, p) for s in lights]                           # 1a
    tot = F(0.0)
    with np.errstate(all="ignore"):
        for v in imps:                                                                # 1b
            if v > 0.0:
                tot = tot + v
        if not tot > 0.0:
            return None, tot, imps, False
        x = F(choice_draw(word)) * tot                                                # 1c
        acc, last = F(0.0), None
        for i, v in enumerate(imps):
            if v > 0.0:
                acc = acc + v
                last = i
                if x < acc:
                    return i, tot, imps, False
    return last, tot, imps, True


def sample_light_weighted(scene, seed, light, lights, pixel, sample, ev_in, p, n, weight, t_min=1e-4):
    """Steps 1a .. 1c, cone_ref's steps 2 .. 9 and 11 for li, and 10' for one Lambertian hit -> cone_ref.sample_light_cone's dict for the
    chosen light with j, li and c the weighted step's, and tot, imp (the list), fallback."""
    key = wr.key_of(seed)
    b0 = oracle.philox((int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF, int(ev_in) & 0xFFFFFFFF, 1), key)
    j, tot, imps, fallback = choose_light(scene, light, lights, p, b0[0])
    if j is None:
        return dict(j=None, li=None, tries=0, d2=None, r2=None, k=None, wx=None, ns=None, shadow=False, visible=False, front=None, c=None,
                    word=int(b0[0]), tot=float(tot), imp=[float(v) for v in imps], fallback=False)
    li = int(lights[j])
    # the cone sample of li: with a one-entry list word x chooses entry 0 whatever it is; words y, z, w and the later blocks are the same
    out = cr.sample_light_cone(scene, seed, light, (li,), pixel, sample, ev_in, p, n, weight, t_min)
    assert out["li"] == li and out["word"] == int(b0[0])
    out.update(j=j, tot=float(tot), imp=[float(v) for v in imps], fallback=fallback)
    if out["c"] is not None:
        with np.errstate(all="ignore"):
            wgt = ((F(2.0) * F(out["k"])) * F(out["ns"])) * (tot / imps[j])           # 10'
            out["c"] = [float((F(weight[k]) * F(light.emission[li][k])) * wgt) for k in range(3)]
    return out


def bounce_weighted(scene, queue, seed, npix, light, lights, no_direct=False, t_min=1e-4):
    """nee_ref.bounce_direct with sample_light_weighted."""
    return nr.bounce_direct(scene, queue, seed, npix, light, lights, sample_light_weighted, no_direct, t_min)


def step_weighted(scene, queue, seed, npix, light, lights, no_direct=False, t_min=1e-4):
    """nee_ref.step_direct with sample_light_weighted (direct->flags = 10)."""
    return nr.step_direct(scene, queue, seed, npix, light, lights, sample_light_weighted, no_direct, t_min)


def render_weighted(flat, ocam, width, height, spp, light, **frame):
    """rt_render_wavefront_nee_sampled with direct_flags = 10: nee_ref.render_direct (whose keywords `frame` holds) with sample_light_weighted."""
    return nr.render_direct(flat, ocam, width, height, spp, light, sample_light_weighted, **frame)


def weighted_sample_bound(emission=None, lights=None):
    """The largest value one sample can add in one channel under the weighted choice, whatever the geometry, per unit of throughput: a
    light hit adds throughput * e; a light sample adds (throughput * albedo) * e_j * 2 k ns tot / imp_j with albedo <= 1, ns <= 1,
    k = q / (1 + cm) <= q = r2 / d2 and e_j / max(e_j) <= 1 per channel, so e_j * 2 k / imp_j <= 2 and the sample adds at most
    2 tot <= 2 sum_i (r2_i / d2_i) max(e_i) < 2 sum_i max(e_i), the sum over the list's entries (a positive imp_i has d2 > r2)."""
    if emission is None:
        emission = many_light_scene()[1].emission
    e = np.array(emission, dtype=np.float64)
    if lights is None:
        lights = nr.light_list(e)
    total = sum(max(0.0, float(np.nanmax(e[s]))) for s in lights if 0 <= s < len(e) and not np.isnan(e[s]).all())
    return max(float(np.nanmax(e)), 2.0 * total)


# ---- the hand-built weighted queue of the GPU tests: hard by construction, checked by tests/test_weighted_host.py -------------------------

SEED, HAND_N, HAND_NPIX = cr.SEED, cr.HAND_N, cr.HAND_NPIX
T_MIN = cr.T_MIN
# cone_ref's fifteen entries -- two of them name no sphere, sphere 8's largest channel is a NaN -- and sphere 15, the Metal occluder, which
# does not emit, behind them: the last entry of the list is not its last positive one
LIGHTS = cr.LIGHTS + (15,)
FIRST_POSITIVE, LAST_POSITIVE = 0, 14               # list positions of spheres 14 and 20
# the list under which every hit point inside light 19 has tot = 0: the light that holds it, an entry that names no sphere, a sphere that
# does not emit
INNER_LIGHTS = (99, 19, 15)
# cone_ref's table has two lights that exist to pass the 2^16 clamp under area sampling: sphere 9 radiates 2e6 and sphere 16 3e7.  A choice
# proportional to (r2 / d2) max(e) takes one of them with probability 1 - 4e-6 at every hit point of the queue, and no search over samples
# would reach another entry.  Here they radiate what their neighbours do; the spheres, the paths' rays and the list are cone_ref's.
TAMED = {9: (2.0, 1.0, 0.5), 16: (3.0, 1.0, 0.5)}
# slot -> what it was rebuilt to do (test_weighted_host.py checks each with the statement); every slot below 63
CASES = {1: "inside_one", 19: "first_positive", 23: "below_horizon", 25: "blocked", 31: "first_try", 37: "later_block", 43: "beside",
         cr.NEAR_SLOT: "last_positive"}
DIRECT_SLOTS = cr.DIRECT_SLOTS
ALL_WAVE, LAST_LANE_WAVE = cr.ALL_WAVE, cr.LAST_LANE_WAVE


def _matches(what, s):
    if what == "inside_one":                        # the hit point lies inside light 19, whose weight is 0: another light is chosen, and a ray
        return s["imp"][LIGHTS.index(19)] == 0.0 and s["li"] not in (None, 19) and s["shadow"]      # traced (it ends on 19's inner face)
    if what == "first_positive":
        return s["j"] == FIRST_POSITIVE and s["visible"]
    if what == "last_positive":
        return s["j"] == LAST_POSITIVE and s["visible"] and s["front"] == 0
    if what == "below_horizon":
        return s["ns"] is not None and s["ns"] <= 0.0
    if what == "blocked":
        return s["li"] == 14 and s["shadow"] and not s["visible"]
    if what == "first_try":
        return s["tries"] == 1 and s["visible"]
    if what == "later_block":
        return s["tries"] >= 3 and s["visible"]
    if what == "beside":                            # cone_ref's other tangent frame
        return s["li"] == 18 and abs(s["wx"]) > 0.9 and s["visible"]
    if what == "shadow":
        return s["shadow"]
    raise KeyError(what)


@functools.lru_cache(None)
def hand_queue():
    """(flat, queue, light, lights): cone_ref.hand_queue()'s spheres and 513 paths, its emission table with the entries of TAMED, the list
    LIGHTS, and the slots of CASES and the two waves of the second workgroup searched again -- with the statement alone -- so that the
    WEIGHTED sample of each is the named case.  Read-only."""
    flat, base_q, base_light, _ = cr.hand_queue()
    emission = np.array(base_light.emission, copy=True)
    for s, e in TAMED.items():
        emission[s] = e
    light = lr.Light(base_light.sky_bottom, base_light.sky_top, emission)
    q = {f: np.array(base_q[f], copy=True) for f in pr.FIELDS}
    scene = Scene(flat)

    def search(k, what):
        """Slot k, a path that ends on Lambertian sphere 0: the sample below 4000 that makes its light sample `what`."""
        idx, _, p, nrm, _ = fast_hit(scene, q["origin"][k].tolist(), q["dir"][k].tolist(), T_MIN)
        assert idx == 0, (k, idx)
        pixel = int(q["pixel"][k])
        ev_in = int(q["event"][k]) & 0x7FFFFFFF
        with np.errstate(all="ignore"):
            weight = [float(F(q["throughput"][k][c]) * F(flat[0]["albedo"][c])) for c in range(3)]
        for sample in range(4000):
            if _matches(what, sample_light_weighted(scene, SEED, light, LIGHTS, pixel, sample, ev_in, p, nrm, weight, T_MIN)):
                q["sample"][k] = sample
                return
        raise AssertionError(f"no sample below 4000 makes slot {k} the case {what}")

    for k, what in CASES.items():
        search(k, what)
    for k in ALL_WAVE:
        search(k, "shadow")
    search(LAST_LANE_WAVE[-1], "shadow")
    for a in list(q.values()) + [emission]:
        a.setflags(write=False)
    return flat, q, light, LIGHTS


@functools.lru_cache(None)
def hand_step(count, no_direct=False, lights=LIGHTS):
    """The statement's answer for the first `count` paths of hand_queue() (computed once per setting, read-only)."""
    flat, q, light, _ = hand_queue()
    out, adds, live, shadow = step_weighted(flat, pr.prefix(q, count), SEED, HAND_NPIX, light, lights, no_direct, T_MIN)
    for a in list(out.values()) + [adds]:
        a.setflags(write=False)
    return out, adds, live, shadow


# ---- the weighted book frame ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def book_frame(max_depth, batch=257):
    """The statement's weighted frame of lights_ref.book_case() at `max_depth` -> (fix, rays, shadow rays), read-only."""
    flat, light, _ = lr.book_case()
    fix, rays, shadow = render_weighted(flat, oracle.book1_camera(lr.BW, lr.BH), lr.BW, lr.BH, lr.BSPP, light, max_depth=max_depth, seed=1, batch=batch)
    fix.setflags(write=False)
    return fix, rays, shadow


# ---- the eight-light scene: where a uniform choice buys nothing ------------------------------------------------------------------------------

MANY_W, MANY_H, MANY_SPP, MANY_DEPTH = nr.STAT_W, nr.STAT_H, nr.STAT_SPP, nr.STAT_DEPTH
MANY_SEEDS = nr.STAT_SEEDS
MANY_LIGHTS = [((-4.0, 0.2, -1.0), 0.2, (20.0, 16.0, 12.0)), ((-2.5, 0.15, 1.5), 0.15, (30.0, 10.0, 10.0)), ((-0.5, 0.1, 0.8), 0.1, (10.0, 30.0, 10.0)),
               ((0.9, 0.12, 2.0), 0.12, (10.0, 10.0, 30.0)), ((2.6, 0.2, 0.9), 0.2, (20.0, 20.0, 20.0)), ((4.0, 0.25, -1.5), 0.25, (16.0, 16.0, 8.0)),
               ((0.0, 0.15, -3.0), 0.15, (30.0, 30.0, 30.0)), ((-3.0, 0.1, -4.0), 0.1, (40.0, 32.0, 24.0))]


def many_light_scene():
    """(flat, light): a Lambertian ground with a Metal, a Dialectric and a Lambertian sphere on it, and eight small Lambertian lights
    resting on the ground around them -- the shape of the book scene at night lit by a handful of its small spheres --; a black sky.  Camera:
    nee_ref.stat_camera().  At any hit point of the ground one or two lights are near and the rest far: the uniform choice takes a far one
    seven times out of eight and weighs the near one with 2 k * 8 * ns when it comes."""
    import rtiow_amd as rt
    spheres = [((0.0, -1000.0, 0.0), 1000.0, wr.LAMBERTIAN, (0.6, 0.6, 0.6), 0.0),
               ((-1.5, 0.5, 0.0), 0.5, wr.METAL, (0.8, 0.8, 0.8), 0.0),
               ((1.5, 0.5, 0.0), 0.5, wr.DIALECTRIC, (1.0, 1.0, 1.0), 1.5),
               ((0.3, 0.35, 1.2), 0.35, wr.LAMBERTIAN, (0.7, 0.3, 0.3), 0.0)]
    spheres += [(centre, radius, wr.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0) for centre, radius, _ in MANY_LIGHTS]
    flat = np.zeros(len(spheres), dtype=rt.SPHERE_DTYPE)
    for k, (centre, radius, kind, albedo, param) in enumerate(spheres):
        flat[k]["center"], flat[k]["radius"], flat[k]["albedo"], flat[k]["param"], flat[k]["kind"] = centre, radius, albedo, param, kind
    emission = np.zeros((len(spheres), 3))
    for k, (_, _, e) in enumerate(MANY_LIGHTS, start=4):
        emission[k] = e
    return flat, lr.Light((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), emission)


def indirect_pixels(lit_depth_one_frames):
    """The pixels [H, W] whose sums are zero in every one of the lit frames at max_depth = 1: no camera ray of any seed ends on a light."""
    return ~np.array([f.any(axis=2) for f in lit_depth_one_frames]).any(axis=0)


def many_numbers(frames_a, frames_b, mask):
    """From 16 frames each of two estimators (u64 [H, W, 3], one per seed) and the indirect pixels -> (the mean of the per-seed differences
    of the energy summed over those pixels, its standard error, the per-pixel variance over the seeds summed over those pixels for a and
    for b, and the same two variances over the whole frame)."""
    a = np.array([f.astype(np.float64) for f in frames_a]) / 4294967296.0
    b = np.array([f.astype(np.float64) for f in frames_b]) / 4294967296.0
    diff = a[:, mask].sum(axis=(1, 2)) - b[:, mask].sum(axis=(1, 2))
    stderr = float(diff.std(ddof=1) / np.sqrt(len(diff)))
    va, vb = a.var(axis=0, ddof=1), b.var(axis=0, ddof=1)
    return float(diff.mean()), stderr, float(va[mask].sum()), float(vb[mask].sum()), float(va.sum()), float(vb.sum())
