"""CPU reference of the ray queries (include/rtiow_hip.h "ray queries") -- a test helper.

The DEFINITION is the literal loop of mod.rs:54-70: oracle_sphere_hit(c, r, o, d, t_min, closest_so_far) per sphere in list order, the
record taken from the winner (`literal_hit`).  A fast form for rays inside the analysed range (`fast_hit`): oracle_world_hit for
(index, t), a miss unless t <= t_max, oracle_sphere_hit on the winner for the record -- used only because tests/test_trace_host.py shows it
equal to the literal loop.  Nothing here but what oracle/ already exports.  A NaN is written as the quiet NaN 0x7FF8000000000000, as the
header says (the sign of a generated NaN differs between processors).
"""
import ctypes as C
import math

import numpy as np

import oracle

QNAN_BITS = np.uint64(0x7FF8000000000000)
T_MIN = 1e-4
D3 = C.c_double * 3


class Scene:
    """A flat scene prepared for many queries: the oracle's pointer, and every centre / radius as ctypes values."""

    def __init__(self, flat):
        self.flat = np.ascontiguousarray(flat)
        assert self.flat.dtype.itemsize == 72
        self.n = int(self.flat.shape[0])
        self.ptr = self.flat.ctypes.data_as(C.POINTER(oracle.sphere))
        self.centres = [D3(*[float(x) for x in rec["center"]]) for rec in self.flat]
        self.radii = [float(rec["radius"]) for rec in self.flat]


MISS = (-1, math.inf, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0)


def literal_hit(scene, o, d, t_min, t_max):
    """mod.rs:54-70 as written -> (index, t, point, normal, front_face); MISS without a hit."""
    lib = oracle.load()
    co, cd = D3(*o), D3(*d)
    t, front = C.c_double(0.0), C.c_int(0)
    p, nrm = D3(), D3()
    closest, best = float(t_max), MISS
    for k in range(scene.n):
        if lib.oracle_sphere_hit(scene.centres[k], scene.radii[k], co, cd, t_min, closest, C.byref(t), p, nrm, C.byref(front)):
            closest = t.value                                                   # mod.rs:63-64
            best = (k, t.value, tuple(p), tuple(nrm), int(front.value))
    return best


def fast_hit(scene, o, d, t_min, t_max=math.inf):
    """The same answer for a ray inside the analysed range (tests/test_trace_host.py proves it on the book scene); with t_max = +inf,
    HittableList::hit(ray, t_min, +inf) and the winner's HitRecord for ANY ray (tests/features_ref.py: a NaN root is a hit there)."""
    lib = oracle.load()
    co, cd = D3(*o), D3(*d)
    t = C.c_double(0.0)
    idx = lib.oracle_world_hit(scene.ptr, scene.n, co, cd, t_min, C.byref(t))
    if idx < 0 or t.value > t_max:
        return MISS
    t2, front = C.c_double(0.0), C.c_int(0)
    p, nrm = D3(), D3()
    got = lib.oracle_sphere_hit(scene.centres[idx], scene.radii[idx], co, cd, t_min, math.inf, C.byref(t2), p, nrm, C.byref(front))
    assert got == 1
    assert t2.value == t.value or (t2.value != t2.value and t.value != t.value)      # the same root, NaN included
    return idx, t.value, tuple(p), tuple(nrm), int(front.value)


def in_analysed_range(o, d, t_max):
    """True only for rays the kernel certainly answers in the order-independent form (|d|^2 as f32 inside (1e-20, 1e20), |o|_1 < 1e15,
    t_max not a NaN), with a decade of margin: in doubt the literal loop, which is the definition, answers."""
    with np.errstate(over="ignore", invalid="ignore"):
        df = np.asarray(d, dtype=np.float64).astype(np.float32).astype(np.float64)
        of = np.asarray(o, dtype=np.float64).astype(np.float32).astype(np.float64)
        a, o1 = float((df * df).sum()), float(np.abs(of).sum())
    return bool(np.isfinite(df).all() and np.isfinite(of).all() and 1e-19 < a < 1e19 and o1 < 1e14 and t_max == t_max)


def trace(scene, origins, dirs, t_max=None, t_min=T_MIN, literal=False):
    """-> dict(index i32 [n], t f64 [n], point f64 [n,3], normal f64 [n,3], front_face u8 [n]): rt_trace_rays as the header defines it."""
    if not isinstance(scene, Scene):
        scene = Scene(scene)
    origins, dirs = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = origins.shape[0]
    t_max = np.full(n, math.inf) if t_max is None else np.asarray(t_max, dtype=np.float64)
    out = dict(index=np.full(n, -1, dtype=np.int32), t=np.full(n, math.inf), point=np.zeros((n, 3)), normal=np.zeros((n, 3)),
               front_face=np.zeros(n, dtype=np.uint8))
    for k in range(n):
        o, d, tm = origins[k].tolist(), dirs[k].tolist(), float(t_max[k])
        use_fast = not literal and in_analysed_range(o, d, tm)
        idx, t, p, nrm, front = (fast_hit if use_fast else literal_hit)(scene, o, d, t_min, tm)
        out["index"][k], out["t"][k], out["point"][k], out["normal"][k], out["front_face"][k] = idx, t, p, nrm, front
    for name in ("t", "point", "normal"):
        out[name] = canonical(out[name])
    for a in out.values():
        a.setflags(write=False)
    return out


def canonical(a):
    a = np.array(a, dtype=np.float64)
    a.view(np.uint64)[np.isnan(a)] = QNAN_BITS
    return a


def bits(a):
    """f64 -> the u64 patterns, so that NaN compares and -0.0 differs from 0.0."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, names=("index", "t", "point", "normal", "front_face")):
    """A query's outputs against the reference's, bit for bit."""
    for name in names:
        g, w = got[name], want[name]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if name in ("t", "point", "normal"):
            assert g.dtype == np.float64
            bad = bits(g) != bits(w)
        else:
            assert g.dtype == w.dtype, (name, g.dtype)
            bad = g != w
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: {g[bad][:3]} != {w[bad][:3]}"


def permuted(want, perm):
    return {k: v[perm] for k, v in want.items()}


# ---- ray sets shared by the CPU and the GPU tests -------------------------------------------------------------------------------------

def degenerate_rays():
    """(origins [6,3], dirs [6,3]): the rays outside, or at the edge of, the analysed range -- a zero direction, a NaN component, an
    infinite component, a component of 1e-31 (the footprint "cannot tell"; the filter still applies), an origin at 1e16, |d|^2 < 1e-20."""
    o = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.5, 0.0], [1e16, 0.5, 0.0], [0.0, 0.0, 0.0]])
    d = np.array([[0.0, 0.0, 0.0], [0.0, math.nan, -1.0], [0.0, math.inf, -1.0], [0.3, 1e-31, -1.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1e-11]])
    return o, d


T_MAX_CLASSES = ("inf", "log_uniform", "root", "below_root", "zero", "negative", "nan")


def t_max_of(cls, root, rng):
    """A t_max of the named class for a ray whose unclipped root is `root` (+inf for a miss)."""
    if cls == "inf":
        return math.inf
    if cls == "log_uniform":
        return float(10.0 ** rng.uniform(-2.0, 2.0))
    if cls == "root":
        return root                                                             # exactly the root: a hit
    if cls == "below_root":
        return float(np.nextafter(root, -math.inf))                             # a miss, or the hit behind it
    return {"zero": 0.0, "negative": -1.0, "nan": math.nan}[cls]


def unit_directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)
