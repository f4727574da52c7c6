"""Ray queries without a GPU (include/rtiow_hip.h "ray queries"): the reference's fast form against the literal
loop of mod.rs:54-70, the context-free validation of the four entry points, the struct layouts against the header, and
test_the_trace_cases_are_hard: that the cases of tests/test_gpu_trace_viewpoints.py hold what the kernel can go wrong on."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import rtiow_amd as rt
import trace_ref as tr
from grid_model import minimal_scale, model_grid_cells
from rtiow_amd import _ffi
from test_gpu_trace_viewpoints import N_WAVE, ONE_SIDED, case, scene_of
from test_gpu_viewpoints import CAMERAS, SCENES, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_fast_form_equals_the_literal_loop(oracle_mod):
    """On the book scene, about 300 rays of the three kinds (camera rays, bounce rays, rays from inside the bounding box), every t_max
    class among them: oracle_world_hit + the t_max comparison + the winner's record is HittableList::hit as written."""
    sc = scene_of("book")
    n_in = 0
    seen = set()
    for camera in ("lens2", "in_glass"):
        origins, dirs, t_max, classes, want = case("book", camera)
        inside = np.array([tr.in_analysed_range(origins[k], dirs[k], t_max[k]) for k in range(len(t_max))])
        literal = tr.trace(sc, origins[inside], dirs[inside], t_max[inside], literal=True)
        tr.same({k: v[inside] for k, v in want.items()}, literal)
        n_in += int(inside.sum())
        seen |= {c for c, ok in zip(classes, inside) if ok and c}
        assert (literal["index"] >= 0).any() and (literal["index"] < 0).any()
    assert n_in >= 300 and seen == set(tr.T_MAX_CLASSES) - {"nan"}          # (a NaN t_max is outside the range: the literal loop answers)


def test_hand_answers(oracle_mod):
    """A unit sphere 5 in front of the origin: t = 4 along -z, a root equal to t_max is a hit, one ulp below it is not; from inside a
    sphere the far root; coincident spheres: the later one."""
    import features_ref as fr
    scenes = {name: tr.Scene(flat) for name, (flat, _) in fr.hand_scenes().items()}
    o, d = np.zeros((1, 3)), np.array([[0.0, 0.0, -1.0]])
    one = lambda name, tm, org=o: tr.trace(scenes[name], org, d, np.array([tm]), literal=True)
    r = one("one_sphere", math.inf)
    assert r["index"][0] == 0 and r["t"][0] == 4.0 and r["point"][0].tolist() == [0.0, 0.0, -4.0] and r["normal"][0].tolist() == [0.0, 0.0, 1.0]
    assert r["front_face"][0] == 1
    assert one("one_sphere", 4.0)["index"][0] == 0 and one("one_sphere", np.nextafter(4.0, 0.0))["index"][0] == -1
    miss = one("one_sphere", 0.0)
    assert miss["index"][0] == -1 and miss["t"][0] == math.inf and not miss["point"].any() and not miss["normal"].any() and miss["front_face"][0] == 0
    assert one("one_sphere", math.nan)["index"][0] == 0                      # a NaN t_max fails no comparison
    assert one("coincident", math.inf)["index"][0] == 1
    inside = one("inside", math.inf, np.array([[0.0, 0.0, 1.0]]))
    assert inside["t"][0] == 5.0 and inside["front_face"][0] == 0 and inside["normal"][0].tolist() == [0.0, 0.0, 1.0]
    assert one("negative_radius", math.inf)["normal"][0].tolist() == [0.0, 0.0, 1.0] and one("negative_radius", math.inf)["front_face"][0] == 0
    zero = tr.trace(scenes["one_sphere"], o, np.zeros((1, 3)))               # a zero direction: 0 / 0, a NaN root, accepted as written
    assert zero["index"][0] == 0 and tr.bits(zero["t"])[0] == tr.QNAN_BITS and tr.bits(zero["point"])[0, 2] == tr.QNAN_BITS


# ---- the C ABI without a context ---------------------------------------------------------------------------------------------------

def _err(lib):
    return lib.rt_last_error().decode()


def test_the_four_symbols_resolve():
    lib = _ffi.load()
    for name in ("rt_trace_rays_device", "rt_trace_rays", "rt_occluded_device", "rt_occluded"):
        assert name in [n for n, _, _ in _ffi.SYMBOLS] and getattr(lib, name)
    assert lib.rt_abi_version() == 5
    assert callable(rt.trace_rays_torch) and callable(rt.occluded_torch)


def _structs(n=4, **null):
    """(rays, hits, the arrays that keep them alive); null=...: fields left NULL."""
    m = 4                                       # (the arrays are never read here: every call ends in validation)
    keep = dict(origin=np.zeros((m, 3)), dir=np.ones((m, 3)), t_max=np.ones(m), index=np.full(m, 77, dtype=np.int32),
                occluded=np.full(m, 77, dtype=np.uint8))
    p = lambda name: None if null.get(name) else keep[name].ctypes.data
    return _ffi.rt_rays(p("origin"), p("dir"), p("t_max"), n), _ffi.rt_hits(p("index"), None, None, None, None), keep


def test_hits_is_null():
    lib = _ffi.load()
    rays, _, keep = _structs()
    for fn in (lib.rt_trace_rays_device, lib.rt_trace_rays):
        assert fn(None, C.byref(rays), 1e-4, None, None) == -1 and "hits is NULL" in _err(lib), _err(lib)


@pytest.mark.parametrize("form", ["trace_device", "trace_host", "occluded_device", "occluded_host"])
@pytest.mark.parametrize("kw,t_min,msg", [
    (dict(rays=True), 1e-4, "rays is NULL"),
    (dict(n=-1), 1e-4, "n must be in [0, 2^31]"),
    (dict(n=2 ** 31 + 1), 1e-4, "n must be in [0, 2^31]"),
    (dict(), 0.0, "t_min must be > 0 and finite"),
    (dict(), -1.0, "t_min must be > 0 and finite"),
    (dict(), math.inf, "t_min must be > 0 and finite"),
    (dict(), math.nan, "t_min must be > 0 and finite"),
    (dict(origin=True), 1e-4, "rays->origin is NULL"),
    (dict(dir=True), 1e-4, "rays->dir is NULL"),
    (dict(out=True), 1e-4, "the required output"),
    (dict(), 1e-4, "ctx is NULL"),
    (dict(n=0, origin=True, dir=True, out=True), 1e-4, "ctx is NULL"),       # n == 0 needs no array: the next check speaks
    (dict(n=2 ** 31), 1e-4, "ctx is NULL"),                                  # the largest batch is legal
])
def test_context_free_validation(form, kw, t_min, msg):
    """Every reason comes before the context is looked at, and nothing is touched."""
    lib = _ffi.load()
    occl = form.startswith("occluded")
    rays, hits, keep = _structs(kw.get("n", 4), origin=kw.get("origin"), dir=kw.get("dir"), index=kw.get("out"))
    pr = None if kw.get("rays") else C.byref(rays)
    if occl:
        out = None if kw.get("out") else keep["occluded"].ctypes.data_as(C.c_void_p)
        rc = (lib.rt_occluded_device if form.endswith("device") else lib.rt_occluded)(None, pr, t_min, out, None)
    else:
        rc = (lib.rt_trace_rays_device if form.endswith("device") else lib.rt_trace_rays)(None, pr, t_min, C.byref(hits), None)
    assert rc == -1 and msg in _err(lib), _err(lib)
    assert (keep["index"] == 77).all() and (keep["occluded"] == 77).all()


def test_python_layer_rejects_bad_shapes():
    """(before any library call: a Renderer is not needed for the check itself)"""
    with pytest.raises(ValueError):
        rt.Renderer._ray_arrays(np.zeros((4, 3)), np.zeros((5, 3)), None)
    with pytest.raises(ValueError):
        rt.Renderer._ray_arrays(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(3))
    rays, keep = rt.Renderer._ray_arrays(np.zeros((4, 3), dtype=np.float32), np.zeros((4, 3)), None)
    assert rays.n == 4 and rays.t_max is None and keep[0].dtype == np.float64


def test_struct_layouts_agree_with_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow_hip.h")).read(), flags=re.S)
    for name, cls in (("rt_rays", _ffi.rt_rays), ("rt_hits", _ffi.rt_hits)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, hdr).group(1)
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                m = re.match(r"\s*(const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*$", decl)
                fields.append((m.group(4), bool(m.group(3)), m.group(2)))
        assert [f[0] for f in fields] == [f[0] for f in cls._fields_], name
        offset = 0
        for (fname, is_ptr, ctype), (_, ffi_type) in zip(fields, cls._fields_):
            assert is_ptr == (ffi_type is C.c_void_p) and (is_ptr or ctype == "int64_t"), (name, fname)
            assert getattr(cls, fname).offset == offset and C.sizeof(ffi_type) == 8, (name, fname)
            offset += 8
        assert C.sizeof(cls) == offset
    assert C.sizeof(_ffi.rt_rays) == 32 and C.sizeof(_ffi.rt_hits) == 40
    for fn in ("rt_trace_rays_device", "rt_trace_rays", "rt_occluded_device", "rt_occluded"):
        assert re.search(r"\bint %s\(rt_context \*ctx, const rt_rays \*rays, double t_min, " % fn, hdr), fn


# ---- the viewpoint cases are hard ----------------------------------------------------------------------------------------------------

# The (scene, camera) cases in which NO wave that the kernel scans by cell set (no lane "cannot tell") has a union of footprints below its
# bounding rectangle, pinned by name: every other gridded case is asserted to have one, and a listed case that gains one fails the test
# too, so the suite's hardness cannot drift either way.  Per case: (cells of the union, cells of the rectangle) of waves 0, 1, 2, "ct" where
# a lane cannot tell.  Wave 2 holds the 1e-31 lane ("cannot tell") whenever the case's rotation of degenerate kinds reaches it.
UNION_IS_THE_RECTANGLE = {
    # the 10 x 10 grid (LDS row words): one case
    ("big", "dz_0"),                # ct (d.z = 0 exactly); 4/4: the hit points lie in one 2 x 2 block; ct (37/100 otherwise)
    # the book's 4 x 4 grid (one 64-bit mask): a few dozen rays in the bounding box reach all 16 cells
    ("book", "ground_x_20"),        # 8/8; 3/3; 16/16
    ("book", "ground_x_90"),        # 0/0 (the frame looks over the box); 1/1; ct (13/16 otherwise)
    ("book", "up_inside"),          # 1/1 (straight up from one cell); 0/0; ct (15/16 otherwise)
    ("book", "dz_0"),               # ct; 6/6; 16/16
    # the giants' 2 x 2 grid: a union below the rectangle takes exactly three cells, or a diagonal pair
    ("giants", "ground_x_20"),      # 0/0; 2/2; ct (3/4 otherwise)
    ("giants", "ground_x_90"),      # 1/1; 0/0; ct (2/4 otherwise)
    ("giants", "ground_z_90"),      # 0/0; 2/2; ct
    ("giants", "down"),             # 4/4; 4/4; ct (3/4 otherwise)
    ("giants", "down_rolled"),      # 4/4; 4/4; ct (2/4 otherwise)
    ("giants", "in_glass"),         # 2/2; 4/4; ct
    ("giants", "below_ground"),     # 4/4; 4/4; 1/1
    ("giants", "fov170"),           # 0/0; 0/0; ct
    ("giants", "dz_0"),             # ct; 2/2; ct
}


def footprint_cells(o, d, g, G):
    """grid_model's footprints of a wave's rays -> (kind [lanes], the union of the lanes' row runs as a set of cells, the cells of the
    bounding rectangle of the lanes that have a rectangle)."""
    ix0, ix1, iz0, iz1, kind = model_grid_cells(o, d, g, G, minimal_scale(g), None, shrink=1.0)
    rlo, rhi = model_grid_cells.row_runs
    union = set()
    for k in np.flatnonzero(kind == 1):
        for z in range(int(iz0[k]), int(iz1[k]) + 1):
            union |= {(z, x) for x in range(int(rlo[k, z]), int(rhi[k, z]) + 1)}
    has = kind == 1
    rect = int((ix1[has].max() - ix0[has].min() + 1) * (iz1[has].max() - iz0[has].min() + 1)) if has.any() else 0
    return kind, union, rect


def test_the_trace_cases_are_hard(oracle_mod, monkeypatch):
    """With the reference alone: every (scene, camera) case has hits and misses, a ray in every t_max class, a wave that holds rays inside
    and outside the analysed range, and -- on the gridded scenes -- a wave (no lane "cannot tell") whose union of footprints is smaller
    than its bounding rectangle, so that the `ray` scheme's cell set is not the `wave` scheme's rectangle: in every case but the 14 that
    UNION_IS_THE_RECTANGLE pins by name (1 of 54 on the large grids, 4 of 18 on the book's 4 x 4, 9 of 18 on the giants' 2 x 2)."""
    assert len(ONE_SIDED) <= 2 and all(SCENES[s][0] != "boulders" and c in CAMERAS for s, c in UNION_IS_THE_RECTANGLE)
    for scene in SCENES:
        flat, G, n_global, g, _ = layout(monkeypatch, scene)
        for camera in CAMERAS:
            origins, dirs, t_max, classes, want = case(scene, camera)
            assert origins.shape == (3 * N_WAVE, 3)
            both = (want["index"] >= 0).any() and (want["index"] < 0).any()
            assert both != ((scene, camera) in ONE_SIDED), (scene, camera)
            assert set(classes) - {""} == set(tr.T_MAX_CLASSES), (scene, camera)
            inside = np.array([tr.in_analysed_range(origins[k], dirs[k], t_max[k]) for k in range(len(t_max))])
            mixed = [w for w in range(3) if inside[64 * w:64 * w + 64].any() and not inside[64 * w:64 * w + 64].all()]
            assert mixed, (scene, camera)
            # the root classes really cut: a ray with t_max exactly at its root hits, and some ray one ulp below it answers differently
            cls = np.array(classes)
            at_root = (cls == "root") & np.isfinite(t_max)
            assert (want["index"][at_root] >= 0).all(), (scene, camera)
            if G > 0:
                smaller = False
                for w in range(3):
                    sl = slice(64 * w, 64 * w + 64)
                    lanes = np.flatnonzero(inside[sl]) + 64 * w
                    kind, union, rect = footprint_cells(origins[lanes], dirs[lanes], g, G)
                    smaller = smaller or (not (kind == -1).any() and 0 < len(union) < rect)
                assert smaller != ((scene, camera) in UNION_IS_THE_RECTANGLE), (scene, camera, G)
    # the cell set in LDS row words is exercised by 53 of the 54 cases on the three large grids, the single mask by 23 of 36
    large = [s for s in SCENES if SCENES[s][0] == "big"]
    assert sum(s in large for s, _ in UNION_IS_THE_RECTANGLE) == 1 and len(UNION_IS_THE_RECTANGLE) == 14
