"""The staging arena on the GPU (rt_host::Stage, rt_host.hpp): ONE context goes through every host-buffer entry
point, in sequence, at frame sizes that make its arena grow (7 x 5 -> 64 x 36), stay (-> 7 x 5 -> 33 x 17: smaller calls inside a larger
arena, whose bytes are whatever the calls before left there) and be laid out differently from call to call.  Every result must equal,
bit for bit, the same call on a context created for that call alone -- whose arena is fresh and exactly as large as the call needs.  An
optional buffer that is absent right after a call that had it (rt_denoise without counts after one with, rt_temporal without history
after one with) must not see the stale block: tests/test_stage_layout_host.py checks on the CPU that the denoise input used here gives
different results with and without its counts.  The ray queries, the wavefront steps and the wavefront frames go through the same
sequence with and without their optional buffers (t_max and the hit's fields, sky_dir and select, the emission table and the light list
made from it, the counters a caller may leave out: rays_traced and shadow_rays NULL through raw ctypes), rt_scatter also with out_dir
being dirs itself: one block that goes up and comes down.  rt_render_adaptive goes through with and without out_half, and
rt_filter_tube_device, whose buffers have one fixed size, sits among the calls that change the arena's.  The file asserts nothing about
the arena itself, only about results, messages and times."""
import ctypes as C
import time

import numpy as np
import pytest

import rtiow_amd as rt
from rtiow_amd import _ffi
from test_stage_layout_host import DENOISE_LEVELS, staging_inputs

pytestmark = pytest.mark.gpu

SIZES = [(7, 5), (64, 36), (7, 5), (33, 17)]
ORDER = SIZES + SIZES[::-1]
SPP, ADAPTIVE_SPP, ADAPTIVE_STEP = 2, 8, 2
TIMED = ("features_ids", "features_no_ids", "denoise_count", "denoise_no_count", "temporal_history_count", "temporal_no_history",
         "trace_rays_all_tmax", "trace_rays_index", "occluded", "camera_rays", "scatter", "scatter_in_place", "accumulate_sky_select",
         "accumulate_plain")
WAVEFRONT_DEPTH = 8


def render_fix_only(r, cam, p):
    """rt_render with out_sum = NULL (Renderer.render always asks for the f32 sums)"""
    out = np.zeros((p.height, p.width, 3), dtype=np.uint64)
    c = cam.to_rt_camera()
    _ffi.check(r._lib.rt_render(r._h, C.byref(c), C.byref(p), None, out.ctypes.data_as(C.c_void_p), None), "rt_render")
    return out


def wavefront_counters_null(r, cam, p, lighting=None, direct=False):
    """A wavefront host frame with rays_traced = NULL (direct: rt_render_wavefront_nee, shadow_rays = NULL too): the counters the kernels
    add to are scratch of the call, not buffers of the caller's (Renderer.render_wavefront always asks for them)"""
    fix = np.zeros((p.height, p.width, 3), dtype=np.uint64)
    c = cam.to_rt_camera()
    head, out = (r._h, C.byref(c), C.byref(p)), fix.ctypes.data_as(C.c_void_p)
    if lighting is None:
        _ffi.check(r._lib.rt_render_wavefront(*head, out, None, None), "rt_render_wavefront")
        return (fix,)
    table = lighting.table(r.n_spheres)
    light = lighting.struct(table.ctypes.data if table is not None else None, table.shape[0] if table is not None else 0)
    if direct:
        _ffi.check(r._lib.rt_render_wavefront_nee(*head, C.byref(light), out, None, None, None), "rt_render_wavefront_nee")
    else:
        _ffi.check(r._lib.rt_render_wavefront_lit(*head, C.byref(light), out, None, None), "rt_render_wavefront_lit")
    return (fix,)


def wavefront_nee(r, cam, p, lighting):
    fix, rays, stats = r.render_wavefront(cam, p, lighting=lighting, direct=True)
    return fix, np.uint64(rays), np.uint64(stats["shadow_rays"])


def path_inputs(w, h, n_spheres):
    """One ray or path per pixel, made on the host alone: rays from the book camera's eye to points near the ground (most hit a sphere;
    dirs is the whole way there, so a t_max below 1 cuts a ray short of its point), and for rt_scatter hits made up per path -- every
    sphere of the list in turn, a miss on every seventh -- since the step looks only at the sphere's material and the hit's own numbers."""
    n = w * h
    g = np.random.default_rng(1000 * w + h)
    eye = np.array([13.0, 2.0, 3.0])
    target = np.stack([g.uniform(-11.0, 11.0, n), g.uniform(0.0, 1.0, n), g.uniform(-11.0, 11.0, n)], axis=1)
    normal = g.normal(size=(n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    index = (np.arange(n) % n_spheres).astype(np.int32)
    index[::7] = -1
    return dict(n=n, origins=np.tile(eye, (n, 1)), dirs=target - eye, t_max=g.uniform(0.3, 1.2, n), index=index, point=target, normal=normal,
                front=(g.integers(0, 2, n)).astype(np.uint8), pixel=g.permutation(n).astype(np.uint32), sample=g.integers(0, 4, n).astype(np.uint32),
                event=g.integers(1, 9, n).astype(np.uint32), weight=g.uniform(0.0, 1.0, (n, 3)), select=(g.integers(0, 3, n) > 0).astype(np.uint8),
                fix=g.integers(0, 1 << 40, (h, w, 3)).astype(np.uint64), filler=g.uniform(-1.0, 1.0, (3, n, 3)))


def timed(d, *names):
    """a host form's dict as the tuple this file compares: the named arrays, the kernel's ms last"""
    return tuple(d[k] for k in names) + (d["kernel_ms"],)


def scatter(r, v, in_place):
    """rt_scatter into buffers that hold something already (what the step leaves unwritten keeps the caller's bytes); in place: out_dir
    IS dirs.  The directions the caller is left with come back too."""
    dirs = v["dirs"].copy()
    out = {"out_origin": v["filler"][0].copy(), "out_dir": dirs if in_place else v["filler"][1].copy(), "attenuation": v["filler"][2].copy()}
    res = r.scatter(3, dirs, v["index"], v["point"], v["normal"], v["front"], v["pixel"], v["sample"], v["event"], out=out)
    assert (res["out_dir"] is dirs) == in_place
    return (dirs,) + timed(res, "out_origin", "out_dir", "attenuation", "status", "event")


def accumulate(r, v, **optional):
    fix = v["fix"].copy()
    return fix, r.accumulate(fix, v["pixel"], v["weight"], **optional)


def calls(w, h, flat):
    """[(name, f(renderer) -> tuple of arrays [, kernel ms last for the names in TIMED])]: the sequence at one frame size; flat: the scene."""
    n_spheres = len(flat)
    cam, cams = rt.book1_camera(w, h), rt.orbit_cameras(2, w, h)
    p = rt.make_params(w, h, SPP, seed=1)
    (fix, count, spp, feat, feat_spp), (pfix, plen, pfeat, pspp) = staging_inputs(w, h)
    history = (pfix, plen, pfeat, pspp, rt.orbit_cameras(16, w, h)[1])
    dn, tp = rt.make_denoise(levels=DENOISE_LEVELS), rt.make_temporal()
    x = np.linspace(0.0, 3.0, w * h + 1)
    v = path_inputs(w, h, n_spheres)
    wp = rt.make_params(w, h, SPP, max_depth=WAVEFRONT_DEPTH, seed=1)
    lights = rt.Lighting((0.3, 0.2, 0.1), (0.1, 0.2, 0.9), {0: (0.25, 0.125, 0.0625), 5: (4.0, 3.0, 2.0)})
    no_table = rt.Lighting(lights.sky_bottom, lights.sky_top)
    tube = path_inputs(8, 8, n_spheres)                                  # (64 rays: one wave of the known-answer kernel, whatever the frame)
    ap, ad = rt.make_params(w, h, ADAPTIVE_SPP, seed=1), rt.make_adaptive(ADAPTIVE_STEP, 0.05)
    return [
        ("render_both", lambda r: r.render(cam, p)[:2]),
        ("render_sum", lambda r: r.render(cam, p, want_fix=False)[:1]),
        ("render_fix", lambda r: (render_fix_only(r, cam, p),)),
        ("render_rgba8", lambda r: r.render_rgba8(cam, p)[:1]),
        ("render_pixels", lambda r: r.render_pixels(cam, p, np.arange(0, w * h, 3))[:1]),
        ("render_frames", lambda r: r.render_frames(cams, p, sample_stride=SPP)[:1]),
        ("render_frames_rgba8_flip", lambda r: r.render_frames_rgba8(cams, p, flip=True)[:1]),
        ("render_frames_rgba8", lambda r: r.render_frames_rgba8(cams, p, flip=False)[:1]),
        ("features_ids", lambda r: r.render_features(cam, p)),
        ("features_no_ids", lambda r: (lambda f, _, ms: (f, ms))(*r.render_features(cam, p, want_ids=False))),
        ("features_to_f32", lambda r: (r.features_to_f32(feat, feat_spp),)),
        ("denoise_count", lambda r: r.denoise(fix, spp, feat, feat_spp, dn, count=count)),
        ("denoise_no_count", lambda r: r.denoise(fix, spp, feat, feat_spp, dn)),
        ("temporal_history_count", lambda r: r.temporal(fix, spp, feat, feat_spp, cam, history, tp, count=count)),
        ("temporal_no_history", lambda r: r.temporal(fix, spp, feat, feat_spp, cam, None, tp)),
        ("resolve_rgba8", lambda r: (r.resolve_rgba8(fix, spp),)),
        ("resolve_rgba8_counts", lambda r: (r.resolve_rgba8_counts(fix, count),)),
        ("render_adaptive", lambda r: r.render_adaptive(cam, ap, ad)[:3]),
        ("render_adaptive_no_half", lambda r: (lambda fix, _, count, st: (fix, count))(*r.render_adaptive(cam, ap, ad, want_half=False))),
        ("filter_tube", lambda r: (lambda h, rows, bound, rho: (h, rows, bound, np.float32(rho)))(*r.filter_tube(tube["origins"], tube["dirs"], flat[:32]))),
        ("quantize", lambda r: (r.quantize(x),)),
        ("philox", lambda r: (np.array(r.philox((w, h, 3, 4), (5, 6)), dtype=np.uint64),)),
        ("trace_rays_all_tmax", lambda r: timed(r.trace_rays(v["origins"], v["dirs"], t_max=v["t_max"]), "index", "t", "point", "normal", "front_face")),
        ("trace_rays_index", lambda r: timed(r.trace_rays(v["origins"], v["dirs"], want=()), "index")),
        ("occluded", lambda r: timed(r.occluded(v["origins"], v["dirs"], t_max=v["t_max"]), "occluded")),
        ("camera_rays", lambda r: timed(r.camera_rays(cam, w, h, 7, v["pixel"], v["sample"]), "origin", "dir", "event")),
        ("scatter", lambda r: scatter(r, v, False)),
        ("scatter_in_place", lambda r: scatter(r, v, True)),
        ("accumulate_sky_select", lambda r: accumulate(r, v, sky_dir=v["dirs"], select=v["select"])),
        ("accumulate_plain", lambda r: accumulate(r, v)),
        ("render_wavefront", lambda r: (lambda fix, rays: (fix, np.uint64(rays)))(*r.render_wavefront(cam, wp))),
        ("render_wavefront_lit_table", lambda r: (lambda fix, rays: (fix, np.uint64(rays)))(*r.render_wavefront(cam, wp, lighting=lights))),
        ("render_wavefront_lit_none", lambda r: (lambda fix, rays: (fix, np.uint64(rays)))(*r.render_wavefront(cam, wp, lighting=no_table))),
        ("render_wavefront_nee_table", lambda r: wavefront_nee(r, cam, wp, lights)),
        ("render_wavefront_nee_none", lambda r: wavefront_nee(r, cam, wp, no_table)),                     # (no light list, emission NULL)
        ("render_wavefront_nee_no_counters", lambda r: wavefront_counters_null(r, cam, wp, lights, direct=True)),
        ("render_wavefront_no_counter", lambda r: wavefront_counters_null(r, cam, wp)),
        ("render_wavefront_lit_no_counter", lambda r: wavefront_counters_null(r, cam, wp, lights)),
    ]


def arrays(name, result):
    return result[:-1] if name in TIMED else result


@pytest.fixture(scope="module")
def fresh(book1_flat):
    """(size, name) -> the call's arrays from a context created for that call alone; computed once per size."""
    cache = {}

    def get(size):
        if size not in cache:
            cache[size] = {}
            for name, call in calls(*size, book1_flat):
                with rt.Renderer(0) as r:
                    r.upload_scene(book1_flat)
                    cache[size][name] = arrays(name, call(r))
                for a in cache[size][name]:
                    if isinstance(a, np.ndarray):
                        a.setflags(write=False)
        return cache[size]
    return get


def test_one_context_through_every_host_form(book1_flat, fresh):
    bad = rt.make_denoise(levels=0)
    with rt.Renderer(0) as r:
        r.upload_scene(book1_flat)
        for step, size in enumerate(ORDER):
            want = fresh(size)
            for name, call in calls(*size, book1_flat):
                if name == "temporal_history_count":                  # a rejected call in mid-sequence: its usual message, and the next call correct
                    (fix, _, spp, feat, feat_spp), _ = staging_inputs(*size)
                    with pytest.raises(_ffi.RtiowHipError, match=r"denoise: levels must be 1\.\.\d+ \(is 0\)"):
                        r.denoise(fix, spp, feat, feat_spp, bad)
                t0 = time.perf_counter()
                got = call(r)
                wall_ms = (time.perf_counter() - t0) * 1e3
                if name in TIMED:
                    assert 0.0 < got[-1] < wall_ms, (step, size, name, got[-1], wall_ms)
                got = arrays(name, got)
                assert len(got) == len(want[name]) and all(g.dtype == v.dtype and np.array_equal(g, v) for g, v in zip(got, want[name])), (step, size, name)


def test_the_sequence_tells_a_present_buffer_from_an_absent_one(fresh):
    """(what makes the test above a test: the calls with and without the optional buffer differ on these inputs)"""
    for size in set(SIZES):
        want = fresh(size)
        assert not np.array_equal(want["denoise_count"][0], want["denoise_no_count"][0])
        assert not np.array_equal(want["temporal_history_count"][0], want["temporal_no_history"][0])
        assert not np.array_equal(want["render_frames_rgba8_flip"][0], want["render_frames_rgba8"][0])
        assert not np.array_equal(want["trace_rays_all_tmax"][0], want["trace_rays_index"][0])            # (index with t_max, without)
        assert not np.array_equal(want["accumulate_sky_select"][0], want["accumulate_plain"][0])
        assert not np.array_equal(want["render_wavefront_lit_table"][0], want["render_wavefront_lit_none"][0])
        assert not np.array_equal(want["render_wavefront_lit_none"][0], want["render_wavefront"][0])      # (the sky is not the default's)
        assert not np.array_equal(want["render_wavefront_nee_table"][0], want["render_wavefront_nee_none"][0])
        # a counter left out changes nothing in the sums; a frame without lights traces no shadow ray
        assert np.array_equal(want["render_wavefront_nee_no_counters"][0], want["render_wavefront_nee_table"][0])
        assert np.array_equal(want["render_wavefront_no_counter"][0], want["render_wavefront"][0])
        assert np.array_equal(want["render_wavefront_lit_no_counter"][0], want["render_wavefront_lit_table"][0])
        assert want["render_wavefront_nee_none"][2] == 0
        assert all(np.array_equal(a, b) for a, b in zip(want["render_adaptive_no_half"], want["render_adaptive"][::2]))
        # rt_scatter in place: a scattered path's new direction is in `dirs`, every other path's old one still is; not in place: dirs untouched
        dirs, _, out_dir, _, status = want["scatter"][:5]
        went_on = status == _ffi.RT_SCATTER_SCATTERED
        assert went_on.any() and not went_on.all() and not np.array_equal(dirs[went_on], out_dir[went_on])
        assert np.array_equal(want["scatter_in_place"][0], np.where(went_on[:, None], out_dir, dirs))
    # ... and rt_render_adaptive went past its first round (selection and pixel-list passes beside its frame state in the arena)
    assert any((fresh(size)["render_adaptive"][2] > 2 * ADAPTIVE_STEP).any() for size in set(SIZES))
    # ... and the NEE frame traced shadow rays (its light list and its shadow counter were blocks of the call)
    assert any(fresh(size)["render_wavefront_nee_table"][2] > 0 for size in set(SIZES))
