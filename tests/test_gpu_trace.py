"""Ray queries on the GPU (rt_trace_rays*, rt_occluded*) against tests/trace_ref.py, everything bit for bit:
index, t / point / normal as u64 patterns (so that NaN compares), front_face; occlusion against index >= 0 on every batch."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import features_ref as fr
import rtiow_amd as rt
import trace_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MIN = tr.T_MIN
SIZES = (1, 63, 64, 65, 257)            # a lone ray, a wave less one, a full wave, a wave and one, two workgroups with a ragged last wave


def check(renderer, scene, origins, dirs, t_max, want=None, **kw):
    """One batch through the host forms: closest hit bit for bit, occlusion == (index >= 0).  Returns the reference's answer."""
    want = want or tr.trace(scene, origins, dirs, t_max, **kw)
    got = renderer.trace_rays(origins, dirs, t_max)
    tr.same(got, want)
    occ = renderer.occluded(origins, dirs, t_max)["occluded"]
    assert occ.dtype == np.uint8 and np.array_equal(occ, (want["index"] >= 0).astype(np.uint8)), "occluded"
    return want


# ---- hand scenes ------------------------------------------------------------------------------------------------------------------------

HAND_CLASSES = ("inf", "root", "below_root", "half_root", "above_root", "zero", "negative", "half_t_min", "nan")


def hand_batch(name, n):
    """n rays at the hand scene's sphere, through it and beside it (the sphere fills about half of the directions' square), with t_max
    run through its classes relative to each ray's own unclipped root: +inf; exactly the root (a hit); one ulp below it (a miss, or the
    hit behind it); half the root and 1.25 x the root (from inside a sphere, between the negative near root and the far one: a miss /
    a hit); 0; -1; t_min / 2; NaN."""
    flat, cam = fr.hand_scenes()[name]
    scene = tr.Scene(flat)
    rng = np.random.default_rng(100 + n)
    origin = np.array(cam.to_rt_camera().origin[:])
    target = flat[0]["center"] + np.concatenate([rng.uniform(-2.0, 2.0, (n, 2)), np.zeros((n, 1))], axis=1) * (4.0 if name == "inside" else 1.0)
    dirs = (target - origin) * rng.choice([1.0, 0.25, 3.0], n)[:, None]
    origins = np.tile(origin, (n, 1))
    roots = tr.trace(scene, origins, dirs, literal=True)["t"]
    t_max = np.zeros(n)
    for k in range(n):
        cls, root = HAND_CLASSES[k % len(HAND_CLASSES)], float(roots[k])
        t_max[k] = {"half_root": 0.5 * root, "above_root": 1.25 * root, "half_t_min": 0.5 * T_MIN}.get(cls) if cls in (
            "half_root", "above_root", "half_t_min") else tr.t_max_of(cls, root, rng)
    return scene, origins, dirs, t_max


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_sphere", "inside", "coincident", "glass", "negative_radius"])
def test_hand_scenes(renderer, oracle_mod, name):
    flat, _ = fr.hand_scenes()[name]
    renderer.upload_scene(flat)
    for n in SIZES:
        scene, origins, dirs, t_max = hand_batch(name, n)
        want = check(renderer, scene, origins, dirs, t_max, literal=True)
        no_clip = check(renderer, scene, origins, dirs, None, literal=True)
        if n >= 63:
            hit = no_clip["index"] >= 0
            assert hit.any() and (name == "inside" or (~hit).any())                         # through the sphere and beside it
            assert (want["index"] != no_clip["index"]).any()                                # t_max cuts some of them
            if name == "coincident":
                assert (no_clip["index"][hit] == 1).all()                                   # the later of two equal spheres
            if name == "inside":
                assert hit.all() and not no_clip["front_face"].any()
            cls = np.array([HAND_CLASSES[k % len(HAND_CLASSES)] for k in range(n)])
            assert (want["index"][(cls == "root") & hit] >= 0).all() and (want["index"][(cls == "zero") | (cls == "negative") | (cls == "half_t_min")] == -1).all()


# ---- the book scene ------------------------------------------------------------------------------------------------------------------------

BW, BH = 37, 19


@functools.lru_cache(None)
def book():
    return tr.Scene(rt.random_scene(1).flatten())


@functools.lru_cache(None)
def book_camera_rays():
    """The 37 x 19 camera rays of sample 0, seed 1 (features_ref.camera_ray), pixel g = j * 37 + i at place g."""
    ocam = fr.camera_from_rt(rt.book1_camera(BW, BH).to_rt_camera())
    o, d = np.zeros((BW * BH, 3)), np.zeros((BW * BH, 3))
    for j in range(BH):
        for i in range(BW):
            ro, rd = fr.camera_ray(ocam, BW, BH, 1, i, j, 0)
            o[j * BW + i], d[j * BW + i] = ro[:], rd[:]
    o.setflags(write=False); d.setflags(write=False)
    return o, d


@functools.lru_cache(None)
def book_batch():
    """1 000 rays on the book scene and the reference's answer, computed once: the 703 camera rays, bounce rays from their hit points in
    seeded directions, t_max in every class, the six degenerate rays in the last wave beside ordinary ones."""
    o0, d0 = book_camera_rays()
    first = tr.trace(book(), o0, d0)
    rng = np.random.default_rng(5)
    n1 = 1000 - len(o0)
    pick = rng.integers(0, len(o0), n1)
    o1 = np.where((first["index"][pick] >= 0)[:, None], first["point"][pick], o0[pick] + d0[pick] * 10.0)
    d1 = tr.unit_directions(rng, n1) * rng.choice([1.0, 1e-3, 1e3], n1)[:, None]
    og, dg = tr.degenerate_rays()
    o1[-20:-14], d1[-20:-14] = og, dg
    origins, dirs = np.concatenate([o0, o1]), np.concatenate([d0, d1])
    roots = tr.trace(book(), origins, dirs)["t"]
    t_max = np.array([tr.t_max_of(tr.T_MAX_CLASSES[k % 7] if k % 3 == 0 else "inf", float(roots[k]), rng) for k in range(1000)])
    want = tr.trace(book(), origins, dirs, t_max)
    for a in (origins, dirs, t_max):
        a.setflags(write=False)
    return origins, dirs, t_max, want


@pytest.mark.gpu
def test_degenerate_rays_beside_ordinary_ones(renderer, oracle_mod):
    """One wave: 58 camera rays and a zero direction, a NaN component, an infinite component, a component of 1e-31, an origin at 1e16 and
    |d|^2 < 1e-20.  The rays outside the analysed range take the list as written; their neighbours must not notice."""
    renderer.upload_scene(book().flat)
    o0, d0 = book_camera_rays()
    og, dg = tr.degenerate_rays()
    origins, dirs = np.concatenate([o0[300:329], og, o0[329:358]]), np.concatenate([d0[300:329], dg, d0[329:358]])
    assert len(origins) == 64
    want = check(renderer, book(), origins, dirs, None)
    alone = tr.trace(book(), o0[300:358], d0[300:358])
    tr.same({k: np.concatenate([v[:29], v[35:]]) for k, v in want.items()}, alone)
    assert np.isnan(want["t"][29:35]).any()                                     # a NaN root was accepted, as written
    t_max = np.full(64, 7.5); t_max[::5] = math.nan
    check(renderer, book(), origins, dirs, t_max)


@pytest.mark.gpu
def test_book_scene_ties_the_feature_kernel_to_one_answer(renderer, oracle_mod):
    """The 37 x 19 camera rays: index equals the ids render_features returns for spp = 1, and the eight feature words are quantize / qs of
    the query's outputs."""
    flat = book().flat
    renderer.upload_scene(flat)
    o, d = book_camera_rays()
    got = renderer.trace_rays(o, d)
    tr.same(got, tr.trace(book(), o, d))
    feat, ids, _ = renderer.render_features(rt.book1_camera(BW, BH), rt.make_params(BW, BH, 1, seed=1))
    assert np.array_equal(got["index"].reshape(BH, BW), ids)
    words = np.zeros((BW * BH, 8), dtype=np.uint64)
    for k in np.flatnonzero(got["index"] >= 0):
        rec = flat[got["index"][k]]
        albedo = (1.0, 1.0, 1.0) if int(rec["kind"]) == fr.KIND_DIALECTRIC else tuple(float(x) for x in rec["albedo"])
        words[k] = [fr.quantize(a) for a in albedo] + [fr.qs(float(x)) for x in got["normal"][k]] + [fr.quantize(float(got["t"][k])), 1]
    assert np.array_equal(words.reshape(BH, BW, 8), feat)
    assert (ids >= 0).any() and (ids < 0).any()


@pytest.mark.gpu
def test_optional_outputs(renderer, oracle_mod):
    origins, dirs, t_max, want = book_batch()
    renderer.upload_scene(book().flat)
    names = ("t", "point", "normal", "front_face")
    for drop in names:
        keep = tuple(n for n in names if n != drop)
        got = renderer.trace_rays(origins, dirs, t_max, want=keep)
        assert drop not in got
        tr.same(got, want, names=("index",) + keep)
    tr.same(renderer.trace_rays(origins, dirs, t_max, want=()), want, names=("index",))


@pytest.mark.gpu
def test_knobs_give_equal_bytes(renderer, oracle_mod, monkeypatch):
    """Either candidate scheme, a launch capped at ONE workgroup (n = 1 000: four trips of the grid-stride loop per wave), no grid and a
    9 x 9 grid (81 cells: the row words in LDS on a scene that ships with a small grid): the reference's bytes every time."""
    origins, dirs, t_max, want = book_batch()
    for env in ({}, {"RTIOW_NO_GRID": "1"}, {"RTIOW_GRID_DIM": "9"}):
        for k in ("RTIOW_NO_GRID", "RTIOW_GRID_DIM"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        renderer.upload_scene(book().flat)                                      # the grid knobs are read here
        for scheme in ("wave", "ray"):
            monkeypatch.setenv("RTIOW_TRACE_CANDIDATES", scheme)
            for blocks in (None, "1"):
                if blocks:
                    monkeypatch.setenv("RTIOW_TRACE_GRID_BLOCKS", blocks)
                else:
                    monkeypatch.delenv("RTIOW_TRACE_GRID_BLOCKS", raising=False)
                check(renderer, book(), origins, dirs, t_max, want=want)
        monkeypatch.delenv("RTIOW_TRACE_GRID_BLOCKS", raising=False)
        monkeypatch.delenv("RTIOW_TRACE_CANDIDATES", raising=False)


@pytest.mark.gpu
def test_position_in_the_batch_does_not_matter(renderer, oracle_mod, monkeypatch):
    origins, dirs, t_max, want = book_batch()
    renderer.upload_scene(book().flat)
    perm = np.random.default_rng(9).permutation(len(t_max))
    for scheme in ("wave", "ray"):
        monkeypatch.setenv("RTIOW_TRACE_CANDIDATES", scheme)
        check(renderer, book(), origins[perm], dirs[perm], t_max[perm], want=tr.permuted(want, perm))


@pytest.mark.gpu
def test_device_form_and_torch_equal_the_host_form(renderer, oracle_mod):
    """rt_trace_rays_device / rt_occluded_device on torch tensors, launched on a NON-default torch stream through trace_rays_torch, give
    the host form's bytes; with and without t_max, with a subset of the outputs."""
    import torch
    origins, dirs, t_max, want = book_batch()
    renderer.upload_scene(book().flat)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)
    O, D, Tm = to(origins), to(dirs), to(t_max)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        got = rt.trace_rays_torch(renderer, O, D, Tm)
        occ = rt.occluded_torch(renderer, O, D, Tm)["occluded"]
        some = rt.trace_rays_torch(renderer, O, D, None, want=("t",))
    stream.synchronize()
    assert got["index"].dtype == torch.int32 and got["front_face"].dtype == torch.uint8 and got["point"].shape == (1000, 3)
    tr.same({k: v.cpu().numpy() for k, v in got.items()}, want)
    assert np.array_equal(occ.cpu().numpy(), (want["index"] >= 0).astype(np.uint8))
    assert set(some) == {"index", "t"}
    tr.same({k: v.cpu().numpy() for k, v in some.items()}, renderer.trace_rays(origins, dirs), names=("index", "t"))
    with pytest.raises(ValueError):
        rt.trace_rays_torch(renderer, O.float(), D, None)
    with pytest.raises(ValueError, match="unknown outputs"):
        rt.trace_rays_torch(renderer, O, D, None, want=("t", "depth"))
    with pytest.raises(ValueError, match="renderer's device"):
        rt.trace_rays_torch(renderer, O.cpu(), D.cpu(), None)
    with pytest.raises(ValueError, match="renderer's device"):
        rt.occluded_torch(renderer, O.cpu(), D.cpu(), None)
    assert renderer.device_id == 0 and set(renderer.occluded(origins, dirs, t_max)) == {"occluded", "kernel_ms"}
    # n == 0 succeeds and touches nothing
    empty = renderer.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty["index"].shape == (0,) and renderer.occluded(np.zeros((0, 3)), np.zeros((0, 3)))["occluded"].shape == (0,)


@pytest.mark.gpu
def test_a_query_before_an_upload_and_stats(oracle_mod):
    """RT_ERR_NO_SCENE before an upload; a query takes no launch slot: rt_last_stats still reports the render before it."""
    with rt.Renderer(0) as r:
        with pytest.raises(rt.RtiowHipError, match="rt_upload_scene has not been called"):
            r.trace_rays(np.zeros((1, 3)), np.ones((1, 3)))
        with pytest.raises(rt.RtiowHipError, match="rt_upload_scene has not been called"):
            r.occluded(np.zeros((1, 3)), np.ones((1, 3)))
        r.upload_scene(book().flat)
        _, _, st = r.render(rt.book1_camera(16, 9), rt.make_params(16, 9, 2, seed=3))
        o, d = book_camera_rays()
        r.trace_rays(o[:100], d[:100])
        after = r.last_stats()
        assert after["rays_traced"] == st["rays_traced"] and after["samples"] == st["samples"] == 16 * 9 * 2


@pytest.mark.gpu
def test_a_scan_mode_1_context_refuses_a_query(oracle_mod):
    """RT_ERR_INVALID_ARGUMENT (-1) from all four forms on a context created under RTIOW_SCAN_MODE=1, with or without a scene, and nothing
    is written to the device outputs."""
    import torch
    n = 70
    o0, d0 = book_camera_rays()
    O, D = torch.from_numpy(np.array(o0[:n])).cuda(), torch.from_numpy(np.array(d0[:n])).cuda()
    index = torch.full((n,), 0x5A5A, dtype=torch.int32, device="cuda:0")
    t = torch.full((n,), 7.25, dtype=torch.float64, device="cuda:0")
    occ = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")
    os.environ["RTIOW_SCAN_MODE"] = "1"
    try:
        r = rt.Renderer(0)                                               # RTIOW_SCAN_MODE is read here
    finally:
        os.environ.pop("RTIOW_SCAN_MODE")
    try:
        for uploaded in (False, True):
            if uploaded:
                r.upload_scene(book().flat)
            with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
                r.trace_rays_device(n, O.data_ptr(), D.data_ptr(), index.data_ptr(), d_t_ptr=t.data_ptr())
            with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
                r.occluded_device(n, O.data_ptr(), D.data_ptr(), occ.data_ptr())
            with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
                r.trace_rays(o0[:n], d0[:n])
            with pytest.raises(rt.RtiowHipError, match=r"\(-1\).*RTIOW_SCAN_MODE=1"):
                r.occluded(o0[:n], d0[:n])
    finally:
        r.close()
    torch.cuda.synchronize()
    assert (index == 0x5A5A).all().item() and (t == 7.25).all().item() and (occ == 0x5A).all().item()


@pytest.mark.gpu
def test_pick_of_the_cli_equals_the_python_answer(renderer, oracle_mod):
    exe = os.path.join(ROOT, "host", "rtiow_render")
    w, h = 64, 36
    cam = rt.book1_camera(w, h).to_rt_camera()
    renderer.upload_scene(book().flat)
    kinds = {0: "lambertian", 1: "metal", 2: "dialectric", -1: "none"}
    seen = set()
    for i, j in ((32, 18), (5, 30), (40, 9), (63, 35)):
        u, v = (float(i) + 0.5) / float(w - 1), (float(j) + 0.5) / float(h - 1)
        o = np.array(cam.origin[:])
        d = np.array([((cam.lower_left_corner[k] + u * cam.horizontal[k]) + v * cam.vertical[k]) - cam.origin[k] for k in range(3)])
        got = renderer.trace_rays(o[None], d[None], want=("t", "point"))
        tr.same(got, tr.trace(book(), o[None], d[None]), names=("index", "t", "point"))
        run = subprocess.run([exe, "--width", str(w), "--height", str(h), "--pick", f"{i},{j}"], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        m = re.match(r"pick (\d+) (\d+): index (-?\d+) kind (\w+) t (\S+) point (\S+) (\S+) (\S+)\s*$", run.stdout)
        assert m, run.stdout
        idx = int(got["index"][0])
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (i, j, idx)
        assert m.group(4) == kinds[int(book().flat[idx]["kind"]) if idx >= 0 else -1]
        assert float(m.group(5)) == got["t"][0] and [float(m.group(k)) for k in (6, 7, 8)] == got["point"][0].tolist()
        seen.add(idx >= 0)
    assert seen == {True, False}
    bad = subprocess.run([exe, "--width", str(w), "--height", str(h), "--pick", "64,0"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--pick" in bad.stderr
