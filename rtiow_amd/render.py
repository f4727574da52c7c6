"""Renderer: the host-side caller of the C ABI (stands in for main.rs:122-147).

Nothing here computes radiance: every pixel comes from librtiow_hip.so.
"""
import ctypes as C

import numpy as np

from . import _ffi
from .scene import SPHERE_DTYPE


def make_params(width, height, spp, *, sample_begin=0, max_depth=50, t_min=1e-4, seed=1,
                tile_rows=8, shard_index=0, shard_count=1, flags=0):
    p = _ffi.rt_params()
    p.width, p.height, p.spp, p.sample_begin = int(width), int(height), int(spp), int(sample_begin)
    p.max_depth, p.t_min, p.seed = int(max_depth), float(t_min), int(seed)
    p.tile_rows, p.shard_index, p.shard_count, p.flags = int(tile_rows), int(shard_index), int(shard_count), int(flags)
    return p


def make_adaptive(step, threshold, dark_floor=0.01):
    """rt_adaptive: `step` samples per pass, stop below `threshold` (relative to max(mean radiance, dark_floor))."""
    a = _ffi.rt_adaptive()
    a.step, a.reserved, a.threshold, a.dark_floor = int(step), 0, float(threshold), float(dark_floor)
    return a


def select_pixels_host(fix, half, count, n, adaptive):
    """The adaptive selection on host arrays (rt_select_pixels_host, no GPU): fix, half u64 [H,W,3], count u32 [H,W] ->
    the active pixels' numbers g = j * W + i, ascending (u32)."""
    lib = _ffi.load()
    fix = np.ascontiguousarray(fix, dtype=np.uint64)
    half = np.ascontiguousarray(half, dtype=np.uint64)
    count = np.ascontiguousarray(count, dtype=np.uint32)
    h, w = count.shape
    assert fix.shape == (h, w, 3) and half.shape == (h, w, 3)
    out = np.zeros(h * w, dtype=np.uint32)
    m = C.c_int64(0)
    _ffi.check(lib.rt_select_pixels_host(fix.ctypes.data_as(C.c_void_p), half.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                                         w, h, int(n), C.byref(adaptive), out.ctypes.data_as(C.c_void_p), C.byref(m)), "rt_select_pixels_host")
    return out[:m.value].copy()


def make_denoise(levels=4, sigma_color=0.35, sigma_normal=1.0, sigma_depth=0.2, demodulate=True):
    """rt_denoise: `levels` a-trous levels (hole step 2^l), the edge-stop widths on colour (halved per level), normal and relative depth,
    and whether the filter runs on radiance divided by the first-hit albedo.  The defaults are the best of the sweep in DESIGN.md section 15."""
    d = _ffi.rt_denoise()
    d.levels, d.flags = int(levels), _ffi.RT_DENOISE_DEMODULATE if demodulate else 0
    d.sigma_color, d.sigma_normal, d.sigma_depth = float(sigma_color), float(sigma_normal), float(sigma_depth)
    return d


def _denoise_arrays(fix, feat, count):
    fix = np.ascontiguousarray(fix, dtype=np.uint64)
    feat = np.ascontiguousarray(feat, dtype=np.uint64)
    h, w = fix.shape[0], fix.shape[1]
    assert fix.shape == (h, w, 3) and feat.shape == (h, w, _ffi.RT_FEATURE_WORDS)
    if count is not None:
        count = np.ascontiguousarray(count, dtype=np.uint32)
        assert count.shape == (h, w)
    return fix, feat, count, h, w


def denoise_host(fix, spp, feat, feat_spp, denoise=None, count=None):
    """rt_denoise_host (no GPU): the library's CPU statement of the denoiser.  fix u64 [H,W,3] of `spp` samples (or of count[H,W] u32
    samples per pixel), feat u64 [H,W,8] of `feat_spp` samples -> the denoised one-sample frame u64 [H,W,3]."""
    lib = _ffi.load()
    fix, feat, count, h, w = _denoise_arrays(fix, feat, count)
    dn = denoise if denoise is not None else make_denoise()
    out = np.zeros((h, w, 3), dtype=np.uint64)
    _ffi.check(lib.rt_denoise_host(fix.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p) if count is not None else None, int(spp),
                                   feat.ctypes.data_as(C.c_void_p), int(feat_spp), w, h, C.byref(dn), out.ctypes.data_as(C.c_void_p)),
               "rt_denoise_host")
    return out


DENOISE_VAR_SIGMA_COLOR = 1.0


def make_denoise_var(levels=4, sigma_color=DENOISE_VAR_SIGMA_COLOR, sigma_normal=1.0, sigma_depth=0.2, demodulate=True):
    """The rt_denoise of the variance-guided denoiser (rt_denoise_var*): as make_denoise, but sigma_color is in STANDARD DEVIATIONS of the
    pixel's own noise and does not halve per level.  Its default is the choice of the sweep in DESIGN.md section 25."""
    return make_denoise(levels, sigma_color, sigma_normal, sigma_depth, demodulate)


def _denoise_var_arrays(fix, half, feat, count):
    fix, feat, count, h, w = _denoise_arrays(fix, feat, count)
    half = np.ascontiguousarray(half, dtype=np.uint64)
    assert half.shape == (h, w, 3)
    return fix, half, feat, count, h, w


def denoise_var_host(fix, half, spp, feat, feat_spp, denoise=None, count=None):
    """rt_denoise_var_host (no GPU): the library's CPU statement of the variance-guided denoiser.  As denoise_host, with half u64 [H,W,3]:
    the sums of half of each pixel's samples (render_adaptive's `half`, or the first of two equal accumulated passes)."""
    lib = _ffi.load()
    fix, half, feat, count, h, w = _denoise_var_arrays(fix, half, feat, count)
    dn = denoise if denoise is not None else make_denoise_var()
    out = np.zeros((h, w, 3), dtype=np.uint64)
    _ffi.check(lib.rt_denoise_var_host(fix.ctypes.data_as(C.c_void_p), half.ctypes.data_as(C.c_void_p),
                                       count.ctypes.data_as(C.c_void_p) if count is not None else None, int(spp),
                                       feat.ctypes.data_as(C.c_void_p), int(feat_spp), w, h, C.byref(dn), out.ctypes.data_as(C.c_void_p)),
               "rt_denoise_var_host")
    return out


def make_temporal(alpha_min=0.1, sigma_normal=0.5, sigma_depth=0.1, clamp=True, clamp_scale=1.0):
    """rt_temporal: the least weight of the current frame, the widths of the normal and the relative-depth test that a history tap must
    pass, and whether the history is clamped to the box of the current frame's 3 x 3 neighbourhood (scaled about its centre by
    clamp_scale).  The defaults are those of the sweep in DESIGN.md section 16."""
    t = _ffi.rt_temporal()
    t.flags, t.reserved = (_ffi.RT_TEMPORAL_CLAMP if clamp else 0), 0
    t.alpha_min, t.sigma_normal, t.sigma_depth, t.clamp_scale = float(alpha_min), float(sigma_normal), float(sigma_depth), float(clamp_scale)
    return t


def _rt_cam(cam):
    return cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam


def _temporal_args(fix, spp, feat, feat_spp, cam, history, count):
    """The arguments the host-buffer forms of rt_temporal share, and what must stay alive while they are used.
    history: None (the first frame) or (prev_fix u64 [H,W,3], prev_len u32 [H,W], prev_feat u64 [H,W,8], prev_feat_spp, prev_cam)."""
    fix, feat, count, h, w = _denoise_arrays(fix, feat, count)
    keep = [fix, feat, count, _rt_cam(cam)]
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    if history is None:
        hist = (None, None, None, 0, None)
    else:
        pfix, plen, pfeat, pspp, pcam = history
        pfix, pfeat, plen, ph, pw = _denoise_arrays(pfix, pfeat, plen)
        assert (ph, pw) == (h, w) and plen is not None
        keep += [pfix, plen, pfeat, _rt_cam(pcam)]
        hist = (vp(pfix), vp(plen), vp(pfeat), int(pspp), C.byref(keep[-1]))
    out_fix = np.zeros((h, w, 3), dtype=np.uint64)
    out_len = np.zeros((h, w), dtype=np.uint32)
    head = (vp(fix), vp(count), int(spp), vp(feat), int(feat_spp), C.byref(keep[3]), *hist, w, h)
    return head, out_fix, out_len, keep


def temporal_host(fix, spp, feat, feat_spp, cam, history=None, temporal=None, count=None):
    """rt_temporal_host (no GPU): the library's CPU statement of temporal accumulation.  fix u64 [H,W,3] of `spp` samples (or of
    count[H,W] u32 samples per pixel), feat u64 [H,W,8] of `feat_spp` samples and the frame's camera; history: None for the first frame,
    else (prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam) -- the previous call's two results, the previous frame's feature sums
    and camera.  Returns (the accumulated one-sample frame u64 [H,W,3], the history lengths u32 [H,W])."""
    lib = _ffi.load()
    tp = temporal if temporal is not None else make_temporal()
    head, out_fix, out_len, keep = _temporal_args(fix, spp, feat, feat_spp, cam, history, count)
    _ffi.check(lib.rt_temporal_host(*head, C.byref(tp), out_fix.ctypes.data_as(C.c_void_p), out_len.ctypes.data_as(C.c_void_p)), "rt_temporal_host")
    return out_fix, out_len


# the default sigma_color of render_sequence_var: the swept value with the lowest final-frame RMSE on the night sequence
# (tools/temporal_var_sweep.py, profiles/temporal_var_sweep.txt)
TEMPORAL_VAR_SIGMA_COLOR = 1.5


def _temporal_var_args(fix, spp, feat, feat_spp, cam, history, count):
    """_temporal_args with the second moment: history is None or (prev_fix, prev_len, prev_feat, prev_feat_spp, prev_cam, prev_m2 f64 [H,W,3]).
    -> (head, out_fix, out_len, out_m2, out_var, keep); head ends with prev_m2, width, height."""
    head, out_fix, out_len, keep = _temporal_args(fix, spp, feat, feat_spp, cam, None if history is None else history[:5], count)
    h, w = out_len.shape
    pm2 = None
    if history is not None:
        pm2 = np.ascontiguousarray(history[5], dtype=np.float64)
        assert pm2.shape == (h, w, 3)
        keep.append(pm2)
    head = (*head[:-2], pm2.ctypes.data_as(C.c_void_p) if pm2 is not None else None, w, h)
    return head, out_fix, out_len, np.zeros((h, w, 3), dtype=np.float64), np.zeros((h, w, 3), dtype=np.float64), keep


def temporal_var_host(fix, spp, feat, feat_spp, cam, history=None, temporal=None, count=None):
    """rt_temporal_var_host (no GPU): temporal_host with second moments.  history: None for the first frame, else (prev_fix, prev_len,
    prev_feat, prev_feat_spp, prev_cam, prev_m2) -- the previous call's out_fix, out_len and out_m2, the previous frame's feature sums and
    camera.  Returns (out_fix u64 [H,W,3], out_len u32 [H,W], out_m2 f64 [H,W,3], out_var f64 [H,W,3]: the variance of the accumulated value)."""
    lib = _ffi.load()
    tp = temporal if temporal is not None else make_temporal()
    head, out_fix, out_len, out_m2, out_var, keep = _temporal_var_args(fix, spp, feat, feat_spp, cam, history, count)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _ffi.check(lib.rt_temporal_var_host(*head, C.byref(tp), vp(out_fix), vp(out_len), vp(out_m2), vp(out_var)), "rt_temporal_var_host")
    return out_fix, out_len, out_m2, out_var


def _denoise_var_given_arrays(fix, var, feat, count):
    fix, feat, count, h, w = _denoise_arrays(fix, feat, count)
    var = np.ascontiguousarray(var, dtype=np.float64)
    assert var.shape == (h, w, 3)
    return fix, var, feat, count, h, w


def denoise_var_given_host(fix, var, spp, feat, feat_spp, denoise=None, count=None):
    """rt_denoise_var_given_host (no GPU): denoise_var_host with the variance given -- var f64 [H,W,3], per channel the variance of the
    pixel's mean in radiance units (temporal_var's out_var, with its out_fix and spp = 1)."""
    lib = _ffi.load()
    fix, var, feat, count, h, w = _denoise_var_given_arrays(fix, var, feat, count)
    dn = denoise if denoise is not None else make_denoise_var()
    out = np.zeros((h, w, 3), dtype=np.uint64)
    _ffi.check(lib.rt_denoise_var_given_host(fix.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p),
                                             count.ctypes.data_as(C.c_void_p) if count is not None else None, int(spp),
                                             feat.ctypes.data_as(C.c_void_p), int(feat_spp), w, h, C.byref(dn), out.ctypes.data_as(C.c_void_p)),
               "rt_denoise_var_given_host")
    return out


def shard_rows(params):
    lib = _ffi.load()
    rows = C.c_int32(0)
    _ffi.check(lib.rt_shard_rows(C.byref(params), C.byref(rows)), "rt_shard_rows")
    return rows.value


def shard_row_indices(params):
    """Image row j (0 = bottom) of every compact row of the shard."""
    lib = _ffi.load()
    n = shard_rows(params)
    out = np.empty(n, dtype=np.int32)
    j = C.c_int32(0)
    for r in range(n):
        _ffi.check(lib.rt_shard_row_index(C.byref(params), r, C.byref(j)), "rt_shard_row_index")
        out[r] = j.value
    return out


def stats_dict(st):
    out = {}
    for k, _ in _ffi.rt_stats._fields_:
        v = getattr(st, k)
        out[k] = list(v) if hasattr(v, "__len__") else v
    return out


def tile_layout_host(flat):
    """Where rt_upload_scene puts each sphere in the filter's table of columns (rt_tile_layout_host, no GPU):
    ((grid_dim, n_global), grid[8] f32, slot_of[columns] i32 with -1 for padding)."""
    lib = _ffi.load()
    flat = np.ascontiguousarray(flat, dtype=SPHERE_DTYPE)
    dims = (C.c_int32 * 2)()
    grid = (C.c_float * 8)()
    cap = 2 * len(flat) + (48 + 63 * 63) * 32 + 64
    slot = np.full(cap, -2, dtype=np.int32)
    n = lib.rt_tile_layout_host(flat.ctypes.data_as(C.POINTER(_ffi.rt_sphere)), len(flat), dims, grid,
                                slot.ctypes.data_as(C.POINTER(C.c_int32)), len(slot))
    if n < 0:
        _ffi.check(n, "rt_tile_layout_host")
    return (int(dims[0]), int(dims[1])), np.array(list(grid), dtype=np.float32), slot[:n].copy()


def tube_tile_host(spheres32):
    """Host-side half of one tube-filter tile (no GPU): words (64, 4) u32, bound (32,) f32, rho."""
    lib = _ffi.load()
    sp = np.ascontiguousarray(spheres32)
    assert sp.shape == (32,) and sp.dtype.itemsize == C.sizeof(_ffi.rt_sphere)
    words = np.zeros((64, 4), dtype=np.uint32)
    bound = np.zeros(32, dtype=np.float32)
    rho = C.c_float(0.0)
    _ffi.check(lib.rt_tube_tile_host(sp.ctypes.data_as(C.POINTER(_ffi.rt_sphere)), words.ctypes.data_as(C.c_void_p),
                                     bound.ctypes.data_as(C.c_void_p), C.byref(rho)), "rt_tube_tile_host")
    return words, bound, float(rho.value)


_TRACE_OUTPUTS = ("t", "point", "normal", "front_face")


def _check_want(want):
    unknown = set(want) - set(_TRACE_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")


def _torch_rays(torch, renderer, origins, dirs, t_max):
    n = origins.shape[0] if origins.dim() == 2 else -1
    if not origins.is_cuda or origins.device.index != renderer.device_id:
        raise ValueError(f"origins must be on the renderer's device cuda:{renderer.device_id} (is on {origins.device})")
    tensors = [("origins", origins, (n, 3)), ("dirs", dirs, (n, 3))] + ([("t_max", t_max, (n,))] if t_max is not None else [])
    for name, x, shape in tensors:
        if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or tuple(x.shape) != shape or x.device != origins.device:
            raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape} on the renderer's device")
    return n


def trace_rays_torch(renderer, origins, dirs, t_max=None, t_min=1e-4, want=("t", "point", "normal", "front_face")):
    """Renderer.trace_rays on torch tensors: contiguous float64 tensors on the context's device, launched on torch.cuda.current_stream();
    returns a dict of torch tensors ("index" int32, and what `want` names)."""
    import torch
    _check_want(want)
    n = _torch_rays(torch, renderer, origins, dirs, t_max)
    dev = origins.device
    out = {"index": torch.empty(n, dtype=torch.int32, device=dev)}
    shapes = {"t": ((n,), torch.float64), "point": ((n, 3), torch.float64), "normal": ((n, 3), torch.float64), "front_face": ((n,), torch.uint8)}
    for name in ("t", "point", "normal", "front_face"):
        if name in want:
            out[name] = torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev)
    ptr = lambda name: out[name].data_ptr() if name in out else 0
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        renderer.trace_rays_device(n, origins.data_ptr(), dirs.data_ptr(), ptr("index"), t_max.data_ptr() if t_max is not None else 0, t_min,
                                   ptr("t"), ptr("point"), ptr("normal"), ptr("front_face"), stream)
    return out


def occluded_torch(renderer, origins, dirs, t_max=None, t_min=1e-4):
    """Renderer.occluded on torch tensors, on torch.cuda.current_stream(): a dict with "occluded", a uint8 tensor [n]."""
    import torch
    n = _torch_rays(torch, renderer, origins, dirs, t_max)
    occ = torch.empty(n, dtype=torch.uint8, device=origins.device)
    with torch.cuda.device(origins.device):
        renderer.occluded_device(n, origins.data_ptr(), dirs.data_ptr(), occ.data_ptr(), t_max.data_ptr() if t_max is not None else 0, t_min,
                                 torch.cuda.current_stream().cuda_stream)
    return {"occluded": occ}

# -- wavefront path steps on torch tensors (rt_camera_rays / rt_scatter / rt_accumulate) ------------------------
# The 32-bit unsigned arrays of the C ABI (pixel, sample, event) travel as int32 tensors and the u64 sums as an int64 tensor, each
# holding the same bits.

def _torch_check(torch, renderer, items):
    """items: (name, tensor, dtype, shape); every tensor contiguous, on the renderer's device."""
    for name, x, dtype, shape in items:
        if not x.is_cuda or x.device.index != renderer.device_id:
            raise ValueError(f"{name} must be on the renderer's device cuda:{renderer.device_id} (is on {x.device})")
        if x.dtype != dtype or not x.is_contiguous() or tuple(x.shape) != shape:
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} (is {x.dtype} {tuple(x.shape)})")


def camera_rays_torch(renderer, cam, width, height, seed, pixel, sample):
    """Renderer.camera_rays on torch tensors, on torch.cuda.current_stream(): pixel, sample int32 [n] -> a dict of "origin", "dir"
    float64 [n, 3] and "event" int32 [n]."""
    import torch
    n = pixel.shape[0] if pixel.dim() == 1 else -1
    _torch_check(torch, renderer, [("pixel", pixel, torch.int32, (n,)), ("sample", sample, torch.int32, (n,))])
    dev = pixel.device
    out = {"origin": torch.empty((n, 3), dtype=torch.float64, device=dev), "dir": torch.empty((n, 3), dtype=torch.float64, device=dev),
           "event": torch.empty(n, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        renderer.camera_rays_device(cam, width, height, seed, n, pixel.data_ptr(), sample.data_ptr(), out["origin"].data_ptr(),
                                    out["dir"].data_ptr(), out["event"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def scatter_torch(renderer, seed, dirs, index, point, normal, front_face, pixel, sample, event, out=None):
    """Renderer.scatter on torch tensors, on torch.cuda.current_stream().  dirs, point, normal float64 [n, 3]; index, pixel, sample, event
    int32 [n]; front_face uint8 [n] -- the hit exactly as trace_rays_torch returns it.  `event` is advanced in place.  out (optional): a
    dict of tensors to write to, any of "out_origin", "out_dir" (may be `dirs` itself), "attenuation" float64 [n, 3], "status" uint8 [n];
    what it does not name is allocated (uninitialised where the step does not write).  Returns the dict of the four outputs."""
    import torch
    n = index.shape[0] if index.dim() == 1 else -1
    dev = index.device
    res = dict(out or {})
    for name in ("out_origin", "out_dir", "attenuation"):
        if name not in res:
            res[name] = torch.empty((n, 3), dtype=torch.float64, device=dev)
    if "status" not in res:
        res["status"] = torch.empty(n, dtype=torch.uint8, device=dev)
    _torch_check(torch, renderer, [("dirs", dirs, torch.float64, (n, 3)), ("index", index, torch.int32, (n,)), ("point", point, torch.float64, (n, 3)),
                                   ("normal", normal, torch.float64, (n, 3)), ("front_face", front_face, torch.uint8, (n,)),
                                   ("pixel", pixel, torch.int32, (n,)), ("sample", sample, torch.int32, (n,)), ("event", event, torch.int32, (n,)),
                                   ("out_origin", res["out_origin"], torch.float64, (n, 3)), ("out_dir", res["out_dir"], torch.float64, (n, 3)),
                                   ("attenuation", res["attenuation"], torch.float64, (n, 3)), ("status", res["status"], torch.uint8, (n,))])
    with torch.cuda.device(dev):
        renderer.scatter_device(seed, n, dirs.data_ptr(), index.data_ptr(), point.data_ptr(), normal.data_ptr(), front_face.data_ptr(),
                                pixel.data_ptr(), sample.data_ptr(), event.data_ptr(), res["out_origin"].data_ptr(), res["out_dir"].data_ptr(),
                                res["attenuation"].data_ptr(), res["status"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    return res


def accumulate_torch(renderer, fix, pixel, weight, sky_dir=None, select=None):
    """Renderer.accumulate on torch tensors, on torch.cuda.current_stream(): adds to `fix`, an int64 tensor [..., 3] holding the u64 sums'
    bits (entry pixel[k] of its flattened [npix, 3]).  pixel int32 [n], weight float64 [n, 3], sky_dir float64 [n, 3] or None, select
    uint8 [n] or None."""
    import torch
    n = pixel.shape[0] if pixel.dim() == 1 else -1
    items = [("fix", fix, torch.int64, tuple(fix.shape)), ("pixel", pixel, torch.int32, (n,)), ("weight", weight, torch.float64, (n, 3))]
    if sky_dir is not None:
        items.append(("sky_dir", sky_dir, torch.float64, (n, 3)))
    if select is not None:
        items.append(("select", select, torch.uint8, (n,)))
    _torch_check(torch, renderer, items)
    if fix.dim() < 1 or fix.shape[-1] != 3:
        raise ValueError(f"fix must be [..., 3] (is {tuple(fix.shape)})")
    with torch.cuda.device(fix.device):
        renderer.accumulate_device(n, pixel.data_ptr(), weight.data_ptr(), fix.data_ptr(), fix.numel() // 3,
                                   sky_dir.data_ptr() if sky_dir is not None else 0, select.data_ptr() if select is not None else 0,
                                   torch.cuda.current_stream().cuda_stream)


def render_wavefront_torch(renderer, cam, params, batch=1 << 20):
    """The reference wavefront integrator: rt_render's frame from nothing but the path steps, the ray query and torch indexing, on
    torch.cuda.current_stream().  Batches of `batch` (pixel, sample) pairs, pixel-major; each batch: camera rays, then up to max_depth
    times { closest hit; the misses add throughput * sky to the sums; scatter; throughput *= attenuation; ended paths are dropped }.
    Honours width, height, spp, sample_begin, max_depth, t_min and seed of `params` (flags 0, shard_count 1).  Returns (the sums as an
    int64 tensor [H, W, 3] holding the u64 bits rt_render_device writes, the number of rays traced)."""
    import torch
    if params.flags != 0 or params.shard_count != 1:
        raise ValueError("render_wavefront_torch takes flags == 0 and shard_count == 1")
    if batch < 1:
        raise ValueError("batch must be >= 1")
    W, H, spp, seed = int(params.width), int(params.height), int(params.spp), int(params.seed)
    dev = torch.device("cuda", renderer.device_id)
    fix = torch.zeros((H, W, 3), dtype=torch.int64, device=dev)
    total, rays = W * H * spp, 0
    for begin in range(0, total, int(batch)):
        item = torch.arange(begin, min(begin + int(batch), total), dtype=torch.int64, device=dev)
        pixel = torch.div(item, spp, rounding_mode="floor").to(torch.int32)
        sample = (item % spp + int(params.sample_begin)).to(torch.int32)
        cr = camera_rays_torch(renderer, cam, W, H, seed, pixel, sample)
        origin, dirs, event = cr["origin"], cr["dir"], cr["event"]
        thr = torch.ones((pixel.shape[0], 3), dtype=torch.float64, device=dev)
        for _ in range(int(params.max_depth)):
            if pixel.shape[0] == 0:
                break
            rays += int(pixel.shape[0])
            hit = trace_rays_torch(renderer, origin, dirs, t_min=float(params.t_min), want=("point", "normal", "front_face"))
            accumulate_torch(renderer, fix, pixel, thr, sky_dir=dirs, select=(hit["index"] < 0).to(torch.uint8))
            sc = scatter_torch(renderer, seed, dirs, hit["index"], hit["point"], hit["normal"], hit["front_face"], pixel, sample, event)
            keep = torch.nonzero(sc["status"] == _ffi.RT_SCATTER_SCATTERED).squeeze(1)      # (the one host wait of a bounce: its length)
            thr = thr[keep] * sc["attenuation"][keep]
            pixel, sample, event, origin, dirs = pixel[keep], sample[keep], event[keep], sc["out_origin"][keep], sc["out_dir"][keep]
    return fix, rays


# -- the device path queue (rt_paths_begin_device / rt_paths_step_device) -----------------------------------------

class PathQueue:
    """An rt_path_queue of `capacity` slots as torch tensors on `device`: count int32 [1], pixel / sample / event int32 [capacity],
    origin / dir / throughput float64 [capacity, 3], scratch int32 [rt_path_scratch_words(capacity)] (the 32-bit unsigned arrays travel
    as int32 tensors holding the same bits).  The live paths are slots [0, count), and count lives on the device: reading it
    (`int(q.count)`) is a host wait the integrator itself never takes."""
    FIELDS = ("count", "pixel", "sample", "event", "origin", "dir", "throughput", "scratch")

    def __init__(self, capacity, device):
        import torch
        capacity = int(capacity)
        words = int(_ffi.load().rt_path_scratch_words(capacity))
        if words == 0:
            raise ValueError(f"capacity must be in [1, 2^24] (is {capacity})")
        self.capacity, self.device = capacity, torch.device(device)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=self.device)
        f64 = lambda: torch.zeros((capacity, 3), dtype=torch.float64, device=self.device)
        self.count, self.pixel, self.sample, self.event = i32(1), i32(capacity), i32(capacity), i32(capacity)
        self.origin, self.dir, self.throughput = f64(), f64(), f64()
        self.scratch = i32(words)

    def struct(self):
        """The rt_path_queue naming the tensors' memory (valid while they live)."""
        return _ffi.rt_path_queue(self.capacity, *[getattr(self, f).data_ptr() for f in self.FIELDS])


def _check_queue(renderer, q, name):
    if q.device.type != "cuda" or q.device.index != renderer.device_id:
        raise ValueError(f"{name} must be on the renderer's device cuda:{renderer.device_id} (is on {q.device})")


def paths_begin_torch(renderer, cam, width, height, seed, spp, sample_begin, first_item, n, queue):
    """rt_paths_begin_device on a PathQueue, on torch.cuda.current_stream(): slots [0, n) become the items first_item .. first_item + n - 1
    (pixel = item // spp, sample = sample_begin + item % spp) with their camera rays, throughput 1; count = n.  No host wait."""
    import torch
    _check_queue(renderer, queue, "queue")
    with torch.cuda.device(queue.device):
        renderer.paths_begin_device(cam, width, height, seed, spp, sample_begin, first_item, n, queue.struct(), torch.cuda.current_stream().cuda_stream)


def paths_begin_pixels_torch(renderer, cam, width, height, seed, spp, sample_begin, first_item, n, pixels, queue):
    """rt_paths_begin_pixels_device on a PathQueue, on torch.cuda.current_stream(): slots [0, n) become the items first_item ..
    first_item + n - 1 of the LIST (index = item // spp, pixel = pixels[index], sample = sample_begin + item % spp) with their camera rays
    over the full width x height frame, throughput 1; count = n.  pixels: an int32 tensor on the renderer's device holding the u32 pixel
    numbers.  No host wait."""
    import torch
    _check_queue(renderer, queue, "queue")
    _torch_check(torch, renderer, [("pixels", pixels, torch.int32, (pixels.shape[0] if pixels.dim() else 0,))])
    with torch.cuda.device(queue.device):
        renderer.paths_begin_pixels_device(cam, width, height, seed, spp, sample_begin, first_item, n, pixels.data_ptr(), int(pixels.shape[0]),
                                           queue.struct(), torch.cuda.current_stream().cuda_stream)


class Lighting:
    """What lights a frame of the path queue (rt_lighting): the sky's colour where the unit direction's y is -1
    (sky_bottom) and +1 (sky_top), and the radiance of emissive spheres.  emission: None (no lights), an [n, 3] array with one row per
    sphere of the scene in list order, a {sphere index: (r, g, b)} dict (every other sphere emits nothing), or -- for the device forms --
    a float64 torch tensor [n, 3] on the renderer's device.  A sphere is a light iff a channel of its row is > 0; a path that hits a
    light adds throughput * e and ends.  The defaults are the reference's sky and no light: the unlit frame bit for bit."""

    def __init__(self, sky_bottom=(1.0, 1.0, 1.0), sky_top=(0.5, 0.7, 1.0), emission=None):
        self.sky_bottom, self.sky_top = tuple(float(x) for x in sky_bottom), tuple(float(x) for x in sky_top)
        if len(self.sky_bottom) != 3 or len(self.sky_top) != 3:
            raise ValueError("sky_bottom and sky_top are (r, g, b)")
        self.emission = emission
        self._device_table = self._device_lights = self._device_list = None

    def _is_tensor(self):
        return hasattr(self.emission, "data_ptr")

    def table(self, n_spheres):
        """The emission as a contiguous float64 array [n_spheres, 3] on the host, or None."""
        e = self.emission
        if e is None:
            return None
        if self._is_tensor():
            e = e.detach().cpu().numpy()
        if isinstance(e, dict):
            out = np.zeros((int(n_spheres), 3), dtype=np.float64)
            for index, rgb in e.items():
                if not 0 <= int(index) < int(n_spheres):
                    raise ValueError(f"emission names sphere {index}; the scene has {n_spheres}")
                out[int(index)] = rgb
            return out
        out = np.ascontiguousarray(e, dtype=np.float64)
        if out.ndim != 2 or out.shape[1] != 3:
            raise ValueError(f"emission must be [n, 3] (is {out.shape})")
        return out

    def device_table(self, renderer):
        """The emission as a float64 tensor [n, 3] on the renderer's device (kept alive by this object), or None."""
        if self.emission is None:
            return None
        import torch
        t = self.emission
        if not self._is_tensor():
            key = (renderer.n_spheres or 0, renderer.device_id)
            if self._device_table is None or self._device_table[0] != key:          # (built once per scene length: the object is a value)
                self._device_table = (key, torch.from_numpy(np.array(self.table(key[0]))).to(torch.device("cuda", renderer.device_id)))
            t = self._device_table[1]
        _torch_check(torch, renderer, [("emission", t, torch.float64, (t.shape[0] if t.dim() else 0, 3))])
        return t

    def light_list(self, n_spheres):
        """rt_light_list of the emission table: the indices of the spheres that are lights, ascending, as an int32 array -- what direct
        lighting (direct=True) samples."""
        table = self.table(n_spheres)
        rows = 0 if table is None else int(table.shape[0])
        out, n = np.zeros(max(rows, 1), dtype=np.int32), C.c_int32(0)
        _ffi.check(_ffi.load().rt_light_list(table.ctypes.data if rows else None, rows, out.ctypes.data, C.byref(n)), "rt_light_list")
        return out[:n.value].copy()

    def device_lights(self, renderer, direct=True):
        """The light list as an int32 tensor on the renderer's device (kept alive by this object): light_list() for direct=True, else
        `direct` itself -- a sequence of sphere indices or an int32 tensor on the device."""
        import torch
        dev = torch.device("cuda", renderer.device_id)
        if direct is True:
            key = (renderer.n_spheres or 0, renderer.device_id)
            if self._device_lights is None or self._device_lights[0] != key:
                self._device_lights = (key, torch.from_numpy(self.light_list(key[0])).to(dev))
            t = self._device_lights[1]
        elif hasattr(direct, "data_ptr"):
            t = direct
        else:
            t = self._device_list = torch.tensor([int(x) for x in direct], dtype=torch.int32, device=dev)
        _torch_check(torch, renderer, [("direct", t, torch.int32, (t.shape[0] if t.dim() else 0,))])
        return t

    def struct(self, emission_ptr=None, n_emission=0):
        """The rt_lighting naming `emission_ptr` (host or device, as the entry point wants it)."""
        return _ffi.rt_lighting((C.c_double * 3)(*self.sky_bottom), (C.c_double * 3)(*self.sky_top), emission_ptr or None, int(n_emission), 0)


class Environment:
    """An environment cube map for the lit path queue (rt_environment): the background the camera sees and the light
    the scene is lit by.  texels: radiance [6, N, N, 3], N a power of two up to RT_ENV_MAX_SIZE -- a numpy array, or for the device forms a
    float64 torch tensor on the renderer's device.  Face f = 2 * axis + (negative ? 1 : 0); texel (f, i, j) covers the in-face
    coordinates a in [2 i / N - 1, 2 (i + 1) / N - 1) and b likewise from j, (a, b) being the other two axes in axis order.
    sample=True: Lambertian hits importance-sample the map by the running sums of rt_environment_cdf and trace a shadow ray towards
    it; sample=False: the map is only looked up by the paths that miss.  sums: running sums [6 * N * N] the device forms are to search
    in the place of rt_environment_cdf's (a numpy array; the host form always builds its own)."""

    def __init__(self, texels, sample=True, sums=None):
        self.texels, self.sample, self.given_sums = texels, bool(sample), sums
        shape = tuple(texels.shape)
        if len(shape) != 4 or shape[0] != 6 or shape[1] != shape[2] or shape[3] != 3:
            raise ValueError(f"texels must be [6, N, N, 3] (is {shape})")
        self.size = int(shape[1])
        if self.size < 1 or self.size > _ffi.RT_ENV_MAX_SIZE or self.size & (self.size - 1):
            raise ValueError(f"the face edge must be a power of two in [1, {_ffi.RT_ENV_MAX_SIZE}] (is {self.size})")
        self._device = None

    def _is_tensor(self):
        return hasattr(self.texels, "data_ptr")

    def table(self):
        """The texels as a contiguous float64 array [6, N, N, 3] on the host."""
        t = self.texels.detach().cpu().numpy() if self._is_tensor() else self.texels
        return np.ascontiguousarray(t, dtype=np.float64)

    def cdf(self):
        """rt_environment_cdf of the texels: the running sums [6 * N * N] that sampling searches, float64."""
        t = self.table()
        out = np.zeros(6 * self.size * self.size, dtype=np.float64)
        _ffi.check(_ffi.load().rt_environment_cdf(t.ctypes.data, self.size, out.ctypes.data), "rt_environment_cdf")
        return out

    def save(self, path):
        """The texels as raw little-endian float64; the size follows from the byte count."""
        with open(path, "wb") as f:
            f.write(self.table().astype("<f8").tobytes())

    @classmethod
    def load(cls, path, sample=True):
        raw = np.fromfile(path, dtype="<f8")
        n = int(round((raw.size / 18) ** 0.5)) if raw.size else 0
        if n < 1 or 18 * n * n != raw.size:
            raise ValueError(f"{path}: {raw.size * 8} bytes are not 6 * N * N * 3 float64")
        return cls(raw.astype(np.float64).reshape(6, n, n, 3), sample=sample)

    @classmethod
    def sun_sky(cls, size, sun_dir=(0.3, 0.8, 0.5), sun_radiance=(400.0, 360.0, 300.0), cos_radius=0.995, bottom=(1.0, 1.0, 1.0),
                top=(0.5, 0.7, 1.0), sample=True):
        """A procedural map: at each texel's centre direction u the sky bottom * (1 - t) + top * t with t = (u.y + 1) / 2, and where
        dot(u, unit(sun_dir)) >= cos_radius the sun's radiance on top of it; if no centre lies inside the sun's disc, the texel that
        sun_dir names gets it."""
        n = int(size)
        centre = (np.arange(n, dtype=np.float64) + 0.5) * (2.0 / n) - 1.0
        a, b = np.meshgrid(centre, centre, indexing="ij")
        texels = np.zeros((6, n, n, 3), dtype=np.float64)
        sun = np.asarray(sun_dir, dtype=np.float64)
        sun = sun / np.linalg.norm(sun)
        inside = np.zeros((6, n, n), dtype=bool)
        for f in range(6):
            on = np.full_like(a, -1.0 if f & 1 else 1.0)
            d = np.stack({0: (on, a, b), 1: (a, on, b), 2: (a, b, on)}[f >> 1], axis=-1)
            u = d / np.linalg.norm(d, axis=-1, keepdims=True)
            t = 0.5 * (u[..., 1] + 1.0)
            texels[f] = np.asarray(bottom, dtype=np.float64) * (1.0 - t)[..., None] + np.asarray(top, dtype=np.float64) * t[..., None]
            inside[f] = u @ sun >= cos_radius
        if not inside.any():
            ax = int(np.argmax(np.abs(sun)))
            m = abs(sun[ax])
            rest = [sun[k] / m for k in range(3) if k != ax]
            row = lambda c: min(n - 1, max(0, int((c + 1.0) * 0.5 * n)))
            inside[2 * ax + (1 if sun[ax] < 0.0 else 0), row(rest[0]), row(rest[1])] = True
        texels[inside] += np.asarray(sun_radiance, dtype=np.float64)
        return cls(texels, sample=sample)

    def device(self, renderer, sample=None):
        """(the texels, the running sums or None) as float64 tensors on the renderer's device, kept alive by this object."""
        import torch
        dev = torch.device("cuda", renderer.device_id)
        if self._device is None or self._device[0] != renderer.device_id:
            texels = self.texels.contiguous() if self._is_tensor() else torch.from_numpy(self.table()).to(dev)
            sums = self.cdf() if self.given_sums is None else np.ascontiguousarray(self.given_sums, dtype=np.float64)
            if sums.shape != (6 * self.size * self.size,):
                raise ValueError(f"sums must be [{6 * self.size * self.size}] (is {sums.shape})")
            self._device = (renderer.device_id, texels, torch.from_numpy(sums).to(dev))
        _, texels, cdf = self._device
        _torch_check(torch, renderer, [("texels", texels, torch.float64, (6, self.size, self.size, 3))])
        return texels, (cdf if (self.sample if sample is None else sample) else None)

    def struct(self, texels_ptr, cdf_ptr=None):
        """The rt_environment naming the two pointers (host or device, as the entry point wants them)."""
        return _ffi.rt_environment(texels_ptr or None, cdf_ptr or None, self.size, 0)


def _direct_flags(sampling, direct):
    """rt_direct.flags of sampling="area" (the light sampled by area: 0), "cone" (by solid angle: RT_DIRECT_CONE) or
    "weighted" (by solid angle, the light chosen by its contribution at the hit point: RT_DIRECT_WEIGHTED | RT_DIRECT_CONE; section 23)."""
    if sampling not in ("area", "cone", "weighted"):
        raise ValueError(f'sampling must be "area", "cone" or "weighted" (is {sampling!r})')
    if sampling != "area" and direct is False:
        raise ValueError(f'sampling="{sampling}" belongs to direct lighting (direct=...)')
    return {"area": 0, "cone": _ffi.RT_DIRECT_CONE, "weighted": _ffi.RT_DIRECT_WEIGHTED | _ffi.RT_DIRECT_CONE}[sampling]


def paths_step_torch(renderer, seed, qin, qout, fix, rays=None, t_min=1e-4, lighting=None, direct=False, no_direct=False, shadow_rays=None,
                     sampling="area", environment=None):
    """rt_paths_step_device on two PathQueues, on torch.cuda.current_stream(): one bounce of the live paths of `qin`; the survivors go to
    `qout` in order.  fix: an int64 tensor [..., 3] holding the u64 sums' bits, added to; rays: an int64 tensor [1] that gains the live
    count, or None.  lighting: a Lighting (rt_paths_step_lit_device; its emission a float64 tensor [n, 3] on the device, or what
    Lighting.device_table makes of it), None: the unlit step.  direct: True (rt_paths_step_nee_device with the lighting's own light
    list) or a list of sphere indices / an int32 tensor on the device; no_direct: RT_STEP_NO_DIRECT; shadow_rays: an int64 tensor [1] that
    gains the shadow rays traced, or None; sampling: "area", "cone" or "weighted", how direct lighting samples a light.  environment: an
    Environment (rt_paths_step_env_device; no_direct and shadow_rays as for direct lighting, with which it does not combine).  No host
    wait."""
    import torch
    _check_queue(renderer, qin, "qin")
    _check_queue(renderer, qout, "qout")
    items = [("fix", fix, torch.int64, tuple(fix.shape))] + ([("rays", rays, torch.int64, (1,))] if rays is not None else [])
    items += [("shadow_rays", shadow_rays, torch.int64, (1,))] if shadow_rays is not None else []
    _torch_check(torch, renderer, items)
    if fix.dim() < 1 or fix.shape[-1] != 3:
        raise ValueError(f"fix must be [..., 3] (is {tuple(fix.shape)})")
    with torch.cuda.device(qin.device):
        renderer.paths_step_device(seed, qin.struct(), qout.struct(), fix.data_ptr(), fix.numel() // 3, rays.data_ptr() if rays is not None else 0,
                                   t_min, torch.cuda.current_stream().cuda_stream, lighting=lighting, direct=direct, no_direct=no_direct,
                                   d_shadow_rays_ptr=shadow_rays.data_ptr() if shadow_rays is not None else 0, sampling=sampling,
                                   environment=environment)


class Renderer:
    """One rt_context (one GPU)."""

    def __init__(self, device_id=0):
        self._lib = _ffi.load()
        h = C.c_void_p()
        _ffi.check(self._lib.rt_create(int(device_id), C.byref(h)), "rt_create")
        self._h = h
        self.device_id = int(device_id)
        self.n_spheres = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- scene ---------------------------------------------------------------
    def upload_scene(self, world):
        """world: HittableList, or a numpy array of SPHERE_DTYPE records."""
        flat = world.flatten() if hasattr(world, "flatten") and not isinstance(world, np.ndarray) else world
        flat = np.ascontiguousarray(flat, dtype=SPHERE_DTYPE)
        ptr = flat.ctypes.data_as(C.POINTER(_ffi.rt_sphere))
        _ffi.check(self._lib.rt_upload_scene(self._h, ptr, int(flat.shape[0])), "rt_upload_scene")
        self.n_spheres = int(flat.shape[0])

    # -- host-buffer render --------------------------------------------------
    def render(self, cam, params, want_fix=True):
        """Returns (sum f32 [rows,W,3], fix u64 [rows,W,3] or None, stats dict)."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        rows = shard_rows(params)
        out_sum = np.zeros((rows, params.width, 3), dtype=np.float32)
        out_fix = np.zeros((rows, params.width, 3), dtype=np.uint64) if want_fix else None
        st = _ffi.rt_stats()
        _ffi.check(self._lib.rt_render(self._h, C.byref(rc), C.byref(params),
                                       out_sum.ctypes.data_as(C.c_void_p),
                                       out_fix.ctypes.data_as(C.c_void_p) if want_fix else None,
                                       C.byref(st)), "rt_render")
        return out_sum, out_fix, stats_dict(st)

    # -- main.rs:122-145 in one call ---------------------------------------------
    def render_rgba8(self, cam, params, flip=True):
        """Render + Color::to_rgba + flip with the sums kept on the device (rt_render_rgba8): returns
        (RGBA8 [rows,W,4] -- the bytes ImageBuffer::from_vec takes at main.rs:147 --, stats dict)."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        rows = shard_rows(params)
        out = np.zeros((rows, params.width, 4), dtype=np.uint8)
        st = _ffi.rt_stats()
        _ffi.check(self._lib.rt_render_rgba8(self._h, C.byref(rc), C.byref(params), int(bool(flip)),
                                             out.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_rgba8")
        return out, stats_dict(st)

    # -- device-buffer render (pointers come from e.g. torch tensors) ---------
    def render_device(self, cam, params, d_fix_ptr, stream=0):
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        _ffi.check(self._lib.rt_render_device(self._h, C.byref(rc), C.byref(params),
                                              C.c_void_p(d_fix_ptr), C.c_void_p(stream)), "rt_render_device")

    def fix_to_f32_device(self, d_fix_ptr, count, d_out_ptr, stream=0):
        _ffi.check(self._lib.rt_fix_to_f32_device(self._h, C.c_void_p(d_fix_ptr), int(count),
                                                  C.c_void_p(d_out_ptr), C.c_void_p(stream)), "rt_fix_to_f32_device")

    def resolve_rgba8_device(self, d_fix_ptr, width, rows, spp, flip, d_rgba_ptr, stream=0):
        _ffi.check(self._lib.rt_resolve_rgba8_device(self._h, C.c_void_p(d_fix_ptr), int(width), int(rows),
                                                     int(spp), int(flip), C.c_void_p(d_rgba_ptr),
                                                     C.c_void_p(stream)), "rt_resolve_rgba8_device")

    def last_stats(self):
        st = _ffi.rt_stats()
        _ffi.check(self._lib.rt_last_stats(self._h, C.byref(st)), "rt_last_stats")
        return stats_dict(st)

    # -- pixel lists and adaptive sampling ---------------------------------------
    def render_pixels(self, cam, params, pixels):
        """params.spp samples of the listed pixels (g = j * W + i, j = 0 the bottom row; any order, duplicates allowed) through
        rt_render_pixels: returns (fix u64 [n,3], entry k for pixels[k] -- the dense render's sums at that pixel --, stats dict)."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        out = np.zeros((len(px), 3), dtype=np.uint64)
        st = _ffi.rt_stats()
        _ffi.check(self._lib.rt_render_pixels(self._h, C.byref(rc), C.byref(params), px.ctypes.data_as(C.c_void_p), len(px),
                                              out.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_pixels")
        return out, (stats_dict(st) if len(px) else None)

    def render_pixels_device(self, cam, params, d_pixels_ptr, n_pixels, d_fix_ptr, stream=0):
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        _ffi.check(self._lib.rt_render_pixels_device(self._h, C.byref(rc), C.byref(params), C.c_void_p(d_pixels_ptr), int(n_pixels),
                                                     C.c_void_p(d_fix_ptr), C.c_void_p(stream)), "rt_render_pixels_device")

    def select_pixels_device(self, d_fix_ptr, d_half_ptr, d_count_ptr, width, height, n, adaptive, d_list_ptr, d_n_ptr, stream=0):
        _ffi.check(self._lib.rt_select_pixels_device(self._h, C.c_void_p(d_fix_ptr), C.c_void_p(d_half_ptr), C.c_void_p(d_count_ptr),
                                                     int(width), int(height), int(n), C.byref(adaptive), C.c_void_p(d_list_ptr),
                                                     C.c_void_p(d_n_ptr), C.c_void_p(stream)), "rt_select_pixels_device")

    def select_pixels(self, fix, half, count, n, adaptive):
        """The adaptive selection ON THE DEVICE (rt_select_pixels_device) for host arrays: the state goes up through torch
        tensors, the list comes back.  Same result as select_pixels_host."""
        import torch
        count = np.ascontiguousarray(count, dtype=np.uint32)
        h, w = count.shape
        dev = torch.device("cuda", torch.cuda.current_device())
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t).copy()).to(dev)
        d_fix = up(np.asarray(fix, dtype=np.uint64).reshape(h, w, 3), np.int64)
        d_half = up(np.asarray(half, dtype=np.uint64).reshape(h, w, 3), np.int64)
        d_count = up(count, np.int32)
        d_list = torch.zeros(h * w, dtype=torch.int32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        self.select_pixels_device(d_fix.data_ptr(), d_half.data_ptr(), d_count.data_ptr(), w, h, n, adaptive,
                                  d_list.data_ptr(), d_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        m = int(d_n.cpu().numpy().view(np.uint32)[0])
        return d_list.cpu().numpy().view(np.uint32)[:m].copy()

    select_pixels_host = staticmethod(select_pixels_host)

    def render_adaptive(self, cam, params, adaptive, want_half=True):
        """rt_render_adaptive: params.spp is the cap.  Returns (fix u64 [H,W,3], half u64 [H,W,3] or None, count u32 [H,W], stats dict)."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        h, w = params.height, params.width
        fix = np.zeros((h, w, 3), dtype=np.uint64)
        half = np.zeros((h, w, 3), dtype=np.uint64) if want_half else None
        count = np.zeros((h, w), dtype=np.uint32)
        st = _ffi.rt_stats()
        _ffi.check(self._lib.rt_render_adaptive(self._h, C.byref(rc), C.byref(params), C.byref(adaptive), fix.ctypes.data_as(C.c_void_p),
                                                half.ctypes.data_as(C.c_void_p) if want_half else None,
                                                count.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_adaptive")
        return fix, half, count, stats_dict(st)

    def resolve_rgba8_counts(self, fix, count, flip=True):
        """fix u64 [rows,W,3], count u32 [rows,W] -> RGBA8 [rows,W,4]: Color::to_rgba with each pixel's own sample count."""
        fix = np.ascontiguousarray(fix, dtype=np.uint64)
        count = np.ascontiguousarray(count, dtype=np.uint32)
        rows, width = fix.shape[0], fix.shape[1]
        assert count.shape == (rows, width)
        out = np.zeros((rows, width, 4), dtype=np.uint8)
        _ffi.check(self._lib.rt_resolve_rgba8_counts(self._h, fix.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p), width, rows,
                                                     int(bool(flip)), out.ctypes.data_as(C.c_void_p)), "rt_resolve_rgba8_counts")
        return out

    # -- frame batches: many cameras, one launch -----------------------------------
    @staticmethod
    def _camera_array(cams):
        """Cameras (scene.Camera, rt_camera, or a float64 array [F,19]) -> contiguous float64 [F,19]: the rt_camera records."""
        if isinstance(cams, np.ndarray):
            a = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 19)
        else:
            from .scene import cameras_to_array
            a = cameras_to_array(cams)
        return a

    def render_frames(self, cams, params, sample_stride=0):
        """rt_render_frames: every camera of `cams` over the uploaded scene in ONE launch; frame f is the dense render of cams[f]
        with sample_begin + f * sample_stride.  Returns (fix u64 [F,H,W,3], stats dict -- None for an empty batch)."""
        a = self._camera_array(cams)
        out = np.zeros((len(a), params.height, params.width, 3), dtype=np.uint64)
        st = _ffi.rt_stats()
        _ffi.check(self._lib.rt_render_frames(self._h, a.ctypes.data_as(C.c_void_p), len(a), int(sample_stride), C.byref(params),
                                              out.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_frames")
        return out, (stats_dict(st) if len(a) else None)

    def render_frames_rgba8(self, cams, params, sample_stride=0, flip=True):
        """rt_render_frames_rgba8: the batch + Color::to_rgba + the row flip per frame, the sums kept on the device.
        Returns (RGBA8 [F,H,W,4], stats dict -- None for an empty batch)."""
        a = self._camera_array(cams)
        out = np.zeros((len(a), params.height, params.width, 4), dtype=np.uint8)
        st = _ffi.rt_stats()
        _ffi.check(self._lib.rt_render_frames_rgba8(self._h, a.ctypes.data_as(C.c_void_p), len(a), int(sample_stride), C.byref(params),
                                                    int(bool(flip)), out.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_frames_rgba8")
        return out, (stats_dict(st) if len(a) else None)

    def render_frames_device(self, d_cams_ptr, n_frames, sample_stride, params, d_fix_ptr, stream=0):
        _ffi.check(self._lib.rt_render_frames_device(self._h, C.c_void_p(d_cams_ptr), int(n_frames), int(sample_stride), C.byref(params),
                                                     C.c_void_p(d_fix_ptr), C.c_void_p(stream)), "rt_render_frames_device")

    # -- feature buffers: first-hit albedo, normal, depth, hit count, object id ------
    def render_features(self, cam, params, want_ids=True):
        """rt_render_features: what the first hit of every camera ray of the dense render shows.  Returns (feat u64 [H,W,8] -- exact
        sums of albedo rgb, normal xyz (two's complement), depth t and the hit count --, ids i32 [H,W] or None -- the list index the
        call's first sample hits, -1 for a miss --, the kernel's time in ms)."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        h, w = params.height, params.width
        feat = np.zeros((h, w, _ffi.RT_FEATURE_WORDS), dtype=np.uint64)
        ids = np.zeros((h, w), dtype=np.int32) if want_ids else None
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_render_features(self._h, C.byref(rc), C.byref(params), feat.ctypes.data_as(C.c_void_p),
                                                ids.ctypes.data_as(C.c_void_p) if want_ids else None, C.byref(ms)), "rt_render_features")
        return feat, ids, float(ms.value)

    def render_features_device(self, cam, params, d_feat_ptr, d_ids_ptr=0, stream=0):
        """rt_render_features_device: d_feat_ptr device [H,W,8] u64, d_ids_ptr device [H,W] i32 or 0; asynchronous on `stream`."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        _ffi.check(self._lib.rt_render_features_device(self._h, C.byref(rc), C.byref(params), C.c_void_p(d_feat_ptr),
                                                       C.c_void_p(d_ids_ptr) if d_ids_ptr else None, C.c_void_p(stream)),
                   "rt_render_features_device")

    def features_to_f32(self, feat, spp):
        """rt_features_to_f32: exact sums u64 [rows,W,8] of `spp` samples -> f32 [rows,W,8] = mean albedo rgb, mean normal xyz, mean
        depth over the hitting samples (0 without one), alpha = hits / spp."""
        feat = np.ascontiguousarray(feat, dtype=np.uint64)
        rows, width = feat.shape[0], feat.shape[1]
        assert feat.shape == (rows, width, _ffi.RT_FEATURE_WORDS)
        out = np.zeros((rows, width, _ffi.RT_FEATURE_WORDS), dtype=np.float32)
        _ffi.check(self._lib.rt_features_to_f32(self._h, feat.ctypes.data_as(C.c_void_p), width, rows, int(spp),
                                                out.ctypes.data_as(C.c_void_p)), "rt_features_to_f32")
        return out

    def features_to_f32_device(self, d_feat_ptr, width, rows, spp, d_out_ptr, stream=0):
        _ffi.check(self._lib.rt_features_to_f32_device(self._h, C.c_void_p(d_feat_ptr), int(width), int(rows), int(spp),
                                                       C.c_void_p(d_out_ptr), C.c_void_p(stream)), "rt_features_to_f32_device")

    # -- ray queries: closest hit and occlusion for the caller's rays -----------------
    @staticmethod
    def _ray_arrays(origins, dirs, t_max):
        origins = np.ascontiguousarray(origins, dtype=np.float64)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64)
        n = origins.shape[0] if origins.ndim == 2 else -1
        if origins.shape != (n, 3) or dirs.shape != (n, 3):
            raise ValueError(f"origins and dirs must both be [n, 3] (are {origins.shape}, {dirs.shape})")
        if t_max is not None:
            t_max = np.ascontiguousarray(t_max, dtype=np.float64)
            if t_max.shape != (n,):
                raise ValueError(f"t_max must be [n] (is {t_max.shape})")
        rays = _ffi.rt_rays(origins.ctypes.data, dirs.ctypes.data, t_max.ctypes.data if t_max is not None else None, n)
        return rays, (origins, dirs, t_max)

    def trace_rays(self, origins, dirs, t_max=None, t_min=1e-4, want=("t", "point", "normal", "front_face")):
        """rt_trace_rays: HittableList::hit(ray, t_min, t_max[k]) of every ray against the uploaded scene.  origins, dirs f64 [n, 3] (dirs
        not normalised), t_max f64 [n] or None (+inf).  Returns a dict: "index" i32 [n] (-1: a miss) and whichever of "t" f64 [n] (+inf),
        "point" f64 [n, 3], "normal" f64 [n, 3], "front_face" u8 [n] `want` names, and "kernel_ms"."""
        _check_want(want)
        rays, keep = self._ray_arrays(origins, dirs, t_max)
        n = int(rays.n)
        out = {"index": np.zeros(n, dtype=np.int32)}
        shapes = {"t": ((n,), np.float64), "point": ((n, 3), np.float64), "normal": ((n, 3), np.float64), "front_face": ((n,), np.uint8)}
        for name in ("t", "point", "normal", "front_face"):
            if name in want:
                out[name] = np.zeros(*shapes[name])
        hits = _ffi.rt_hits(*[out[name].ctypes.data if name in out else None for name in ("index", "t", "point", "normal", "front_face")])
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_trace_rays(self._h, C.byref(rays), float(t_min), C.byref(hits), C.byref(ms)), "rt_trace_rays")
        out["kernel_ms"] = float(ms.value)
        return out

    def occluded(self, origins, dirs, t_max=None, t_min=1e-4):
        """rt_occluded.  Returns a dict, as trace_rays does: "occluded" u8 [n], 1 where trace_rays would return an index >= 0, and "kernel_ms"."""
        rays, keep = self._ray_arrays(origins, dirs, t_max)
        occ = np.zeros(int(rays.n), dtype=np.uint8)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_occluded(self._h, C.byref(rays), float(t_min), occ.ctypes.data_as(C.c_void_p), C.byref(ms)), "rt_occluded")
        return {"occluded": occ, "kernel_ms": float(ms.value)}

    def trace_rays_device(self, n, d_origin_ptr, d_dir_ptr, d_index_ptr, d_t_max_ptr=0, t_min=1e-4, d_t_ptr=0, d_point_ptr=0, d_normal_ptr=0,
                          d_front_ptr=0, stream=0):
        """rt_trace_rays_device on raw device pointers (0: left out); asynchronous on `stream`."""
        rays = _ffi.rt_rays(d_origin_ptr or None, d_dir_ptr or None, d_t_max_ptr or None, int(n))
        hits = _ffi.rt_hits(d_index_ptr or None, d_t_ptr or None, d_point_ptr or None, d_normal_ptr or None, d_front_ptr or None)
        _ffi.check(self._lib.rt_trace_rays_device(self._h, C.byref(rays), float(t_min), C.byref(hits), C.c_void_p(stream)), "rt_trace_rays_device")

    def occluded_device(self, n, d_origin_ptr, d_dir_ptr, d_occluded_ptr, d_t_max_ptr=0, t_min=1e-4, stream=0):
        """rt_occluded_device on raw device pointers; d_occluded_ptr: device [n] u8; asynchronous on `stream`."""
        rays = _ffi.rt_rays(d_origin_ptr or None, d_dir_ptr or None, d_t_max_ptr or None, int(n))
        _ffi.check(self._lib.rt_occluded_device(self._h, C.byref(rays), float(t_min), C.c_void_p(d_occluded_ptr) if d_occluded_ptr else None,
                                                C.c_void_p(stream)), "rt_occluded_device")

    # -- wavefront path steps: camera rays, material scatter, accumulate ---------------
    @staticmethod
    def _u32(x, name, n=None):
        x = np.ascontiguousarray(x, dtype=np.uint32)
        if x.ndim != 1 or (n is not None and x.shape[0] != n):
            raise ValueError(f"{name} must be [n] (is {x.shape})")
        return x

    @staticmethod
    def _v3(x, name, n):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (n, 3):
            raise ValueError(f"{name} must be [{n}, 3] (is {x.shape})")
        return x

    def camera_rays(self, cam, width, height, seed, pixel, sample, flags=0):
        """rt_camera_rays: the camera ray rt_render traces for (pixel[k], sample[k]) of a width x height frame.  pixel, sample u32 [n].
        Returns a dict: "origin", "dir" f64 [n, 3], "event" u32 [n] (the next unused Philox block) and "kernel_ms"."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        pixel = self._u32(pixel, "pixel")
        n = int(pixel.shape[0])
        sample = self._u32(sample, "sample", n)
        out = {"origin": np.zeros((n, 3)), "dir": np.zeros((n, 3)), "event": np.zeros(n, dtype=np.uint32)}
        b = _ffi.rt_camera_batch(pixel.ctypes.data, sample.ctypes.data, out["origin"].ctypes.data, out["dir"].ctypes.data, out["event"].ctypes.data, n)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_camera_rays(self._h, C.byref(rc), int(width), int(height), int(seed), int(flags), C.byref(b), C.byref(ms)),
                   "rt_camera_rays")
        out["kernel_ms"] = float(ms.value)
        return out

    def scatter(self, seed, dirs, index, point, normal, front_face, pixel, sample, event, out=None, flags=0):
        """rt_scatter: Scatter::scatter of the uploaded sphere index[k] for the hit as trace_rays returns it.  `event` (u32 [n]) is not
        modified: the advanced values come back as "event".  out (optional): a dict of C-contiguous arrays to write to, any of "out_origin",
        "out_dir" (may be `dirs` itself), "attenuation" f64 [n, 3]; what the step does not write keeps its bytes.  Returns a dict:
        "out_origin", "out_dir", "attenuation", "status" u8 [n] (RT_SCATTER_*), "event" and "kernel_ms"."""
        index = np.ascontiguousarray(index, dtype=np.int32)
        n = int(index.shape[0])
        dirs, point, normal = self._v3(dirs, "dirs", n), self._v3(point, "point", n), self._v3(normal, "normal", n)
        front_face = np.ascontiguousarray(front_face, dtype=np.uint8)
        pixel, sample = self._u32(pixel, "pixel", n), self._u32(sample, "sample", n)
        res = dict(out or {})
        for name in ("out_origin", "out_dir", "attenuation"):
            if name not in res:
                res[name] = np.zeros((n, 3))
            a = res[name]
            if a.dtype != np.float64 or a.shape != (n, 3) or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a C-contiguous float64 array [{n}, 3]")
        res["status"] = np.zeros(n, dtype=np.uint8)
        res["event"] = np.array(self._u32(event, "event", n), copy=True)
        b = _ffi.rt_scatter_batch(dirs.ctypes.data, index.ctypes.data, point.ctypes.data, normal.ctypes.data, front_face.ctypes.data,
                                  pixel.ctypes.data, sample.ctypes.data, res["event"].ctypes.data, res["out_origin"].ctypes.data,
                                  res["out_dir"].ctypes.data, res["attenuation"].ctypes.data, res["status"].ctypes.data, n)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_scatter(self._h, int(seed), int(flags), C.byref(b), C.byref(ms)), "rt_scatter")
        res["kernel_ms"] = float(ms.value)
        return res

    def accumulate(self, fix, pixel, weight, sky_dir=None, select=None):
        """rt_accumulate: adds quantize(weight * sky(sky_dir)) -- weight itself without sky_dir -- to entry pixel[k] of `fix`, a C-contiguous
        u64 array [..., 3], IN PLACE.  select u8 [n] or None.  Returns the kernel's time in ms."""
        if fix.dtype != np.uint64 or not fix.flags.c_contiguous or fix.ndim < 1 or fix.shape[-1] != 3:
            raise ValueError("fix must be a C-contiguous uint64 array [..., 3]")
        pixel = self._u32(pixel, "pixel")
        n = int(pixel.shape[0])
        weight = self._v3(weight, "weight", n)
        sky_dir = self._v3(sky_dir, "sky_dir", n) if sky_dir is not None else None
        select = np.ascontiguousarray(select, dtype=np.uint8) if select is not None else None
        b = _ffi.rt_accumulate_batch(pixel.ctypes.data, weight.ctypes.data, sky_dir.ctypes.data if sky_dir is not None else None,
                                     select.ctypes.data if select is not None else None, n)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_accumulate(self._h, C.byref(b), fix.ctypes.data_as(C.c_void_p), fix.size // 3, C.byref(ms)), "rt_accumulate")
        return float(ms.value)

    def camera_rays_device(self, cam, width, height, seed, n, d_pixel_ptr, d_sample_ptr, d_origin_ptr, d_dir_ptr, d_event_ptr, stream=0, flags=0):
        """rt_camera_rays_device on raw device pointers; asynchronous on `stream`."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        b = _ffi.rt_camera_batch(d_pixel_ptr or None, d_sample_ptr or None, d_origin_ptr or None, d_dir_ptr or None, d_event_ptr or None, int(n))
        _ffi.check(self._lib.rt_camera_rays_device(self._h, C.byref(rc), int(width), int(height), int(seed), int(flags), C.byref(b),
                                                   C.c_void_p(stream)), "rt_camera_rays_device")

    def scatter_device(self, seed, n, d_dir_ptr, d_index_ptr, d_point_ptr, d_normal_ptr, d_front_ptr, d_pixel_ptr, d_sample_ptr, d_event_ptr,
                       d_out_origin_ptr, d_out_dir_ptr, d_attenuation_ptr, d_status_ptr, stream=0, flags=0):
        """rt_scatter_device on raw device pointers; d_event_ptr is read and written; asynchronous on `stream`."""
        b = _ffi.rt_scatter_batch(*[p or None for p in (d_dir_ptr, d_index_ptr, d_point_ptr, d_normal_ptr, d_front_ptr, d_pixel_ptr, d_sample_ptr,
                                                        d_event_ptr, d_out_origin_ptr, d_out_dir_ptr, d_attenuation_ptr, d_status_ptr)], int(n))
        _ffi.check(self._lib.rt_scatter_device(self._h, int(seed), int(flags), C.byref(b), C.c_void_p(stream)), "rt_scatter_device")

    def accumulate_device(self, n, d_pixel_ptr, d_weight_ptr, d_fix_ptr, npix, d_sky_dir_ptr=0, d_select_ptr=0, stream=0):
        """rt_accumulate_device on raw device pointers; d_fix_ptr: device [npix][3] u64, added to; asynchronous on `stream`."""
        b = _ffi.rt_accumulate_batch(d_pixel_ptr or None, d_weight_ptr or None, d_sky_dir_ptr or None, d_select_ptr or None, int(n))
        _ffi.check(self._lib.rt_accumulate_device(self._h, C.byref(b), C.c_void_p(d_fix_ptr) if d_fix_ptr else None, int(npix),
                                                  C.c_void_p(stream)), "rt_accumulate_device")

    # -- the device path queue and the frame rendered from it ----------------------------
    def paths_begin_device(self, cam, width, height, seed, spp, sample_begin, first_item, n, queue, stream=0, flags=0):
        """rt_paths_begin_device; queue: an _ffi.rt_path_queue of device pointers (PathQueue.struct()); asynchronous on `stream`."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        _ffi.check(self._lib.rt_paths_begin_device(self._h, C.byref(rc), int(width), int(height), int(seed), int(flags), int(spp), int(sample_begin),
                                                   int(first_item), int(n), C.byref(queue), C.c_void_p(stream)), "rt_paths_begin_device")

    def _device_lighting(self, lighting):
        """(the rt_lighting of a device form, the tensor it names -- to be kept until the call has been made)."""
        table = lighting.device_table(self)
        return lighting.struct(table.data_ptr() if table is not None else None, table.shape[0] if table is not None else 0), table

    def _device_direct(self, lighting, direct, flags=0):
        """(the rt_direct of a device form, the tensor it names -- to be kept until the call has been made)."""
        if lighting is None:
            raise ValueError("direct lighting needs a Lighting")
        lights = lighting.device_lights(self, direct)
        n = int(lights.shape[0])
        return _ffi.rt_direct(lights.data_ptr() if n else None, n, flags), lights

    def _env_lighting(self, lighting, direct, environment):
        """The Lighting an environment call takes (None: the default one, whose sky the environment replaces and which has no light)."""
        if direct is not False and direct is not None:
            raise ValueError("environment= does not combine with direct= (the environment and sphere lights are not sampled in one step)")
        return lighting if lighting is not None else Lighting()

    def paths_step_device(self, seed, qin, qout, d_fix_ptr, npix, d_rays_ptr=0, t_min=1e-4, stream=0, flags=0, lighting=None, direct=False,
                          no_direct=False, d_shadow_rays_ptr=0, sampling="area", environment=None):
        """rt_paths_step_device, or with a Lighting rt_paths_step_lit_device, or with direct (True: the lighting's own light list, else
        the indices) rt_paths_step_nee_device -- no_direct: RT_STEP_NO_DIRECT; d_shadow_rays_ptr: a device u64 or 0; sampling: "area",
        "cone" (RT_DIRECT_CONE: the light sampled by solid angle) or "weighted" (... and chosen by its contribution at the hit) --; qin, qout:
        _ffi.rt_path_queue structs of device pointers; asynchronous on `stream`.  environment: an Environment: rt_paths_step_env_device
        with the lighting's emission table (no lighting: no sphere emits), no_direct and d_shadow_rays_ptr as above."""
        direct_flags = _direct_flags(sampling, direct if lighting is not None else False)
        head = (self._h, int(seed), int(flags), float(t_min), C.byref(qin), C.byref(qout), C.c_void_p(d_fix_ptr) if d_fix_ptr else None, int(npix),
                C.c_void_p(d_rays_ptr) if d_rays_ptr else None)
        if environment is not None:
            light, _keep = self._device_lighting(self._env_lighting(lighting, direct, environment))
            texels, cdf = environment.device(self)
            env = environment.struct(texels.data_ptr(), cdf.data_ptr() if cdf is not None else None)
            _ffi.check(self._lib.rt_paths_step_env_device(*head, C.byref(light), C.byref(env), _ffi.RT_STEP_NO_DIRECT if no_direct else 0,
                                                          C.c_void_p(d_shadow_rays_ptr) if d_shadow_rays_ptr else None, C.c_void_p(stream)),
                       "rt_paths_step_env_device")
            return
        if lighting is None:
            _ffi.check(self._lib.rt_paths_step_device(*head, C.c_void_p(stream)), "rt_paths_step_device")
            return
        if direct is not False:
            d, _keep_list = self._device_direct(lighting, direct, direct_flags)
            light, _keep = self._device_lighting(lighting)
            _ffi.check(self._lib.rt_paths_step_nee_device(*head, C.byref(light), C.byref(d), _ffi.RT_STEP_NO_DIRECT if no_direct else 0,
                                                          C.c_void_p(d_shadow_rays_ptr) if d_shadow_rays_ptr else None, C.c_void_p(stream)),
                       "rt_paths_step_nee_device")
            return
        if no_direct:
            raise ValueError("no_direct belongs to the direct-lighting step (direct=...)")
        light, _keep = self._device_lighting(lighting)
        _ffi.check(self._lib.rt_paths_step_lit_device(*head, C.byref(light), C.c_void_p(stream)), "rt_paths_step_lit_device")

    def render_wavefront(self, cam, params, lighting=None, direct=False, sampling="area", environment=None):
        """rt_render_wavefront: the frame through the device path queue -> (the exact sums u64 [H, W, 3], the rays traced): what
        Renderer.render returns as `fix` and as stats["rays_traced"].  lighting: a Lighting (rt_render_wavefront_lit: a settable sky and
        emissive spheres), None: the unlit frame.  direct=True (rt_render_wavefront_nee: shadow rays towards the lighting's lights at
        Lambertian hits) -> (the sums, the rays traced, stats) with stats["shadow_rays"] the shadow rays traced.  sampling="cone"
        (rt_render_wavefront_nee_sampled with RT_DIRECT_CONE): the lights are sampled by solid angle instead of by area;
        sampling="weighted" (RT_DIRECT_WEIGHTED | RT_DIRECT_CONE): ... and chosen by their contribution at the hit point, not uniformly.
        environment: an Environment (rt_render_wavefront_env: the cube map in the place of the sky, sampled at Lambertian hits when
        environment.sample) -> (the sums, the rays traced, stats) as for direct lighting, with which it does not combine."""
        direct_flags = _direct_flags(sampling, direct if direct else False)
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        fix = np.zeros((params.height, params.width, 3), dtype=np.uint64)
        rays = C.c_uint64(0)
        if environment is not None:
            light, _keep = self._host_lighting(self._env_lighting(lighting, direct, environment))
            texels, shadow = environment.table(), C.c_uint64(0)
            env = environment.struct(texels.ctypes.data)
            _ffi.check(self._lib.rt_render_wavefront_env(self._h, C.byref(rc), C.byref(params), C.byref(light), C.byref(env), int(environment.sample),
                                                         fix.ctypes.data_as(C.c_void_p), C.byref(rays), C.byref(shadow), None),
                       "rt_render_wavefront_env")
            return fix, int(rays.value), {"rays_traced": int(rays.value), "shadow_rays": int(shadow.value)}
        if direct and lighting is None:
            raise ValueError("direct lighting needs a Lighting")
        if lighting is None:
            _ffi.check(self._lib.rt_render_wavefront(self._h, C.byref(rc), C.byref(params), fix.ctypes.data_as(C.c_void_p), C.byref(rays), None),
                       "rt_render_wavefront")
            return fix, int(rays.value)
        table = lighting.table(self.n_spheres or 0)
        light = lighting.struct(table.ctypes.data if table is not None else None, table.shape[0] if table is not None else 0)
        if direct:
            shadow = C.c_uint64(0)
            if direct_flags:
                _ffi.check(self._lib.rt_render_wavefront_nee_sampled(self._h, C.byref(rc), C.byref(params), C.byref(light), direct_flags,
                                                                     fix.ctypes.data_as(C.c_void_p), C.byref(rays), C.byref(shadow), None),
                           "rt_render_wavefront_nee_sampled")
            else:
                _ffi.check(self._lib.rt_render_wavefront_nee(self._h, C.byref(rc), C.byref(params), C.byref(light), fix.ctypes.data_as(C.c_void_p),
                                                             C.byref(rays), C.byref(shadow), None), "rt_render_wavefront_nee")
            return fix, int(rays.value), {"rays_traced": int(rays.value), "shadow_rays": int(shadow.value)}
        _ffi.check(self._lib.rt_render_wavefront_lit(self._h, C.byref(rc), C.byref(params), C.byref(light), fix.ctypes.data_as(C.c_void_p),
                                                     C.byref(rays), None), "rt_render_wavefront_lit")
        return fix, int(rays.value)

    def render_wavefront_device(self, cam, params, d_fix_ptr, d_rays_ptr=0, stream=0, lighting=None, direct=False, d_shadow_rays_ptr=0,
                                sampling="area", environment=None):
        """rt_render_wavefront_device on raw device pointers (d_fix [H][W][3] u64, d_rays one u64 or 0); asynchronous on `stream`.
        lighting: a Lighting (rt_render_wavefront_lit_device; its emission as in paths_step_torch), None: the unlit frame.  direct (as
        in paths_step_device): rt_render_wavefront_nee_device; d_shadow_rays_ptr: a device u64 that receives the shadow rays traced, or 0;
        sampling: "area", "cone" or "weighted", as in paths_step_device.  environment: an Environment (rt_render_wavefront_env_device)."""
        direct_flags = _direct_flags(sampling, direct if lighting is not None else False)
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        tail = (C.c_void_p(d_fix_ptr) if d_fix_ptr else None, C.c_void_p(d_rays_ptr) if d_rays_ptr else None, C.c_void_p(stream))
        if environment is not None:
            light, _keep = self._device_lighting(self._env_lighting(lighting, direct, environment))
            texels, cdf = environment.device(self)
            env = environment.struct(texels.data_ptr(), cdf.data_ptr() if cdf is not None else None)
            _ffi.check(self._lib.rt_render_wavefront_env_device(self._h, C.byref(rc), C.byref(params), C.byref(light), C.byref(env), tail[0], tail[1],
                                                                C.c_void_p(d_shadow_rays_ptr) if d_shadow_rays_ptr else None, tail[2]),
                       "rt_render_wavefront_env_device")
            return
        if lighting is None:
            _ffi.check(self._lib.rt_render_wavefront_device(self._h, C.byref(rc), C.byref(params), *tail), "rt_render_wavefront_device")
            return
        if direct is not False:
            d, _keep_list = self._device_direct(lighting, direct, direct_flags)
            light, _keep = self._device_lighting(lighting)
            _ffi.check(self._lib.rt_render_wavefront_nee_device(self._h, C.byref(rc), C.byref(params), C.byref(light), C.byref(d), tail[0], tail[1],
                                                                C.c_void_p(d_shadow_rays_ptr) if d_shadow_rays_ptr else None, tail[2]),
                       "rt_render_wavefront_nee_device")
            return
        light, _keep = self._device_lighting(lighting)
        _ffi.check(self._lib.rt_render_wavefront_lit_device(self._h, C.byref(rc), C.byref(params), C.byref(light), *tail),
                   "rt_render_wavefront_lit_device")

    # -- wavefront frames over pixel lists, accumulated and adaptively sampled ----
    def paths_begin_pixels_device(self, cam, width, height, seed, spp, sample_begin, first_item, n, d_pixels_ptr, n_pixels, queue, stream=0, flags=0):
        """rt_paths_begin_pixels_device; d_pixels_ptr: device [n_pixels] u32 (0: no list); queue: an _ffi.rt_path_queue; asynchronous on `stream`."""
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        _ffi.check(self._lib.rt_paths_begin_pixels_device(self._h, C.byref(rc), int(width), int(height), int(seed), int(flags), int(spp),
                                                          int(sample_begin), int(first_item), int(n), C.c_void_p(d_pixels_ptr) if d_pixels_ptr else None,
                                                          int(n_pixels), C.byref(queue), C.c_void_p(stream)), "rt_paths_begin_pixels_device")

    def _host_lighting(self, lighting):
        """(the rt_lighting of a host form or None, the table it names -- to be kept until the call has been made)."""
        if lighting is None:
            return None, None
        table = lighting.table(self.n_spheres or 0)
        return lighting.struct(table.ctypes.data if table is not None else None, table.shape[0] if table is not None else 0), table

    def render_wavefront_pixels(self, cam, params, pixels=None, lighting=None, direct=False, sampling="area", into=None):
        """rt_render_wavefront_pixels: params.spp samples of the listed pixels (g = j * W + i, j = 0 the bottom row; any order; a pixel listed m
        times gets its samples' sums m times; None: every pixel) through the device path queue -> (fix u64 [H, W, 3], stats).  The frame
        is FRAME-ADDRESSED: pixel g's sums are at fix[g // W, g % W] -- Renderer.render_pixels' result is compact --, an unlisted pixel's
        are zero.  lighting, direct and sampling as in render_wavefront.  into: a frame of sums u64 [H, W, 3] to ADD this call's samples to
        (RT_FLAG_ACCUMULATE is set for the call; the array is not written, the sum is returned).  stats: rays_traced, shadow_rays and
        kernel_ms of THIS call."""
        direct_flags = _direct_flags(sampling, direct if direct else False)
        if direct and lighting is None:
            raise ValueError("direct lighting needs a Lighting")
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        h, w = params.height, params.width
        p = _ffi.rt_params.from_buffer_copy(params)
        if into is None:
            fix = np.zeros((h, w, 3), dtype=np.uint64)
        else:
            fix = np.array(into, dtype=np.uint64, order="C", copy=True).reshape(h, w, 3)
            p.flags |= _ffi.RT_FLAG_ACCUMULATE
        px = None if pixels is None else np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        n = h * w if px is None else len(px)
        keep = np.zeros(1, dtype=np.uint32)                                      # (an empty list is still a list: a pointer that is not NULL)
        ptr = None if px is None else (px if len(px) else keep).ctypes.data_as(C.c_void_p)
        light, _keep = self._host_lighting(lighting)
        rays, shadow, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0.0)
        _ffi.check(self._lib.rt_render_wavefront_pixels(self._h, C.byref(rc), C.byref(p), C.byref(light) if light is not None else None,
                                                        int(bool(direct)), direct_flags, ptr, n, fix.ctypes.data_as(C.c_void_p), C.byref(rays),
                                                        C.byref(shadow), C.byref(ms)), "rt_render_wavefront_pixels")
        return fix, {"rays_traced": int(rays.value), "shadow_rays": int(shadow.value), "kernel_ms": float(ms.value)}

    def render_wavefront_pixels_device(self, cam, params, d_pixels_ptr, n_pixels, d_fix_ptr, d_rays_ptr=0, stream=0, lighting=None, direct=False,
                                       d_shadow_rays_ptr=0, sampling="area"):
        """rt_render_wavefront_pixels_device on raw device pointers: d_pixels [n_pixels] u32 (0: the identity list, n_pixels = W * H), d_fix
        [H][W][3] u64 frame-addressed, d_rays / d_shadow_rays one u64 each or 0; params.flags may hold RT_FLAG_ACCUMULATE; asynchronous on
        `stream`.  lighting, direct, sampling: as in render_wavefront_device."""
        direct_flags = _direct_flags(sampling, direct if lighting is not None else False)
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        opt = lambda ptr: C.c_void_p(ptr) if ptr else None
        light = d = _keep = _keep_list = None
        if lighting is not None:
            light, _keep = self._device_lighting(lighting)
        if direct is not False:
            d, _keep_list = self._device_direct(lighting, direct, direct_flags)
        _ffi.check(self._lib.rt_render_wavefront_pixels_device(self._h, C.byref(rc), C.byref(params), C.byref(light) if light is not None else None,
                                                               C.byref(d) if d is not None else None, opt(d_pixels_ptr), int(n_pixels), opt(d_fix_ptr),
                                                               opt(d_rays_ptr), opt(d_shadow_rays_ptr), C.c_void_p(stream)),
                   "rt_render_wavefront_pixels_device")

    def render_wavefront_adaptive(self, cam, params, adaptive, lighting=None, direct=False, sampling="area", want_half=True):
        """rt_render_wavefront_adaptive: render_adaptive's loop and rule over the wavefront frame, lit or not; params.spp is the cap.  Returns
        (fix u64 [H,W,3], half u64 [H,W,3] or None, count u32 [H,W], stats) with stats["rays"] the path rays, stats["shadow_rays"] the
        shadow rays, stats["samples"] the samples rendered (the sum of count) and stats["kernel_ms"] the rounds' device time."""
        direct_flags = _direct_flags(sampling, direct if direct else False)
        if direct and lighting is None:
            raise ValueError("direct lighting needs a Lighting")
        rc = cam.to_rt_camera() if hasattr(cam, "to_rt_camera") else cam
        h, w = params.height, params.width
        fix = np.zeros((h, w, 3), dtype=np.uint64)
        half = np.zeros((h, w, 3), dtype=np.uint64) if want_half else None
        count = np.zeros((h, w), dtype=np.uint32)
        light, _keep = self._host_lighting(lighting)
        rays, shadow, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0.0)
        _ffi.check(self._lib.rt_render_wavefront_adaptive(self._h, C.byref(rc), C.byref(params), C.byref(adaptive),
                                                          C.byref(light) if light is not None else None, int(bool(direct)), direct_flags,
                                                          fix.ctypes.data_as(C.c_void_p), half.ctypes.data_as(C.c_void_p) if want_half else None,
                                                          count.ctypes.data_as(C.c_void_p), C.byref(rays), C.byref(shadow), C.byref(ms)),
                   "rt_render_wavefront_adaptive")
        return fix, half, count, {"rays": int(rays.value), "shadow_rays": int(shadow.value), "samples": int(count.sum(dtype=np.uint64)),
                                  "kernel_ms": float(ms.value)}

    # -- denoiser: an edge-avoiding a-trous filter driven by the feature buffers -------
    def denoise(self, fix, spp, feat, feat_spp, denoise=None, count=None):
        """rt_denoise: fix u64 [H,W,3] of `spp` samples (or of count[H,W] u32 samples per pixel: the adaptive frame), feat u64 [H,W,8] of
        `feat_spp` samples -> (the denoised ONE-SAMPLE frame u64 [H,W,3] -- resolve it with spp = 1 --, the kernels' time in ms)."""
        fix, feat, count, h, w = _denoise_arrays(fix, feat, count)
        dn = denoise if denoise is not None else make_denoise()
        out = np.zeros((h, w, 3), dtype=np.uint64)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_denoise(self._h, fix.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p) if count is not None else None,
                                        int(spp), feat.ctypes.data_as(C.c_void_p), int(feat_spp), w, h, C.byref(dn),
                                        out.ctypes.data_as(C.c_void_p), C.byref(ms)), "rt_denoise")
        return out, float(ms.value)

    def denoise_device(self, d_fix_ptr, spp, d_feat_ptr, feat_spp, width, height, denoise, d_work_ptr, d_out_ptr, d_count_ptr=0, stream=0):
        """rt_denoise_device: device pointers; d_work_ptr: denoise_workspace_bytes(width, height) bytes; asynchronous on `stream`."""
        _ffi.check(self._lib.rt_denoise_device(self._h, C.c_void_p(d_fix_ptr), C.c_void_p(d_count_ptr) if d_count_ptr else None, int(spp),
                                               C.c_void_p(d_feat_ptr), int(feat_spp), int(width), int(height), C.byref(denoise),
                                               C.c_void_p(d_work_ptr), C.c_void_p(d_out_ptr), C.c_void_p(stream)), "rt_denoise_device")

    @staticmethod
    def denoise_workspace_bytes(width, height):
        n = C.c_int64(0)
        _ffi.check(_ffi.load().rt_denoise_workspace_bytes(int(width), int(height), C.byref(n)), "rt_denoise_workspace_bytes")
        return int(n.value)

    denoise_host = staticmethod(denoise_host)

    # -- variance-guided denoiser: the colour stop in units of the noise the half-sample sums show -------
    def denoise_var(self, fix, half, spp, feat, feat_spp, denoise=None, count=None):
        """rt_denoise_var: as denoise, with half u64 [H,W,3], the sums of half of each pixel's samples -> (the denoised ONE-SAMPLE frame
        u64 [H,W,3], the kernels' time in ms)."""
        fix, half, feat, count, h, w = _denoise_var_arrays(fix, half, feat, count)
        dn = denoise if denoise is not None else make_denoise_var()
        out = np.zeros((h, w, 3), dtype=np.uint64)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_denoise_var(self._h, fix.ctypes.data_as(C.c_void_p), half.ctypes.data_as(C.c_void_p),
                                            count.ctypes.data_as(C.c_void_p) if count is not None else None, int(spp),
                                            feat.ctypes.data_as(C.c_void_p), int(feat_spp), w, h, C.byref(dn), out.ctypes.data_as(C.c_void_p),
                                            C.byref(ms)), "rt_denoise_var")
        return out, float(ms.value)

    def denoise_var_device(self, d_fix_ptr, d_half_ptr, spp, d_feat_ptr, feat_spp, width, height, denoise, d_work_ptr, d_out_ptr, d_count_ptr=0,
                           stream=0):
        """rt_denoise_var_device: device pointers; d_work_ptr: denoise_var_workspace_bytes(width, height) bytes; asynchronous on `stream`."""
        _ffi.check(self._lib.rt_denoise_var_device(self._h, C.c_void_p(d_fix_ptr), C.c_void_p(d_half_ptr) if d_half_ptr else None,
                                                   C.c_void_p(d_count_ptr) if d_count_ptr else None, int(spp), C.c_void_p(d_feat_ptr),
                                                   int(feat_spp), int(width), int(height), C.byref(denoise), C.c_void_p(d_work_ptr),
                                                   C.c_void_p(d_out_ptr), C.c_void_p(stream)), "rt_denoise_var_device")

    @staticmethod
    def denoise_var_workspace_bytes(width, height):
        n = C.c_int64(0)
        _ffi.check(_ffi.load().rt_denoise_var_workspace_bytes(int(width), int(height), C.byref(n)), "rt_denoise_var_workspace_bytes")
        return int(n.value)

    denoise_var_host = staticmethod(denoise_var_host)

    # -- temporal accumulation: the previous result, reprojected through the first hit ------
    def temporal(self, fix, spp, feat, feat_spp, cam, history=None, temporal=None, count=None):
        """rt_temporal: the arguments of temporal_host, on the device -> (the accumulated ONE-SAMPLE frame u64 [H,W,3], the history
        lengths u32 [H,W], the kernel's time in ms).  Feed the two arrays back as the next frame's history (with this frame's feat and camera)."""
        tp = temporal if temporal is not None else make_temporal()
        head, out_fix, out_len, keep = _temporal_args(fix, spp, feat, feat_spp, cam, history, count)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_temporal(self._h, *head, C.byref(tp), out_fix.ctypes.data_as(C.c_void_p), out_len.ctypes.data_as(C.c_void_p),
                                         C.byref(ms)), "rt_temporal")
        return out_fix, out_len, float(ms.value)

    def temporal_device(self, d_fix_ptr, spp, d_feat_ptr, feat_spp, cam, width, height, temporal, d_out_fix_ptr, d_out_len_ptr, history=None,
                        d_count_ptr=0, stream=0):
        """rt_temporal_device: device pointers, asynchronous on `stream`; history: None or (d_prev_fix_ptr, d_prev_len_ptr, d_prev_feat_ptr,
        prev_feat_spp, prev_cam) -- the cameras are host objects.  The outputs must not overlap the history: ping-pong."""
        vp = lambda q: C.c_void_p(q) if q else None
        rc = _rt_cam(cam)
        if history is None:
            hist = (None, None, None, 0, None)
        else:
            pc = _rt_cam(history[4])
            hist = (vp(history[0]), vp(history[1]), vp(history[2]), int(history[3]), C.byref(pc))
        _ffi.check(self._lib.rt_temporal_device(self._h, vp(d_fix_ptr), vp(d_count_ptr), int(spp), vp(d_feat_ptr), int(feat_spp), C.byref(rc), *hist,
                                                int(width), int(height), C.byref(temporal), vp(d_out_fix_ptr), vp(d_out_len_ptr), C.c_void_p(stream)),
                   "rt_temporal_device")

    temporal_host = staticmethod(temporal_host)

    def render_sequence(self, cams, params, sample_stride, feature_spp, temporal=None, denoise=None, flip=True):
        """An animation over the uploaded scene with temporal accumulation: render_frames (ONE launch; frame f takes the samples
        sample_begin + f * sample_stride on), per frame render_features with that frame's sample_begin (the guides see the frame's own camera
        rays), rt_temporal chained over the frames with ping-pong history, optionally rt_denoise on each accumulated frame (spp = 1, the frame's
        own guides), and the one-sample resolve.  temporal: an rt_temporal (None: make_temporal()); denoise: an rt_denoise or None (no spatial
        filter).  Returns (RGBA8 [F,H,W,4], the last frame's history lengths u32 [H,W])."""
        a = self._camera_array(cams)
        tp = temporal if temporal is not None else make_temporal()
        w, h = params.width, params.height
        fixes, _ = self.render_frames(a, params, sample_stride)
        out = np.zeros((len(a), h, w, 4), dtype=np.uint8)
        history, lengths = None, np.zeros((h, w), dtype=np.uint32)
        for f in range(len(a)):
            cam = _ffi.rt_camera.from_buffer_copy(a[f].tobytes())
            fp = make_params(w, h, feature_spp, sample_begin=params.sample_begin + f * int(sample_stride), t_min=params.t_min, seed=params.seed)
            feat, _, _ = self.render_features(cam, fp, want_ids=False)
            acc, lengths, _ = self.temporal(fixes[f], params.spp, feat, feature_spp, cam, history, tp)
            history = (acc, lengths, feat, feature_spp, cam)
            shown = self.denoise(acc, 1, feat, feature_spp, denoise)[0] if denoise is not None else acc
            out[f] = self.resolve_rgba8(shown, 1, flip=flip)
        return out, lengths

    # -- temporal accumulation with second moments, and the variance-guided denoiser fed by its variance ------
    def temporal_var(self, fix, spp, feat, feat_spp, cam, history=None, temporal=None, count=None):
        """rt_temporal_var: the arguments of temporal_var_host, on the device -> (out_fix, out_len, out_m2, out_var, the kernel's time in ms).
        Feed the first three back as the next frame's history (with this frame's feat and camera)."""
        tp = temporal if temporal is not None else make_temporal()
        head, out_fix, out_len, out_m2, out_var, keep = _temporal_var_args(fix, spp, feat, feat_spp, cam, history, count)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_temporal_var(self._h, *head, C.byref(tp), vp(out_fix), vp(out_len), vp(out_m2), vp(out_var), C.byref(ms)),
                   "rt_temporal_var")
        return out_fix, out_len, out_m2, out_var, float(ms.value)

    def temporal_var_device(self, d_fix_ptr, spp, d_feat_ptr, feat_spp, cam, width, height, temporal, d_out_fix_ptr, d_out_len_ptr, d_out_m2_ptr,
                            d_out_var_ptr, history=None, d_count_ptr=0, stream=0):
        """rt_temporal_var_device: device pointers, asynchronous on `stream`; history: None or (d_prev_fix_ptr, d_prev_len_ptr, d_prev_feat_ptr,
        prev_feat_spp, prev_cam, d_prev_m2_ptr) -- the cameras are host objects.  The outputs must not overlap the history: ping-pong."""
        vp = lambda q: C.c_void_p(q) if q else None
        rc = _rt_cam(cam)
        if history is None:
            hist = (None, None, None, 0, None, None)
        else:
            pc = _rt_cam(history[4])
            hist = (vp(history[0]), vp(history[1]), vp(history[2]), int(history[3]), C.byref(pc), vp(history[5]))
        _ffi.check(self._lib.rt_temporal_var_device(self._h, vp(d_fix_ptr), vp(d_count_ptr), int(spp), vp(d_feat_ptr), int(feat_spp), C.byref(rc),
                                                    *hist, int(width), int(height), C.byref(temporal), vp(d_out_fix_ptr), vp(d_out_len_ptr),
                                                    vp(d_out_m2_ptr), vp(d_out_var_ptr), C.c_void_p(stream)), "rt_temporal_var_device")

    temporal_var_host = staticmethod(temporal_var_host)

    def denoise_var_given(self, fix, var, spp, feat, feat_spp, denoise=None, count=None):
        """rt_denoise_var_given: as denoise_var, with var f64 [H,W,3] in half's place -> (the denoised ONE-SAMPLE frame u64 [H,W,3], the
        kernels' time in ms)."""
        fix, var, feat, count, h, w = _denoise_var_given_arrays(fix, var, feat, count)
        dn = denoise if denoise is not None else make_denoise_var()
        out = np.zeros((h, w, 3), dtype=np.uint64)
        ms = C.c_float(0.0)
        _ffi.check(self._lib.rt_denoise_var_given(self._h, fix.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p),
                                                  count.ctypes.data_as(C.c_void_p) if count is not None else None, int(spp),
                                                  feat.ctypes.data_as(C.c_void_p), int(feat_spp), w, h, C.byref(dn), out.ctypes.data_as(C.c_void_p),
                                                  C.byref(ms)), "rt_denoise_var_given")
        return out, float(ms.value)

    def denoise_var_given_device(self, d_fix_ptr, d_var_ptr, spp, d_feat_ptr, feat_spp, width, height, denoise, d_work_ptr, d_out_ptr, d_count_ptr=0,
                                 stream=0):
        """rt_denoise_var_given_device: device pointers; d_work_ptr: denoise_var_workspace_bytes(width, height) bytes; asynchronous on `stream`."""
        _ffi.check(self._lib.rt_denoise_var_given_device(self._h, C.c_void_p(d_fix_ptr), C.c_void_p(d_var_ptr) if d_var_ptr else None,
                                                         C.c_void_p(d_count_ptr) if d_count_ptr else None, int(spp), C.c_void_p(d_feat_ptr),
                                                         int(feat_spp), int(width), int(height), C.byref(denoise), C.c_void_p(d_work_ptr),
                                                         C.c_void_p(d_out_ptr), C.c_void_p(stream)), "rt_denoise_var_given_device")

    denoise_var_given_host = staticmethod(denoise_var_given_host)

    def render_sequence_var(self, cams, params, sample_stride, feature_spp, temporal=None, denoise=None, lighting=None, direct=False,
                            sampling="area", flip=True):
        """render_sequence with second moments and the variance-guided filter: per frame render_features, rt_temporal_var with ping-pong
        history, rt_denoise_var_given on the accumulated frame with the variance that call returns (spp = 1, the frame's own guides), and the
        one-sample resolve.  The frames come from render_frames (ONE launch) when lighting is None; otherwise frame f is render_wavefront
        with sample_begin + f * sample_stride and this lighting, direct and sampling.  temporal: an rt_temporal (None: make_temporal());
        denoise: an rt_denoise (None: make_denoise_var(sigma_color=TEMPORAL_VAR_SIGMA_COLOR)).  Returns (RGBA8 [F,H,W,4], the last frame's
        history lengths u32 [H,W], the last frame's out_var f64 [H,W,3])."""
        a = self._camera_array(cams)
        tp = temporal if temporal is not None else make_temporal()
        dn = denoise if denoise is not None else make_denoise_var(sigma_color=TEMPORAL_VAR_SIGMA_COLOR)
        w, h = params.width, params.height
        fixes = self.render_frames(a, params, sample_stride)[0] if lighting is None else None
        out = np.zeros((len(a), h, w, 4), dtype=np.uint8)
        history, lengths, var = None, np.zeros((h, w), dtype=np.uint32), np.zeros((h, w, 3), dtype=np.float64)
        for f in range(len(a)):
            cam = _ffi.rt_camera.from_buffer_copy(a[f].tobytes())
            begin = params.sample_begin + f * int(sample_stride)
            if lighting is None:
                fix = fixes[f]
            else:
                fp = make_params(w, h, params.spp, sample_begin=begin, max_depth=params.max_depth, t_min=params.t_min, seed=params.seed)
                fix = self.render_wavefront(cam, fp, lighting=lighting, direct=direct, sampling=sampling)[0]
            gp = make_params(w, h, feature_spp, sample_begin=begin, t_min=params.t_min, seed=params.seed)
            feat, _, _ = self.render_features(cam, gp, want_ids=False)
            acc, lengths, m2, var, _ = self.temporal_var(fix, params.spp, feat, feature_spp, cam, history, tp)
            history = (acc, lengths, feat, feature_spp, cam, m2)
            out[f] = self.resolve_rgba8(self.denoise_var_given(acc, var, 1, feat, feature_spp, dn)[0], 1, flip=flip)
        return out, lengths, var

    # -- to_rgba + flip --------------------------------------------------------
    def resolve_rgba8(self, fix, spp, flip=True):
        """fix: exact sums u64 [rows,W,3] -> RGBA8 [rows,W,4] (vec3.rs:403-421, main.rs:141-145)."""
        fix = np.ascontiguousarray(fix, dtype=np.uint64)
        rows, width = fix.shape[0], fix.shape[1]
        out = np.zeros((rows, width, 4), dtype=np.uint8)
        _ffi.check(self._lib.rt_resolve_rgba8(self._h, fix.ctypes.data_as(C.c_void_p), width, rows,
                                              int(spp), int(bool(flip)), out.ctypes.data_as(C.c_void_p)),
                   "rt_resolve_rgba8")
        return out

    def f64_div_sqrt(self, a, b):
        """Device-side a/b and sqrt(a) in f64 (known-answer test hook)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        q = np.zeros_like(a)
        r = np.zeros_like(a)
        _ffi.check(self._lib.rt_f64_div_sqrt_device(self._h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                                    int(a.size), q.ctypes.data_as(C.c_void_p),
                                                    r.ctypes.data_as(C.c_void_p)), "rt_f64_div_sqrt_device")
        return q, r

    def quantize(self, x):
        """The kernel's own quantisation of radiance values to the 2^-32 grid (known-answer test hook)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        q = np.zeros(x.shape, dtype=np.uint64)
        _ffi.check(self._lib.rt_quantize_device(self._h, x.ctypes.data_as(C.c_void_p), int(x.size), q.ctypes.data_as(C.c_void_p)),
                   "rt_quantize_device")
        return q

    def unit_accept(self, words):
        """The kernel's own rejection tests and word -> uniform rules on (n, 3) Philox words (known-answer test hook):
        returns (accept u32 [n]: bit 0 unit sphere, bit 1 unit disk; uniforms f64 [n, 4] = u01(wx), u11(wx), u11(wy), u11(wz))."""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 3)
        acc = np.zeros(len(w), dtype=np.uint32)
        uni = np.zeros((len(w), 4), dtype=np.float64)
        _ffi.check(self._lib.rt_unit_accept_device(self._h, w.ctypes.data_as(C.c_void_p), len(w), acc.ctypes.data_as(C.c_void_p),
                                                   uni.ctypes.data_as(C.c_void_p)), "rt_unit_accept_device")
        return acc, uni

    def filter_products(self, r1, r2, s, bf16x3=True):
        """Matrix-pipe filter products HB = R1 x S^T, Q = R2 x S^T of scan modes 2/3 (known-answer test
        hook; cross-check build only)."""
        if not _ffi.has_crosscheck_modes():
            raise _ffi.RtiowHipError("rt_filter_products_device needs the -DRTIOW_CROSSCHECK_MODES build (RTIOW_HIP_LIB)")
        r1 = np.ascontiguousarray(r1, dtype=np.float32).reshape(64, 4)
        r2 = np.ascontiguousarray(r2, dtype=np.float32).reshape(64, 4)
        s = np.ascontiguousarray(s, dtype=np.float32).reshape(16, 4)
        hb = np.zeros((64, 16), dtype=np.float32)
        q = np.zeros((64, 16), dtype=np.float32)
        _ffi.check(self._lib.rt_filter_products_device(self._h, r1.ctypes.data_as(C.c_void_p), r2.ctypes.data_as(C.c_void_p),
                                                       s.ctypes.data_as(C.c_void_p), int(bool(bf16x3)),
                                                       hb.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)),
                   "rt_filter_products_device")
        return hb, q

    def filter_lifted(self, o, d, spheres16):
        """One tile of the single-contraction filter (scan mode 4; cross-check build only), as the kernel evaluates it.

        o, d: (64, 3) f64 rays; spheres16: structured array (SPHERE_DTYPE) of 16 spheres.
        Returns D (64, 16) f32, R (64, 11) f32 per-ray terms, C (16, 11) f32 per-sphere terms."""
        if not _ffi.has_crosscheck_modes():
            raise _ffi.RtiowHipError("rt_filter_lifted_device needs the -DRTIOW_CROSSCHECK_MODES build (RTIOW_HIP_LIB)")
        o = np.ascontiguousarray(o, dtype=np.float64).reshape(64, 3)
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(64, 3)
        sp = np.ascontiguousarray(spheres16)
        assert sp.shape == (16,) and sp.dtype.itemsize == C.sizeof(_ffi.rt_sphere)
        D = np.zeros((64, 16), dtype=np.float32)
        R = np.zeros((64, 11), dtype=np.float32)
        Cc = np.zeros((16, 11), dtype=np.float32)
        _ffi.check(self._lib.rt_filter_lifted_device(self._h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                                     sp.ctypes.data_as(C.POINTER(_ffi.rt_sphere)),
                                                     D.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p),
                                                     Cc.ctypes.data_as(C.c_void_p)), "rt_filter_lifted_device")
        return D, R, Cc

    def grid_cells(self, o, d, grid, grid_dim, scale, runs=True):
        """The tile grid's footprint of n rays as the shipped kernel computes it (rt_device.hpp grid_cells / grid_row_run;
        cross-check build only).  o, d: (n, 3) f64; grid: the 8 f32 of tile_layout_host.
        Returns rect (n, 5) i32 = (verdict, ix0, nx, iz0, nz) and, with runs, (n, 63, 2) i32 = (rx0, rnx) of row iz0 + k."""
        if not _ffi.has_crosscheck_modes():
            raise _ffi.RtiowHipError("rt_grid_cells_device needs the -DRTIOW_CROSSCHECK_MODES build (RTIOW_HIP_LIB)")
        o = np.ascontiguousarray(o, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)
        assert o.shape == d.shape
        g = (C.c_float * 8)(*[float(v) for v in np.asarray(grid, dtype=np.float32)])
        rect = np.zeros((len(o), 5), dtype=np.int32)
        rr = np.zeros((len(o), 63, 2), dtype=np.int32) if runs else None
        _ffi.check(self._lib.rt_grid_cells_device(self._h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), len(o), g,
                                                  int(grid_dim), float(scale), rect.ctypes.data_as(C.c_void_p),
                                                  rr.ctypes.data_as(C.c_void_p) if runs else None), "rt_grid_cells_device")
        return (rect, rr) if runs else rect

    def filter_tube(self, o, d, spheres32):
        """One tile of the tube filter (the shipped scan mode), as the kernel evaluates it.

        o, d: (64, 3) f64 rays; spheres32: structured array (SPHERE_DTYPE) of 32 spheres.
        Returns h (64, 32, 2) f32, rows (64, 9) f32, bound (32,) f32, rho."""
        o = np.ascontiguousarray(o, dtype=np.float64).reshape(64, 3)
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(64, 3)
        sp = np.ascontiguousarray(spheres32)
        assert sp.shape == (32,) and sp.dtype.itemsize == C.sizeof(_ffi.rt_sphere)
        h = np.zeros((64, 32, 2), dtype=np.float32)
        rows = np.zeros((64, 9), dtype=np.float32)
        bound = np.zeros(32, dtype=np.float32)
        rho = C.c_float(0.0)
        _ffi.check(self._lib.rt_filter_tube_device(self._h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                                   sp.ctypes.data_as(C.POINTER(_ffi.rt_sphere)),
                                                   h.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                                   bound.ctypes.data_as(C.c_void_p), C.byref(rho)), "rt_filter_tube_device")
        return h, rows, bound, float(rho.value)

    def philox(self, ctr, key):
        c = (C.c_uint32 * 4)(*ctr)
        k = (C.c_uint32 * 2)(*key)
        o = (C.c_uint32 * 4)()
        _ffi.check(self._lib.rt_philox_device(self._h, c, k, o), "rt_philox_device")
        return tuple(int(x) for x in o)
