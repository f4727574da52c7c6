"""ctypes binding of librtiow_hip.so (include/rtiow_hip.h).

The library is the only compute backend: there is no Python or CPU fallback.
Loading fails loudly when the shared object has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or ./build_lib.sh).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTIOW_HIP_LIB: load another build of the same ABI instead (the tests use it for the cross-check
# build tools/librtiow_hip_xcheck.so, which also carries scan modes 2-4 and their known-answer hooks)
LIB_PATH = os.environ.get("RTIOW_HIP_LIB") or os.path.join(_HERE, "librtiow_hip.so")


class rt_sphere(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("radius", C.c_double), ("albedo", C.c_double * 3),
                ("param", C.c_double), ("kind", C.c_int32), ("reserved", C.c_int32)]


class rt_camera(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("lower_left_corner", C.c_double * 3),
                ("horizontal", C.c_double * 3), ("vertical", C.c_double * 3),
                ("u", C.c_double * 3), ("v", C.c_double * 3), ("lens_radius", C.c_double)]


class rt_params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32),
                ("sample_begin", C.c_int32), ("max_depth", C.c_int32), ("t_min", C.c_double),
                ("seed", C.c_uint64), ("tile_rows", C.c_int32), ("shard_index", C.c_int32),
                ("shard_count", C.c_int32), ("flags", C.c_uint32)]


class rt_stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays_traced", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("candidates", C.c_uint64), ("exact_roots", C.c_uint64), ("kernel_ms", C.c_float), ("n_spheres", C.c_int32),
                ("grid_blocks", C.c_int32), ("block_threads", C.c_int32), ("scan_mode", C.c_int32), ("kernel_variant", C.c_int32),
                ("live_per_bounce", C.c_uint64 * 64), ("direct_samples", C.c_uint64)]


class rt_adaptive(C.Structure):
    _fields_ = [("step", C.c_int32), ("reserved", C.c_int32), ("threshold", C.c_double), ("dark_floor", C.c_double)]


class rt_denoise(C.Structure):
    _fields_ = [("levels", C.c_int32), ("flags", C.c_uint32), ("sigma_color", C.c_double), ("sigma_normal", C.c_double),
                ("sigma_depth", C.c_double)]


class rt_temporal(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("alpha_min", C.c_double), ("sigma_normal", C.c_double),
                ("sigma_depth", C.c_double), ("clamp_scale", C.c_double)]


class rt_rays(C.Structure):
    _fields_ = [("origin", C.c_void_p), ("dir", C.c_void_p), ("t_max", C.c_void_p), ("n", C.c_int64)]


class rt_hits(C.Structure):
    _fields_ = [("index", C.c_void_p), ("t", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("front_face", C.c_void_p)]


class rt_camera_batch(C.Structure):
    _fields_ = [("pixel", C.c_void_p), ("sample", C.c_void_p), ("origin", C.c_void_p), ("dir", C.c_void_p), ("event", C.c_void_p), ("n", C.c_int64)]


class rt_scatter_batch(C.Structure):
    _fields_ = [("dir", C.c_void_p), ("index", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("front_face", C.c_void_p),
                ("pixel", C.c_void_p), ("sample", C.c_void_p), ("event", C.c_void_p), ("out_origin", C.c_void_p), ("out_dir", C.c_void_p),
                ("attenuation", C.c_void_p), ("status", C.c_void_p), ("n", C.c_int64)]


class rt_accumulate_batch(C.Structure):
    _fields_ = [("pixel", C.c_void_p), ("weight", C.c_void_p), ("sky_dir", C.c_void_p), ("select", C.c_void_p), ("n", C.c_int64)]


class rt_path_queue(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("count", C.c_void_p), ("pixel", C.c_void_p), ("sample", C.c_void_p), ("event", C.c_void_p),
                ("origin", C.c_void_p), ("dir", C.c_void_p), ("throughput", C.c_void_p), ("scratch", C.c_void_p)]


class rt_lighting(C.Structure):
    _fields_ = [("sky_bottom", C.c_double * 3), ("sky_top", C.c_double * 3), ("emission", C.c_void_p), ("n_emission", C.c_int32),
                ("flags", C.c_uint32)]


class rt_direct(C.Structure):
    _fields_ = [("lights", C.c_void_p), ("n_lights", C.c_int32), ("flags", C.c_uint32)]


class rt_environment(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("cdf", C.c_void_p), ("size", C.c_int32), ("flags", C.c_uint32)]


RT_FLAG_ACCUMULATE = 0x1
RT_FLAG_NO_FILTER = 0x2
RT_FLAG_DIAG_STATS = 0x4
RT_FLAG_UNIFORM53 = 0x8
RT_FLAG_OVERLAPPED = 0x10
RT_FLAG_KNOWN = 0x1f
RT_FEATURE_WORDS = 8        # u64 sums per pixel of a feature buffer: albedo rgb, normal xyz, depth, hits
RT_DENOISE_DEMODULATE = 0x1
RT_DENOISE_MAX_LEVELS = 8
RT_DENOISE_ALBEDO_FLOOR = 0.015625
RT_TEMPORAL_CLAMP = 0x1
RT_TEMPORAL_MAX_LEN = 65535
RT_TEMPORAL_VAR_MIN_LEN = 4
RT_PATH_EVENT_DIRECT = 0x80000000
RT_STEP_NO_DIRECT = 0x1
RT_DIRECT_CONE = 0x2
RT_DIRECT_WEIGHTED = 0x8
RT_ENV_MAX_SIZE = 1024
RT_SCATTER_ABSORBED, RT_SCATTER_SCATTERED, RT_SCATTER_MISS, RT_SCATTER_BAD_INDEX = 0, 1, 2, 3

# every symbol include/rtiow_hip.h declares: (name, restype, argtypes)
_VP = C.c_void_p
SYMBOLS = [
    ("rt_create", C.c_int, [C.c_int32, C.POINTER(_VP)]),
    ("rt_destroy", C.c_int, [_VP]),
    ("rt_upload_scene", C.c_int, [_VP, C.POINTER(rt_sphere), C.c_int32]),
    ("rt_shard_rows", C.c_int, [C.POINTER(rt_params), C.POINTER(C.c_int32)]),
    ("rt_shard_row_index", C.c_int, [C.POINTER(rt_params), C.c_int32, C.POINTER(C.c_int32)]),
    ("rt_render", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, _VP, C.POINTER(rt_stats)]),
    ("rt_render_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, _VP]),
    ("rt_fix_to_f32_device", C.c_int, [_VP, _VP, C.c_int64, _VP, _VP]),
    ("rt_last_stats", C.c_int, [_VP, C.POINTER(rt_stats)]),
    ("rt_resolve_rgba8_device", C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _VP, _VP]),
    ("rt_resolve_rgba8", C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _VP]),
    ("rt_render_rgba8", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int32, _VP, C.POINTER(rt_stats)]),
    ("rt_render_pixels_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, C.c_int64, _VP, _VP]),
    ("rt_render_pixels", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, C.c_int64, _VP, C.POINTER(rt_stats)]),
    ("rt_select_pixels_device", C.c_int, [_VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(rt_adaptive), _VP, _VP, _VP]),
    ("rt_select_pixels_host", C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(rt_adaptive), _VP, C.POINTER(C.c_int64)]),
    ("rt_render_adaptive", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_adaptive), _VP, _VP, _VP, C.POINTER(rt_stats)]),
    ("rt_resolve_rgba8_counts_device", C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP]),
    ("rt_resolve_rgba8_counts", C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP]),
    ("rt_render_frames_device", C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.POINTER(rt_params), _VP, _VP]),
    ("rt_render_frames", C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.POINTER(rt_params), _VP, C.POINTER(rt_stats)]),
    ("rt_render_frames_rgba8", C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.POINTER(rt_params), C.c_int32, _VP, C.POINTER(rt_stats)]),
    ("rt_render_features_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, _VP, _VP]),
    ("rt_render_features", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, _VP, C.POINTER(C.c_float)]),
    ("rt_features_to_f32_device", C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int64, _VP, _VP]),
    ("rt_features_to_f32", C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int64, _VP]),
    ("rt_denoise_workspace_bytes", C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("rt_denoise_device", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP, _VP, _VP]),
    ("rt_denoise", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP, C.POINTER(C.c_float)]),
    ("rt_denoise_host", C.c_int, [_VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP]),
    # the variance-guided denoiser: the same struct, and the half-sample sums behind fix
    ("rt_denoise_var_workspace_bytes", C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("rt_denoise_var_device", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP, _VP, _VP]),
    ("rt_denoise_var", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP, C.POINTER(C.c_float)]),
    ("rt_denoise_var_host", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP]),
    ("rt_temporal_device", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(rt_camera), _VP, _VP, _VP, C.c_int64, C.POINTER(rt_camera),
                                     C.c_int32, C.c_int32, C.POINTER(rt_temporal), _VP, _VP, _VP]),
    ("rt_temporal", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(rt_camera), _VP, _VP, _VP, C.c_int64, C.POINTER(rt_camera),
                              C.c_int32, C.c_int32, C.POINTER(rt_temporal), _VP, _VP, C.POINTER(C.c_float)]),
    ("rt_temporal_host", C.c_int, [_VP, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(rt_camera), _VP, _VP, _VP, C.c_int64, C.POINTER(rt_camera),
                                   C.c_int32, C.c_int32, C.POINTER(rt_temporal), _VP, _VP]),
    # temporal accumulation with second moments: prev_m2 behind prev_cam, out_m2 and out_var behind out_len
    ("rt_temporal_var_device", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(rt_camera), _VP, _VP, _VP, C.c_int64,
                                         C.POINTER(rt_camera), _VP, C.c_int32, C.c_int32, C.POINTER(rt_temporal), _VP, _VP, _VP, _VP, _VP]),
    ("rt_temporal_var", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(rt_camera), _VP, _VP, _VP, C.c_int64, C.POINTER(rt_camera),
                                  _VP, C.c_int32, C.c_int32, C.POINTER(rt_temporal), _VP, _VP, _VP, _VP, C.POINTER(C.c_float)]),
    ("rt_temporal_var_host", C.c_int, [_VP, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(rt_camera), _VP, _VP, _VP, C.c_int64, C.POINTER(rt_camera),
                                       _VP, C.c_int32, C.c_int32, C.POINTER(rt_temporal), _VP, _VP, _VP, _VP]),
    # the variance-guided denoiser with the variance given: rt_denoise_var's arguments, var [H][W][3] f64 in half's place
    ("rt_denoise_var_given_device", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP, _VP,
                                              _VP]),
    ("rt_denoise_var_given", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP,
                                       C.POINTER(C.c_float)]),
    ("rt_denoise_var_given_host", C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(rt_denoise), _VP]),
    ("rt_trace_rays_device", C.c_int, [_VP, C.POINTER(rt_rays), C.c_double, C.POINTER(rt_hits), _VP]),
    ("rt_trace_rays", C.c_int, [_VP, C.POINTER(rt_rays), C.c_double, C.POINTER(rt_hits), C.POINTER(C.c_float)]),
    ("rt_occluded_device", C.c_int, [_VP, C.POINTER(rt_rays), C.c_double, _VP, _VP]),
    ("rt_occluded", C.c_int, [_VP, C.POINTER(rt_rays), C.c_double, _VP, C.POINTER(C.c_float)]),
    ("rt_camera_rays_device", C.c_int, [_VP, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.POINTER(rt_camera_batch), _VP]),
    ("rt_camera_rays", C.c_int, [_VP, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.POINTER(rt_camera_batch),
                        C.POINTER(C.c_float)]),
    ("rt_scatter_device", C.c_int, [_VP, C.c_uint64, C.c_uint32, C.POINTER(rt_scatter_batch), _VP]),
    ("rt_scatter", C.c_int, [_VP, C.c_uint64, C.c_uint32, C.POINTER(rt_scatter_batch), C.POINTER(C.c_float)]),
    ("rt_accumulate_device", C.c_int, [_VP, C.POINTER(rt_accumulate_batch), _VP, C.c_int64, _VP]),
    ("rt_accumulate", C.c_int, [_VP, C.POINTER(rt_accumulate_batch), _VP, C.c_int64, C.POINTER(C.c_float)]),
    ("rt_path_scratch_words", C.c_int64, [C.c_int64]),
    ("rt_paths_begin_device", C.c_int, [_VP, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int64,
                                        C.c_int64, C.POINTER(rt_path_queue), _VP]),
    ("rt_paths_step_device", C.c_int, [_VP, C.c_uint64, C.c_uint32, C.c_double, C.POINTER(rt_path_queue), C.POINTER(rt_path_queue), _VP, C.c_int64,
                                       _VP, _VP]),
    ("rt_render_wavefront_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, _VP, _VP]),
    ("rt_render_wavefront", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), _VP, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    ("rt_paths_step_lit_device", C.c_int, [_VP, C.c_uint64, C.c_uint32, C.c_double, C.POINTER(rt_path_queue), C.POINTER(rt_path_queue), _VP,
                                           C.c_int64, _VP, C.POINTER(rt_lighting), _VP]),
    ("rt_render_wavefront_lit_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), _VP, _VP, _VP]),
    ("rt_render_wavefront_lit", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), _VP, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_float)]),
    ("rt_light_list", C.c_int, [_VP, C.c_int32, _VP, C.POINTER(C.c_int32)]),
    ("rt_paths_step_nee_device", C.c_int, [_VP, C.c_uint64, C.c_uint32, C.c_double, C.POINTER(rt_path_queue), C.POINTER(rt_path_queue), _VP,
                                           C.c_int64, _VP, C.POINTER(rt_lighting), C.POINTER(rt_direct), C.c_uint32, _VP, _VP]),
    ("rt_render_wavefront_nee_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), C.POINTER(rt_direct), _VP,
                                                 _VP, _VP, _VP]),
    ("rt_render_wavefront_nee", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), _VP, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    ("rt_render_wavefront_nee_sampled", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), C.c_uint32, _VP,
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    ("rt_paths_begin_pixels_device", C.c_int, [_VP, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int64,
                                               C.c_int64, _VP, C.c_int64, C.POINTER(rt_path_queue), _VP]),
    ("rt_render_wavefront_pixels_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), C.POINTER(rt_direct), _VP,
                                                    C.c_int64, _VP, _VP, _VP, _VP]),
    ("rt_render_wavefront_pixels", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), C.c_int32, C.c_uint32, _VP,
                                             C.c_int64, _VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    ("rt_render_wavefront_adaptive", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_adaptive), C.POINTER(rt_lighting),
                                               C.c_int32, C.c_uint32, _VP, _VP, _VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_float)]),
    # the environment cube map: the pure host table, the step, the two frames (the host form: sample behind env)
    ("rt_environment_cdf", C.c_int, [_VP, C.c_int32, _VP]),
    ("rt_paths_step_env_device", C.c_int, [_VP, C.c_uint64, C.c_uint32, C.c_double, C.POINTER(rt_path_queue), C.POINTER(rt_path_queue), _VP,
                                           C.c_int64, _VP, C.POINTER(rt_lighting), C.POINTER(rt_environment), C.c_uint32, _VP, _VP]),
    ("rt_render_wavefront_env_device", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), C.POINTER(rt_environment),
                                                 _VP, _VP, _VP, _VP]),
    ("rt_render_wavefront_env", C.c_int, [_VP, C.POINTER(rt_camera), C.POINTER(rt_params), C.POINTER(rt_lighting), C.POINTER(rt_environment),
                                          C.c_int32, _VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    ("rt_last_error", C.c_char_p, []),
    ("rt_backend_name", C.c_char_p, []),
    ("rt_abi_version", C.c_int32, []),
    ("rt_build_source_sha", C.c_char_p, []),
    ("rt_philox_device", C.c_int, [_VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("rt_f64_div_sqrt_device", C.c_int, [_VP, _VP, _VP, C.c_int32, _VP, _VP]),
    ("rt_quantize_device", C.c_int, [_VP, _VP, C.c_int32, _VP]),
    ("rt_unit_accept_device", C.c_int, [_VP, _VP, C.c_int32, _VP, _VP]),
    ("rt_tube_tile_host", C.c_int, [C.POINTER(rt_sphere), _VP, _VP, C.POINTER(C.c_float)]),
    ("rt_tile_layout_host", C.c_int, [C.POINTER(rt_sphere), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32]),
    ("rt_filter_tube_device", C.c_int, [_VP, _VP, _VP, C.POINTER(rt_sphere), _VP, _VP, _VP, C.POINTER(C.c_float)]),
]

# declared under RTIOW_CROSSCHECK_MODES in the header: present only in the cross-check build
XCHECK_SYMBOLS = [
    ("rt_filter_products_device", C.c_int, [_VP, _VP, _VP, _VP, C.c_int32, _VP, _VP]),
    ("rt_filter_lifted_device", C.c_int, [_VP, _VP, _VP, C.POINTER(rt_sphere), _VP, _VP, _VP]),
    ("rt_grid_cells_device", C.c_int, [_VP, _VP, _VP, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.c_float, _VP, _VP]),
]

# include/rtiow_hip_diag.h: diagnostics outside the C ABI of rtiow_hip.h
DIAG_SYMBOLS = [
    ("rt_last_dense_body", C.c_int32, [_VP]),
]

_lib = None


class RtiowHipError(RuntimeError):
    pass


def load():
    """Returns the loaded library with prototypes set; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtiowHipError(
            f"{LIB_PATH} not found: build it with ./build_lib.sh (hipcc --offload-arch=gfx950); "
            "there is no CPU fallback for the render path")
    # One process, one HIP runtime.  PyTorch ships its own libamdhip64.so.7 and the dynamic
    # loader binds every later request for that SONAME to whichever copy came first; PyTorch
    # only works on its own copy, this library works on either.  So when torch is installed
    # it is imported first (device memory, streams and torch.distributed come from it anyway).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    for name, res, args in DIAG_SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, res, args in XCHECK_SYMBOLS:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def has_crosscheck_modes():
    """True when the loaded library is the -DRTIOW_CROSSCHECK_MODES build (scan modes 2-4 and their hooks)."""
    return hasattr(load(), "rt_filter_lifted_device")


def check(rc, what):
    if rc != 0:
        msg = load().rt_last_error().decode("utf-8", "replace")
        raise RtiowHipError(f"{what} failed ({rc}): {msg}")
