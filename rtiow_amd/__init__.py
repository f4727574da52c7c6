"""rtiow_amd -- MI355X-native hot path of Druthyn/rtiow.

The package holds only what the path needs: the HIP megakernel and its C ABI
(csrc/, built into librtiow_hip.so), a ctypes binding, and a host-side mirror
of the reference's scene interface (Camera, Sphere, Lambertian, Metal,
Dialectric, HittableList, random_scene).  See DESIGN.md.
"""
from .scene import (Camera, Color, Dialectric, HittableList, Lambertian, Metal, Point3, Scatter,
                    Sphere, Vec3, book1_camera, random_scene, save_scene, load_scene, SPHERE_DTYPE,
                    orbit_cameras, save_cameras, load_cameras, cameras_to_array)
from .render import Renderer, make_params, make_adaptive, make_denoise, denoise_host, make_denoise_var, denoise_var_host, make_temporal, temporal_host, temporal_var_host, denoise_var_given_host, select_pixels_host, shard_rows, shard_row_indices, tube_tile_host, tile_layout_host, trace_rays_torch, occluded_torch, camera_rays_torch, scatter_torch, accumulate_torch, render_wavefront_torch, PathQueue, paths_begin_torch, paths_begin_pixels_torch, paths_step_torch, Lighting, Environment
from .image import write_ppm, read_ppm, write_png, read_png, save_checkpoint, load_checkpoint
from ._ffi import RtiowHipError, RT_FLAG_ACCUMULATE, RT_FLAG_NO_FILTER, RT_FLAG_DIAG_STATS, RT_FLAG_UNIFORM53, RT_FLAG_OVERLAPPED, RT_FEATURE_WORDS, RT_DENOISE_DEMODULATE, RT_TEMPORAL_CLAMP, RT_TEMPORAL_MAX_LEN, RT_TEMPORAL_VAR_MIN_LEN

__all__ = ["Camera", "Color", "Dialectric", "HittableList", "Lambertian", "Metal", "Point3", "Scatter",
           "Sphere", "Vec3", "book1_camera", "random_scene", "SPHERE_DTYPE", "orbit_cameras", "save_cameras", "load_cameras", "cameras_to_array", "Renderer", "make_params", "make_adaptive", "make_denoise", "denoise_host", "make_denoise_var", "denoise_var_host", "make_temporal", "temporal_host", "temporal_var_host", "denoise_var_given_host", "select_pixels_host",
           "trace_rays_torch", "occluded_torch", "camera_rays_torch", "scatter_torch", "accumulate_torch", "render_wavefront_torch", "PathQueue", "paths_begin_torch", "paths_begin_pixels_torch", "paths_step_torch", "Lighting", "Environment", "shard_rows", "shard_row_indices", "tube_tile_host", "tile_layout_host", "write_ppm", "read_ppm", "write_png", "read_png", "save_scene", "load_scene", "save_checkpoint", "load_checkpoint", "RtiowHipError", "RT_FLAG_ACCUMULATE", "RT_FLAG_NO_FILTER", "RT_FLAG_DIAG_STATS", "RT_FLAG_UNIFORM53", "RT_FLAG_OVERLAPPED", "RT_FEATURE_WORDS", "RT_DENOISE_DEMODULATE", "RT_TEMPORAL_CLAMP", "RT_TEMPORAL_MAX_LEN", "RT_TEMPORAL_VAR_MIN_LEN"]
