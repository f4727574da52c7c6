//! Raw FFI of `librtiow_hip.so` (C ABI: `include/rtiow_hip.h`, ABI version 5).
//!
//! UNCOMPILED: there is no rustc/cargo in the build image of this repository, so this file has never
//! been through a Rust compiler.  What IS checked (tests/test_rust_binding.py, CPU): every `#[repr(C)]`
//! struct below has the same fields, in the same order and of the same C type, as its counterpart in
//! include/rtiow_hip.h; the `const` assertions state the sizes and offsets the C side is tested for
//! (tests/test_cabi.py); and the `extern "C"` block declares exactly the functions the header declares.
//!
//! What the entry points stand in for in the reference (Druthyn/rtiow): the iterator expression at
//! src/main.rs:122-139 (`rt_render`), `Color::to_rgba` src/vec3.rs:403-421 + the flip src/main.rs:141-145
//! (`rt_resolve_rgba8`), both in one call with the sums kept on the device (`rt_render_rgba8`: the bytes
//! `ImageBuffer::from_vec` takes at src/main.rs:147), the capture of `&world` at src/main.rs:135 (`rt_upload_scene`).
#![allow(non_camel_case_types, dead_code)]

use core::mem::{offset_of, size_of};
use std::os::raw::{c_char, c_void};

pub const RTIOW_HIP_ABI_VERSION: i32 = 5;

pub const RT_OK: i32 = 0;
pub const RT_ERR_INVALID_ARGUMENT: i32 = -1;
pub const RT_ERR_NO_DEVICE: i32 = -2;
pub const RT_ERR_HIP: i32 = -3;
pub const RT_ERR_NO_SCENE: i32 = -4;
pub const RT_ERR_OUT_OF_MEMORY: i32 = -5;

/// Material kinds: the three `impl Scatter` of src/materials.rs.
pub const RT_LAMBERTIAN: i32 = 0;
pub const RT_METAL: i32 = 1;
pub const RT_DIALECTRIC: i32 = 2;

pub const RT_FLAG_ACCUMULATE: u32 = 0x1;
pub const RT_FLAG_NO_FILTER: u32 = 0x2;
pub const RT_FLAG_DIAG_STATS: u32 = 0x4;
pub const RT_FLAG_UNIFORM53: u32 = 0x8;
pub const RT_FLAG_OVERLAPPED: u32 = 0x10;
pub const RT_FLAG_KNOWN: u32 = 0x1f;

/// The two limits of the boundary where the reference's own types are unbounded (include/rtiow_hip.h): the length of
/// `HittableList` (src/shapes/mod.rs:52) and the pixel sum (src/main.rs:127,135: here exact u64 sums of samples clamped at 2^16).
pub const RT_MAX_SPHERES: i32 = 1 << 24;
pub const RT_SAMPLE_CLAMP: f64 = 65536.0;

/// Opaque `rt_context`.
#[repr(C)]
pub struct rt_context {
    _private: [u8; 0],
}

/// One sphere, flattened (src/shapes/sphere.rs:9-13 + src/materials.rs:9-11,34-37,64-66).  LIST ORDER IS
/// PART OF THE INPUT: on equal t the later sphere wins (src/shapes/mod.rs:61-67).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct rt_sphere {
    pub center: [f64; 3],
    pub radius: f64,
    pub albedo: [f64; 3],
    pub param: f64,
    pub kind: i32,
    pub reserved: i32,
}

/// src/camera.rs:4-13 minus `w` (never read by `get_ray`).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct rt_camera {
    pub origin: [f64; 3],
    pub lower_left_corner: [f64; 3],
    pub horizontal: [f64; 3],
    pub vertical: [f64; 3],
    pub u: [f64; 3],
    pub v: [f64; 3],
    pub lens_radius: f64,
}

/// What src/main.rs:24-28,44 fixes at compile time, plus sharding.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct rt_params {
    pub width: i32,
    pub height: i32,
    pub spp: i32,
    pub sample_begin: i32,
    pub max_depth: i32,
    pub t_min: f64,
    pub seed: u64,
    pub tile_rows: i32,
    pub shard_index: i32,
    pub shard_count: i32,
    pub flags: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct rt_stats {
    pub samples: u64,
    pub rays_traced: u64,
    pub sphere_tests: u64,
    pub candidates: u64,
    pub exact_roots: u64,
    pub kernel_ms: f32,
    pub n_spheres: i32,
    pub grid_blocks: i32,
    pub block_threads: i32,
    pub scan_mode: i32,
    pub kernel_variant: i32,
    pub live_per_bounce: [u64; 64],
    pub direct_samples: u64,
}

/// Adaptive sampling (`rt_render_adaptive`, `rt_select_pixels_*`): `step` samples per pass; a pixel stops once its error
/// estimate -- the mean absolute difference of its two half-buffer means over sqrt(max(mean, dark_floor)) -- is <= threshold.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_adaptive {
    pub step: i32,
    pub reserved: i32,
    pub threshold: f64,
    pub dark_floor: f64,
}

/// The denoiser's options (`rt_denoise`, `rt_denoise_device`, `rt_denoise_host`): `levels` a-trous levels with hole step 2^l,
/// `flags` = `RT_DENOISE_DEMODULATE` or 0, and the widths of the three edge-stops (colour, halved per level; normal; relative depth).
/// (The C header spells the type `struct rt_denoise`: it shares its name with the host-buffer entry point.)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_denoise {
    pub levels: i32,
    pub flags: u32,
    pub sigma_color: f64,
    pub sigma_normal: f64,
    pub sigma_depth: f64,
}

/// The options of temporal accumulation (`rt_temporal`, `rt_temporal_device`, `rt_temporal_host`): `flags` = `RT_TEMPORAL_CLAMP` or 0,
/// the least weight of the current frame, the widths of the normal and the relative-depth test a history tap must pass, and the scale of
/// the neighbourhood clamp.  (The C header spells the type `struct rt_temporal`: it shares its name with the host-buffer entry point.)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_temporal {
    pub flags: u32,
    pub reserved: u32,
    pub alpha_min: f64,
    pub sigma_normal: f64,
    pub sigma_depth: f64,
    pub clamp_scale: f64,
}

pub const RT_TEMPORAL_CLAMP: u32 = 0x1;
pub const RT_TEMPORAL_MAX_LEN: u32 = 65535;

pub const RT_DENOISE_DEMODULATE: u32 = 0x1;
pub const RT_DENOISE_MAX_LEVELS: i32 = 8;
pub const RT_DENOISE_ALBEDO_FLOOR: f64 = 0.015625;

// Layout assertions: the numbers tests/test_cabi.py asserts on the C side (ctypes mirrors of the header).
const _: () = assert!(size_of::<rt_sphere>() == 72);
const _: () = assert!(offset_of!(rt_sphere, kind) == 64);
const _: () = assert!(size_of::<rt_camera>() == 152);
const _: () = assert!(size_of::<rt_params>() == 56);
const _: () = assert!(offset_of!(rt_params, t_min) == 24);
const _: () = assert!(offset_of!(rt_params, seed) == 32);
const _: () = assert!(size_of::<rt_stats>() == 584);
const _: () = assert!(offset_of!(rt_stats, live_per_bounce) == 64);
const _: () = assert!(offset_of!(rt_adaptive, threshold) == 8);
const _: () = assert!(offset_of!(rt_adaptive, dark_floor) == 16);
const _: () = assert!(offset_of!(rt_denoise, sigma_color) == 8);
const _: () = assert!(offset_of!(rt_denoise, sigma_depth) == 24);
const _: () = assert!(32 == size_of::<rt_denoise>());
const _: () = assert!(offset_of!(rt_temporal, alpha_min) == 8);
const _: () = assert!(offset_of!(rt_temporal, clamp_scale) == 32);
const _: () = assert!(40 == size_of::<rt_temporal>());

/// A batch of rays for `rt_trace_rays` / `rt_occluded`, structure-of-arrays: `origin` and `dir` are `[n][3]` (the direction is not
/// normalised), `t_max` is `[n]` or null (+inf for every ray).  Host pointers for the host forms, device pointers for the device forms.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_rays {
    pub origin: *const f64,
    pub dir: *const f64,
    pub t_max: *const f64,
    pub n: i64,
}

/// Where `rt_trace_rays` writes: `index` (`[n]`, required: the winner's place in the uploaded list, -1 a miss) and, each optional (null),
/// `t` `[n]`, `point` `[n][3]`, `normal` `[n][3]`, `front_face` `[n]`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_hits {
    pub index: *mut i32,
    pub t: *mut f64,
    pub point: *mut f64,
    pub normal: *mut f64,
    pub front_face: *mut u8,
}

const _: () = assert!(offset_of!(rt_rays, n) == 24);
const _: () = assert!(32 == size_of::<rt_rays>());
const _: () = assert!(offset_of!(rt_hits, front_face) == 32);
const _: () = assert!(40 == size_of::<rt_hits>());

/// `RT_SCATTER_*`: what `rt_scatter` writes to `status`.
pub const RT_SCATTER_ABSORBED: u8 = 0;
pub const RT_SCATTER_SCATTERED: u8 = 1;
pub const RT_SCATTER_MISS: u8 = 2;
pub const RT_SCATTER_BAD_INDEX: u8 = 3;

/// The paths of `rt_camera_rays`, structure-of-arrays: `pixel` and `sample` `[n]` in; `origin`, `dir` `[n][3]` and `event` `[n]` out.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_camera_batch {
    pub pixel: *const u32,
    pub sample: *const u32,
    pub origin: *mut f64,
    pub dir: *mut f64,
    pub event: *mut u32,
    pub n: i64,
}

/// The paths of `rt_scatter`: the incoming `dir`, the hit as `rt_trace_rays` wrote it, the path's `(pixel, sample)` and its `event`
/// (in and out); `out_origin`, `out_dir` (may be `dir`), `attenuation` `[n][3]` and `status` `[n]` out.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_scatter_batch {
    pub dir: *const f64,
    pub index: *const i32,
    pub point: *const f64,
    pub normal: *const f64,
    pub front_face: *const u8,
    pub pixel: *const u32,
    pub sample: *const u32,
    pub event: *mut u32,
    pub out_origin: *mut f64,
    pub out_dir: *mut f64,
    pub attenuation: *mut f64,
    pub status: *mut u8,
    pub n: i64,
}

/// The samples of `rt_accumulate`: `pixel` `[n]`, `weight` `[n][3]`, `sky_dir` `[n][3]` or null, `select` `[n]` or null.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_accumulate_batch {
    pub pixel: *const u32,
    pub weight: *const f64,
    pub sky_dir: *const f64,
    pub select: *const u8,
    pub n: i64,
}

/// A path queue (`rt_paths_begin_device`, `rt_paths_step_device`): structure-of-arrays in DEVICE memory, caller-owned.  The live paths are
/// slots `[0, *count)`; `count` is one device word the kernels read and the host never does.  `scratch`: `rt_path_scratch_words(capacity)` words.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_path_queue {
    pub capacity: i64,
    pub count: *mut u32,
    pub pixel: *mut u32,
    pub sample: *mut u32,
    pub event: *mut u32,
    pub origin: *mut f64,
    pub dir: *mut f64,
    pub throughput: *mut f64,
    pub scratch: *mut u32,
}

/// What lights a frame of the path queue (`rt_paths_step_lit_device`, `rt_render_wavefront_lit*`): the two ends of the sky gradient and one
/// radiance per uploaded sphere (`emission`: `[n_emission][3]`, a DEVICE pointer in the `_device` forms, a host pointer in
/// `rt_render_wavefront_lit`; null: no lights).  A sphere is a light iff a channel of its entry is `> 0`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_lighting {
    pub sky_bottom: [f64; 3],
    pub sky_top: [f64; 3],
    pub emission: *const f64,
    pub n_emission: i32,
    pub flags: u32,
}

const _: () = assert!(offset_of!(rt_lighting, sky_top) == 24);
const _: () = assert!(offset_of!(rt_lighting, emission) == 48);
const _: () = assert!(offset_of!(rt_lighting, n_emission) == 56);
const _: () = assert!(offset_of!(rt_lighting, flags) == 60);
const _: () = assert!(64 == size_of::<rt_lighting>());

/// Bit 31 of a path's `event` word: its last scatter sampled the lights directly (`rt_paths_step_nee_device`).
pub const RT_PATH_EVENT_DIRECT: u32 = 0x8000_0000;
/// The only legal step flag of `rt_paths_step_nee_device`: the step neither samples lights nor sets the bit.
pub const RT_STEP_NO_DIRECT: u32 = 1;
/// A bit of `rt_direct.flags`: the light is sampled by solid angle (a uniform direction of the cone it subtends), not by area.
pub const RT_DIRECT_CONE: u32 = 2;
/// A bit of `rt_direct.flags`, legal only together with `RT_DIRECT_CONE` (the legal values are 0, 2 and 10): the light is chosen by
/// what it can contribute at the hit point, `(r^2 / d^2) max(e)`, not uniformly.
pub const RT_DIRECT_WEIGHTED: u32 = 8;

/// The lights that next-event estimation samples (`rt_paths_step_nee_device`, `rt_render_wavefront_nee_device`): `lights`:
/// `[n_lights]` sphere indices, a DEVICE pointer; `rt_light_list` makes the list of an emission table on the host.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_direct {
    pub lights: *const i32,
    pub n_lights: i32,
    pub flags: u32,
}

const _: () = assert!(offset_of!(rt_direct, n_lights) == 8);
const _: () = assert!(offset_of!(rt_direct, flags) == 12);
const _: () = assert!(16 == size_of::<rt_direct>());

/// The largest `rt_environment.size`.
pub const RT_ENV_MAX_SIZE: i32 = 1024;

/// An environment cube map for the lit path queue (`rt_paths_step_env_device`, `rt_render_wavefront_env*`): `texels`:
/// `[6][size][size][3]` radiance, `cdf`: `[6 * size * size]` running sums from `rt_environment_cdf` or null (looked up, never
/// sampled); DEVICE pointers in the `_device` forms, HOST pointers in `rt_render_wavefront_env`.  `size`: a power of two.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_environment {
    pub texels: *const f64,
    pub cdf: *const f64,
    pub size: i32,
    pub flags: u32,
}

const _: () = assert!(offset_of!(rt_environment, cdf) == 8);
const _: () = assert!(offset_of!(rt_environment, size) == 16);
const _: () = assert!(offset_of!(rt_environment, flags) == 20);
const _: () = assert!(24 == size_of::<rt_environment>());
const _: () = assert!(offset_of!(rt_path_queue, count) == 8);
const _: () = assert!(offset_of!(rt_path_queue, scratch) == 64);
const _: () = assert!(72 == size_of::<rt_path_queue>());
const _: () = assert!(offset_of!(rt_camera_batch, n) == 40);
const _: () = assert!(48 == size_of::<rt_camera_batch>());
const _: () = assert!(offset_of!(rt_scatter_batch, n) == 96);
const _: () = assert!(104 == size_of::<rt_scatter_batch>());
const _: () = assert!(offset_of!(rt_accumulate_batch, n) == 32);
const _: () = assert!(40 == size_of::<rt_accumulate_batch>());

#[link(name = "rtiow_hip")]
extern "C" {
    pub fn rt_create(device_id: i32, out: *mut *mut rt_context) -> i32;
    pub fn rt_destroy(ctx: *mut rt_context) -> i32;
    pub fn rt_upload_scene(ctx: *mut rt_context, spheres: *const rt_sphere, n: i32) -> i32;
    pub fn rt_shard_rows(p: *const rt_params, out_rows: *mut i32) -> i32;
    pub fn rt_shard_row_index(p: *const rt_params, compact_row: i32, out_j: *mut i32) -> i32;
    pub fn rt_render(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params,
                     out_sum: *mut f32, out_fix: *mut u64, stats: *mut rt_stats) -> i32;
    pub fn rt_render_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params,
                            d_fix: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_fix_to_f32_device(ctx: *mut rt_context, d_fix: *const c_void, count: i64,
                                d_out_f32: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_last_stats(ctx: *mut rt_context, stats: *mut rt_stats) -> i32;
    pub fn rt_resolve_rgba8_device(ctx: *mut rt_context, d_fix: *const c_void, width: i32, rows: i32,
                                   spp: i64, flip: i32, d_rgba: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_resolve_rgba8(ctx: *mut rt_context, fix: *const u64, width: i32, rows: i32,
                            spp: i64, flip: i32, out_rgba: *mut u8) -> i32;
    pub fn rt_render_rgba8(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, flip: i32,
                           out_rgba: *mut u8, stats: *mut rt_stats) -> i32;
    /// src/main.rs:122-139 for a LIST of pixels (g = j * width + i, j = 0 the bottom row); d_fix: [n_pixels][3] u64, entry k for d_pixels[k].
    pub fn rt_render_pixels_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, d_pixels: *const u32,
                                   n_pixels: i64, d_fix: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_render_pixels(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, pixels: *const u32,
                            n_pixels: i64, out_fix: *mut u64, stats: *mut rt_stats) -> i32;
    /// Which pixels still need samples after a round that brought them to `n` (ascending pixel numbers).
    pub fn rt_select_pixels_device(ctx: *mut rt_context, d_fix: *const c_void, d_half: *const c_void, d_count: *const c_void,
                                   width: i32, height: i32, n: i32, a: *const rt_adaptive, d_list_out: *mut c_void,
                                   d_n_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_select_pixels_host(fix: *const u64, half: *const u64, count: *const u32, width: i32, height: i32, n: i32,
                                 a: *const rt_adaptive, list_out: *mut u32, n_out: *mut i64) -> i32;
    /// src/main.rs:130-137 with a per-pixel number of samples; `p.spp` is the most a pixel may get.
    pub fn rt_render_adaptive(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, a: *const rt_adaptive,
                              out_fix: *mut u64, out_half: *mut u64, out_count: *mut u32, stats: *mut rt_stats) -> i32;
    /// `Color::to_rgba` (src/vec3.rs:403-421) with each pixel's own sample count.
    pub fn rt_resolve_rgba8_counts_device(ctx: *mut rt_context, d_fix: *const c_void, d_count: *const c_void, width: i32,
                                          rows: i32, flip: i32, d_rgba: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_resolve_rgba8_counts(ctx: *mut rt_context, fix: *const u64, count: *const u32, width: i32, rows: i32,
                                   flip: i32, out_rgba: *mut u8) -> i32;
    /// Frame batches: src/main.rs:108-139 once per camera, in ONE launch.  `d_cams`: DEVICE [n_frames] rt_camera; `d_fix`: device
    /// [n_frames][height][width][3] u64.  Frame f is the dense render of camera f with `sample_begin + f * sample_stride`.
    pub fn rt_render_frames_device(ctx: *mut rt_context, d_cams: *const rt_camera, n_frames: i32, sample_stride: i32,
                                   p: *const rt_params, d_fix: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_render_frames(ctx: *mut rt_context, cams: *const rt_camera, n_frames: i32, sample_stride: i32,
                            p: *const rt_params, out_fix: *mut u64, stats: *mut rt_stats) -> i32;
    /// ... + `Color::to_rgba` and the row flip per frame: `out_rgba` is [n_frames][height][width][4].
    pub fn rt_render_frames_rgba8(ctx: *mut rt_context, cams: *const rt_camera, n_frames: i32, sample_stride: i32,
                                  p: *const rt_params, flip: i32, out_rgba: *mut u8, stats: *mut rt_stats) -> i32;
    /// Feature buffers: what the FIRST hit of every camera ray shows (bounce 0 of `ray_color`, src/main.rs:38-57).  `d_feat`: device
    /// [height][width][8] u64 exact sums (albedo rgb, normal xyz as two's complement, depth t, hits); `d_ids`: device
    /// [height][width] i32 (list index of the first sample's hit, -1 for a miss) or null.
    pub fn rt_render_features_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, d_feat: *mut c_void,
                                     d_ids: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_render_features(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, out_feat: *mut u64,
                              out_ids: *mut i32, kernel_ms: *mut f32) -> i32;
    /// ... -> f32 [rows][width][8]: mean albedo, mean normal, mean depth over the hitting samples, alpha = hits / spp.
    pub fn rt_features_to_f32_device(ctx: *mut rt_context, d_feat: *const c_void, width: i32, rows: i32, spp: i64,
                                     d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_features_to_f32(ctx: *mut rt_context, feat: *const u64, width: i32, rows: i32, spp: i64, out: *mut f32) -> i32;
    /// The denoiser: an edge-avoiding a-trous filter on the radiance sums, driven by the feature sums of the same camera; the result is a
    /// ONE-SAMPLE frame of exact sums (resolve it with spp = 1).  `d_count` / `count`: each pixel's own number of samples (the adaptive
    /// frame) or null (every pixel has `spp`).  `d_work`: `rt_denoise_workspace_bytes` bytes of device memory, the caller's.
    pub fn rt_denoise_workspace_bytes(width: i32, height: i32, out_bytes: *mut i64) -> i32;
    pub fn rt_denoise_device(ctx: *mut rt_context, d_fix: *const c_void, d_count: *const c_void, spp: i64, d_feat: *const c_void,
                             feat_spp: i64, width: i32, height: i32, dn: *const rt_denoise, d_work: *mut c_void,
                             d_out_fix: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_denoise(ctx: *mut rt_context, fix: *const u64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64,
                      width: i32, height: i32, dn: *const rt_denoise, out_fix: *mut u64, kernel_ms: *mut f32) -> i32;
    /// The same filter on host buffers, no device needed.
    pub fn rt_denoise_host(fix: *const u64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64, width: i32, height: i32,
                           dn: *const rt_denoise, out_fix: *mut u64) -> i32;
    /// The variance-guided denoiser: the same filter with its colour stop in units of the local standard deviation.  `d_half` / `half`:
    /// the sums of half of each pixel's samples (what the adaptive drivers return, or the first of two equal accumulated passes); the
    /// per-pixel variance they give travels through the levels.  `sigma_color` is in standard deviations and does not halve per level.
    /// `d_work`: `rt_denoise_var_workspace_bytes` bytes of device memory (19 doubles per pixel), the caller's.
    pub fn rt_denoise_var_workspace_bytes(width: i32, height: i32, out_bytes: *mut i64) -> i32;
    pub fn rt_denoise_var_device(ctx: *mut rt_context, d_fix: *const c_void, d_half: *const c_void, d_count: *const c_void, spp: i64,
                                 d_feat: *const c_void, feat_spp: i64, width: i32, height: i32, dn: *const rt_denoise,
                                 d_work: *mut c_void, d_out_fix: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_denoise_var(ctx: *mut rt_context, fix: *const u64, half: *const u64, count: *const u32, spp: i64, feat: *const u64,
                          feat_spp: i64, width: i32, height: i32, dn: *const rt_denoise, out_fix: *mut u64,
                          kernel_ms: *mut f32) -> i32;
    /// The same filter on host buffers, no device needed.
    pub fn rt_denoise_var_host(fix: *const u64, half: *const u64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64,
                               width: i32, height: i32, dn: *const rt_denoise, out_fix: *mut u64) -> i32;
    /// Temporal accumulation over a STATIC scene: the current frame's sums blended with the previous call's result, fetched where each
    /// pixel's first-hit point lay in the previous camera's image.  History: all four of `prev_fix`, `prev_len`, `prev_feat`, `prev_cam`
    /// or none (null: the first frame).  The cameras and the options are HOST pointers in every form.  `out_fix` is a ONE-SAMPLE frame of
    /// exact sums, `out_len` the number of frames behind each pixel; they must not overlap the history (ping-pong).
    pub fn rt_temporal_device(ctx: *mut rt_context, d_fix: *const c_void, d_count: *const c_void, spp: i64, d_feat: *const c_void,
                              feat_spp: i64, cam: *const rt_camera, d_prev_fix: *const c_void, d_prev_len: *const c_void,
                              d_prev_feat: *const c_void, prev_feat_spp: i64, prev_cam: *const rt_camera, width: i32, height: i32,
                              tp: *const rt_temporal, d_out_fix: *mut c_void, d_out_len: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_temporal(ctx: *mut rt_context, fix: *const u64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64,
                       cam: *const rt_camera, prev_fix: *const u64, prev_len: *const u32, prev_feat: *const u64, prev_feat_spp: i64,
                       prev_cam: *const rt_camera, width: i32, height: i32, tp: *const rt_temporal, out_fix: *mut u64,
                       out_len: *mut u32, kernel_ms: *mut f32) -> i32;
    /// The same accumulation on host buffers, no device needed.
    pub fn rt_temporal_host(fix: *const u64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64, cam: *const rt_camera,
                            prev_fix: *const u64, prev_len: *const u32, prev_feat: *const u64, prev_feat_spp: i64,
                            prev_cam: *const rt_camera, width: i32, height: i32, tp: *const rt_temporal, out_fix: *mut u64,
                            out_len: *mut u32) -> i32;
    /// Temporal accumulation with second moments: `rt_temporal` with `prev_m2` (`[H][W][3]` f64, the previous call's `out_m2`) as a fifth
    /// part of the history -- all five or none --, and two more outputs: `out_m2`, the accumulated mean of the squared frame means, and
    /// `out_var`, per channel the variance of the accumulated value.  `out_fix` and `out_len` are `rt_temporal`'s bits.
    pub fn rt_temporal_var_device(ctx: *mut rt_context, d_fix: *const c_void, d_count: *const c_void, spp: i64, d_feat: *const c_void,
                                  feat_spp: i64, cam: *const rt_camera, d_prev_fix: *const c_void, d_prev_len: *const c_void,
                                  d_prev_feat: *const c_void, prev_feat_spp: i64, prev_cam: *const rt_camera, d_prev_m2: *const c_void,
                                  width: i32, height: i32, tp: *const rt_temporal, d_out_fix: *mut c_void, d_out_len: *mut c_void,
                                  d_out_m2: *mut c_void, d_out_var: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_temporal_var(ctx: *mut rt_context, fix: *const u64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64,
                           cam: *const rt_camera, prev_fix: *const u64, prev_len: *const u32, prev_feat: *const u64, prev_feat_spp: i64,
                           prev_cam: *const rt_camera, prev_m2: *const f64, width: i32, height: i32, tp: *const rt_temporal,
                           out_fix: *mut u64, out_len: *mut u32, out_m2: *mut f64, out_var: *mut f64, kernel_ms: *mut f32) -> i32;
    /// The same accumulation on host buffers, no device needed.
    pub fn rt_temporal_var_host(fix: *const u64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64, cam: *const rt_camera,
                                prev_fix: *const u64, prev_len: *const u32, prev_feat: *const u64, prev_feat_spp: i64,
                                prev_cam: *const rt_camera, prev_m2: *const f64, width: i32, height: i32, tp: *const rt_temporal,
                                out_fix: *mut u64, out_len: *mut u32, out_m2: *mut f64, out_var: *mut f64) -> i32;
    /// The variance-guided denoiser with the variance given: `rt_denoise_var` with `var` (`[H][W][3]` f64, per channel the variance of the
    /// pixel's mean: `rt_temporal_var`'s `out_var`) in `half`'s place; the workspace is `rt_denoise_var_workspace_bytes`.
    pub fn rt_denoise_var_given_device(ctx: *mut rt_context, d_fix: *const c_void, d_var: *const c_void, d_count: *const c_void, spp: i64,
                                       d_feat: *const c_void, feat_spp: i64, width: i32, height: i32, dn: *const rt_denoise,
                                       d_work: *mut c_void, d_out_fix: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_denoise_var_given(ctx: *mut rt_context, fix: *const u64, var: *const f64, count: *const u32, spp: i64, feat: *const u64,
                                feat_spp: i64, width: i32, height: i32, dn: *const rt_denoise, out_fix: *mut u64,
                                kernel_ms: *mut f32) -> i32;
    /// The same filter on host buffers, no device needed.
    pub fn rt_denoise_var_given_host(fix: *const u64, var: *const f64, count: *const u32, spp: i64, feat: *const u64, feat_spp: i64,
                                     width: i32, height: i32, dn: *const rt_denoise, out_fix: *mut u64) -> i32;
    /// Ray queries: `HittableList::hit(ray, t_min, t_max[k])` of every ray of the batch against the uploaded list (closest hit), and
    /// whether it would hit at all (occlusion, `[n]` u8).  The device forms are asynchronous on `stream`; the structs are host pointers.
    pub fn rt_trace_rays_device(ctx: *mut rt_context, rays: *const rt_rays, t_min: f64, hits: *const rt_hits, stream: *mut c_void) -> i32;
    pub fn rt_trace_rays(ctx: *mut rt_context, rays: *const rt_rays, t_min: f64, hits: *const rt_hits, kernel_ms: *mut f32) -> i32;
    pub fn rt_occluded_device(ctx: *mut rt_context, rays: *const rt_rays, t_min: f64, d_occluded: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_occluded(ctx: *mut rt_context, rays: *const rt_rays, t_min: f64, occluded: *mut u8, kernel_ms: *mut f32) -> i32;
    pub fn rt_camera_rays_device(ctx: *mut rt_context, cam: *const rt_camera, width: i32, height: i32, seed: u64, flags: u32,
                                 batch: *const rt_camera_batch, stream: *mut c_void) -> i32;
    pub fn rt_camera_rays(ctx: *mut rt_context, cam: *const rt_camera, width: i32, height: i32, seed: u64, flags: u32,
                          batch: *const rt_camera_batch, kernel_ms: *mut f32) -> i32;
    pub fn rt_scatter_device(ctx: *mut rt_context, seed: u64, flags: u32, batch: *const rt_scatter_batch, stream: *mut c_void) -> i32;
    pub fn rt_scatter(ctx: *mut rt_context, seed: u64, flags: u32, batch: *const rt_scatter_batch, kernel_ms: *mut f32) -> i32;
    pub fn rt_accumulate_device(ctx: *mut rt_context, batch: *const rt_accumulate_batch, d_fix: *mut c_void, npix: i64,
                                stream: *mut c_void) -> i32;
    pub fn rt_accumulate(ctx: *mut rt_context, batch: *const rt_accumulate_batch, fix: *mut u64, npix: i64, kernel_ms: *mut f32) -> i32;
    /// The device path queue: `rt_paths_begin_device` fills slots `[0, n)` with the camera rays of the items `first_item ..` (pixel-major);
    /// `rt_paths_step_device` is one bounce of every live path of `input` -- closest hit, the sky term of a miss added to `d_fix`, scatter,
    /// throughput -- with the survivors written to `output` in order; `rt_render_wavefront*` render the whole frame from the two,
    /// `rt_render_device`'s sums bit for bit.  The device forms are asynchronous on `stream` and take no host wait.
    pub fn rt_path_scratch_words(capacity: i64) -> i64;
    pub fn rt_paths_begin_device(ctx: *mut rt_context, cam: *const rt_camera, width: i32, height: i32, seed: u64, flags: u32, spp: i32,
                                 sample_begin: i32, first_item: i64, n: i64, q: *const rt_path_queue, stream: *mut c_void) -> i32;
    pub fn rt_paths_step_device(ctx: *mut rt_context, seed: u64, flags: u32, t_min: f64, input: *const rt_path_queue,
                                output: *const rt_path_queue, d_fix: *mut c_void, npix: i64, d_rays: *mut c_void,
                                stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, d_fix: *mut c_void,
                                      d_rays: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, fix: *mut u64, rays_traced: *mut u64,
                               kernel_ms: *mut f32) -> i32;
    /// The path queue with a settable sky and emissive spheres: a miss adds the sky of `light`, a hit on a sphere whose entry of
    /// `light.emission` has a channel `> 0` adds `throughput * e` and ends the path.  With the reference's sky and no table these are the
    /// unlit forms bit for bit.
    pub fn rt_paths_step_lit_device(ctx: *mut rt_context, seed: u64, flags: u32, t_min: f64, input: *const rt_path_queue,
                                    output: *const rt_path_queue, d_fix: *mut c_void, npix: i64, d_rays: *mut c_void,
                                    light: *const rt_lighting, stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_lit_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                          d_fix: *mut c_void, d_rays: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_lit(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                   fix: *mut u64, rays_traced: *mut u64, kernel_ms: *mut f32) -> i32;
    /// Direct lighting (next-event estimation) in the lit path queue: at a Lambertian hit one light of `direct` is sampled by area and
    /// a shadow ray decides whether it adds; the same expectation as the lit forms.  `rt_light_list` is a pure host function.
    pub fn rt_light_list(emission: *const f64, n_emission: i32, lights_out: *mut i32, n_lights_out: *mut i32) -> i32;
    pub fn rt_paths_step_nee_device(ctx: *mut rt_context, seed: u64, flags: u32, t_min: f64, input: *const rt_path_queue,
                                    output: *const rt_path_queue, d_fix: *mut c_void, npix: i64, d_rays: *mut c_void,
                                    light: *const rt_lighting, direct: *const rt_direct, step_flags: u32, d_shadow_rays: *mut c_void,
                                    stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_nee_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                          direct: *const rt_direct, d_fix: *mut c_void, d_rays: *mut c_void, d_shadow_rays: *mut c_void,
                                          stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_nee(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                   fix: *mut u64, rays_traced: *mut u64, shadow_rays: *mut u64, kernel_ms: *mut f32) -> i32;
    pub fn rt_render_wavefront_nee_sampled(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                           direct_flags: u32, fix: *mut u64, rays_traced: *mut u64, shadow_rays: *mut u64,
                                           kernel_ms: *mut f32) -> i32;
    /// Wavefront frames over pixel lists (frame-addressed sums, RT_FLAG_ACCUMULATE) and the adaptive loop over them.
    pub fn rt_paths_begin_pixels_device(ctx: *mut rt_context, cam: *const rt_camera, width: i32, height: i32, seed: u64, flags: u32,
                                        spp: i32, sample_begin: i32, first_item: i64, n: i64, d_pixels: *const u32, n_pixels: i64,
                                        q: *const rt_path_queue, stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_pixels_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                             direct: *const rt_direct, d_pixels: *const u32, n_pixels: i64, d_fix: *mut c_void,
                                             d_rays: *mut c_void, d_shadow_rays: *mut c_void, stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_pixels(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                      direct: i32, direct_flags: u32, pixels: *const u32, n_pixels: i64, fix: *mut u64,
                                      rays_traced: *mut u64, shadow_rays: *mut u64, kernel_ms: *mut f32) -> i32;
    pub fn rt_render_wavefront_adaptive(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, a: *const rt_adaptive,
                                        light: *const rt_lighting, direct: i32, direct_flags: u32, out_fix: *mut u64, out_half: *mut u64,
                                        out_count: *mut u32, rays_traced: *mut u64, shadow_rays: *mut u64, kernel_ms: *mut f32) -> i32;
    /// An environment cube map in the place of the sky: looked up on a miss, importance-sampled at Lambertian hits by the running sums
    /// `rt_environment_cdf` (a pure host function) builds; the shadow ray is visible iff it meets no sphere.
    pub fn rt_environment_cdf(texels: *const f64, size: i32, cdf_out: *mut f64) -> i32;
    pub fn rt_paths_step_env_device(ctx: *mut rt_context, seed: u64, flags: u32, t_min: f64, input: *const rt_path_queue,
                                    output: *const rt_path_queue, d_fix: *mut c_void, npix: i64, d_rays: *mut c_void,
                                    light: *const rt_lighting, env: *const rt_environment, step_flags: u32, d_shadow_rays: *mut c_void,
                                    stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_env_device(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                          env: *const rt_environment, d_fix: *mut c_void, d_rays: *mut c_void, d_shadow_rays: *mut c_void,
                                          stream: *mut c_void) -> i32;
    pub fn rt_render_wavefront_env(ctx: *mut rt_context, cam: *const rt_camera, p: *const rt_params, light: *const rt_lighting,
                                   env: *const rt_environment, sample: i32, fix: *mut u64, rays_traced: *mut u64, shadow_rays: *mut u64,
                                   kernel_ms: *mut f32) -> i32;
    pub fn rt_last_error() -> *const c_char;
    pub fn rt_backend_name() -> *const c_char;
    pub fn rt_abi_version() -> i32;
    pub fn rt_build_source_sha() -> *const c_char;
    pub fn rt_f64_div_sqrt_device(ctx: *mut rt_context, a: *const f64, b: *const f64, n: i32,
                                  out_div: *mut f64, out_sqrt: *mut f64) -> i32;
    pub fn rt_quantize_device(ctx: *mut rt_context, x: *const f64, n: i32, out: *mut u64) -> i32;
    pub fn rt_unit_accept_device(ctx: *mut rt_context, words: *const u32, n: i32, out_accept: *mut u32,
                                 out_uniforms: *mut f64) -> i32;
    pub fn rt_filter_tube_device(ctx: *mut rt_context, o: *const f64, d: *const f64, spheres32: *const rt_sphere,
                                 out_h: *mut f32, out_rows: *mut f32, out_bound: *mut f32, out_rho: *mut f32) -> i32;
    pub fn rt_tube_tile_host(spheres32: *const rt_sphere, out_words: *mut u32, out_bound: *mut f32,
                             out_rho: *mut f32) -> i32;
    pub fn rt_tile_layout_host(spheres: *const rt_sphere, n: i32, out_dims: *mut i32, out_grid: *mut f32,
                               out_slot_of: *mut i32, cap: i32) -> i32;
    pub fn rt_philox_device(ctx: *mut rt_context, ctr: *const u32, key: *const u32, out: *mut u32) -> i32;
}
