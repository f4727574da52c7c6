// rtiow_render -- the reference's main() (src/main.rs:104-177) on the GPU path: build the scene,
// build the camera, render through the C ABI, flip + to_rgba, save the image (main.rs:177 `image_buffer.save("image.png")`:
// an RGBA8 PNG when --out ends in .png, else the same bytes without alpha as a P6 PPM; no preview window).
//
//   rtiow_render [--width W] [--height H] [--spp N] [--depth D] [--seed S] [--scene-seed S]
//                [--grid LO HI] [--device K] [--out image.png|image.ppm] [--dump-scene scene.bin] [--scene scene.bin]
//                [--devices 0,1,..  [--tile-rows T] [--force-rccl]] [--uniform53] [--two-calls] [--passes N]
//                [--adaptive THRESHOLD [--step N]]
//                [--cameras cams.bin | --orbit N  [--sample-stride S]] [--dump-cameras cams.bin] [--features features.npy]
//                [--denoise [--feature-spp N] [--denoise-levels L] [--sigma-color X] [--sigma-normal X] [--sigma-depth X]]
//                [--denoise-variance [--feature-spp N] [--denoise-levels L] [--sigma-color X] [--sigma-normal X] [--sigma-depth X]]
//                [--temporal [--alpha-min X] [--temporal-sigma-normal X] [--temporal-sigma-depth X] [--temporal-clamp X]]
//                [--pick I,J] [--wavefront [--sky B_r,B_g,B_b:T_r,T_g,T_b] [--emit INDEX:r,g,b]... [--direct | --direct-cone | --direct-weighted]
//                 [--env FILE [--env-sample]]]
//   rtiow_render --reassembly-plan H T N     (no GPU: the strided copies that put N shards' rows back in image order)
//   rtiow_render --test-png W H out.png      (no GPU: a fixed pattern through the PNG writer -- r = 7x + 13y, g = x ^ y, b = x y, mod 256, alpha 255)
//
// Single device: ONE call, rt_render_rgba8 (the sums stay on the device); --two-calls takes them through host memory
// instead (rt_render, then rt_resolve_rgba8): the same bytes.
// --passes N: main.rs:130-137's sample loop as N additive launches (sample_begin, RT_FLAG_ACCUMULATE | RT_FLAG_OVERLAPPED) issued alternately on TWO streams of one
// context, so that pass k + 1 fills the end-of-launch tail of pass k (a context holds two launches' state); the sums are exact integers, so the
// image is the one the single call gives, byte for byte.
// --adaptive THRESHOLD [--step N, default 8]: main.rs:130-137 with a per-pixel number of samples (rt_render_adaptive: passes of N samples, a pixel
// stops once its error estimate is <= THRESHOLD; --spp is the most a pixel may get, a multiple of 2 N) and Color::to_rgba with each pixel's own
// count (rt_resolve_rgba8_counts); the summary line adds the mean / min / max samples per pixel.  Single device.
// --cameras FILE (raw 152-byte rt_camera records, as --dump-cameras and rtiow_amd.save_cameras write them) or --orbit N (a turntable of N
// cameras about the y axis, frame 0 = the book camera): a FRAME BATCH -- every camera in ONE launch (rt_render_frames_rgba8: main.rs:108-145
// once per camera; the sums stay on the device) -- written as PREFIX_0000.png, PREFIX_0001.png, ... for --out PREFIX (.ppm if PREFIX ends in
// .ppm; a trailing .png is dropped from the prefix).  Frame f renders the samples [f S, f S + spp), S = --sample-stride (default: spp, every
// frame its own random numbers; 0: the same ones for all).  Single device, one call.
// --features FILE: next to the image, the first-hit feature buffers of the same frame and samples (rt_render_features, then rt_features_to_f32:
// mean albedo rgb, mean normal xyz, mean depth t over the hitting samples, alpha = hits / spp) as a NumPy .npy file: a 128-byte header and the
// f32 [H][W][8] array, rows as the ABI has them (j = 0, the BOTTOM row, first), little-endian.  Single device; not with --uniform53, and
// not with --adaptive (whose image gives every pixel its own number of samples: the features would not be those samples').
// --denoise: renders the frame's exact sums (rt_render, or rt_render_adaptive with --adaptive), renders the first-hit features of the same camera
// with --feature-spp N samples (default 8; rt_render_features), filters (rt_denoise: --denoise-levels, default 4, and the three sigmas, defaults
// 0.35 / 1.0 / 0.2, demodulated; with --adaptive the count buffer goes in, every pixel divided by its own number of samples), resolves the
// one-sample result (rt_resolve_rgba8 with spp = 1) and saves that.  Single device; not with --uniform53, --passes, --two-calls, --features.
// --temporal (with --cameras / --orbit): the frames of the batch accumulated over time (rt_temporal).  The batch's exact sums
// (rt_render_frames, one launch), per frame the first-hit features of its camera with --feature-spp N samples starting at the frame's own
// sample_begin (rt_render_features), rt_temporal chained over the frames with two pairs of history buffers used in turn (--alpha-min, default 0.1;
// --temporal-sigma-normal 0.5; --temporal-sigma-depth 0.1; --temporal-clamp X: the scale of the neighbourhood clamp, default 1, a negative X switches
// it off), with --denoise also rt_denoise on each accumulated frame (spp = 1, the frame's own features), then the one-sample resolve; the
// frames are written as the batch writes them.  --denoise goes with a batch only together with --temporal.
// --temporal --denoise-variance (with --cameras / --orbit): the same sequence with second moments: rt_temporal_var in
// rt_temporal's place, with a fifth history buffer, and on each accumulated frame rt_denoise_var_given with the variance that call returned
// (spp = 1; --sigma-color in standard deviations, default 1.5 here: the sweep of section 26).  No half sums are needed, so --spp may be odd.  With --wavefront and its --sky,
// --emit and --direct* switches every frame is rendered through the device path queue (frame f with sample_begin = f S) instead of by the
// batch launch.  --denoise-variance goes with a batch only together with --temporal.
// --wavefront: the same frame through the device path queue (rt_render_wavefront: per batch one begin and --depth fused bounce steps, DESIGN.md
// section 19), then rt_resolve_rgba8: the bytes of the default run.  Single device; with none of the other modes.
// --sky B_r,B_g,B_b:T_r,T_g,T_b and --emit INDEX:r,g,b (repeatable), both only with --wavefront: the frame lit by a settable sky -- colour B
// where the unit ray direction's y is -1, T where it is +1; the reference's is 1,1,1:0.5,0.7,1 -- and by emissive spheres -- sphere INDEX of
// the scene's list radiates (r, g, b), a path that reaches it adds throughput * (r, g, b) and ends -- (rt_render_wavefront_lit, DESIGN.md
// section 20).  --sky 0,0,0:0,0,0 --emit 0:4,3.2,2.4 is a night frame lit by one sphere.
// --direct, only with --wavefront and at least one --emit: next-event estimation -- at every Lambertian hit a shadow ray towards a point of
// one emissive sphere, so that small lights are found at sample counts where the random walk alone hits them almost never; the same
// expectation as without it (rt_render_wavefront_nee).  The number of shadow rays goes to stderr.
// --direct-cone: --direct with the light sampled by solid angle -- a uniform direction of the cone the sphere subtends -- instead of by area:
// a bounded weight however close the light, no sample lost on its far side, two to three times the shadow rays
// (rt_render_wavefront_nee_sampled with RT_DIRECT_CONE).  The rules of --direct; not together with it.
// --direct-weighted: --direct-cone with the light chosen by what it can contribute at the hit point -- (r^2 / d^2) max(e) -- instead of
// uniformly: what a frame lit by many small lights needs (RT_DIRECT_WEIGHTED | RT_DIRECT_CONE).  The rules of
// --direct; not together with either of the other two.
// --env FILE: an environment cube map in the place of the sky (rt_render_wavefront_env): raw little-endian f64
// [6][N][N][3], N -- a power of two -- from the byte count; --env-sample: Lambertian hits importance-sample it with a shadow ray.  Needs
// --wavefront; --emit still lights; not together with --direct*.  (The single frame and the --temporal --denoise-variance sequence.)
// --wavefront ... --adaptive THRESHOLD [--step N]: the adaptive loop over the device path queue's frame (rt_render_wavefront_adaptive, DESIGN.md
// section 24), with --sky, --emit and --direct* as without it; the resolve and the summary line are --adaptive's.  Not with --denoise.
// --denoise-variance: the variance-guided denoiser (rt_denoise_var) with --denoise's option switches; --sigma-color is then
// in standard deviations of the pixel's own noise (default 1) and does not halve per level.  The filter needs the sums of HALF of each
// pixel's samples: without --adaptive the frame is rendered as two passes of spp / 2 (an odd --spp exits 2) -- pass 1 is kept as `half`, pass 2
// renders the samples from sample_begin = spp / 2 on top of it, which gives the sums of one pass --; with --adaptive the loop's own half
// and count buffers go in.  Legal with --wavefront, --sky, --emit, --direct* and --adaptive included (rt_render_wavefront_pixels with
// RT_FLAG_ACCUMULATE, rt_render_wavefront_adaptive); then rt_render_features, rt_denoise_var and the one-sample resolve.  Not together with
// --denoise; --wavefront --denoise stays refused.  Single device; not with --uniform53, --passes, --two-calls, --features; with --cameras or
// --orbit only together with --temporal (above).
// --pick I,J: no image; what the book camera's pixel (I, J) (J = 0 the BOTTOM row) of a --width x --height frame shows: the ray through the pixel's
// centre and the lens centre -- u = (I + 0.5) / (W - 1), v = (J + 0.5) / (H - 1), direction ((lower_left_corner + u horizontal) + v vertical) - origin --
// in ONE call of rt_trace_rays, printed as "pick I J: index K kind NAME t T point X Y Z" (%.17g; a miss: index -1 kind none t inf).  Single device.
// --devices: the frame's rows are dealt round-robin to one rt_context per listed device, each driven by
// its own host thread, and gathered with ONE RCCL ncclGather to the first device (host/rtiow_multi.hpp).
// A device may be listed more than once (two contexts on one GPU from two threads: the threading rule of
// include/rtiow_hip.h); RCCL does not allow that within a communicator, so such a list gathers with plain
// device copies.  --force-rccl runs the RCCL path even for a single device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rtiow_host.hpp"
#include "rtiow_multi.hpp"

static int die(const char *what, int rc)
{
    std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, rt_last_error());
    return 1;
}

// a NumPy .npy file (format version 1.0) of a little-endian f32 [h][w][c] array: the magic, the version, the header's length (118:
// the whole preamble is 128 bytes), the dict padded with spaces up to a closing newline, then the raw floats
static bool write_npy_f32(const char *path, const float *data, int h, int w, int c)
{
    char head[128];
    std::memset(head, ' ', sizeof(head));
    std::memcpy(head, "\x93NUMPY\x01\x00\x76\x00", 10);
    char dict[118];
    const int n = std::snprintf(dict, sizeof(dict), "{'descr': '<f4', 'fortran_order': False, 'shape': (%d, %d, %d), }", h, w, c);
    if (n < 0 || n >= (int)sizeof(dict)) return false;
    std::memcpy(head + 10, dict, (size_t)n);
    head[127] = '\n';
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t count = (size_t)h * w * c;
    const bool ok = std::fwrite(head, 1, sizeof(head), f) == sizeof(head) && std::fwrite(data, sizeof(float), count, f) == count;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    int width = 400, height = 225, spp = 10, depth = 50, device = 0, lo = -11, hi = 11;
    unsigned long long seed = 1, scene_seed = 1;
    std::string out = "image.ppm", dump, scene_file;
    std::vector<int> devices;                    // --devices 0,1,...: one context + host thread per entry
    bool force_rccl = false, uniform53 = false, two_calls = false, wavefront = false;
    int passes = 1;
    int tile_rows = 1;
    bool adaptive = false;
    double threshold = 0.0;
    int step = 8;
    std::string cameras_file, dump_cameras, features_file;
    int orbit = 0, sample_stride = -1;           // (-1: spp)
    bool denoise = false;
    bool denoise_var = false, sigma_color_set = false;      // --denoise-variance: --sigma-color is in standard deviations, default 1
    int feature_spp = 8;
    struct rt_denoise dn{};
    dn.levels = 4; dn.flags = RT_DENOISE_DEMODULATE; dn.sigma_color = 0.35; dn.sigma_normal = 1.0; dn.sigma_depth = 0.2;
    bool pick = false;
    int pick_i = 0, pick_j = 0;
    bool lit = false;                            // --sky / --emit: the lit wavefront frame
    bool direct_cone = false;                    // --direct-cone: ... sampled by solid angle instead of by area
    bool direct_weighted = false;                // --direct-weighted: ... and chosen by their contribution at the hit point
    bool direct = false;                         // --direct: ... with shadow rays towards the lights (next-event estimation)
    std::string env_file;                        // --env FILE: an environment cube map (raw little-endian f64 [6][N][N][3]) in the place of the sky
    bool env_sample = false;                     // --env-sample: ... importance-sampled at Lambertian hits
    std::vector<double> env_texels;
    rt_environment env{};
    rt_lighting light{};
    light.sky_bottom[0] = light.sky_bottom[1] = light.sky_bottom[2] = 1.0;
    light.sky_top[0] = 0.5; light.sky_top[1] = 0.7; light.sky_top[2] = 1.0;
    struct Emit { long index; double rgb[3]; };
    std::vector<Emit> emits;
    bool temporal = false;
    struct rt_temporal tp{};
    tp.flags = RT_TEMPORAL_CLAMP; tp.alpha_min = 0.1; tp.sigma_normal = 0.5; tp.sigma_depth = 0.1; tp.clamp_scale = 1.0;
    if (argc == 5 && !std::strcmp(argv[1], "--reassembly-plan")) {
        const int H = std::atoi(argv[2]), T = std::atoi(argv[3]), n = std::atoi(argv[4]);
        if (H < 1 || T < 1 || n < 1) { std::fprintf(stderr, "--reassembly-plan H T N: all >= 1\n"); return 2; }
        for (int k = 0; k < n; ++k)
            for (const rtiow::RowCopy &c : rtiow::reassembly_plan(H, T, n, k))
                std::printf("%d %d %d %d %d %d %d\n", k, c.dst_row, c.src_row, c.rows, c.pieces, c.dst_pitch_rows, c.src_pitch_rows);
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "--test-png")) {
        const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
        if (W < 1 || H < 1) { std::fprintf(stderr, "--test-png W H out.png: W, H >= 1\n"); return 2; }
        std::vector<unsigned char> px((size_t)W * H * 4);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                unsigned char *q = &px[((size_t)y * W + x) * 4];
                q[0] = (unsigned char)(7 * x + 13 * y); q[1] = (unsigned char)(x ^ y); q[2] = (unsigned char)(x * y); q[3] = 255;
            }
        if (!rtiow::write_png(argv[4], px.data(), W, H)) { std::perror(argv[4]); return 1; }
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        auto arg = [&](const char *n) { return !std::strcmp(argv[i], n) && i + 1 < argc; };
        if (arg("--width")) width = std::atoi(argv[++i]);
        else if (arg("--height")) height = std::atoi(argv[++i]);
        else if (arg("--spp")) spp = std::atoi(argv[++i]);
        else if (arg("--depth")) depth = std::atoi(argv[++i]);
        else if (arg("--seed")) seed = std::strtoull(argv[++i], nullptr, 0);
        else if (arg("--scene-seed")) scene_seed = std::strtoull(argv[++i], nullptr, 0);
        else if (arg("--device")) device = std::atoi(argv[++i]);
        else if (arg("--out")) out = argv[++i];
        else if (arg("--devices")) { for (char *t = std::strtok(argv[++i], ","); t; t = std::strtok(nullptr, ",")) devices.push_back(std::atoi(t)); }
        else if (arg("--tile-rows")) tile_rows = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--force-rccl")) force_rccl = true;
        else if (!std::strcmp(argv[i], "--uniform53")) uniform53 = true;
        else if (!std::strcmp(argv[i], "--two-calls")) two_calls = true;
        else if (!std::strcmp(argv[i], "--wavefront")) wavefront = true;
        else if (!std::strcmp(argv[i], "--direct")) direct = true;
        else if (!std::strcmp(argv[i], "--direct-cone")) direct_cone = true;
        else if (!std::strcmp(argv[i], "--direct-weighted")) direct_weighted = true;
        else if (arg("--passes")) passes = std::atoi(argv[++i]);
        else if (arg("--adaptive")) { adaptive = true; threshold = std::atof(argv[++i]); }
        else if (arg("--step")) step = std::atoi(argv[++i]);
        else if (arg("--dump-scene")) dump = argv[++i];
        else if (arg("--cameras")) cameras_file = argv[++i];
        else if (arg("--orbit")) orbit = std::atoi(argv[++i]);
        else if (arg("--sample-stride")) sample_stride = std::atoi(argv[++i]);
        else if (arg("--dump-cameras")) dump_cameras = argv[++i];
        else if (arg("--features")) features_file = argv[++i];
        else if (!std::strcmp(argv[i], "--denoise")) denoise = true;
        else if (!std::strcmp(argv[i], "--denoise-variance")) denoise_var = true;
        else if (arg("--feature-spp")) feature_spp = std::atoi(argv[++i]);
        else if (arg("--denoise-levels")) dn.levels = std::atoi(argv[++i]);
        else if (arg("--sigma-color")) { dn.sigma_color = std::atof(argv[++i]); sigma_color_set = true; }
        else if (arg("--sigma-normal")) dn.sigma_normal = std::atof(argv[++i]);
        else if (arg("--sigma-depth")) dn.sigma_depth = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--temporal")) temporal = true;
        else if (arg("--alpha-min")) tp.alpha_min = std::atof(argv[++i]);
        else if (arg("--temporal-sigma-normal")) tp.sigma_normal = std::atof(argv[++i]);
        else if (arg("--temporal-sigma-depth")) tp.sigma_depth = std::atof(argv[++i]);
        else if (arg("--temporal-clamp")) {
            tp.clamp_scale = std::atof(argv[++i]);
            if (tp.clamp_scale < 0.0) { tp.flags = 0u; tp.clamp_scale = 1.0; }
        }
        else if (arg("--sky")) {
            double *b = light.sky_bottom, *t = light.sky_top;
            char tail = 0;
            if (std::sscanf(argv[++i], "%lf,%lf,%lf:%lf,%lf,%lf%c", &b[0], &b[1], &b[2], &t[0], &t[1], &t[2], &tail) != 6) {
                std::fprintf(stderr, "--sky B_r,B_g,B_b:T_r,T_g,T_b\n");
                return 2;
            }
            lit = true;
        }
        else if (arg("--emit")) {
            Emit e{};
            char tail = 0;
            if (std::sscanf(argv[++i], "%ld:%lf,%lf,%lf%c", &e.index, &e.rgb[0], &e.rgb[1], &e.rgb[2], &tail) != 4) {
                std::fprintf(stderr, "--emit INDEX:r,g,b\n");
                return 2;
            }
            emits.push_back(e);
            lit = true;
        }
        else if (arg("--env")) env_file = argv[++i];
        else if (!std::strcmp(argv[i], "--env-sample")) env_sample = true;
        else if (arg("--scene")) scene_file = argv[++i];
        else if (arg("--pick")) {
            if (std::sscanf(argv[++i], "%d,%d", &pick_i, &pick_j) != 2) { std::fprintf(stderr, "--pick I,J\n"); return 2; }
            pick = true;
        }
        else if (!std::strcmp(argv[i], "--grid") && i + 2 < argc) { lo = std::atoi(argv[++i]); hi = std::atoi(argv[++i]); }
        else { std::fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
    }
    const rtiow::HittableList world = rtiow::random_scene(scene_seed, lo, hi);      // main.rs:106
    std::vector<rt_sphere> flat = world.flatten();
    if (!scene_file.empty()) {                   // a flat scene file instead of random_scene()
        FILE *f = std::fopen(scene_file.c_str(), "rb");
        if (!f) { std::perror(scene_file.c_str()); return 1; }
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        if (bytes < 0 || bytes % (long)sizeof(rt_sphere)) { std::fprintf(stderr, "%s: not a whole number of 72-byte records\n", scene_file.c_str()); return 1; }
        flat.resize((size_t)bytes / sizeof(rt_sphere));
        if (std::fread(flat.data(), sizeof(rt_sphere), flat.size(), f) != flat.size()) { std::perror(scene_file.c_str()); return 1; }
        std::fclose(f);
    }
    if (!dump.empty()) {                         // the flat scene file: count + 72-byte records
        FILE *f = std::fopen(dump.c_str(), "wb");
        if (!f) { std::perror(dump.c_str()); return 1; }
        std::fwrite(flat.data(), sizeof(rt_sphere), flat.size(), f);
        std::fclose(f);
        std::printf("%zu spheres -> %s\n", flat.size(), dump.c_str());
        return 0;
    }
    const bool batch = !cameras_file.empty() || orbit != 0;
    if (pick) {
        if (batch || !devices.empty() || width < 2 || height < 2 || pick_i < 0 || pick_i >= width || pick_j < 0 || pick_j >= height) {
            std::fprintf(stderr, "--pick I,J: a pixel of the --width x --height frame (both >= 2) of the book camera, on one device\n");
            return 2;
        }
        const rt_camera c = rtiow::Camera(rtiow::Point3(13, 2, 3), rtiow::Point3(0, 0, 0), rtiow::Vec3(0, 1, 0), 20.0,
                                          (double)width / (double)height, 0.1, 10.0).flat();      // main.rs:108-118
        const double u = ((double)pick_i + 0.5) / (double)(width - 1), v = ((double)pick_j + 0.5) / (double)(height - 1);
        double o[3], d[3], t = 0.0, point[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; ++k) {
            o[k] = c.origin[k];
            d[k] = ((c.lower_left_corner[k] + u * c.horizontal[k]) + v * c.vertical[k]) - c.origin[k];
        }
        int32_t index = -1;
        rt_rays rays{};
        rays.origin = o; rays.dir = d; rays.t_max = nullptr; rays.n = 1;
        rt_hits hits{};
        hits.index = &index; hits.t = &t; hits.point = point;
        rt_context *ctx = nullptr;
        int rc = rt_create(device, &ctx);
        if (rc) return die("rt_create", rc);
        rc = rt_upload_scene(ctx, flat.data(), (int32_t)flat.size());
        if (!rc) rc = rt_trace_rays(ctx, &rays, 0.0001, &hits, nullptr);
        if (rc) { die("rt_trace_rays", rc); rt_destroy(ctx); return 1; }
        rt_destroy(ctx);
        static const char *const kinds[] = {"lambertian", "metal", "dialectric"};
        const int kind = index >= 0 ? flat[(size_t)index].kind : -1;
        std::printf("pick %d %d: index %d kind %s t %.17g point %.17g %.17g %.17g\n", pick_i, pick_j, index,
                    kind >= 0 && kind < 3 ? kinds[kind] : "none", t, point[0], point[1], point[2]);
        return 0;
    }
    if (!features_file.empty() && (!devices.empty() || !cameras_file.empty() || orbit != 0 || uniform53 || adaptive)) {
        std::fprintf(stderr, "--features renders on one device and goes with none of --devices, --cameras, --orbit, --uniform53, --adaptive\n");
        return 2;
    }
    if (temporal && (!batch || !devices.empty() || passes > 1 || adaptive || uniform53 || two_calls)) {
        std::fprintf(stderr, "--temporal accumulates a frame batch (--cameras / --orbit) on one device and goes with none of --devices, --passes, --adaptive, --uniform53, --two-calls\n");
        return 2;
    }
    if (denoise_var && denoise) {
        std::fprintf(stderr, "--denoise and --denoise-variance are two filters for the same frame: give one of them\n");
        return 2;
    }
    if (denoise_var && (!devices.empty() || (batch && !temporal) || uniform53 || passes > 1 || two_calls || !features_file.empty())) {
        std::fprintf(stderr, "--denoise-variance renders on one device and goes with none of --devices, --cameras, --orbit, --temporal, --uniform53, --passes, --two-calls, --features\n");
        return 2;
    }
    if (denoise_var && !temporal && !adaptive && (spp < 2 || spp % 2 != 0)) {
        std::fprintf(stderr, "--denoise-variance renders the frame as two passes of spp / 2: --spp must be even and >= 2 (is %d)\n", spp);
        return 2;
    }
    if (denoise_var && !sigma_color_set) dn.sigma_color = temporal ? 1.5 : 1.0;      // (the sweeps of DESIGN.md sections 25 and 26)
    if (denoise && (!devices.empty() || (batch && !temporal) || uniform53 || passes > 1 || two_calls || !features_file.empty())) {
        std::fprintf(stderr, "--denoise renders on one device and goes with none of --devices, --cameras, --orbit, --uniform53, --passes, --two-calls, --features\n");
        return 2;
    }
    if (batch && (!devices.empty() || passes > 1 || adaptive || uniform53 || two_calls || (wavefront && !(temporal && denoise_var)))) {
        std::fprintf(stderr, "--cameras / --orbit render a frame batch on one device and go with none of --devices, --passes, --adaptive, --uniform53, --two-calls, --wavefront\n");
        return 2;
    }
    if (!cameras_file.empty() && orbit != 0) { std::fprintf(stderr, "--cameras and --orbit: one or the other\n"); return 2; }
    if (orbit < 0) { std::fprintf(stderr, "--orbit N: N >= 1\n"); return 2; }
    if (!dump_cameras.empty()) {                 // the camera file: 152-byte records (the --orbit turntable, or the book camera alone)
        const std::vector<rt_camera> cams = rtiow::orbit_cameras(orbit > 0 ? orbit : 1, width, height);
        if (!rtiow::save_cameras(dump_cameras.c_str(), cams)) { std::perror(dump_cameras.c_str()); return 1; }
        std::printf("%zu cameras -> %s\n", cams.size(), dump_cameras.c_str());
        return 0;
    }
    // what --wavefront's lighting switches must obey, and the emission table they make: asked by the single frame and by the sequence
    // that renders its frames through the path queue.  0, or the exit code
    std::vector<double> emission;                // --emit: one (r, g, b) per sphere of the list
    auto check_lighting = [&]() -> int {
        if (lit && !wavefront) {
            std::fprintf(stderr, "--sky and --emit light the frame of the device path queue only: they need --wavefront\n");
            return 2;
        }
        if (direct && (!wavefront || emits.empty())) {
            std::fprintf(stderr, "--direct samples the lights of the device path queue's frame: it needs --wavefront and at least one --emit\n");
            return 2;
        }
        if (direct_cone && direct) {
            std::fprintf(stderr, "--direct and --direct-cone are two ways to sample the same lights: give one of them\n");
            return 2;
        }
        if (direct_weighted && (direct || direct_cone)) {
            std::fprintf(stderr, "--direct, --direct-cone and --direct-weighted are three ways to sample the same lights: give one of them\n");
            return 2;
        }
        if (direct_weighted && (!wavefront || emits.empty())) {
            std::fprintf(stderr, "--direct-weighted samples the lights of the device path queue's frame: it needs --wavefront and at least one --emit\n");
            return 2;
        }
        if (direct_cone && (!wavefront || emits.empty())) {
            std::fprintf(stderr, "--direct-cone samples the lights of the device path queue's frame: it needs --wavefront and at least one --emit\n");
            return 2;
        }
        if (env_sample && env_file.empty()) {
            std::fprintf(stderr, "--env-sample samples the map of --env FILE: it needs --env\n");
            return 2;
        }
        if (!env_file.empty() && (!wavefront || direct || direct_cone || direct_weighted)) {
            std::fprintf(stderr, "--env lights the frame of the device path queue: it needs --wavefront and does not combine with --direct, "
                         "--direct-cone or --direct-weighted\n");
            return 2;
        }
        if (!env_file.empty()) {                 // the size follows from the byte count: 6 * N * N * 3 doubles
            FILE *f = std::fopen(env_file.c_str(), "rb");
            if (!f) { std::perror(env_file.c_str()); return 1; }
            double buf[4096];
            size_t got;
            while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) env_texels.insert(env_texels.end(), buf, buf + got);
            std::fclose(f);
            int32_t n = 1;
            while ((size_t)18 * n * n < env_texels.size() && n < RT_ENV_MAX_SIZE) n *= 2;
            if (env_texels.empty() || (size_t)18 * n * n != env_texels.size()) {
                std::fprintf(stderr, "%s: %zu doubles are not 6 * N * N * 3 with N a power of two up to %d\n", env_file.c_str(), env_texels.size(),
                             RT_ENV_MAX_SIZE);
                return 1;
            }
            env.texels = env_texels.data(); env.cdf = nullptr; env.size = n; env.flags = 0u;
        }
        if (!emits.empty()) {
            emission.assign(flat.size() * 3, 0.0);
            for (const Emit &e : emits) {
                if (e.index < 0 || (size_t)e.index >= flat.size()) {
                    std::fprintf(stderr, "--emit %ld: the scene has %zu spheres\n", e.index, flat.size());
                    return 2;
                }
                for (int c = 0; c < 3; ++c) emission[(size_t)e.index * 3 + c] = e.rgb[c];
            }
            light.emission = emission.data(); light.n_emission = (int32_t)flat.size();
        }
        return 0;
    };
    const bool any_direct = direct || direct_cone || direct_weighted;
    const uint32_t direct_flags = direct_weighted ? (RT_DIRECT_WEIGHTED | RT_DIRECT_CONE) : direct_cone ? RT_DIRECT_CONE : 0u;
    // one frame through the device path queue, lit and sampled as the switches say
    auto render_wavefront_frame = [&](rt_context *ctx, const rt_camera *cam, const rt_params *q, uint64_t *fix, uint64_t *rays, float *ms) -> int {
        int rc = RT_OK;
        uint64_t shadow = 0;
        if (!env_file.empty()) {
            if ((rc = rt_render_wavefront_env(ctx, cam, q, &light, &env, env_sample ? 1 : 0, fix, rays, &shadow, ms)))
                return die("rt_render_wavefront_env", rc);
            if (env_sample) std::fprintf(stderr, "shadow rays: %llu\n", (unsigned long long)shadow);
        } else if (direct) {
            if ((rc = rt_render_wavefront_nee(ctx, cam, q, &light, fix, rays, &shadow, ms))) return die("rt_render_wavefront_nee", rc);
        } else if (direct_cone || direct_weighted) {
            if ((rc = rt_render_wavefront_nee_sampled(ctx, cam, q, &light, direct_flags, fix, rays, &shadow, ms)))
                return die("rt_render_wavefront_nee_sampled", rc);
        } else if (lit) {
            if ((rc = rt_render_wavefront_lit(ctx, cam, q, &light, fix, rays, ms))) return die("rt_render_wavefront_lit", rc);
        } else if ((rc = rt_render_wavefront(ctx, cam, q, fix, rays, ms))) {
            return die("rt_render_wavefront", rc);
        }
        if (any_direct) std::fprintf(stderr, "shadow rays: %llu\n", (unsigned long long)shadow);
        return 0;
    };
    if (batch) {
        if (temporal && denoise_var)             // (the one batch that may render through the path queue: its lighting switches are held to their rules)
            if (const int bad = check_lighting()) return bad;
        std::vector<rt_camera> cams;
        if (orbit > 0) cams = rtiow::orbit_cameras(orbit, width, height);
        else if (!rtiow::load_cameras(cameras_file.c_str(), cams) || cams.empty()) {
            std::fprintf(stderr, "%s: cannot read a whole number (>= 1) of 152-byte camera records\n", cameras_file.c_str());
            return 1;
        }
        rt_params p{};
        p.width = width; p.height = height; p.spp = spp; p.sample_begin = 0; p.max_depth = depth;
        p.t_min = 0.0001; p.seed = seed; p.tile_rows = 8; p.shard_index = 0; p.shard_count = 1; p.flags = 0u;
        const int stride = sample_stride < 0 ? spp : sample_stride;
        const size_t npix = (size_t)width * height;
        std::vector<uint8_t> rgba(npix * 4 * cams.size());
        rt_stats st{};
        rt_context *ctx = nullptr;
        int rc = rt_create(device, &ctx);
        if (rc) return die("rt_create", rc);
        rc = rt_upload_scene(ctx, flat.data(), (int32_t)flat.size());
        if (rc) { die("rt_upload_scene", rc); rt_destroy(ctx); return 1; }
        if (temporal) {
            // the batch's exact sums in one launch; then frame after frame: the guides of the frame's own camera rays, the accumulation over the
            // previous call's result (two pairs of history buffers, used in turn), optionally the spatial filter, the one-sample resolve
            // --denoise-variance: the second moment rides along (a fifth history buffer) and the filter takes the variance the accumulation
            // returns; --wavefront: every frame through the path queue, one after the other, instead of the batch launch
            std::vector<uint64_t> fix(npix * 3 * (wavefront ? 1 : cams.size())), feat[2], acc[2], clean;
            std::vector<uint32_t> len[2];
            std::vector<double> m2[2], var;
            for (int k = 0; k < 2; ++k) { feat[k].resize(npix * RT_FEATURE_WORDS); acc[k].resize(npix * 3); len[k].resize(npix); }
            if (denoise || denoise_var) clean.resize(npix * 3);
            if (denoise_var) { m2[0].resize(npix * 3); m2[1].resize(npix * 3); var.resize(npix * 3); }
            if (!wavefront) {
                rc = rt_render_frames(ctx, cams.data(), (int32_t)cams.size(), stride, &p, fix.data(), &st);
                if (rc) { die("rt_render_frames", rc); rt_destroy(ctx); return 1; }
            }
            float tp_ms = 0.0f;
            size_t with_history = 0, hit_pixels = 0;
            for (size_t f = 0; f < cams.size() && !rc; ++f) {
                const int w = (int)(f & 1), r = 1 - w;
                rt_params fp = p;
                fp.spp = feature_spp; fp.sample_begin = (int32_t)f * stride;
                float ms = 0.0f;
                const uint64_t *frame = fix.data() + (wavefront ? 0 : f * npix * 3);
                if (wavefront) {
                    rt_params q = p;
                    q.sample_begin = (int32_t)f * stride;
                    uint64_t rays = 0;
                    if ((rc = render_wavefront_frame(ctx, &cams[f], &q, fix.data(), &rays, &ms))) break;
                    st.rays_traced += rays; st.kernel_ms += ms; st.samples += (uint64_t)npix * (uint64_t)spp;
                }
                rc = rt_render_features(ctx, &cams[f], &fp, feat[w].data(), nullptr, nullptr);
                if (rc) { die("rt_render_features", rc); break; }
                if (denoise_var) {
                    rc = rt_temporal_var(ctx, frame, nullptr, spp, feat[w].data(), feature_spp, &cams[f], f ? acc[r].data() : nullptr,
                                         f ? len[r].data() : nullptr, f ? feat[r].data() : nullptr, feature_spp, f ? &cams[f - 1] : nullptr,
                                         f ? m2[r].data() : nullptr, width, height, &tp, acc[w].data(), len[w].data(), m2[w].data(), var.data(), &ms);
                    if (rc) { die("rt_temporal_var", rc); break; }
                } else {
                    rc = rt_temporal(ctx, frame, nullptr, spp, feat[w].data(), feature_spp, &cams[f], f ? acc[r].data() : nullptr,
                                     f ? len[r].data() : nullptr, f ? feat[r].data() : nullptr, feature_spp, f ? &cams[f - 1] : nullptr, width, height,
                                     &tp, acc[w].data(), len[w].data(), &ms);
                    if (rc) { die("rt_temporal", rc); break; }
                }
                tp_ms += ms;
                if (f + 1 == cams.size())
                    for (size_t k = 0; k < npix; ++k) { hit_pixels += feat[w][k * RT_FEATURE_WORDS + 7] != 0; with_history += len[w][k] >= 2; }
                if (denoise) {
                    rc = rt_denoise(ctx, acc[w].data(), nullptr, 1, feat[w].data(), feature_spp, width, height, &dn, clean.data(), nullptr);
                    if (rc) { die("rt_denoise", rc); break; }
                }
                if (denoise_var) {
                    rc = rt_denoise_var_given(ctx, acc[w].data(), var.data(), nullptr, 1, feat[w].data(), feature_spp, width, height, &dn, clean.data(),
                                              nullptr);
                    if (rc) { die("rt_denoise_var_given", rc); break; }
                }
                rc = rt_resolve_rgba8(ctx, denoise || denoise_var ? clean.data() : acc[w].data(), width, height, 1, 1, rgba.data() + f * npix * 4);
                if (rc) die("rt_resolve_rgba8", rc);
            }
            if (rc) { rt_destroy(ctx); return 1; }
            std::printf("temporal: alpha_min %g, sigmas %g / %g, clamp %s %g, features at %d spp%s; accumulation kernels %.3f ms; last frame: %zu of %zu hit pixels with history\n",
                        tp.alpha_min, tp.sigma_normal, tp.sigma_depth, (tp.flags & RT_TEMPORAL_CLAMP) ? "on" : "off", tp.clamp_scale, feature_spp,
                        denoise ? ", each frame denoised" : denoise_var ? ", second moments carried, each frame denoised by its variance" : "", tp_ms,
                        with_history, hit_pixels);
        } else {
            rc = rt_render_frames_rgba8(ctx, cams.data(), (int32_t)cams.size(), stride, &p, 1, rgba.data(), &st);
            if (rc) { die("rt_render_frames_rgba8", rc); rt_destroy(ctx); return 1; }
        }
        rt_destroy(ctx);
        std::string prefix = out, ext = ".png";
        if (prefix.size() >= 4 && (prefix.compare(prefix.size() - 4, 4, ".png") == 0 || prefix.compare(prefix.size() - 4, 4, ".ppm") == 0)) {
            ext = prefix.substr(prefix.size() - 4);
            prefix.resize(prefix.size() - 4);
        }
        for (size_t f = 0; f < cams.size(); ++f) {
            char num[32];
            std::snprintf(num, sizeof(num), "_%04zu", f);
            const std::string name = prefix + num + ext;
            const uint8_t *px = rgba.data() + f * npix * 4;
            if (ext == ".png") {
                if (!rtiow::write_png(name.c_str(), px, width, height)) { std::perror(name.c_str()); return 1; }
            } else {
                FILE *fo = std::fopen(name.c_str(), "wb");
                if (!fo) { std::perror(name.c_str()); return 1; }
                std::fprintf(fo, "P6\n%d %d\n255\n", width, height);
                for (size_t k = 0; k < npix; ++k) std::fwrite(&px[4 * k], 1, 3, fo);
                std::fclose(fo);
            }
        }
        std::printf("%zu frames of %dx%d spp %d, sample stride %d, %s: %llu rays, kernel %.3f ms (%.1f Msamples/s) -> %s_0000%s ...\n",
                    cams.size(), width, height, spp, stride, wavefront ? "the path queue" : "one launch", (unsigned long long)st.rays_traced, st.kernel_ms,
                    (double)st.samples / st.kernel_ms / 1e3, prefix.c_str(), ext.c_str());
        return 0;
    }
    const rtiow::Camera cam(rtiow::Point3(13, 2, 3), rtiow::Point3(0, 0, 0), rtiow::Vec3(0, 1, 0), 20.0,
                            (double)width / (double)height, 0.1, 10.0);             // main.rs:108-118
    rt_params p{};
    p.width = width; p.height = height; p.spp = spp; p.sample_begin = 0; p.max_depth = depth;
    p.t_min = 0.0001; p.seed = seed; p.tile_rows = 8; p.shard_index = 0; p.shard_count = 1; p.flags = uniform53 ? RT_FLAG_UNIFORM53 : 0u;
    const size_t npix = (size_t)width * height;
    const rt_camera rc_cam = cam.flat();
    std::vector<uint8_t> rgba(npix * 4);
    rt_stats st{};
    std::string count_note;
    if (adaptive && (!devices.empty() || passes > 1 || two_calls || uniform53)) {
        std::fprintf(stderr, "--adaptive runs on one device and goes with none of --devices, --passes, --two-calls, --uniform53\n");
        return 2;
    }
    if (wavefront && (!devices.empty() || denoise || passes > 1 || two_calls || uniform53 || !features_file.empty())) {
        std::fprintf(stderr, "--wavefront runs on one device and goes with none of --devices, --denoise, --passes, --two-calls, --uniform53, --features\n");
        return 2;
    }
    if (!env_file.empty() && adaptive) {
        std::fprintf(stderr, "--env is not built for --adaptive: the adaptive loop's frames take no environment\n");
        return 2;
    }
    if (const int bad = check_lighting()) return bad;
    if (!devices.empty()) {
        // one rt_context per listed device, each driven by its own host thread; rows dealt round-robin;
        // one RCCL gather of the exact sums to the first device (main.rs:122-123 + the ordered collect() :139)
        p.tile_rows = tile_rows;
        std::string err;
        int copy_calls = 0;
        if (rtiow::render_sharded(devices, force_rccl, flat, rc_cam, p, rgba.data(), &st, &err, &copy_calls)) {
            std::fprintf(stderr, "render_sharded failed: %s\n", err.c_str());
            return 1;
        }
        std::printf("%zu shards, tiles of %d rows: %d device copies put the rows back in image order\n", devices.size(), tile_rows, copy_calls);
    } else {
        rt_context *ctx = nullptr;
        int rc = rt_create(device, &ctx);
        if (rc) return die("rt_create", rc);
        rc = rt_upload_scene(ctx, flat.data(), (int32_t)flat.size());
        if (rc) return die("rt_upload_scene", rc);
        std::vector<uint64_t> dn_fix;                // --denoise: the frame's sums ...
        std::vector<uint32_t> dn_count;              // ... and, with --adaptive, every pixel's own number of samples
        if (denoise_var) {
            // the variance-guided denoiser: the frame's sums, the sums of half of every pixel's samples and (adaptive) the counts -- from the
            // dense kernel or the device path queue --, then the guides, the filter and the one-sample resolve
            std::vector<uint64_t> fix(npix * 3), half(npix * 3);
            std::vector<uint32_t> count;
            uint64_t rays = 0, shadow = 0;
            if (adaptive) {
                rt_adaptive ad{};
                ad.step = step; ad.reserved = 0; ad.threshold = threshold; ad.dark_floor = 0.01;
                count.resize(npix);
                if (wavefront) {
                    rc = rt_render_wavefront_adaptive(ctx, &rc_cam, &p, &ad, lit ? &light : nullptr, any_direct ? 1 : 0, direct_flags, fix.data(),
                                                      half.data(), count.data(), &rays, &shadow, &st.kernel_ms);
                    if (rc) return die("rt_render_wavefront_adaptive", rc);
                    st.rays_traced = rays;
                    st.samples = 0;
                    for (uint32_t c : count) st.samples += c;
                } else {
                    rc = rt_render_adaptive(ctx, &rc_cam, &p, &ad, fix.data(), half.data(), count.data(), &st);
                    if (rc) return die("rt_render_adaptive", rc);
                }
                uint32_t cmin = count[0], cmax = count[0];
                for (uint32_t c : count) { cmin = c < cmin ? c : cmin; cmax = c > cmax ? c : cmax; }
                char note[160];
                std::snprintf(note, sizeof(note), " adaptive threshold %g step %d: %.1f samples per pixel (min %u, max %u),", threshold, step,
                              (double)st.samples / (double)npix, cmin, cmax);
                count_note = note;
            } else {
                rt_params q = p;                 // two passes of spp / 2: the first is `half`, the second renders the later samples on top of it
                q.spp = spp / 2;
                if (wavefront) {
                    float ms = 0.0f;
                    rc = rt_render_wavefront_pixels(ctx, &rc_cam, &q, lit ? &light : nullptr, any_direct ? 1 : 0, direct_flags, nullptr, (int64_t)npix,
                                                    half.data(), &rays, &shadow, &ms);
                    if (rc) return die("rt_render_wavefront_pixels", rc);
                    st.kernel_ms = ms;
                    fix = half;
                    q.sample_begin = spp / 2; q.flags |= RT_FLAG_ACCUMULATE;
                    rc = rt_render_wavefront_pixels(ctx, &rc_cam, &q, lit ? &light : nullptr, any_direct ? 1 : 0, direct_flags, nullptr, (int64_t)npix,
                                                    fix.data(), &rays, &shadow, &ms);
                    if (rc) return die("rt_render_wavefront_pixels", rc);
                    st.kernel_ms += ms; st.rays_traced = rays;
                } else {
                    rt_stats st2{};
                    rc = rt_render(ctx, &rc_cam, &q, nullptr, half.data(), &st);
                    if (rc) return die("rt_render", rc);
                    q.sample_begin = spp / 2;
                    rc = rt_render(ctx, &rc_cam, &q, nullptr, fix.data(), &st2);
                    if (rc) return die("rt_render", rc);
                    for (size_t k = 0; k < npix * 3; ++k) fix[k] += half[k];        // exact integer sums: what one pass of spp samples gives
                    st.rays_traced += st2.rays_traced; st.kernel_ms += st2.kernel_ms;
                }
                st.samples = (uint64_t)npix * (uint64_t)spp;
            }
            if (any_direct) std::fprintf(stderr, "shadow rays: %llu\n", (unsigned long long)shadow);
            rt_params fp = p;
            fp.spp = feature_spp;
            std::vector<uint64_t> feat(npix * RT_FEATURE_WORDS), clean(npix * 3);
            float feat_ms = 0.0f, dn_ms = 0.0f;
            rc = rt_render_features(ctx, &rc_cam, &fp, feat.data(), nullptr, &feat_ms);
            if (rc) return die("rt_render_features", rc);
            rc = rt_denoise_var(ctx, fix.data(), half.data(), adaptive ? count.data() : nullptr, spp, feat.data(), feature_spp, width, height, &dn,
                                clean.data(), &dn_ms);
            if (rc) return die("rt_denoise_var", rc);
            rc = rt_resolve_rgba8(ctx, clean.data(), width, height, 1, 1, rgba.data());
            if (rc) return die("rt_resolve_rgba8", rc);
            std::printf("denoised by variance: %d levels, sigmas %g (standard deviations) / %g / %g, features at %d spp (kernel %.3f ms), filter kernels %.3f ms\n",
                        dn.levels, dn.sigma_color, dn.sigma_normal, dn.sigma_depth, feature_spp, feat_ms, dn_ms);
        } else if (adaptive && wavefront) {      // the adaptive loop over the device path queue's frame, lit or not; then the resolve with counts
            rt_adaptive ad{};
            ad.step = step; ad.reserved = 0; ad.threshold = threshold; ad.dark_floor = 0.01;
            std::vector<uint64_t> fix(npix * 3);
            std::vector<uint32_t> count(npix);
            uint64_t rays = 0, shadow = 0;
            rc = rt_render_wavefront_adaptive(ctx, &rc_cam, &p, &ad, lit ? &light : nullptr, any_direct ? 1 : 0, direct_flags, fix.data(), nullptr,
                                              count.data(), &rays, &shadow, &st.kernel_ms);
            if (rc) return die("rt_render_wavefront_adaptive", rc);
            if (any_direct) std::fprintf(stderr, "shadow rays: %llu\n", (unsigned long long)shadow);
            rc = rt_resolve_rgba8_counts(ctx, fix.data(), count.data(), width, height, 1, rgba.data());
            if (rc) return die("rt_resolve_rgba8_counts", rc);
            uint32_t cmin = count[0], cmax = count[0];
            uint64_t samples = 0;
            for (uint32_t c : count) { cmin = c < cmin ? c : cmin; cmax = c > cmax ? c : cmax; samples += c; }
            st.rays_traced = rays; st.samples = samples;
            char note[160];
            std::snprintf(note, sizeof(note), " adaptive threshold %g step %d: %.1f samples per pixel (min %u, max %u),", threshold, step,
                          (double)st.samples / (double)npix, cmin, cmax);
            count_note = note;
        } else if (adaptive) {
            rt_adaptive ad{};
            ad.step = step; ad.reserved = 0; ad.threshold = threshold; ad.dark_floor = 0.01;
            std::vector<uint64_t> fix(npix * 3);
            std::vector<uint32_t> count(npix);
            rc = rt_render_adaptive(ctx, &rc_cam, &p, &ad, fix.data(), nullptr, count.data(), &st);
            if (rc) return die("rt_render_adaptive", rc);
            if (!denoise) {
                rc = rt_resolve_rgba8_counts(ctx, fix.data(), count.data(), width, height, 1, rgba.data());
                if (rc) return die("rt_resolve_rgba8_counts", rc);
            }
            uint32_t cmin = count[0], cmax = count[0];
            for (uint32_t c : count) { cmin = c < cmin ? c : cmin; cmax = c > cmax ? c : cmax; }
            char note[160];
            std::snprintf(note, sizeof(note), " adaptive threshold %g step %d: %.1f samples per pixel (min %u, max %u),", threshold, step,
                          (double)st.samples / (double)npix, cmin, cmax);
            count_note = note;
            if (denoise) { dn_fix.swap(fix); dn_count.swap(count); }
        } else if (denoise) {
            dn_fix.resize(npix * 3);
            rc = rt_render(ctx, &rc_cam, &p, nullptr, dn_fix.data(), &st);               // main.rs:122-136
            if (rc) return die("rt_render", rc);
        } else if (passes > 1) {
            // progressive passes, overlapped: device buffers, two streams, every pass adds its samples to the same exact sums
            if (passes > spp) { std::fprintf(stderr, "--passes %d: more passes than samples per pixel\n", passes); return 2; }
            auto hip_die = [](hipError_t e, const char *what) { std::fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); return 1; };
            hipError_t e = hipSetDevice(device);
            if (e != hipSuccess) return hip_die(e, "hipSetDevice");
            hipStream_t st2[2] = {nullptr, nullptr};
            void *d_fix = nullptr, *d_rgba = nullptr;
            for (int k = 0; k < 2; ++k) if ((e = hipStreamCreateWithFlags(&st2[k], hipStreamNonBlocking)) != hipSuccess) return hip_die(e, "hipStreamCreate");
            if ((e = hipMalloc(&d_fix, npix * 3 * sizeof(uint64_t))) != hipSuccess) return hip_die(e, "hipMalloc");
            if ((e = hipMalloc(&d_rgba, npix * 4)) != hipSuccess) return hip_die(e, "hipMalloc");
            if ((e = hipMemset(d_fix, 0, npix * 3 * sizeof(uint64_t))) != hipSuccess) return hip_die(e, "hipMemset");      // zero BEFORE any stream adds to it
            unsigned long long rays = 0;
            float kernel_ms = 0.0f;
            int begin = 0;
            for (int k = 0; k < passes; ++k) {
                rt_params q = p;
                q.spp = spp / passes + (k < spp % passes ? 1 : 0);      // the samples dealt as evenly as they go
                q.sample_begin = begin; q.flags |= RT_FLAG_ACCUMULATE | RT_FLAG_OVERLAPPED;
                begin += q.spp;
                rc = rt_render_device(ctx, &rc_cam, &q, d_fix, st2[k & 1]);
                if (rc) return die("rt_render_device", rc);
            }
            for (int k = 0; k < 2; ++k) if ((e = hipStreamSynchronize(st2[k])) != hipSuccess) return hip_die(e, "hipStreamSynchronize");
            rc = rt_last_stats(ctx, &st);                                // (the latest launch only; the ray count below is the frame's)
            if (rc) return die("rt_last_stats", rc);
            rays = st.rays_traced * (unsigned long long)passes; kernel_ms = st.kernel_ms * passes;   // (an estimate for the summary line)
            st.rays_traced = rays; st.kernel_ms = kernel_ms;
            rc = rt_resolve_rgba8_device(ctx, d_fix, width, height, spp, 1, d_rgba, st2[0]);
            if (rc) return die("rt_resolve_rgba8_device", rc);
            if ((e = hipMemcpyAsync(rgba.data(), d_rgba, npix * 4, hipMemcpyDeviceToHost, st2[0])) != hipSuccess) return hip_die(e, "hipMemcpyAsync");
            if ((e = hipStreamSynchronize(st2[0])) != hipSuccess) return hip_die(e, "hipStreamSynchronize");
            (void)hipFree(d_fix); (void)hipFree(d_rgba);
            for (int k = 0; k < 2; ++k) (void)hipStreamDestroy(st2[k]);
        } else if (wavefront) {                  // the device path queue: the same sums, then the same resolve
            std::vector<uint64_t> fix(npix * 3);
            uint64_t rays = 0;
            if (render_wavefront_frame(ctx, &rc_cam, &p, fix.data(), &rays, &st.kernel_ms)) return 1;
            st.rays_traced = rays; st.samples = (uint64_t)npix * (uint64_t)spp;
            rc = rt_resolve_rgba8(ctx, fix.data(), width, height, spp, 1, rgba.data());
            if (rc) return die("rt_resolve_rgba8", rc);
        } else if (two_calls) {                  // the sums through host memory: rt_render, then rt_resolve_rgba8 (same bytes)
            std::vector<uint64_t> fix(npix * 3);
            rc = rt_render(ctx, &rc_cam, &p, nullptr, fix.data(), &st);                  // main.rs:122-136
            if (rc) return die("rt_render", rc);
            rc = rt_resolve_rgba8(ctx, fix.data(), width, height, spp, 1, rgba.data());  // main.rs:137,141-145
            if (rc) return die("rt_resolve_rgba8", rc);
        } else {
            // main.rs:122-145 in one call: the sums stay on the device, the flipped RGBA8 bytes come back
            rc = rt_render_rgba8(ctx, &rc_cam, &p, 1, rgba.data(), &st);
            if (rc) return die("rt_render_rgba8", rc);
        }
        if (denoise) {
            // the guides: the first hits of the same camera's rays, feature_spp samples per pixel; then the filter and the one-sample resolve
            rt_params fp = p;
            fp.spp = feature_spp;
            std::vector<uint64_t> feat(npix * RT_FEATURE_WORDS), clean(npix * 3);
            float feat_ms = 0.0f, dn_ms = 0.0f;
            rc = rt_render_features(ctx, &rc_cam, &fp, feat.data(), nullptr, &feat_ms);
            if (rc) return die("rt_render_features", rc);
            rc = rt_denoise(ctx, dn_fix.data(), adaptive ? dn_count.data() : nullptr, spp, feat.data(), feature_spp, width, height, &dn, clean.data(), &dn_ms);
            if (rc) return die("rt_denoise", rc);
            rc = rt_resolve_rgba8(ctx, clean.data(), width, height, 1, 1, rgba.data());
            if (rc) return die("rt_resolve_rgba8", rc);
            std::printf("denoised: %d levels, sigmas %g / %g / %g, features at %d spp (kernel %.3f ms), filter kernels %.3f ms\n", dn.levels,
                        dn.sigma_color, dn.sigma_normal, dn.sigma_depth, feature_spp, feat_ms, dn_ms);
        }
        if (!features_file.empty()) {
            // what the first hit of the frame's camera rays shows: the same pixels and sample indices as the image
            std::vector<uint64_t> feat(npix * RT_FEATURE_WORDS);
            std::vector<float> f32(npix * RT_FEATURE_WORDS);
            float feat_ms = 0.0f;
            rc = rt_render_features(ctx, &rc_cam, &p, feat.data(), nullptr, &feat_ms);
            if (rc) return die("rt_render_features", rc);
            rc = rt_features_to_f32(ctx, feat.data(), width, height, spp, f32.data());
            if (rc) return die("rt_features_to_f32", rc);
            if (!write_npy_f32(features_file.c_str(), f32.data(), height, width, RT_FEATURE_WORDS)) { std::perror(features_file.c_str()); return 1; }
            std::printf("features %dx%dx%d f32 (albedo, normal, depth, alpha), kernel %.3f ms -> %s\n", height, width, RT_FEATURE_WORDS, feat_ms,
                        features_file.c_str());
        }
        rt_destroy(ctx);
    }
    if (out.size() >= 4 && out.compare(out.size() - 4, 4, ".png") == 0) {             // main.rs:177
        if (!rtiow::write_png(out.c_str(), rgba.data(), width, height)) { std::perror(out.c_str()); return 1; }
    } else {
        FILE *f = std::fopen(out.c_str(), "wb");
        if (!f) { std::perror(out.c_str()); return 1; }
        std::fprintf(f, "P6\n%d %d\n255\n", width, height);
        for (size_t k = 0; k < npix; ++k) std::fwrite(&rgba[4 * k], 1, 3, f);
        std::fclose(f);
    }
    std::printf("%dx%d spp %d:%s %llu rays, kernel %.3f ms (%.1f Msamples/s) -> %s\n", width, height, spp, count_note.c_str(),
                (unsigned long long)st.rays_traced, st.kernel_ms,
                (adaptive ? (double)st.samples : npix * (double)spp) / st.kernel_ms / 1e3, out.c_str());
    return 0;
}
