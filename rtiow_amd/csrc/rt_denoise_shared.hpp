// rt_denoise_shared.hpp -- what the two a-trous denoisers share beyond their arithmetic (DESIGN.md sections 15 and 25), stated ONCE for
// rt_denoise.hip and denoise/rt_denoise_var.hip, which include it behind rt_host.hpp and their core header; denoise/rt_temporal_var.hip
// includes it too, for the host part only (its prepare kernel feeds rt_denoise_var's levels).
//   device  the tile geometry, the tiling of the sub-lattices, the load of a record, the gather form's body, a staged tile's planes
//           (the tile form's body is rt_denoise_tile.inc, which uses them), the finish body;
//   host    the diagnostic knob, the grid cap, the checks of a frame's size and of the settings, the tiling arithmetic, one level's launch.
// The __global__ functions stay in their units, under their pinned names: every body here is inlined into them, and each keeps the
// opcode sequence it had when the units stated all this twice (tests/test_source_layout_host.py, tests/test_denoise_var_host.py).  The
// stores of the prepare kernels are not here: behind a function they lose that sequence.  A unit's frame (DnFrame, DvFrame) names its
// record as Frame::Rec; what only the record with a variance has sits under if constexpr (Rec::kVar).
#pragma once

namespace rt {

constexpr int kDnBlock = 256;
constexpr int kDnTile = 16;                         // a workgroup's tile of one sub-lattice: 16 x 16 pixels
constexpr int kDnSide = kDnTile + 4;                // ... and its halo of two taps on every side
constexpr int kDnCells = kDnSide * kDnSide;
constexpr long long kDnMaxBlocks = 1 << 20;         // grid-stride loops beyond (a launch's work-items fit 32 bits)

// The tile form: a workgroup per 16 x 16 tile of one sub-lattice (pixels with i % s == ri, j % s == rj), the records staged in LDS.
// tiles_x, tiles_y: tiles per sub-lattice (of the widest one; narrower ones have empty tiles); nri = min(s, width) residues in x.
struct DnTiling {
    uint32_t tiles_x, tiles_y, nri, n_tiles;
};

template <class Frame>
__device__ __forceinline__ void dn_load_tap(const Frame &F, unsigned long long p, typename Frame::Rec *t)
{
    const double *c = F.cin + 3 * p, *g = F.box + 3 * p, *q = F.guide + 4 * p;
    t->c[0] = c[0]; t->c[1] = c[1]; t->c[2] = c[2];
    t->g[0] = g[0]; t->g[1] = g[1]; t->g[2] = g[2];
    t->n[0] = q[0]; t->n[1] = q[1]; t->n[2] = q[2];
    t->z = q[3];
    if constexpr (Frame::Rec::kVar) t->var = F.vin[p];
}

// the gather form: one lane per pixel, every tap from global memory
template <class Frame>
__device__ __forceinline__ void dn_gather_body(const Frame &F)
{
    using Rec = typename Frame::Rec;
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < F.npix; p += stride) {
        const uint32_t j = (uint32_t)p / F.width, i = (uint32_t)p - j * F.width;            // npix <= 2^31: p fits 32 bits
        Rec centre;
        dn_load_tap(F, p, &centre);
        const long long s = F.L.step;
        auto tap = [&](int dx, int dy, Rec *t) {
            // (in-frame: the pixel function asks for no other tap)
            const long long q = (long long)p + (s * dy) * (long long)F.width + s * dx;
            dn_load_tap(F, (unsigned long long)q, t);
        };
        double out[3];
        [[maybe_unused]] double var;
        if constexpr (Rec::kVar)                    // (level_pixel_var and level_pixel, by the name both records have)
            rt_dn::level_pixel_of((long long)i, (long long)j, (long long)F.width, (long long)F.height, F.L, F.sc2, F.gv[p], centre, tap, out, &var);
        else
            rt_dn::level_pixel_of((long long)i, (long long)j, (long long)F.width, (long long)F.height, F.L, 0.0, 0.0, centre, tap, out, nullptr);
        F.cout[3 * p + 0] = out[0]; F.cout[3 * p + 1] = out[1]; F.cout[3 * p + 2] = out[2];
        if constexpr (Rec::kVar) F.vout[p] = var;
    }
}

// A staged tile: the records of its (16 + 4)^2 cells in LDS, plane-major (a wave's lanes touch consecutive doubles of one plane) --
// c 3, g 3, n 3, z, and var where the record has one.
template <class Rec>
constexpr int kDnPlanes = Rec::kVar ? 11 : 10;

// one record into its cell
template <class Rec>
__device__ __forceinline__ void dn_stage(double (&s_rec)[kDnPlanes<Rec>][kDnCells], int cell, const Rec &r)
{
    s_rec[0][cell] = r.c[0]; s_rec[1][cell] = r.c[1]; s_rec[2][cell] = r.c[2];
    s_rec[3][cell] = r.g[0]; s_rec[4][cell] = r.g[1]; s_rec[5][cell] = r.g[2];
    s_rec[6][cell] = r.n[0]; s_rec[7][cell] = r.n[1]; s_rec[8][cell] = r.n[2];
    s_rec[9][cell] = r.z;
    if constexpr (Rec::kVar) s_rec[10][cell] = r.var;
}

// ... and one of them back
template <class Rec>
__device__ __forceinline__ void dn_staged(const double (&s_rec)[kDnPlanes<Rec>][kDnCells], int cell, Rec *q)
{
    q->c[0] = s_rec[0][cell]; q->c[1] = s_rec[1][cell]; q->c[2] = s_rec[2][cell];
    q->g[0] = s_rec[3][cell]; q->g[1] = s_rec[4][cell]; q->g[2] = s_rec[5][cell];
    q->n[0] = s_rec[6][cell]; q->n[1] = s_rec[7][cell]; q->n[2] = s_rec[8][cell];
    q->z = s_rec[9][cell];
    if constexpr (Rec::kVar) q->var = s_rec[10][cell];
}

__device__ __forceinline__ void dn_finish_body(const double *c, const double *mod, unsigned long long npix, unsigned long long *out)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kDnBlock;
    for (unsigned long long p = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x; p < npix; p += stride) {
        uint64_t q[3];
        rt_dn::finish(c + 3 * p, mod + 3 * p, q);
        out[3 * p + 0] = q[0]; out[3 * p + 1] = q[1]; out[3 * p + 2] = q[2];
    }
}

// RTIOW_DENOISE_LEVEL_KERNEL (diagnostic, read per call by both denoisers): -1 not set, 0 gather, 1 tile
inline int dn_level_kernel_knob()
{
    const char *e = getenv("RTIOW_DENOISE_LEVEL_KERNEL");
    if (!e || !*e) return -1;
    if (!strcmp(e, "gather")) return 0;
    if (!strcmp(e, "tile")) return 1;
    return -1;
}

inline unsigned dn_blocks_for(unsigned long long items)
{
    unsigned long long b = (items + kDnBlock - 1) / kDnBlock;
    if (b > (unsigned long long)kDnMaxBlocks) b = (unsigned long long)kDnMaxBlocks;
    return (unsigned)(b < 1 ? 1 : b);
}

// a frame the kernels can index: both sides >= 1, at most 2^31 pixels.  who: "denoise", "denoise_var workspace", ...
inline int dn_check_frame(const char *who, int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return rt_host::fail(RT_ERR_INVALID_ARGUMENT, "%s: bad width/height (%d, %d)", who, width, height);
    if ((long long)width * height > (1ll << 31))
        return rt_host::fail(RT_ERR_INVALID_ARGUMENT, "%s: width * height must be <= 2^31 (is %lld)", who, (long long)width * height);
    return RT_OK;
}

inline int dn_workspace_bytes(const char *who, int32_t width, int32_t height, int doubles, int64_t *out_bytes)
{
    if (!out_bytes) return rt_host::fail(RT_ERR_INVALID_ARGUMENT, "%s: out_bytes is NULL", who);
    if (int rc = dn_check_frame(who, width, height)) return rc;
    *out_bytes = (int64_t)width * height * doubles * (int64_t)sizeof(double);
    return RT_OK;
}

// what every form of both denoisers checks behind its NULL pointers, in this order; none of it needs a context
inline int dn_check_settings(const char *who, const struct rt_denoise *dn, int64_t spp, bool has_count, int64_t feat_spp, int32_t width,
                             int32_t height)
{
    using rt_host::fail;
    if (dn->levels < 1 || dn->levels > RT_DENOISE_MAX_LEVELS)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: levels must be 1..%d (is %d)", who, RT_DENOISE_MAX_LEVELS, dn->levels);
    if (dn->flags & ~RT_DENOISE_DEMODULATE) return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", who, dn->flags);
    if (!(dn->sigma_color > 0.0) || !(dn->sigma_normal > 0.0) || !(dn->sigma_depth > 0.0) || !std::isfinite(dn->sigma_color) ||
        !std::isfinite(dn->sigma_normal) || !std::isfinite(dn->sigma_depth))
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: every sigma must be > 0 and finite (%g, %g, %g)", who, dn->sigma_color, dn->sigma_normal,
                    dn->sigma_depth);
    if (int rc = dn_check_frame(who, width, height)) return rc;
    if (!has_count && spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "%s: spp >= 1 without a count buffer (is %lld)", who, (long long)spp);
    if (feat_spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "%s: feat_spp >= 1 (is %lld)", who, (long long)feat_spp);
    return RT_OK;
}

// The tiling of the sub-lattices of hole step s: min(s, width) x min(s, height) of them, each ceil(ceil(width / s) / 16) tiles wide.
// false: the tile number does not fit 31 bits (it is a 32-bit integer in the kernel), the level takes the gather form.
inline bool dn_tiling(unsigned long long s, unsigned long long width, unsigned long long height, DnTiling *T)
{
    const unsigned long long nri = s < width ? s : width, nrj = s < height ? s : height;
    const unsigned long long tiles_x = ((width + s - 1) / s + kDnTile - 1) / kDnTile, tiles_y = ((height + s - 1) / s + kDnTile - 1) / kDnTile;
    const unsigned long long n_tiles = nri * tiles_x * nrj * tiles_y;
    if (n_tiles >= (1ull << 31)) return false;
    T->tiles_x = (uint32_t)tiles_x; T->tiles_y = (uint32_t)tiles_y; T->nri = (uint32_t)nri; T->n_tiles = (uint32_t)n_tiles;
    return true;
}

// One level's taps over the frame F: the tile form if it is wanted and can number its tiles, else the gather form.
template <class Frame>
inline void dn_launch_level(const Frame &F, bool want_tile, void (*tile_kernel)(const Frame, const DnTiling), void (*gather_kernel)(const Frame),
                            hipStream_t stream)
{
    DnTiling T;
    if (want_tile && dn_tiling((unsigned long long)F.L.step, F.width, F.height, &T)) {
        const unsigned tgrid = (unsigned)(T.n_tiles > (unsigned long long)kDnMaxBlocks ? (unsigned long long)kDnMaxBlocks : T.n_tiles);
        hipLaunchKernelGGL(tile_kernel, dim3(tgrid), dim3(kDnBlock), 0, stream, F, T);
    } else {
        hipLaunchKernelGGL(gather_kernel, dim3(dn_blocks_for(F.npix)), dim3(kDnBlock), 0, stream, F);
    }
}

// The variance-guided filter behind its prepare kernel -- the statistics and the taps of every level, then finish into d_out_fix -- for
// the two entries that differ only in where the variance comes from.  Defined in denoise/rt_denoise_var.hip beside its kernels; called
// from there and from denoise/rt_temporal_var.hip (rt_denoise_var_given_device).  k: the partitioned workspace, prepared.
int dn_var_levels_device(const struct rt_denoise *dn, rt_dn::Work k, int32_t width, int32_t height, void *d_out_fix, hipStream_t stream);

} // namespace rt
