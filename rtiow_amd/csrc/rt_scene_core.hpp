// rt_scene_core.hpp -- the scene's tables as every render kernel reads them, built on the host from the caller's sphere list: the exact
// geometry and material records, the f32 filter records, and for the shipped scan mode (5, the tube filter) which column of the table
// holds which sphere, the grid the kernel finds tiles with, and the B operands.  Pure: plain C++17, rtiow_hip.h and the standard
// library only -- no HIP, no environment, no context; what the environment and the context used to decide comes in as Knobs.
// rt_api.hip's rt_upload_scene validates, calls build() and copies the vectors to the device; tests/scene_tables_main.cpp compiles this
// header alone under ASan + UBSan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rtiow_hip.h"

namespace rt_scene {

// ANY change to what a table holds -- a record's layout, the order of the columns, a rounding, the grid choice -- bumps this, together
// with the static_assert on it in rt_api.hip: that file is one of bench.py's hashed sources and this header is not, so the edit there
// is what moves kernel_source_sha and keeps recorded counters from being replayed against other tables.
constexpr int kTablesVersion = 1;

// What the build shares with the device code, stated here and pinned against rt:: (rt_device.hpp, rt_params.hpp) by static_asserts in
// rt_api.hip, the one place that sees both sides.
constexpr float kUnitRoundoff = 5.9604644775390625e-08f;                // 2^-24
constexpr float kFilterKU = 128.0f * kUnitRoundoff;                     // 2^-17
constexpr float kTubeBasisErr = 64.0f * kUnitRoundoff;
constexpr float kTubeCenterErr = 640.0f * kUnitRoundoff;
constexpr int kMatStride = 10;      // doubles per material record

// 16 bytes of a B operand: the layout of HIP's uint4
struct Word4 { uint32_t x, y, z, w; };
inline Word4 make_word4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return Word4{x, y, z, w}; }

// K' of the scan filter for one sphere (rt_device.hpp):
// |c|^2 (1-kappa) - r^2 (1+2 kappa) in f64, rounded DOWN to f32 (a smaller K' keeps more);
// spheres outside f32's comfortable range get -inf: always kept.
inline float filter_kprime(const rt_sphere &s, double KU)
{
    const double kappa = KU / (1.0 - KU);
    const double r2 = s.radius * s.radius;
    const double c2 = s.center[0] * s.center[0] + s.center[1] * s.center[1] + s.center[2] * s.center[2];
    if (!(r2 > 1e-30) || !(c2 + r2 < 1e30)) return -INFINITY;
    const double exact = c2 * (1.0 - kappa) - r2 * (1.0 + 2.0 * kappa);
    float kp = (float)(exact - std::fabs(exact) * 1e-12);
    if ((double)kp > exact) kp = std::nextafterf(kp, -INFINITY);
    return kp;
}

inline uint32_t host_bf16_rne(float x)
{
    uint32_t u; memcpy(&u, &x, 4);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
inline void host_split_bf16x3(float x, uint32_t p[3])
{
    auto back = [](uint32_t b) { uint32_t u = b << 16; float f; memcpy(&f, &u, 4); return f; };
    p[0] = host_bf16_rne(x);
    const float r1 = x - back(p[0]);
    p[1] = host_bf16_rne(r1);
    const float r2 = r1 - back(p[1]);
    p[2] = host_bf16_rne(r2);
}

// ---- MODE 5 (tube filter, rt_device.hpp): per-sphere columns and bounds ----
// Radius floor rho: the rows of a ray are scaled by rho / (rho + e_ray), which keeps the test sound for
// every sphere whose bound is >= rho; smaller spheres are tested with the bound rho.  The lower quartile
// of the radii leaves three quarters of the scene untouched and keeps the scaling close to 1.
inline float tube_radius_floor(const rt_sphere *spheres, int n, const char *skip)
{
    std::vector<double> r;
    for (int i = 0; i < n; ++i)
        if (!(skip && skip[i]) && std::fabs(spheres[i].radius) > 1e-15 && std::fabs(spheres[i].radius) < 1e15)
            r.push_back(std::fabs(spheres[i].radius));
    if (r.empty()) return 1.0f;
    std::nth_element(r.begin(), r.begin() + r.size() / 4, r.end());
    return (float)r[r.size() / 4];
}
// bound of one sphere: max(R, rho), R = r (1+64u) + 640u |c| rounded up; +inf outside the analysed range
inline float tube_bound(const rt_sphere &s, float rho)
{
    const double r = std::fabs(s.radius);
    const double c2 = s.center[0] * s.center[0] + s.center[1] * s.center[1] + s.center[2] * s.center[2];
    if (!(r * r > 1e-30) || !(c2 + r * r < 1e30)) return INFINITY;
    const double R = r * (1.0 + (double)kTubeBasisErr) + (double)kTubeCenterErr * std::sqrt(c2);
    float f = (float)(R * (1.0 + 1e-12));
    if ((double)f < R) f = std::nextafterf(f, INFINITY);
    return f > rho ? f : rho;
}
// sigma of one sphere: 2 (1 - 2^-6) / bound, rounded DOWN to a bf16 (rt_device.hpp: "kept" <=> |H| < 2);
// 0 for a sphere outside the analysed range (bound = +inf): H = 0, always kept.  Returns the bf16 bit pattern.
inline uint32_t tube_sigma_bits(float bound)
{
    if (!(bound < INFINITY)) return 0u;
    const float f = (float)(2.0 * (1.0 - 1.0 / 64.0) / (double)bound);
    uint32_t u; memcpy(&u, &f, 4);
    return u >> 16;                                    // truncation = rounding down (sigma > 0)
}
// one tile of 32 columns: B operands [64] (lane l = column l&31, K-slots 8(l>>5)..+7) and, for the tests, the
// bounds [32] the columns were scaled with.  `s[c] == nullptr`: a column no ray keeps (padding, always-exact list):
// all zero but for K-slot 15, where 4 meets the 1 every ray carries there.
inline void tube_tile(const rt_sphere *const s[32], float rho, Word4 out_b[64], float out_r[32])
{
    for (int c = 0; c < 32; ++c) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        out_r[c] = -1.0f;
        if (s[c]) {
            out_r[c] = tube_bound(*s[c], rho);
            const uint32_t sg = tube_sigma_bits(out_r[c]);
            uint32_t sgu = sg << 16; float sigma; memcpy(&sigma, &sgu, 4);
            if (sg != 0u) {                            // (always-kept columns keep sigma = 0, c = 0: H = 0)
                for (int i = 0; i < 3; ++i) {
                    // two bf16 pieces of sigma * (the f64 centre): |sigma c - (y1 + y2)| <= 2^-16 |sigma c|
                    const double ci = s[c]->center[i] * (double)sigma;
                    const uint32_t y1 = host_bf16_rne((float)ci);
                    uint32_t u1 = y1 << 16; float f1; memcpy(&f1, &u1, 4);
                    const uint32_t y2 = host_bf16_rne((float)(ci - (double)f1));
                    w[2 * i + 0] = y1 | (y2 << 16);
                    w[2 * i + 1] = y1 | (y2 << 16);
                }
            }
            w[6] = sg | (sg << 16);                    // sigma against the three exact pieces of t
            w[7] = sg;
        } else {
            w[7] = 0x4080u << 16;                      // K-slot 15: 4.0 -> H = 4 for every ray: never kept
        }
        out_b[c] = make_word4(w[0], w[1], w[2], w[3]);
        out_b[32 + c] = make_word4(w[4], w[5], w[6], w[7]);
    }
}
// a single full tile from 32 spheres, with a rho of its own (the known-answer hooks): the tile and its bounds; -> rho
inline float full_tile(const rt_sphere *spheres32, Word4 out_b[64], float out_r[32])
{
    const float rho = tube_radius_floor(spheres32, 32, nullptr);
    const rt_sphere *col[32];
    for (int c = 0; c < 32; ++c) col[c] = &spheres32[c];
    tube_tile(col, rho, out_b, out_r);
    return rho;
}

// MODE 5 numbers candidates by table column in 26 bits (the pool word of rt_kernels.hpp is column << 6 | ray), and the
// large-grid kernel keeps one 64-bit word per grid row in LDS with one lane per row (a run of columns is (1 << n) - 1 << x0).
constexpr size_t kMaxColumns = (size_t)1 << 26;
constexpr int kMaxGridDim = 63;

// What the environment (at upload) and the context used to supply
struct Knobs {
    int scan_mode = 5;              // the context's filter (RTIOW_SCAN_MODE, read at rt_create): only its tables are built
    int no_grid = 0;                // RTIOW_NO_GRID=1 (diagnostic): columns in list order, every tile scanned
    int grid_dim = 0;               // RTIOW_GRID_DIM=G (diagnostic): cells per side; 0: chosen by cost
};

// Where MODE 5 puts each sphere in its table of columns (tiles of 32), and the grid the kernel finds tiles with.
struct TileLayout {
    int grid_dim = 0, n_global = 0;
    float grid[8] = {};             // rt_params.hpp, KParams::grid
    float scale = 0.0f;             // sum over axes of the largest |coordinate| of the grid's box
    std::vector<int> slot_of;       // column -> place in the caller's list, -1 = padding; a multiple of 32 long
};

// The spheres that skip the filter and are always tested exactly: much larger than the rest of the scene (the
// ground), the filter would keep them for nearly every ray.  The choice only moves work, never results.
inline std::vector<int> always_exact_list(const rt_sphere *spheres, int n)
{
    std::vector<int> out;
    if (n <= 0) return out;
    std::vector<double> radii(n);
    for (int i = 0; i < n; ++i) radii[i] = std::fabs(spheres[i].radius);
    std::vector<double> sorted = radii;
    std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
    const double big = 8.0 * sorted[n / 2];
    std::vector<int> order;
    for (int i = 0; i < n; ++i) if (radii[i] > big) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return radii[x] > radii[y]; });
    for (size_t k = 0; k < order.size() && k < 8; ++k) out.push_back(order[k]);
    return out;
}
// never[i] = 1: sphere i is on the always-exact list and gets no column
inline std::vector<char> never_mask(const std::vector<int> &always, int n)
{
    std::vector<char> never(n > 0 ? n : 1, 0);
    for (int i : always) never[i] = 1;
    return never;
}

inline TileLayout tile_layout(const rt_sphere *spheres, int n, const char *never, const Knobs &knobs)
{
    TileLayout L;
    // ---- which column of the table holds which sphere --------------------------------------------------
    // Spheres are put into tiles of 32 columns by WHERE they are, so that a wave only scans the tiles its rays
    // can reach (rt_device.hpp, grid_cells): a square grid over the xz extent of the small spheres, one tile
    // per cell (what does not fit a cell's 32 columns overflows), preceded by "global" tiles that every ray scans:
    // spheres too large for a cell and the overflow.  The order of the columns decides nothing: ties are resolved
    // on the spheres' positions in the caller's list (slot_orig).  Diagnostic knobs, read at upload:
    // RTIOW_NO_GRID=1 (columns in list order, every tile scanned), RTIOW_GRID_DIM=G (cells per side).
    std::vector<int> filtered;
    for (int i = 0; i < n; ++i) if (!never[i]) filtered.push_back(i);
    std::vector<int> &slot_of = L.slot_of;
    L.grid_dim = 0; L.n_global = 0;
    if (filtered.size() > 64 && !knobs.no_grid) {
        std::vector<double> rr;
        for (int i : filtered) rr.push_back(std::fabs(spheres[i].radius));
        std::nth_element(rr.begin(), rr.begin() + rr.size() / 2, rr.end());
        const double med = rr[rr.size() / 2];
        double x0 = INFINITY, x1 = -INFINITY, z0 = INFINITY, z1 = -INFINITY;
        for (int i : filtered) {
            if (std::fabs(spheres[i].radius) > 3.0 * med) continue;
            x0 = std::min(x0, spheres[i].center[0]); x1 = std::max(x1, spheres[i].center[0]);
            z0 = std::min(z0, spheres[i].center[2]); z1 = std::max(z1, spheres[i].center[2]);
        }
        const double extent = std::max(x1 - x0, z1 - z0);
        // The kernel finds cells with f32 arithmetic on (coordinate - x0) * (1 / cell): the grid exists only while that
        // is meaningful -- a positive extent below 1e15 (coordinates up to 1e15 are legal, so extents up to 2e15 occur)
        // whose cell size has a finite, normal f32 reciprocal.  extent == 0 (every small sphere above the same point):
        // ONE cell of size 1.  Anything else: no grid, every tile scanned, columns in list order.
        const bool one_cell = extent == 0.0;
        const bool grid_ok = one_cell || (extent > 0.0 && extent < 1e15);
        if (grid_ok) {
        // cells(G): the spheres of each cell of a G x G grid, and what does not go into a cell
        std::vector<std::vector<int>> cells;
        std::vector<int> global;
        double cell = 1.0;
        auto assign = [&](int G, bool keep) -> int {       // -> number of global tiles
            cell = one_cell ? 1.0 : extent / G;
            std::vector<int> count((size_t)G * G, 0);
            if (keep) { cells.assign((size_t)G * G, {}); global.clear(); }
            size_t n_glob = 0;
            for (int i : filtered) {
                const double r = std::fabs(spheres[i].radius);
                bool to_cell = !(r > 3.0 * med || r > 0.25 * cell);
                size_t c = 0;
                if (to_cell) {
                    int ix = (int)std::floor((spheres[i].center[0] - x0) / cell), iz = (int)std::floor((spheres[i].center[2] - z0) / cell);
                    ix = std::max(0, std::min(ix, G - 1)); iz = std::max(0, std::min(iz, G - 1));
                    c = (size_t)iz * G + ix;
                    to_cell = count[c] < 32;                        // the cell's tile is full: overflow
                }
                if (to_cell) { ++count[c]; if (keep) cells[c].push_back(i); }
                else { ++n_glob; if (keep) global.push_back(i); }
            }
            return (int)((n_glob + 31) / 32);
        };
        // The grid's resolution: a wave scans the global tiles plus the cells its 64 rays touch, and rays are lines --
        // the cells touched grow like G (measured on the book scenes: about 1.4 G - 1.6 of G x G), while coarse cells
        // overflow into global tiles.  Take the G with the smallest  global tiles + 1.4 G.
        int G = one_cell ? 1 : knobs.grid_dim;
        if (G <= 0) {
            double best = INFINITY;
            for (int g = 1; g <= kMaxGridDim; ++g) {
                if ((double)g * g > (double)filtered.size()) break;
                const int ng = assign(g, false);
                if (ng > 48) continue;                              // (the kernel's list holds 126 tiles)
                const double cost = ng + 1.4 * g;
                if (cost < best) { best = cost; G = g; }
            }
        }
        G = std::max(1, std::min(G, kMaxGridDim));          // (no G qualified: G = 1 will not either, and the grid stays off)
        (void)assign(G, true);
        double ylo = INFINITY, yhi = -INFINITY, pad = 0.0;
        for (const std::vector<int> &c : cells)
            for (int i : c) {
                const double r = std::fabs(spheres[i].radius);
                ylo = std::min(ylo, spheres[i].center[1] - r); yhi = std::max(yhi, spheres[i].center[1] + r);
                pad = std::max(pad, r);
            }
        const int n_global = (int)((global.size() + 31) / 32);
        const float inv_cell = (float)(1.0 / cell);
        if (std::isnormal(inv_cell) && (size_t)(n_global + G * G) * 32 <= (size_t)kMaxColumns && n_global <= 48 && ylo <= yhi) {
            L.grid_dim = G; L.n_global = n_global;
            slot_of.assign((size_t)(n_global + G * G) * 32, -1);
            for (size_t k = 0; k < global.size(); ++k) slot_of[k] = global[k];
            for (size_t c = 0; c < cells.size(); ++c)
                for (size_t k = 0; k < cells[c].size(); ++k) slot_of[((size_t)n_global + c) * 32 + k] = cells[c][k];
            auto down = [](double v) { float f = (float)v; if ((double)f > v) f = std::nextafterf(f, -INFINITY); return f; };
            auto up = [](double v) { float f = (float)v; if ((double)f < v) f = std::nextafterf(f, INFINITY); return f; };
            L.grid[0] = down(x0); L.grid[1] = down(z0);
            // the kernel turns a coordinate into a cell with THESE f32 values; rounding 1/cell either way only
            // shifts cell borders by ~1e-7 cells, which the kernel's own margin (1e-3 cells) covers
            L.grid[2] = inv_cell;
            L.grid[3] = up(x0 + G * cell); L.grid[4] = up(z0 + G * cell);
            L.grid[5] = down(ylo); L.grid[6] = up(yhi); L.grid[7] = up(pad);
            // the kernel's error margins are relative to the size of what a ray can reach inside the grid's box
            const double gs = std::max(std::fabs(x0), std::fabs(x0 + G * cell)) + pad + std::max(std::fabs(ylo), std::fabs(yhi)) +
                              std::max(std::fabs(z0), std::fabs(z0 + G * cell)) + pad;
            L.scale = (float)gs * 1.0001f;
        }
        }   // grid_ok
    }
    if (L.grid_dim == 0) {                              // no grid: the columns in list order, every tile scanned
        slot_of.assign((size_t)((filtered.empty() ? 0 : filtered.back() + 1) + 31) / 32 * 32, -1);
        for (int i : filtered) slot_of[i] = i;
    }
    return L;
}
// the layout of a list as rt_upload_scene would choose it (rt_tile_layout_host)
inline TileLayout list_layout(const rt_sphere *spheres, int n, const Knobs &knobs)
{
    return tile_layout(spheres, n, never_mask(always_exact_list(spheres, n), n).data(), knobs);
}

// The scalars of a scene: what a context keeps of an upload and hands to every kernel (rt_host.hpp, set_scene_params).
struct Header {
    int n_tiles = 0;                // tiles of 16 columns
    int n_global = 0;               // MODE 5: tiles [0, n_global) are scanned for every ray; the rest are grid cells
    int grid_dim = 0;               // MODE 5: cells per side of the xz grid (0: no grid, every tile is scanned)
    float grid[8] = {};             // x0, z0, 1/cell, x1, z1, y lo, y hi, pad (rt_device.hpp, grid_cells)
    float scene_scale = 0.0f;       // MODE 5: KParams::scene_scale
    float tube_rho = 1.0f;          // MODE 5 radius floor
    int n_always = 0;
    int always_idx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// The host vectors exactly as they are uploaded; the ones the scan mode does not read stay empty.
struct Tables {
    Header header;
    std::vector<double> geo;        // [n][4] exact geometry (n = 0: one zero record)
    std::vector<double> mat;        // [n][kMatStride] exact materials
    std::vector<float> filt;        // [n][4] f32 filter records: modes 1-3 (uploaded for mode 1, the source of the mode 2/3 tables)
    std::vector<Word4> btube;       // MODE 5: [tiles/2 + 1][64] B operands
    std::vector<double> geo_slot;   // MODE 5: [slots][4] exact geometry in table (slot) order
    std::vector<uint32_t> slot_orig;    // MODE 5: [slots] list index of the sphere in each column of the table
    std::vector<int> slot_of;       // MODE 5: TileLayout::slot_of (one tile shorter than the tables: they carry a spare)
};

// Validates nothing: rt_upload_scene has checked the list.
inline Tables build(const rt_sphere *spheres, int n, const Knobs &knobs)
{
    Tables T;
    Header &H = T.header;
    const size_t cnt = (size_t)(n > 0 ? n : 1);
    std::vector<double> &geo = T.geo, &mat = T.mat;
    geo.assign(cnt * 4, 0.0); mat.assign(cnt * kMatStride, 0.0);
    for (int i = 0; i < n; ++i) {
        const rt_sphere &s = spheres[i];
        // exact records: radius*radius (sphere.rs:22) and 1.0/radius (vec3.rs:371-375 applied
        // at sphere.rs:37) are per-sphere constants, each one f64 rounding, as in the reference
        const double r2 = s.radius * s.radius;
        geo[4 * i + 0] = s.center[0]; geo[4 * i + 1] = s.center[1]; geo[4 * i + 2] = s.center[2];
        geo[4 * i + 3] = r2;
        double *m = &mat[(size_t)kMatStride * i];
        m[0] = 1.0 / s.radius;
        m[1] = s.param;
        m[2] = s.albedo[0]; m[3] = s.albedo[1]; m[4] = s.albedo[2];
        m[5] = (double)s.kind;
        if (s.kind == RT_DIALECTRIC) {
            // materials.rs:84-87 `1.0/self.ir` and :79 `((1-ri)/(1+ri)).powi(2)` for the two ratios a
            // Dialectric can see (front: 1/ir, back: ir): the reference's own f64 operations, hoisted
            m[6] = 1.0 / s.param;
            double r0 = (1.0 - m[6]) / (1.0 + m[6]); m[7] = r0 * r0;
            r0 = (1.0 - s.param) / (1.0 + s.param); m[8] = r0 * r0;
            m[2] = 1.0; m[3] = 1.0; m[4] = 1.0;                                  // attenuation (1,1,1), :103
        }
    }
    // the spheres that skip the filter (always_exact_list above)
    const std::vector<int> always = always_exact_list(spheres, n);
    H.n_always = 0;
    for (int i : always) H.always_idx[H.n_always++] = i;
    // tile count (tiles of 16 columns) rounded up to even, plus two spare tiles so the pipelined loops
    // never branch on a table bound (padding columns are never kept)
    H.n_tiles = 2 * ((n + 31) / 32);
    // Only the table of the scan mode this context runs is built (RTIOW_SCAN_MODE, read at rt_create).
    if (knobs.scan_mode == 5) {      // the tube filter (shipped)
        const std::vector<char> never = never_mask(always, n);
        H.tube_rho = tube_radius_floor(spheres, n, never.data());
        // which column of the table holds which sphere, and the grid the kernel finds tiles with
        TileLayout L = tile_layout(spheres, n, never.data(), knobs);
        const std::vector<int> &slot_of = L.slot_of;
        H.grid_dim = L.grid_dim; H.n_global = L.n_global;
        for (int k = 0; k < 8; ++k) H.grid[k] = L.grid[k];
        H.scene_scale = L.scale;
        const int n_tiles32 = (int)(slot_of.size() / 32);
        H.n_tiles = 2 * n_tiles32;                             // (counted in 16-column units, as the other scan modes do)
        const size_t ttc = (size_t)n_tiles32 + 1;              // one spare tile: the pipelined loop never branches on a table bound
        std::vector<Word4> &btube = T.btube;
        std::vector<double> &geo_slot = T.geo_slot;
        std::vector<uint32_t> &slot_orig = T.slot_orig;
        btube.resize(ttc * 64);
        std::vector<float> rtube(ttc * 32);
        geo_slot.assign(ttc * 32 * 4, 0.0);
        slot_orig.assign(ttc * 32, 0xFFFFFFFFu);
        for (size_t t = 0; t < ttc; ++t) {
            const rt_sphere *col[32];
            for (int c = 0; c < 32; ++c) {
                const size_t slot = 32 * t + c;
                const int i = slot < slot_of.size() ? slot_of[slot] : -1;
                col[c] = i >= 0 ? &spheres[i] : nullptr;
                if (i >= 0) {
                    slot_orig[slot] = (uint32_t)i;
                    for (int k = 0; k < 4; ++k) geo_slot[4 * slot + k] = geo[4 * (size_t)i + k];
                }
            }
            tube_tile(col, H.tube_rho, &btube[t * 64], &rtube[t * 32]);
        }
        T.slot_of = std::move(L.slot_of);
    }
    // filter records of the f32 evaluation schemes (mode 1, and the sources of the mode 2/3 tables):
    // centre rounded to f32 + K'
    if (knobs.scan_mode >= 1 && knobs.scan_mode <= 3) {
        std::vector<float> &filt = T.filt;
        filt.assign(cnt * 4, 0.0f);
        for (int i = 0; i < n; ++i) {
            const rt_sphere &s = spheres[i];
            filt[4 * i + 0] = (float)s.center[0]; filt[4 * i + 1] = (float)s.center[1];
            filt[4 * i + 2] = (float)s.center[2]; filt[4 * i + 3] = filter_kprime(s, (double)kFilterKU);
        }
    }
    return T;
}

} // namespace rt_scene
