// temporal_var_san_main.cpp -- a stand-alone program around rt_temporal_var_core.hpp and rt_denoise_var_core.hpp (and the core headers they
// include; nothing else of the library), built by tests/test_temporal_var_host.py with g++ -fsanitize=address,undefined -ffp-contract=off
// and run directly.
//
//   temporal_var_san_main CASE.bin
// CASE.bin (little endian): i64 width, height, n_frames, spp, feat_spp, flags, has_count, levels, demodulate; f64 alpha_min, sigma_normal,
// sigma_depth, clamp_scale, then the filter's sigma_color, sigma_normal, sigma_depth; then per frame f64 cam[12] (origin,
// lower_left_corner, horizontal, vertical); u64 fix[H][W][3]; u32 count[H][W] (if has_count); u64 feat[H][W][8].  Chains the frames with
// ping-pong history, filters the last accumulated frame (spp = 1, its own guides) by the variance the chain returned, and prints the
// FNV-1a checksum (64 bits, hexadecimal) of the last frame's out_fix, out_len, out_m2 and out_var bytes followed by the filtered frame's;
// every buffer is a std::vector of exactly the size the contract may touch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_temporal_var_core.hpp"
#include "rt_denoise_var_core.hpp"

template <class T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static rt_tp::Cam cam_of(const std::vector<double> &v)
{
    rt_tp::Cam c;
    for (int k = 0; k < 3; ++k) { c.origin[k] = v[k]; c.llc[k] = v[3 + k]; c.horizontal[k] = v[6 + k]; c.vertical[k] = v[9 + k]; }
    return c;
}

template <class T>
static void fnv(unsigned long long &h, const std::vector<T> &v)
{
    const unsigned char *bytes = (const unsigned char *)v.data();
    for (size_t k = 0; k < v.size() * sizeof(T); ++k) h = (h ^ bytes[k]) * 0x100000001B3ull;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASE.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 1; }
    std::vector<long long> head;
    std::vector<double> opt;
    if (!read_n(f, head, 9) || !read_n(f, opt, 7)) { std::fprintf(stderr, "short header\n"); return 1; }
    const long long width = head[0], height = head[1], n_frames = head[2], spp = head[3], feat_spp = head[4];
    const int levels = (int)head[7];
    if (width < 2 || height < 2 || width * height > (1 << 20) || n_frames < 1 || n_frames > 16 || levels < 1 || levels > rt_dn::kMaxLevels) {
        std::fprintf(stderr, "bad header\n");
        return 1;
    }
    const size_t npix = (size_t)(width * height);
    std::vector<uint64_t> fix, feat, prev_feat, out[2] = {std::vector<uint64_t>(npix * 3), std::vector<uint64_t>(npix * 3)};
    std::vector<uint32_t> count, len[2] = {std::vector<uint32_t>(npix), std::vector<uint32_t>(npix)};
    std::vector<double> m2[2] = {std::vector<double>(npix * 3), std::vector<double>(npix * 3)};
    std::vector<double> var[2] = {std::vector<double>(npix * 3), std::vector<double>(npix * 3)};
    std::vector<double> camv;
    rt_tp::Cam prev_cam{};
    int last = 0;
    for (long long k = 0; k < n_frames; ++k) {
        if (!read_n(f, camv, 12) || !read_n(f, fix, npix * 3) || !read_n(f, count, head[6] ? npix : 0) || !read_n(f, feat, npix * 8)) {
            std::fprintf(stderr, "short file\n");
            return 1;
        }
        const rt_tp::Cam cur = cam_of(camv);
        const int w = (int)(k & 1), r = 1 - w;                  // frame k writes set w and reads set r
        const rt_tp::Const K = rt_tp::constants(cur, k ? &prev_cam : nullptr, width, height, spp, feat_spp, feat_spp, (uint32_t)head[5], opt[0],
                                                opt[1], opt[2], opt[3]);
        rt_tp::BuffersVar B;
        B.fix = fix.data(); B.count = head[6] ? count.data() : nullptr; B.feat = feat.data();
        B.prev_fix = k ? out[r].data() : nullptr; B.prev_len = k ? len[r].data() : nullptr; B.prev_feat = k ? prev_feat.data() : nullptr;
        B.prev_m2 = k ? m2[r].data() : nullptr;
        rt_tp::accumulate_var_host(K, B, out[w].data(), len[w].data(), m2[w].data(), var[w].data());
        prev_feat = feat;
        prev_cam = cur;
        last = w;
    }
    std::fclose(f);
    std::vector<double> work(npix * rt_dn::kVarWorkDoubles);
    std::vector<uint64_t> shown(npix * 3);
    rt_dn::filter_var_given_host(out[last].data(), var[last].data(), nullptr, 1, feat.data(), feat_spp, width, height, levels, head[8] != 0, opt[4],
                                 opt[5], opt[6], work.data(), shown.data());
    unsigned long long h = 0xCBF29CE484222325ull;
    fnv(h, out[last]);
    fnv(h, len[last]);
    fnv(h, m2[last]);
    fnv(h, var[last]);
    fnv(h, shown);
    std::printf("%016llx\n", h);
    return 0;
}
