// denoise_var_san_main.cpp -- a stand-alone program around rt_denoise_var_core.hpp (and, through it, rt_denoise_core.hpp; nothing else of the
// library), built by tests/test_denoise_var_host.py with g++ -fsanitize=address,undefined -ffp-contract=off and run directly.
//
//   denoise_var_san_main CASE.bin
// CASE.bin (little endian): i64 width, height, spp, feat_spp, levels, demodulate, has_count; f64 sigma_color, sigma_normal, sigma_depth;
// u64 fix[H][W][3]; u64 half[H][W][3]; u32 count[H][W] (if has_count); u64 feat[H][W][8].  Prints the FNV-1a checksum (64 bits,
// hexadecimal) of the denoised frame's bytes; every buffer is a std::vector of exactly the size the filter may touch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_denoise_var_core.hpp"

template <class T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASE.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 1; }
    std::vector<long long> head;
    std::vector<double> sigma;
    if (!read_n(f, head, 7) || !read_n(f, sigma, 3)) { std::fprintf(stderr, "short header\n"); return 1; }
    const long long width = head[0], height = head[1], spp = head[2], feat_spp = head[3];
    const int levels = (int)head[4];
    if (width < 1 || height < 1 || width * height > (1 << 20) || levels < 1 || levels > rt_dn::kMaxLevels) { std::fprintf(stderr, "bad header\n"); return 1; }
    const size_t npix = (size_t)(width * height);
    std::vector<uint64_t> fix, half, feat, out(npix * 3);
    std::vector<uint32_t> count;
    if (!read_n(f, fix, npix * 3) || !read_n(f, half, npix * 3) || !read_n(f, count, head[6] ? npix : 0) || !read_n(f, feat, npix * 8)) {
        std::fprintf(stderr, "short file\n");
        return 1;
    }
    std::fclose(f);
    std::vector<double> work(npix * rt_dn::kVarWorkDoubles);
    rt_dn::filter_var_host(fix.data(), half.data(), head[6] ? count.data() : nullptr, spp, feat.data(), feat_spp, width, height, levels, head[5] != 0,
                           sigma[0], sigma[1], sigma[2], work.data(), out.data());
    unsigned long long h = 0xCBF29CE484222325ull;
    const unsigned char *bytes = (const unsigned char *)out.data();
    for (size_t k = 0; k < out.size() * sizeof(uint64_t); ++k) h = (h ^ bytes[k]) * 0x100000001B3ull;
    std::printf("%016llx\n", h);
    return 0;
}
