// env_cdf_san_main.cpp -- a stand-alone program around rt_env_core.hpp (nothing else of the library), built by tests/test_env_host.py with
// -fsanitize=address,undefined: the table of an environment cube map in buffers of exactly the size the function may touch.
//   env_cdf_san_main CASE.bin
// CASE.bin: one little-endian i64 (size), then [6][size][size][3] f64 texels.  Prints the 6 * size * size running sums as 16 hex digits
// each, one per line, and checks on its own what holds for every table: valid_size() on the sizes around the limits, a table that
// never decreases where no weight is NaN, an all-zero map that sums to zero, and NaN and negative channels that count as nothing.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_env_core.hpp"

static int fail(const char *what)
{
    std::fprintf(stderr, "env_cdf_san_main: %s\n", what);
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) return fail("usage: env_cdf_san_main CASE.bin");
    for (int32_t size : {0, -1, 3, 6, 1025, 2048, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()})
        if (rt_env::valid_size(size)) return fail("a bad size passes valid_size");
    for (int32_t size = 1; size <= rt_env::kMaxSize; size *= 2)
        if (!rt_env::valid_size(size)) return fail("a power of two in range fails valid_size");
    // tables the program makes up itself, each in a heap buffer of the exact size
    for (int32_t size : {1, 2, 4}) {
        const size_t n = rt_env::texel_count(size);
        std::vector<double> zero(3 * n, 0.0), out(n, -1.0);
        rt_env::cdf(zero.data(), size, out.data());
        for (double v : out)
            if (v != 0.0) return fail("an all-zero map has a weight");
        std::vector<double> bad(3 * n);
        for (size_t k = 0; k < 3 * n; ++k) bad[k] = k % 3 == 0 ? std::numeric_limits<double>::quiet_NaN() : k % 3 == 1 ? -1.0 : -0.0;
        rt_env::cdf(bad.data(), size, out.data());
        for (double v : out)
            if (v != 0.0) return fail("a NaN or negative channel has a weight");
        std::vector<double> ones(3 * n, 1.0);
        rt_env::cdf(ones.data(), size, out.data());
        for (size_t k = 0; k < n; ++k)
            if (!(out[k] > (k ? out[k - 1] : 0.0))) return fail("a positive map's table does not increase");
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case");
    int64_t size64 = 0;
    if (std::fread(&size64, sizeof(size64), 1, f) != 1 || !rt_env::valid_size((int32_t)size64) || size64 > 64) {
        std::fclose(f);
        return fail("the case's size");
    }
    const int32_t size = (int32_t)size64;
    const size_t n = rt_env::texel_count(size);
    std::vector<double> texels(3 * n), out(n);
    const size_t got = std::fread(texels.data(), sizeof(double), 3 * n, f);
    std::fclose(f);
    if (got != 3 * n) return fail("the case is short");
    rt_env::cdf(texels.data(), size, out.data());
    for (double v : out) {
        uint64_t bits;
        std::memcpy(&bits, &v, sizeof(bits));
        std::printf("%016" PRIx64 "\n", bits);
    }
    return 0;
}
