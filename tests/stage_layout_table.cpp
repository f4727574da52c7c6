// Prints rt_host::StageLayout -- where the blocks of one host-form call lie in the context's staging arena -- for a table of block-size
// lists (tests/test_stage_layout_host.py compiles this for the host only and holds every line to its own statement of the rule).
// No device, no HIP call.
#include <cstdio>
#include <vector>

#include "rt_host.hpp"

static void row(const char *name, const std::vector<size_t> &sizes)
{
    rt_host::StageLayout layout;
    printf("layout %s :", name);
    for (size_t s : sizes) printf(" %zu", s);
    printf(" ->");
    for (size_t s : sizes) printf(" %zu", layout.add(s));
    printf(" | %zu\n", layout.total);
}

// the blocks rt_denoise and rt_temporal declare, in their order (rt_denoise.hip, rt_temporal.hip); a buffer the caller leaves out is a
// block of 0 bytes
static std::vector<size_t> denoise_blocks(size_t w, size_t h, bool count)
{
    const size_t npix = w * h, fix = npix * 3 * 8, feat = npix * 8 * 8, work = npix * 16 * 8;       // (16: kDnWorkDoubles)
    return {fix, feat, fix, work, count ? npix * 4 : 0};
}
static std::vector<size_t> temporal_blocks(size_t w, size_t h, bool count, bool hist)
{
    const size_t npix = w * h, fix = npix * 3 * 8, feat = npix * 8 * 8, len = npix * 4;
    return {fix, feat, count ? len : 0, hist ? fix : 0, hist ? feat : 0, hist ? len : 0, fix, len};
}

int main()
{
    row("none", {});
    const size_t edge[] = {0, 1, 255, 256, 257};
    for (size_t s : edge) {
        char name[32];
        snprintf(name, sizeof(name), "one_%zu", s);
        row(name, {s});
    }
    row("edges", {0, 1, 255, 256, 257});
    row("zero_between", {100, 0, 100});
    row("zeros", {0, 0, 0});
    row("zero_last", {512, 0});
    const size_t frames[][2] = {{7, 5}, {33, 17}};
    for (const auto &f : frames) {
        char name[64];
        for (int count = 0; count < 2; ++count) {
            snprintf(name, sizeof(name), "denoise_%zux%zu_count%d", f[0], f[1], count);
            row(name, denoise_blocks(f[0], f[1], count));
            for (int hist = 0; hist < 2; ++hist) {
                snprintf(name, sizeof(name), "temporal_%zux%zu_count%d_hist%d", f[0], f[1], count, hist);
                row(name, temporal_blocks(f[0], f[1], count, hist));
            }
        }
    }
    return 0;
}
