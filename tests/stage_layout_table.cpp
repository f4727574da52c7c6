// Prints rt_host::StageLayout -- where the blocks of one host-form call lie in the context's staging arena -- for a table of block-size
// lists, and rt_host::StagePlan -- what a call that DECLARES its buffers (direction, the caller's pointer or NULL, bytes) gets: the
// offsets, the total, which blocks have a device pointer and which are copied up and down, in order -- for a table of declared lists
// (tests/test_stage_layout_host.py compiles this for the host only, once more under the sanitizers, and holds every line to its own
// statement of the rule).  No device, no HIP call.
#include <cstdio>
#include <cstring>
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
    const size_t npix = w * h, fix = npix * 3 * 8, feat = npix * 8 * 8, work = npix * 16 * 8;       // (16: rt_dn::kWorkDoubles)
    return {fix, feat, fix, work, count ? npix * 4 : 0};
}
static std::vector<size_t> temporal_blocks(size_t w, size_t h, bool count, bool hist)
{
    const size_t npix = w * h, fix = npix * 3 * 8, feat = npix * 8 * 8, len = npix * 4;
    return {fix, feat, count ? len : 0, hist ? fix : 0, hist ? feat : 0, hist ? len : 0, fix, len};
}

// one declared buffer: direction (i in, o out, b inout, s scratch), whether the caller gave a pointer, bytes
struct Decl { char dir; bool host; size_t bytes; };

static void plan_row(const char *name, const std::vector<Decl> &decls)
{
    static char caller[1];                              // (what a given pointer points at does not matter: nothing is copied here)
    struct { rt_host::StagePlan plan; unsigned char after[64]; } g;
    memset(g.after, 0xA5, sizeof(g.after));
    rt_host::StagePlan &plan = g.plan;
    std::vector<int> ids;
    printf("plan %s :", name);
    for (const Decl &d : decls) {
        const rt_host::StageDir dir = d.dir == 'i' ? rt_host::StageDir::in : d.dir == 'o' ? rt_host::StageDir::out
                                    : d.dir == 'b' ? rt_host::StageDir::inout : rt_host::StageDir::scratch;
        ids.push_back(plan.declare(dir, d.host ? caller : nullptr, d.bytes));
        printf(" %c%d:%zu", d.dir, d.host ? 1 : 0, d.bytes);
    }
    printf(" -> ids");
    for (int id : ids) printf(" %d", id);
    printf(" | offsets");
    for (int k = 0; k < plan.n; ++k) printf(" %zu", plan.blocks[k].offset);
    printf(" | bytes");
    for (int k = 0; k < plan.n; ++k) printf(" %zu", plan.blocks[k].bytes);
    printf(" | total %zu | ptr", plan.layout.total);
    for (int k = 0; k < plan.n; ++k) if (plan.present(k)) printf(" %d", k);
    printf(" | up");
    for (int k = 0; k < plan.n; ++k) if (plan.goes_up(k)) printf(" %d", k);
    printf(" | down");
    for (int k = 0; k < plan.n; ++k) if (plan.comes_down(k)) printf(" %d", k);
    bool intact = true;
    for (unsigned char c : g.after) intact = intact && c == 0xA5;
    // a number no declaration returned names no block
    printf(" | overflow %d | after %s | stray %d\n", plan.overflow ? 1 : 0, intact ? "intact" : "OVERWRITTEN",
           (plan.present(-1) || plan.present(plan.n) || plan.goes_up(-1) || plan.comes_down(plan.n)) ? 1 : 0);
}

// the buffers rt_scatter and rt_trace_rays declare, in their order (wavefront/rt_shade.hip, rt_trace.hip), for n paths or rays
static std::vector<Decl> scatter_decls(size_t n, bool in_place)
{
    const size_t v3 = n * 3 * 8, w32 = n * 4;
    std::vector<Decl> d = {{in_place ? 'b' : 'i', true, v3}, {'i', true, w32}, {'i', true, v3}, {'i', true, v3}, {'i', true, n}, {'i', true, w32},
                           {'i', true, w32}, {'b', true, w32}, {'b', true, v3}};
    if (!in_place) d.push_back({'b', true, v3});
    d.push_back({'b', true, v3});
    d.push_back({'o', true, n});
    return d;
}
static std::vector<Decl> trace_decls(size_t n, bool t_max, bool all)
{
    const size_t v3 = n * 3 * 8;
    return {{'i', true, v3}, {'i', true, v3}, {'i', t_max, n * 8}, {'o', true, n * 4}, {'o', all, n * 8}, {'o', all, v3}, {'o', all, v3}, {'o', all, n}};
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
    plan_row("none", {});
    plan_row("null_middle", {{'i', true, 100}, {'i', false, 300}, {'o', true, 100}});
    plan_row("null_last", {{'i', true, 512}, {'o', false, 64}});
    plan_row("null_each_direction", {{'i', false, 8}, {'o', false, 8}, {'b', false, 8}, {'s', false, 8}});
    plan_row("inout", {{'i', true, 257}, {'b', true, 40}, {'o', true, 1}});
    plan_row("scratch", {{'i', true, 24}, {'s', false, 1000}, {'o', true, 24}});
    plan_row("zero_count_given", {{'i', true, 0}, {'b', true, 0}, {'o', true, 0}, {'s', false, 0}, {'o', true, 16}});
    for (int extra = 0; extra < 3; ++extra) {
        char name[32];
        snprintf(name, sizeof(name), "capacity_plus_%d", extra);
        std::vector<Decl> d;
        for (int k = 0; k < rt_host::StagePlan::kCapacity + extra; ++k) d.push_back({"iobs"[k % 4], k % 5 != 0, (size_t)(k * 37 + 1)});
        plan_row(name, d);
    }
    const size_t counts[] = {35, 2304};
    for (size_t n : counts) {
        char name[64];
        snprintf(name, sizeof(name), "scatter_%zu", n);
        plan_row(name, scatter_decls(n, false));
        snprintf(name, sizeof(name), "scatter_in_place_%zu", n);
        plan_row(name, scatter_decls(n, true));
        snprintf(name, sizeof(name), "trace_all_%zu", n);
        plan_row(name, trace_decls(n, true, true));
        snprintf(name, sizeof(name), "trace_index_%zu", n);
        plan_row(name, trace_decls(n, false, false));
    }
    return 0;
}
