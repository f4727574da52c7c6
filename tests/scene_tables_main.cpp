// scene_tables_main.cpp -- a stand-alone program around rt_scene_core.hpp (nothing else of the library), built by
// tests/test_scene_tables_host.py with g++ -fsanitize=address,undefined -ffp-contract=off and run directly.
//
//   scene_tables_main SPHERES.bin SCAN_MODE NO_GRID GRID_DIM [--dump]
// SPHERES.bin: rt_sphere records (72 bytes each, as the caller of rt_upload_scene passes them), none for the empty list.  Prints the
// header's scalars (floats as their bit patterns), slot_of, and per table "hash NAME <FNV-1a, 64 bits, of its bytes>" ("-": the scan
// mode has no such table); "hash input" is that of the sphere bytes.  --dump adds "dump NAME" lines with each table's words in
// hexadecimal: 64-bit words for geo, mat and geo_slot, 32-bit words for the rest.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_scene_core.hpp"

static unsigned long long fnv1a(const void *data, size_t bytes)
{
    unsigned long long h = 0xCBF29CE484222325ull;
    const unsigned char *b = (const unsigned char *)data;
    for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 0x100000001B3ull;
    return h;
}

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

template <class T>
static void table(const char *name, const std::vector<T> &v, bool dump, bool wide)
{
    if (v.empty()) { std::printf("hash %s -\n", name); return; }
    std::printf("hash %s %016llx\n", name, fnv1a(v.data(), v.size() * sizeof(T)));
    if (!dump) return;
    std::printf("dump %s", name);
    const size_t bytes = v.size() * sizeof(T);
    const unsigned char *b = (const unsigned char *)v.data();
    for (size_t k = 0; k < bytes; k += wide ? 8 : 4) {
        if (wide) { unsigned long long w; std::memcpy(&w, b + k, 8); std::printf(" %llx", w); }
        else { unsigned w; std::memcpy(&w, b + k, 4); std::printf(" %x", w); }
    }
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 5 && !(argc == 6 && !std::strcmp(argv[5], "--dump"))) {
        std::fprintf(stderr, "usage: %s SPHERES.bin SCAN_MODE NO_GRID GRID_DIM [--dump]\n", argv[0]);
        return 2;
    }
    const bool dump = argc == 6;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 1; }
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (size < 0 || size % (long)sizeof(rt_sphere) != 0) { std::fprintf(stderr, "not a whole number of rt_sphere records\n"); return 1; }
    std::vector<rt_sphere> spheres((size_t)size / sizeof(rt_sphere));
    if (!spheres.empty() && std::fread(spheres.data(), sizeof(rt_sphere), spheres.size(), f) != spheres.size()) { std::fprintf(stderr, "short file\n"); return 1; }
    std::fclose(f);
    rt_scene::Knobs knobs;
    knobs.scan_mode = std::atoi(argv[2]); knobs.no_grid = std::atoi(argv[3]); knobs.grid_dim = std::atoi(argv[4]);

    const rt_scene::Tables T = rt_scene::build(spheres.data(), (int)spheres.size(), knobs);
    const rt_scene::Header &H = T.header;
    std::printf("n %zu\nn_tiles %d\nn_global %d\ngrid_dim %d\ngrid", spheres.size(), H.n_tiles, H.n_global, H.grid_dim);
    for (int k = 0; k < 8; ++k) std::printf(" %08x", bits(H.grid[k]));
    std::printf("\nscene_scale %08x\ntube_rho %08x\nn_always %d\nalways_idx", bits(H.scene_scale), bits(H.tube_rho), H.n_always);
    for (int e = 0; e < 8; ++e) std::printf(" %d", H.always_idx[e]);
    std::printf("\nslot_of");
    for (int s : T.slot_of) std::printf(" %d", s);
    std::printf("\nhash input %016llx\n", fnv1a(spheres.data(), spheres.size() * sizeof(rt_sphere)));
    table("geo", T.geo, dump, true);
    table("mat", T.mat, dump, true);
    table("filt", T.filt, dump, false);
    table("btube", T.btube, dump, false);
    table("geo_slot", T.geo_slot, dump, true);
    table("slot_orig", T.slot_orig, dump, false);
    return 0;
}
