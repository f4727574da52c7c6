// round_keys_main.cpp -- a stand-alone program around rt_round_keys.hpp (nothing else of the library), built by
// tests/test_round_key_table_host.py with g++ -fsanitize=address,undefined and run directly.
//
//   round_keys_main KEYS.txt
// KEYS.txt: one key per line, "k0 k1" in hexadecimal.  Prints one line per key: the table's twenty dwords in hexadecimal, in table order
// (dword 2 r: k0's key of round r, dword 2 r + 1: k1's).
#include <cstdio>
#include <vector>

#include "rt_round_keys.hpp"

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s KEYS.txt\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 1; }
    std::vector<unsigned> keys;
    unsigned k0, k1;
    while (std::fscanf(f, "%x %x", &k0, &k1) == 2) { keys.push_back(k0); keys.push_back(k1); }
    std::fclose(f);
    for (size_t i = 0; i + 1 < keys.size(); i += 2) {
        uint32_t table[rt_keys::kTableDwords];
        rt_keys::fill_round_keys(keys[i], keys[i + 1], table);
        for (int k = 0; k < rt_keys::kTableDwords; ++k) std::printf("%s%x", k ? " " : "", table[k]);
        std::printf("\n");
    }
    return 0;
}
