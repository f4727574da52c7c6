// rt_round_keys.hpp -- the ten round-key pairs of Philox4x32-10 for one launch key, as a table ("the scalar port").
//
// A pure header: no HIP, no context, nothing of the library.  The key of a launch is a launch constant, and so are its round keys
//     key_r = (k0 + r * W0, k1 + r * W1)  mod 2^32,   r = 0 .. 9   (Random123's Weyl sequence).
// The dense kernels with the capped redraw read them from device memory with scalar loads (rt_device.hpp, philox4x32_10_table) instead
// of rebuilding them with 18 scalar adds in every Philox block.  Layout: dword 2 r is k0's round key, dword 2 r + 1 is k1's.
#pragma once
#include <stdint.h>

namespace rt_keys {

constexpr uint32_t kWeyl0 = 0x9E3779B9u, kWeyl1 = 0xBB67AE85u;
constexpr int kRounds = 10;
constexpr int kTableDwords = 2 * kRounds;

inline void fill_round_keys(uint32_t k0, uint32_t k1, uint32_t (&table)[kTableDwords])
{
    for (int r = 0; r < kRounds; ++r) {
        table[2 * r + 0] = k0 + (uint32_t)r * kWeyl0;       // (unsigned arithmetic: wraps mod 2^32 by definition)
        table[2 * r + 1] = k1 + (uint32_t)r * kWeyl1;
    }
}

} // namespace rt_keys
