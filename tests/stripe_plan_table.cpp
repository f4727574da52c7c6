// Prints rt_host::plan_stripes (rt_launch.hpp: how many replicas of a block's pixel slots the lane-striped block sums keep) for a table of
// inputs; tests/stripe_plan.py compiles this for the host only and parses it, tests/test_stripe_plan_host.py compares every line with a
// brute-force restatement, tests/test_gpu_striped_sums.py takes its sample counts from it.  No device, no HIP call.
#include <cstdio>

#include "rt_launch.hpp"

int main()
{
    const unsigned blocks[] = {64u, 128u, 192u, 256u, 1024u};
    const int extra[] = {500, 511, 512, 513, 1022, 1023, 1024, 1025, 2000, 32767};
    for (unsigned items : blocks)
        for (int k = 0; k <= 400 + 10; ++k) {
            const int spp = k <= 400 ? k : extra[k - 401];
            for (int bits = 0; bits < 4; ++bits) {
                const bool use_ring = bits & 1, striped = bits & 2;
                const rt_host::StripePlan sp = rt_host::plan_stripes(use_ring, items, spp, striped);
                printf("stripe %u %d %d %d -> %u %u %u\n", items, spp, (int)use_ring, (int)striped, sp.slots, sp.replicas, sp.mask);
            }
        }
    return 0;
}
