// Prints rt_host::plan_launch and rt_host::magic_for for a table of inputs (tests/test_launch_plan_host.py compiles this for the host
// only and compares every line with its own restatement of the rule).  No device, no HIP call.
#include <cstdio>

#include "rt_launch.hpp"

int main()
{
    const int extra[] = {68, 69, 146, 147, 500};
    const unsigned long long thresholds[] = {0ull, 200000000ull};
    for (int k = 0; k <= 40 + 5; ++k) {
        const int spp = k <= 40 ? k : extra[k - 41];
        for (int ring_min = 0; ring_min <= 20; ring_min += 20)
            for (int bits = 0; bits < 8; ++bits)
                for (unsigned long long thr : thresholds)
                    for (int at = 0; at < 2; ++at) {
                        const bool shipped = bits & 1, small_grid = bits & 2, large_allowed = bits & 4;
                        if (!at && thr == 0) continue;                      // (nothing lies below a threshold of 0)
                        const unsigned long long total = at ? thr : thr - 1;
                        const rt_host::LaunchPlan plan = rt_host::plan_launch(spp, ring_min, shipped, small_grid, large_allowed, total, thr);
                        printf("plan %d %d %d %d %d %llu %llu -> %d %u %d\n", spp, ring_min, (int)shipped, (int)small_grid, (int)large_allowed, total, thr,
                               (int)plan.use_ring, plan.block_items, (int)plan.large_blocks);
                    }
    }
    const long long divisors[] = {-1, 0, 1, 2, 3, 7, 10, 100, 500, 1200, 32767, 32768, 65535};
    for (long long d : divisors) printf("magic %lld -> %u\n", d, rt_host::magic_for(d));
    return 0;
}
