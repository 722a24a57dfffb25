// mixed_launch_check.cpp -- how a mixed decode over one pass of units is cut into launches
// (csrc/mixed_launch.hpp), on the CPU: header-only, built with no ROCm include path
// (tests/test_mixed_launch_native.py).
//
// The launcher (apply_mixed.hip launch_apply_mixed_units) caps a launch at 2^30 workgroups; here
// the same split is walked with caps of 1 and 3 workgroups as well, over divisors 1, 2, 6 and 25
// (a natural batch or a tail pass; RS(12,4) 128 KiB; RS(17,3) 200,000 B; RS(4,2) in 4 KiB blocks)
// and passes that begin on and off a stripe boundary, as the chunks of the host pipeline do.  The
// launches must tile the units exactly, in order, and the stripe each launch's kernel computes
// for its local unit u -- id_begin + verdict_quot(vd, u), or id_begin + u for divisor 1 -- must be
// (first_unit + unit) / divisor: the id the caller meant.  With one launch that is
// first_unit / divisor + verdict_quot(vd, local) == (first_unit + local) / divisor.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../repair-pipelining_amd/csrc/mixed_launch.hpp"

using namespace ecx;

static long g_checks = 0;
#define REQUIRE(c)                                                              \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static void walk(int64_t units, int64_t blocks_per_unit, int64_t divisor, int64_t first_unit, int64_t cap) {
    const int64_t per = mixed_units_per_launch(blocks_per_unit, cap);
    REQUIRE(per >= 1);
    REQUIRE(per == 1 || per * blocks_per_unit <= cap);          // the cap holds, but a launch has a unit at least
    REQUIRE((per + 1) * blocks_per_unit > cap || per == 1);     // and no launch is smaller than it must be
    int64_t next = 0, launches = 0;
    std::vector<int> covered((size_t)units, 0);
    for_mixed_launches(units, blocks_per_unit, divisor, first_unit, cap, [&](const MixedLaunch &l) {
        ++launches;
        REQUIRE(l.unit_begin == next);                          // in order, no gap, no overlap
        REQUIRE(l.unit_count >= 1 && l.unit_count <= per);
        REQUIRE(l.unit_begin + l.unit_count <= units);
        REQUIRE(l.unit_count == per || l.unit_begin + l.unit_count == units);  // only the last one is short
        REQUIRE(l.id_begin == (first_unit + l.unit_begin) / divisor);
        if (divisor > 1) {
            REQUIRE(l.vd.divisor == (uint64_t)divisor);
            REQUIRE(l.vd.rem == (uint64_t)((first_unit + l.unit_begin) % divisor));
        }
        for (int64_t u = 0; u < l.unit_count; ++u) {
            const int64_t stripe = divisor > 1 ? l.id_begin + (int64_t)verdict_quot(l.vd, (uint32_t)u)
                                               : l.id_begin + u;
            REQUIRE(stripe == (first_unit + l.unit_begin + u) / divisor);
            ++covered[(size_t)(l.unit_begin + u)];
        }
        next = l.unit_begin + l.unit_count;
    });
    REQUIRE(next == (units > 0 ? units : 0));
    REQUIRE(launches == (units > 0 ? (units + per - 1) / per : 0));
    for (int64_t u = 0; u < units; ++u) REQUIRE(covered[(size_t)u] == 1);
    // one launch over the whole pass: the identity the kernel relies on
    if (divisor > 1) {
        const VerdictDiv vd = verdict_div(divisor, first_unit);
        for (int64_t local = 0; local < units; ++local)
            REQUIRE(first_unit / divisor + (int64_t)verdict_quot(vd, (uint32_t)local) == (first_unit + local) / divisor);
    }
}

int main() {
    const int64_t caps[] = {1, 3, kMixedMaxBlocks};
    const int64_t divisors[] = {1, 2, 6, 25};
    const int64_t blocks[] = {1, 2, 8, 16};  // workgroups per unit: 4 KiB chunks of a block
    for (int64_t cap : caps)
        for (int64_t d : divisors)
            for (int64_t bpu : blocks) {
                // first units on a stripe boundary (0, d, 7 * d) and off it
                const int64_t firsts[] = {0, d, 7 * d, 1, d - 1 > 0 ? d - 1 : 0, d + 1, 7 * d + d / 2, 1000003};
                for (int64_t first : firsts)
                    for (int64_t units : {0, 1, 2, 5, 24, 25, 26, 149, 150, 151, 1000})
                        walk(units, bpu, d, first, cap);
            }
    // units per launch at the real cap
    REQUIRE(mixed_units_per_launch(8, kMixedMaxBlocks) == (int64_t)1 << 27);
    REQUIRE(mixed_units_per_launch(3, kMixedMaxBlocks) == kMixedMaxBlocks / 3);
    REQUIRE(mixed_units_per_launch(kMixedMaxBlocks, kMixedMaxBlocks) == 1);
    REQUIRE(mixed_units_per_launch(kMixedMaxBlocks + 5, kMixedMaxBlocks) == 1);
    // a pass longer than one launch at the real cap, without walking it: the second launch's ids
    {
        const int64_t bpu = 16, d = 6, first = 4, per = mixed_units_per_launch(bpu, kMixedMaxBlocks);
        int64_t seen = 0;
        for_mixed_launches(2 * per + 7, bpu, d, first, kMixedMaxBlocks, [&](const MixedLaunch &l) {
            REQUIRE(l.unit_begin == seen * per);
            REQUIRE(l.unit_count == (seen < 2 ? per : 7));
            REQUIRE(l.id_begin == (first + l.unit_begin) / d && l.vd.rem == (uint64_t)((first + l.unit_begin) % d));
            for (uint32_t u : {0u, 1u, 5u, (uint32_t)(l.unit_count - 1)})
                REQUIRE(l.id_begin + (int64_t)verdict_quot(l.vd, u) == (first + l.unit_begin + u) / d);
            ++seen;
        });
        REQUIRE(seen == 3);
    }
    std::printf("mixed_launch_check: ok (%ld checks)\n", g_checks);
    return 0;
}
