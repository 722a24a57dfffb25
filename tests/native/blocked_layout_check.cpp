// blocked_layout_check.cpp -- the pass plan of a blocked RS batch (csrc/blocked_layout.cpp), on
// the CPU: built from that one file with no ROCm include path (tests/test_blocked_layout_native.py).
//
// Over seeded random (n, nstripes, byte_count, block) and the layout's edge cases it asserts that
// the passes cover [0, nstripes * n * byte_count) exactly once; that every byte of caller stripe
// s, shard i -- placed where blocked_pack (the package's definition of the layout) puts it --
// lands in a unit with unit / divisor == s and in slot i; that full == 0 yields only the tail
// pass, tail == 0 only the body pass, block == byte_count one body unit per stripe; and that
// extents overflowing int64_t are refused.  The verdict index the blocked check kernel computes
// without a division (verdict_div / verdict_quot) is compared with unit / divisor over launches
// split at arbitrary units, over every divisor class (small, powers of two, up to 2^31 - 1, and
// the 2^31.. range that takes the comparison).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../repair-pipelining_amd/csrc/blocked_layout.hpp"

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

// where blocked_pack puts byte b of shard i of stripe s (repair-pipelining_amd/__init__.py)
static int64_t packed_offset(int n, int64_t S, int64_t L, int64_t block, int64_t s, int i, int64_t b) {
    const int64_t full = L / block, tail = L % block, body = full * n * block;
    if (b < full * block) return s * body + (b / block) * n * block + (int64_t)i * block + b % block;
    return S * body + s * n * tail + (int64_t)i * tail + (b - full * block);
}

// the verdict index as launch_check_core and k_gf_check_blocked compute it for unit u of a launch
// that starts at unit s0
static int64_t kernel_verdict(int64_t divisor, int64_t s0, int64_t u) {
    if (divisor == 1) return u;
    const VerdictDiv d = verdict_div(divisor, s0);
    return s0 / divisor + (int64_t)verdict_quot(d, (uint32_t)(u - s0));
}

static void check_shape(int n, int64_t S, int64_t L, int64_t block, std::mt19937_64 &rng) {
    BlockedPlan plan;
    REQUIRE(blocked_plan(n, S, L, block, &plan));
    const int64_t total = S * n * L;
    if (total == 0) {
        REQUIRE(plan.count == 0);
        return;
    }
    const int64_t full = L / block, tail = L % block;
    REQUIRE(plan.count == (full > 0) + (tail > 0));
    int at = 0;
    if (full > 0) {
        const BlockedPass &p = plan.pass[at++];
        REQUIRE(p.offset == 0 && p.slot_bytes == block && p.stripe_stride == n * block);
        REQUIRE(p.units == S * full && p.divisor == full);
    }
    if (tail > 0) {
        const BlockedPass &p = plan.pass[at++];
        REQUIRE(p.offset == S * full * n * block && p.slot_bytes == tail && p.stripe_stride == n * tail);
        REQUIRE(p.units == S && p.divisor == 1);
    }
    if (full == 0) REQUIRE(plan.count == 1 && plan.pass[0].divisor == 1 && plan.pass[0].slot_bytes == tail);
    if (tail == 0) REQUIRE(plan.count == 1 && plan.pass[0].slot_bytes == block);
    if (block == L) REQUIRE(plan.count == 1 && plan.pass[0].units == S && plan.pass[0].divisor == 1);

    // every byte the passes address, counted: exactly once each, none outside the batch
    std::vector<uint8_t> hits((size_t)total, 0);
    for (int k = 0; k < plan.count; ++k) {
        const BlockedPass &p = plan.pass[k];
        for (int64_t u = 0; u < p.units; ++u)
            for (int i = 0; i < n; ++i)
                for (int64_t b = 0; b < p.slot_bytes; ++b) {
                    const int64_t off = p.offset + u * p.stripe_stride + i * p.slot_bytes + b;
                    REQUIRE(off >= 0 && off < total);
                    ++hits[(size_t)off];
                }
    }
    for (int64_t o = 0; o < total; ++o) REQUIRE(hits[(size_t)o] == 1);

    // a launch split of each pass at a random unit, as stripes_per_launch splits a large pass
    int64_t split[2] = {0, 0};
    for (int k = 0; k < plan.count; ++k) split[k] = (int64_t)(rng() % (uint64_t)plan.pass[k].units);
    for (int64_t s = 0; s < S; ++s)
        for (int i = 0; i < n; ++i)
            for (int64_t b = 0; b < L; ++b) {
                const int64_t off = packed_offset(n, S, L, block, s, i, b);
                const int k = plan.count == 2 && off >= plan.pass[1].offset ? 1 : 0;
                const BlockedPass &p = plan.pass[k];
                const int64_t rel = off - p.offset;
                REQUIRE(rel >= 0);
                const int64_t unit = rel / p.stripe_stride, slot = rel % p.stripe_stride / p.slot_bytes;
                REQUIRE(unit < p.units);
                REQUIRE(unit / p.divisor == s);
                REQUIRE(slot == i);
                const int64_t s0 = unit >= split[k] ? split[k] : 0;
                REQUIRE(kernel_verdict(p.divisor, s0, unit) == s);
            }
}

static void check_quotients(std::mt19937_64 &rng) {
    std::vector<uint64_t> divs = {2, 3, 5, 6, 7, 48, 49, 4096, 65535, 65536, 65537, (1ull << 31) - 1, (1ull << 31) - 2,
                                  (1ull << 30), (1ull << 30) + 1, 1ull << 31, (1ull << 31) + 1, 1ull << 32,
                                  (1ull << 40) + 12345, (1ull << 62) - 1};
    for (int r = 0; r < 2000; ++r) divs.push_back(2 + rng() % ((1ull << 31) - 2));
    for (int r = 0; r < 200; ++r) divs.push_back((1ull << 31) + rng() % (1ull << 61));
    const uint32_t kMaxLocal = 1u << 30;  // a launch's units: at most 2^30 workgroups
    for (uint64_t d : divs) {
        std::vector<uint64_t> firsts = {0, 1, d - 1, d, d + 1, 7 * d - 1, 7 * d};
        for (int r = 0; r < 8; ++r) firsts.push_back(rng() % (1ull << 62));
        for (uint64_t s0 : firsts) {
            const VerdictDiv v = verdict_div((int64_t)d, (int64_t)s0);
            REQUIRE(v.rem == s0 % d && v.divisor == d);
            std::vector<uint32_t> locals = {0, 1, kMaxLocal - 1, kMaxLocal};
            if (d - v.rem <= kMaxLocal) {  // the boundary of the first stripe of the launch
                locals.push_back((uint32_t)(d - v.rem));
                locals.push_back((uint32_t)(d - v.rem - 1));
            }
            for (int r = 0; r < 16; ++r) locals.push_back((uint32_t)(rng() % (kMaxLocal + 1ull)));
            for (uint32_t l : locals) REQUIRE(verdict_quot(v, l) == (v.rem + l) / d);
        }
    }
    // every unit of a few whole small launches
    for (uint64_t d : {2ull, 3ull, 6ull, 48ull, 1000ull})
        for (uint64_t s0 : {0ull, 1ull, 5ull, 999ull, 12345ull}) {
            const VerdictDiv v = verdict_div((int64_t)d, (int64_t)s0);
            for (uint32_t l = 0; l < 20000; ++l) REQUIRE(verdict_quot(v, l) == (v.rem + l) / d);
        }
}

int main() {
    std::mt19937_64 rng(20260817);

    // the recommended block and what block_bytes stands for
    REQUIRE(recommended_block(20, 200000) == 32768);
    REQUIRE(recommended_block(16, 4 << 20) == 65536);
    REQUIRE(recommended_block(4, 34) == 34);
    REQUIRE(recommended_block(256, 1 << 20) == 4096);
    REQUIRE(recommended_block(2, 8 << 20) == 524288);
    REQUIRE(recommended_block(20, 0) == 0);
    int64_t blk = -7;
    REQUIRE(resolve_block(20, 200000, 0, &blk) && blk == 32768);
    REQUIRE(resolve_block(20, 200000, 4096, &blk) && blk == 4096);
    blk = -7;
    REQUIRE(!resolve_block(20, 200000, -1, &blk) && blk == -7);

    // the shapes of the GPU parity test, by (n, byte_count, block), and the layout's edges
    struct Shape {
        int n;
        int64_t S, L, block;
    };
    const Shape fixed[] = {
        {20, 3, 200000, 32768}, {16, 2, 3 * 65536 + 4096, 65536}, {16, 2, 3 * 65536, 65536}, {6, 7, 104449, 4096},
        {10, 7, 1001, 64},      {4, 7, 34, 34},                   {6, 7, 100, 4096},         {20, 2, 2 * 4096 + 48, 4096},
        {3, 5, 1, 1},           {3, 5, 7, 1},                     {2, 1, 64, 64},            {2, 1, 64, 65},
        {2, 1, 64, 63},         {5, 0, 100, 10},                  {5, 4, 0, 10},             {1, 3, 10, 3},
    };
    for (const Shape &f : fixed) check_shape(f.n, f.S, f.L, f.block, rng);
    for (int r = 0; r < 400; ++r) {
        const int n = 1 + (int)(rng() % 12);
        const int64_t S = (int64_t)(rng() % 6);
        const int64_t L = (int64_t)(rng() % 300);
        int64_t block = 1 + (int64_t)(rng() % 96);
        if (r % 5 == 0 && L > 0) block = L;                 // one body unit per stripe
        if (r % 5 == 1 && L > 0) block = L + 1 + r % 7;     // full == 0
        if (r % 5 == 2 && L > 0) block = 1 + (int64_t)(rng() % (uint64_t)L);
        check_shape(n, S, L, block, rng);
    }
    for (int r = 0; r < 60; ++r) {  // tail == 0 on purpose
        const int n = 1 + (int)(rng() % 8);
        const int64_t block = 1 + (int64_t)(rng() % 40), full = 1 + (int64_t)(rng() % 9);
        check_shape(n, 1 + (int64_t)(rng() % 5), full * block, block, rng);
    }

    // refusals: a plan that is not made leaves *plan alone
    BlockedPlan plan;
    plan.count = 77;
    const int64_t big = INT64_MAX;
    REQUIRE(!blocked_plan(20, big / 2, 200000, 32768, &plan) && plan.count == 77);      // units * stride
    REQUIRE(!blocked_plan(20, 1, big, big / 4, &plan) && plan.count == 77);             // n * block
    REQUIRE(!blocked_plan(2, big / 2 + 1, 4, 2, &plan) && plan.count == 77);            // nstripes * full
    REQUIRE(!blocked_plan(3, big / 4, 5, 4, &plan) && plan.count == 77);                // body fits, body + tails does not
    REQUIRE(!blocked_plan(3, big / 8, 3, 4, &plan) && plan.count == 77);                // the tails alone
    REQUIRE(!blocked_plan(20, 4, 100, 0, &plan));                                       // no block for bytes to cover
    REQUIRE(!blocked_plan(20, 4, 100, -4096, &plan));
    REQUIRE(!blocked_plan(20, -1, 100, 10, &plan));
    REQUIRE(!blocked_plan(20, 4, -100, 10, &plan));
    // the largest extent that fits is planned
    {
        const int64_t S = big / (20 * 200000);
        REQUIRE(blocked_plan(20, S, 200000, 32768, &plan) && plan.count == 2);
        REQUIRE(plan.pass[0].units == S * 6 && plan.pass[0].divisor == 6 && plan.pass[1].units == S);
        REQUIRE(plan.pass[1].offset == S * 6 * 20 * 32768);
        REQUIRE(!blocked_plan(20, S + 1, 200000, 32768, &plan));
    }
    // nothing to do is a plan of no passes, whatever the block
    REQUIRE(blocked_plan(20, 0, 200000, 0, &plan) && plan.count == 0);
    REQUIRE(blocked_plan(20, 9, 0, 0, &plan) && plan.count == 0);

    check_quotients(rng);

    std::printf("blocked_layout_check: ok (%ld checks)\n", g_checks);
    return 0;
}
