// locate2_plan_check.cpp -- the pair plan of an RS code (csrc/locate2_plan.cpp), on the CPU: built
// from that file, csrc/locate_plan.cpp, csrc/codes.cpp and csrc/gf.cpp with no ROCm include path
// (tests/test_locate2_plan_native.py).
//
// Codes: RS(2,4) (15 pairs, 30 rows, 4 tiles), RS(3,5) (28 pairs of 3 rows straddling the 8-row
// tiles), RS(2,8) (45 pairs of 6 rows, 34 tiles) and RS(12,4) (120 pairs, 30 tiles).  Asserted per
// code: the plan's sizes; that every tile has exactly m records in syndrome order with no mask bit
// at or above its row count; that the rows are pair after pair in lexicographic order, m - 2 each,
// the tile records naming suspect n + p and `members` the pair; and that the interpreter, with the
// wave shortcut and without it, equals a direct search for (a, c) with S(b) = a * H_i ^ c * H_j (and
// for c with S(b) = c * H_j for the single suspects), written here with the field's multiply and
// divide alone, over random syndromes and the syndromes of one, two and three corrupt columns -- at one byte, at
// bytes of one 1 KiB span and of different spans.  The refusals m = 3, m = 9, n = 65, null pointers
// and a matrix with three dependent columns leave *out untouched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../repair-pipelining_amd/csrc/codes.hpp"
#include "../../repair-pipelining_amd/csrc/gf.hpp"
#include "../../repair-pipelining_amd/csrc/locate2_plan.hpp"

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

// H[q][j] of H = [P | I]
static uint8_t h_at(const std::vector<uint8_t> &parity, int k, int q, int j) {
    return j < k ? parity[(size_t)q * k + j] : (uint8_t)(j - k == q ? 1 : 0);
}

// true when there is a scalar c with v = c * H_j
static bool multiple_of(const std::vector<uint8_t> &parity, int k, int m, const uint8_t *v, int j) {
    const Field &f = Field::get();
    int q0 = 0;
    while (h_at(parity, k, q0, j) == 0) ++q0;  // a column of H is never zero
    const uint8_t c = f.div(v[q0], h_at(parity, k, q0, j));  // the only c that fits row q0
    for (int q = 0; q < m; ++q)
        if (f.mul(c, h_at(parity, k, q, j)) != v[q]) return false;
    return true;
}

// suspect[j] = 1 when S(b) = c * H_j has a solution at every b; suspect[n + p] = 1 when
// S(b) = a * H_i ^ c * H_j has one at every b (S(b) = 0 has a = c = 0: such bytes are skipped)
static std::vector<uint8_t> direct(const std::vector<uint8_t> &parity, int k, int m, const std::vector<uint8_t> &syn,
                                   int64_t len) {
    const Field &f = Field::get();
    const int n = k + m;
    std::vector<uint8_t> out((size_t)(n + n * (n - 1) / 2), 1);
    for (int64_t b = 0; b < len; ++b) {
        uint8_t s[8], v[8], any = 0;
        for (int q = 0; q < m; ++q) any |= (s[q] = syn[(size_t)(q * len + b)]);
        if (!any) continue;
        for (int j = 0; j < n; ++j)
            if (!multiple_of(parity, k, m, s, j)) out[(size_t)j] = 0;
        int p = 0;
        for (int i = 0; i < n; ++i) {
            for (int j = i + 1; j < n; ++j, ++p) {
                if (!out[(size_t)(n + p)]) continue;
                bool found = false;
                for (int a = 0; a < 256 && !found; ++a) {
                    for (int q = 0; q < m; ++q) v[q] = s[q] ^ f.mul((uint8_t)a, h_at(parity, k, q, i));
                    found = multiple_of(parity, k, m, v, j);
                }
                if (!found) out[(size_t)(n + p)] = 0;
            }
        }
    }
    return out;
}

static void check_structure(const Locate2Plan &p, int k, int m) {
    const int n = k + m, pairs = n * (n - 1) / 2, rows = pairs * (m - 2);
    REQUIRE(p.k == k && p.m == m && p.n_pairs == pairs);
    REQUIRE(p.n_tiles == (rows + kLocateTileRows - 1) / kLocateTileRows);
    REQUIRE(p.entries.size() == (size_t)p.n_tiles * m * kLocateEntryDwords);
    REQUIRE(p.tiles.size() == (size_t)p.n_tiles * kLocateTileDwords);
    REQUIRE(p.suspect.size() == (size_t)rows && p.members.size() == (size_t)pairs * 2);
    for (int r = 0; r < rows; ++r) REQUIRE(p.suspect[(size_t)r] == n + r / (m - 2));
    int q = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j, ++q) {
            REQUIRE(p.members[(size_t)2 * q] == i && p.members[(size_t)2 * q + 1] == j);
            REQUIRE(pair_index(n, i, j) == q);
        }
    for (int t = 0; t < p.n_tiles; ++t) {
        const uint32_t *tile = p.tiles.data() + (size_t)t * kLocateTileDwords;
        const int nr = std::min(kLocateTileRows, rows - t * kLocateTileRows);
        REQUIRE(tile[0] == (uint32_t)(t * m) && tile[1] == (uint32_t)m && tile[2] == (uint32_t)nr);
        for (int r = 0; r < kLocateTileRows; ++r)
            REQUIRE(tile[4 + r] == (r < nr ? (uint32_t)p.suspect[(size_t)(t * kLocateTileRows + r)] : 0u));
        uint32_t used = 0;
        for (int s = 0; s < m; ++s) {
            const uint32_t *rec = p.entries.data() + ((size_t)t * m + s) * kLocateEntryDwords;
            REQUIRE(rec[0] == (uint32_t)s && rec[3] == 0u);
            REQUIRE(((rec[1] | rec[2]) >> nr) == 0u && (rec[1] & rec[2]) == 0u);
            used |= rec[1] | rec[2];
        }
        REQUIRE(used == (1u << nr) - 1u);  // every row of the tile reads a syndrome
    }
}

static void check_code(int k, int m, int expect_pairs, int expect_tiles) {
    const RsCode code(k, m);
    const Field &f = Field::get();
    const int n = k + m;
    const int64_t len = 2 * kLocate2SpanBytes + 13;  // three spans, the last a short one
    std::vector<uint8_t> parity;
    for (int q = 0; q < m; ++q) parity.insert(parity.end(), code.parity_row(q), code.parity_row(q) + k);
    Locate2Plan plan;
    LocatePlan single;
    REQUIRE(build_locate2_plan(parity.data(), k, m, &plan));
    REQUIRE(build_locate_plan(parity.data(), k, m, &single));
    REQUIRE(plan.n_pairs == expect_pairs && plan.n_tiles == expect_tiles);
    check_structure(plan, k, m);
    const int width = n + plan.n_pairs;

    struct Err { int shard; int64_t byte; uint8_t value; };
    // the shortcut on and off and the direct search agree; returns the answer
    auto run_syn = [&](const std::vector<uint8_t> &syn, int64_t l) {
        std::vector<uint8_t> on((size_t)width, 0xEE), off((size_t)width, 0xEE);
        REQUIRE(emulate_locate2(plan, single, syn.data(), l, l, on.data(), true));
        REQUIRE(emulate_locate2(plan, single, syn.data(), l, l, off.data(), false));
        REQUIRE(on == off);
        REQUIRE(on == direct(parity, k, m, syn, l));
        return on;
    };
    auto run = [&](const std::vector<Err> &errs) {
        std::vector<uint8_t> syn((size_t)(m * len), 0);  // S(b) = the sum of e_j(b) * H_j
        for (const Err &e : errs)
            for (int q = 0; q < m; ++q) syn[(size_t)(q * len + e.byte)] ^= f.mul(e.value, h_at(parity, k, q, e.shard));
        return run_syn(syn, len);
    };
    auto count = [&](const std::vector<uint8_t> &s, int from, int to) {
        int c = 0;
        for (int x = from; x < to; ++x) c += s[(size_t)x];
        return c;
    };
    std::mt19937 rng(2000u * (unsigned)k + (unsigned)m);
    auto value = [&] { return (uint8_t)(1 + rng() % 255); };

    {  // clean: everybody stays a suspect
        const std::vector<uint8_t> s = run({});
        REQUIRE(count(s, 0, width) == width);
    }
    for (int rep = 0; rep < 3; ++rep) {  // random syndromes, 9 bytes
        std::vector<uint8_t> syn((size_t)(m * 9));
        for (uint8_t &v : syn) v = (uint8_t)rng();
        run_syn(syn, 9);
    }
    for (int j = 0; j < n; ++j) {  // one column, in two spans: suspect j and the n - 1 pairs with j
        const std::vector<uint8_t> s = run({{j, (7 * j) % kLocate2SpanBytes, value()}, {j, len - 1 - j % 13, value()}});
        REQUIRE(count(s, 0, n) == 1 && s[(size_t)j] == 1 && count(s, n, width) == n - 1);
        for (int o = 0; o < n; ++o)
            if (o != j) REQUIRE(s[(size_t)(n + pair_index(n, std::min(o, j), std::max(o, j)))] == 1);
    }
    for (int i = 0; i < n; ++i) {  // two columns: no single suspect and exactly the pair
        for (int j = i + 1; j < n; ++j) {
            const int64_t b = (i * 31 + j) % kLocate2SpanBytes;
            const int where = (i + j) % 3;  // the same byte; one span; two spans (two shortcut waves)
            const int64_t b2 = where == 0 ? b : (where == 1 ? (b + 5) % kLocate2SpanBytes : kLocate2SpanBytes + b);
            const std::vector<uint8_t> s = run({{i, b, value()}, {j, b2, value()}});
            REQUIRE(count(s, 0, n) == 0 && count(s, n, width) == 1 && s[(size_t)(n + pair_index(n, i, j))] == 1);
        }
    }
    for (int rep = 0; rep < 2 * n; ++rep) {  // three columns at one byte: whatever the search says
        int a = (int)(rng() % (unsigned)n), b = (int)(rng() % (unsigned)n), c = (int)(rng() % (unsigned)n);
        if (a == b || b == c || a == c) continue;
        const std::vector<uint8_t> s = run({{a, 40, value()}, {b, 40, value()}, {c, 40, value()}});
        REQUIRE(count(s, 0, n) == 0);  // distance m + 1 >= 5: three errors never look like one
    }
    {  // plans that break their invariants are refused
        std::vector<uint8_t> got((size_t)width, 0);
        const std::vector<uint8_t> syn((size_t)(m * len), 0);
        Locate2Plan bad = plan;
        bad.entries[(size_t)kLocateEntryDwords] = 0;  // record 1 of tile 0 no longer names S_1
        REQUIRE(!emulate_locate2(bad, single, syn.data(), len, len, got.data(), true));
        bad = plan;
        bad.tiles[4] = 0;  // a row that names a single suspect
        REQUIRE(!emulate_locate2(bad, single, syn.data(), len, len, got.data(), true));
        bad = plan;
        bad.members[1] = (uint8_t)n;
        REQUIRE(!emulate_locate2(bad, single, syn.data(), len, len, got.data(), true));
        bad = plan;
        bad.members.pop_back();
        REQUIRE(!emulate_locate2(bad, single, syn.data(), len, len, got.data(), true));
        LocatePlan other;
        const RsCode oc(k + 1, m);
        std::vector<uint8_t> op;
        for (int q = 0; q < m; ++q) op.insert(op.end(), oc.parity_row(q), oc.parity_row(q) + k + 1);
        REQUIRE(build_locate_plan(op.data(), k + 1, m, &other));
        REQUIRE(!emulate_locate2(plan, other, syn.data(), len, len, got.data(), true));
    }
}

static std::vector<uint8_t> parity_of(int k, int m) {
    const RsCode c(k, m);
    std::vector<uint8_t> p;
    for (int q = 0; q < m; ++q) p.insert(p.end(), c.parity_row(q), c.parity_row(q) + k);
    return p;
}

static void check_refusals() {
    Locate2Plan out;
    out.k = 77;
    const std::vector<uint8_t> p3 = parity_of(4, 3), p9 = parity_of(4, 9), p65 = parity_of(61, 4), ok = parity_of(2, 4);
    REQUIRE(!build_locate2_plan(p3.data(), 4, 3, &out));
    REQUIRE(!build_locate2_plan(p9.data(), 4, 9, &out));
    REQUIRE(!build_locate2_plan(p65.data(), 61, 4, &out));
    REQUIRE(!build_locate2_plan(ok.data(), 0, 4, &out));
    REQUIRE(!build_locate2_plan(nullptr, 2, 4, &out));
    REQUIRE(!build_locate2_plan(ok.data(), 2, 4, nullptr));
    // H_0 = (1, 1, 0, 0) = I_0 ^ I_1: three dependent columns, though any two are independent
    const std::vector<uint8_t> dep = {1, 1, 1, 2, 0, 3, 0, 4};  // rows (1,1) (1,2) (0,3) (0,4)
    REQUIRE(!build_locate2_plan(dep.data(), 2, 4, &out));
    REQUIRE(out.k == 77 && out.entries.empty());
    REQUIRE(build_locate2_plan(ok.data(), 2, 4, &out) && out.k == 2);
    const std::vector<uint8_t> p60 = parity_of(60, 4);  // n = 64 is the widest accepted
    REQUIRE(build_locate2_plan(p60.data(), 60, 4, &out) && out.n_pairs == 2016);
}

int main() {
    check_code(2, 4, 15, 4);
    check_code(3, 5, 28, 11);
    check_code(2, 8, 45, 34);
    check_code(12, 4, 120, 30);
    check_refusals();
    std::printf("locate2_plan_check: ok (%ld checks)\n", g_checks);
    return 0;
}
