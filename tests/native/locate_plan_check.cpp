// locate_plan_check.cpp -- the locate plan of an RS code (csrc/locate_plan.cpp), on the CPU: built
// from that file, csrc/codes.cpp and csrc/gf.cpp with no ROCm include path
// (tests/test_locate_plan_native.py).
//
// Codes: RS(3,2) (the smallest accepted), RS(4,2) (m = 2), RS(17,3) (40 test rows in 5 tiles),
// RS(5,5) (tiles of 8 rows) and RS(10,8) (m = 8: 126 rows, 16 tiles).  Asserted per code: the
// plan's sizes; that every tile has exactly m records in syndrome order with no mask bit at or
// above its row count; that the row -> candidate table is candidate after candidate, m - 1 rows
// each, and the tile records repeat it; and that the interpreter, over the syndromes of a clean
// stripe, of one corrupt byte in each of the n shards, of two shards corrupt at different bytes and
// of one shard corrupt at two bytes, equals a direct evaluation of "S(b) is a multiple of column
// H_j at every b" written here with the field's multiply alone (the interpreter is handed
// exact-size buffers: the sanitizer build checks them).  The refusals m = 1, m = 9, k = 0, null
// pointers and a zero in parity row 0 leave *out untouched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../repair-pipelining_amd/csrc/codes.hpp"
#include "../../repair-pipelining_amd/csrc/gf.hpp"
#include "../../repair-pipelining_amd/csrc/locate_plan.hpp"

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

// suspect[j] = 1 when at every byte b there is a scalar c with S(b) = c * H_j (c = 0 for S(b) = 0)
static std::vector<uint8_t> direct(const std::vector<uint8_t> &parity, int k, int m,
                                   const std::vector<uint8_t> &syn, int64_t len) {
    const Field &f = Field::get();
    const int n = k + m;
    std::vector<uint8_t> out((size_t)n, 1);
    for (int j = 0; j < n; ++j) {
        for (int64_t b = 0; b < len && out[(size_t)j]; ++b) {
            bool any = false;
            for (int c = 0; c < 256 && !any; ++c) {
                bool all = true;
                for (int q = 0; q < m; ++q) all = all && f.mul((uint8_t)c, h_at(parity, k, q, j)) == syn[(size_t)(q * len + b)];
                any = all;
            }
            if (!any) out[(size_t)j] = 0;
        }
    }
    return out;
}

// the m syndromes [m][len] of a stripe [n][len]
static std::vector<uint8_t> syndromes(const std::vector<uint8_t> &parity, int k, int m,
                                      const std::vector<uint8_t> &stripe, int64_t len) {
    const Field &f = Field::get();
    std::vector<uint8_t> syn((size_t)(m * len), 0);
    for (int q = 0; q < m; ++q)
        for (int j = 0; j < k + m; ++j)
            for (int64_t b = 0; b < len; ++b)
                syn[(size_t)(q * len + b)] ^= f.mul(h_at(parity, k, q, j), stripe[(size_t)(j * len + b)]);
    return syn;
}

static void check_structure(const LocatePlan &p, int k, int m) {
    const int n = k + m, rows = n * (m - 1);
    REQUIRE(p.k == k && p.m == m);
    REQUIRE(p.n_tiles == (rows + kLocateTileRows - 1) / kLocateTileRows);
    REQUIRE(p.entries.size() == (size_t)p.n_tiles * m * kLocateEntryDwords);
    REQUIRE(p.tiles.size() == (size_t)p.n_tiles * kLocateTileDwords);
    REQUIRE(p.candidate.size() == (size_t)rows);
    for (int r = 0; r < rows; ++r) REQUIRE(p.candidate[(size_t)r] == r / (m - 1));
    for (int t = 0; t < p.n_tiles; ++t) {
        const uint32_t *tile = p.tiles.data() + (size_t)t * kLocateTileDwords;
        const int nr = std::min(kLocateTileRows, rows - t * kLocateTileRows);
        REQUIRE(tile[0] == (uint32_t)(t * m) && tile[1] == (uint32_t)m && tile[2] == (uint32_t)nr);
        for (int r = 0; r < kLocateTileRows; ++r)
            REQUIRE(tile[4 + r] == (r < nr ? (uint32_t)p.candidate[(size_t)(t * kLocateTileRows + r)] : 0u));
        uint32_t used = 0;
        for (int q = 0; q < m; ++q) {
            const uint32_t *rec = p.entries.data() + ((size_t)t * m + q) * kLocateEntryDwords;
            REQUIRE(rec[0] == (uint32_t)q && rec[3] == 0u);
            REQUIRE(((rec[1] | rec[2]) >> nr) == 0u && (rec[1] & rec[2]) == 0u);
            used |= rec[1] | rec[2];
        }
        REQUIRE(used == (1u << nr) - 1u);  // every row of the tile reads a syndrome
    }
}

static void check_code(int k, int m, int expect_rows, int expect_tiles) {
    const RsCode code(k, m);
    const int n = k + m;
    const int64_t len = 37;
    std::vector<uint8_t> parity;
    for (int q = 0; q < m; ++q) parity.insert(parity.end(), code.parity_row(q), code.parity_row(q) + k);
    LocatePlan plan;
    REQUIRE(build_locate_plan(parity.data(), k, m, &plan));
    REQUIRE((int)plan.candidate.size() == expect_rows && plan.n_tiles == expect_tiles);
    check_structure(plan, k, m);

    const Field &f = Field::get();
    std::mt19937 rng(1000u * (unsigned)k + (unsigned)m);
    std::vector<uint8_t> clean((size_t)(n * len), 0);
    for (int j = 0; j < k; ++j)
        for (int64_t b = 0; b < len; ++b) clean[(size_t)(j * len + b)] = (uint8_t)rng();
    for (int q = 0; q < m; ++q)
        for (int j = 0; j < k; ++j)
            for (int64_t b = 0; b < len; ++b)
                clean[(size_t)((k + q) * len + b)] ^= f.mul(parity[(size_t)q * k + j], clean[(size_t)(j * len + b)]);

    auto run = [&](const std::vector<uint8_t> &stripe, int expect_one) {
        const std::vector<uint8_t> syn = syndromes(parity, k, m, stripe, len);
        std::vector<uint8_t> got((size_t)n, 0xEE);
        REQUIRE(emulate_locate(plan, syn.data(), len, len, got.data()));
        const std::vector<uint8_t> want = direct(parity, k, m, syn, len);
        REQUIRE(got == want);
        int count = 0;
        for (uint8_t v : got) count += v;
        if (expect_one == -1) REQUIRE(count == n);       // clean: every shard is a suspect
        else if (expect_one >= 0) REQUIRE(count == 1 && got[(size_t)expect_one] == 1);
        else REQUIRE(count == 0);                        // -2: nobody
    };
    run(clean, -1);
    for (int j = 0; j < n; ++j) {  // one corrupt byte in each shard, at a position that moves
        std::vector<uint8_t> s = clean;
        s[(size_t)(j * len + (j * 7) % len)] ^= (uint8_t)(1 + rng() % 255);
        run(s, j);
    }
    for (int j = 0; j < n; ++j) {  // one shard corrupt at two bytes
        std::vector<uint8_t> s = clean;
        s[(size_t)(j * len)] ^= 0x80;
        s[(size_t)(j * len + len - 1)] ^= 0x01;
        run(s, j);
    }
    for (int j = 0; j < n; ++j) {  // two shards corrupt at different bytes
        std::vector<uint8_t> s = clean;
        const int j2 = (j + 1 + (int)(rng() % (unsigned)(n - 1))) % n;
        s[(size_t)(j * len + 3)] ^= (uint8_t)(1 + rng() % 255);
        s[(size_t)(j2 * len + 20)] ^= (uint8_t)(1 + rng() % 255);
        run(s, -2);
    }
    {  // no bytes at all: every shard stays a suspect
        std::vector<uint8_t> got((size_t)n, 0);
        REQUIRE(emulate_locate(plan, nullptr, 0, 0, got.data()));
        for (uint8_t v : got) REQUIRE(v == 1);
    }
    {  // a plan that breaks its invariants is refused
        LocatePlan bad = plan;
        bad.entries[(size_t)kLocateEntryDwords] = 0;  // record 1 of tile 0 no longer names S_1
        std::vector<uint8_t> got((size_t)n, 0);
        const std::vector<uint8_t> syn((size_t)(m * len), 0);
        REQUIRE(!emulate_locate(bad, syn.data(), len, len, got.data()));
        bad = plan;
        bad.tiles[2] = kLocateTileRows + 1;
        REQUIRE(!emulate_locate(bad, syn.data(), len, len, got.data()));
        bad = plan;
        bad.entries.pop_back();
        REQUIRE(!emulate_locate(bad, syn.data(), len, len, got.data()));
    }
}

static void check_refusals() {
    LocatePlan out;
    out.k = 77;
    const RsCode c1(4, 1), c9(4, 9), ok(4, 2);
    std::vector<uint8_t> p9;
    for (int q = 0; q < 9; ++q) p9.insert(p9.end(), c9.parity_row(q), c9.parity_row(q) + 4);
    REQUIRE(!build_locate_plan(c1.parity_row(0), 4, 1, &out));
    REQUIRE(!build_locate_plan(p9.data(), 4, 9, &out));
    REQUIRE(!build_locate_plan(p9.data(), 0, 2, &out));
    REQUIRE(!build_locate_plan(nullptr, 4, 2, &out));
    REQUIRE(!build_locate_plan(p9.data(), 4, 2, nullptr));
    REQUIRE(!build_locate_plan(p9.data(), 255, 2, &out));
    std::vector<uint8_t> zero(p9.begin(), p9.begin() + 8);
    zero[2] = 0;  // parity[0][2]
    REQUIRE(!build_locate_plan(zero.data(), 4, 2, &out));
    REQUIRE(out.k == 77 && out.entries.empty());
}

int main() {
    check_code(3, 2, 5, 1);
    check_code(4, 2, 6, 1);
    check_code(17, 3, 40, 5);
    check_code(5, 5, 40, 5);
    check_code(10, 8, 126, 16);
    check_code(12, 4, 48, 6);
    check_refusals();
    std::printf("locate_plan_check: ok (%ld checks)\n", g_checks);
    return 0;
}
