// tiled_plan_check.cpp -- the tiled plan of a pattern set (csrc/mixed_plan.cpp build_tiled_plan,
// emulate_tiled), on the CPU: built from that file and csrc/gf.cpp with no ROCm include path
// (tests/test_tiled_plan_native.py).
//
// Synthetic maps of 0..8 tiles (the last tile of one of them has a single row) are compiled into
// sets of T = 1, 2, 4 and 8 tiles per pattern at load-ring depths 4, 8 and 20.  Asserted: every
// record's rebased first index and padded count (tests/native/mixed_plan_check.cpp has the T = 1
// plan dword by dword); that padding entries name kDummySlot with zero masks and nothing else does; that every
// (id byte, tile) pair names a record inside exact-size arrays and that the records without a
// tile are empty; that the out-of-place interpreter equals the map computed directly in GF(2^8),
// leaves its input alone and writes only the pattern's output slots; max_out_slot, the depth
// rule and the refusals.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../repair-pipelining_amd/csrc/gf.hpp"
#include "../../repair-pipelining_amd/csrc/mixed_plan.hpp"

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

static uint32_t pack4(const uint8_t *t) {
    return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
}

// the five split-table dwords of coefficient c, as engine.hpp describes them
static void split_tables(uint8_t c, uint32_t *out) {
    const Field &f = Field::get();
    uint8_t lo[8], mid[8], hi[4];
    for (int v = 0; v < 8; ++v) {
        lo[v] = f.mul(c, (uint8_t)v);
        mid[v] = f.mul(c, (uint8_t)(v << 3));
    }
    for (int v = 0; v < 4; ++v) hi[v] = f.mul(c, (uint8_t)(v << 6));
    out[0] = pack4(lo);
    out[1] = pack4(lo + 4);
    out[2] = pack4(mid);
    out[3] = pack4(mid + 4);
    out[4] = pack4(hi);
}

// A synthetic map of `rows` output rows over kIn input slots, cut into tiles of kMixedTileRows
// rows as CompiledMap cuts it: tile t reads `counts[t]` of the inputs.  Outputs go to slots
// 0..rows-1 of a separate buffer.  The entry array starts with `lead` junk entries.
constexpr int kIn = 24;
struct Map {
    int rows = 0, n_tiles = 0;
    std::vector<uint8_t> coef;  // [rows][kIn]
    std::vector<uint32_t> entries, tiles;
    std::vector<int> counts;
    TiledPatternIn in() const { return TiledPatternIn{entries.data(), tiles.data(), n_tiles}; }
};

static Map make_map(int rows, const std::vector<int> &counts, int lead, std::mt19937_64 &rng) {
    Map m;
    m.rows = rows;
    m.counts = counts;
    m.n_tiles = (rows + kMixedTileRows - 1) / kMixedTileRows;
    REQUIRE((int)counts.size() == m.n_tiles);
    m.coef.assign((size_t)rows * kIn, 0);
    m.entries.assign((size_t)lead * kMixedEntryDwords, 0xDEADBEEFu);
    for (int t = 0; t < m.n_tiles; ++t) {
        const int r0 = t * kMixedTileRows, tr = std::min(kMixedTileRows, rows - r0);
        std::vector<int> slots(kIn);
        for (int i = 0; i < kIn; ++i) slots[i] = i;
        for (int i = kIn - 1; i > 0; --i) std::swap(slots[i], slots[rng() % (uint64_t)(i + 1)]);
        uint32_t tile[kMixedTileDwords] = {0};
        tile[0] = (uint32_t)(m.entries.size() / kMixedEntryDwords);
        tile[1] = tile[3] = (uint32_t)counts[t];
        tile[2] = (uint32_t)tr;
        for (int r = 0; r < tr; ++r) tile[4 + r] = (uint32_t)(r0 + r);
        for (int j = 0; j < counts[t]; ++j) {
            uint32_t rec[kMixedEntryDwords] = {0};
            rec[0] = (uint32_t)slots[j];
            for (int r = 0; r < tr; ++r) {
                const uint64_t pick = rng() % 8;
                const uint8_t c = pick == 0 && r > 0 ? 0 : (pick == 1 ? 1 : (uint8_t)(2 + rng() % 254));
                m.coef[(size_t)(r0 + r) * kIn + slots[j]] = c;
                if (c == 1) rec[2] |= 1u << r;
                else if (c) {
                    rec[1] |= 1u << r;
                    split_tables(c, rec + 4 + 5 * r);
                }
            }
            m.entries.insert(m.entries.end(), rec, rec + kMixedEntryDwords);
        }
        m.tiles.insert(m.tiles.end(), tile, tile + kMixedTileDwords);
    }
    if (m.entries.empty()) m.entries.assign(kMixedEntryDwords, 0u);
    if (m.tiles.empty()) m.tiles.assign(kMixedTileDwords, 0u);  // as CompiledMap keeps an empty map
    return m;
}

static void direct(const Map &m, const uint8_t *in, uint8_t *out, int64_t len) {
    const Field &f = Field::get();
    for (int r = 0; r < m.rows; ++r)
        for (int64_t i = 0; i < len; ++i) {
            uint8_t a = 0;
            for (int j = 0; j < kIn; ++j) a ^= f.mul(m.coef[(size_t)r * kIn + j], in[(int64_t)j * len + i]);
            out[(int64_t)r * len + i] = a;
        }
}

static void check_set(const std::vector<Map> &maps, int want_T, int depth, std::mt19937_64 &rng) {
    std::vector<TiledPatternIn> ins;
    for (const Map &m : maps) ins.push_back(m.in());
    TiledPlan plan;
    REQUIRE(build_tiled_plan(ins.data(), (int)ins.size(), depth, &plan));
    const int T = plan.tiles_per_pattern;
    REQUIRE(T == want_T && plan.npatterns == (int)maps.size() && plan.depth == depth);
    // exact-size copies: under AddressSanitizer a record or entry past the plan is a fault
    const std::vector<uint32_t> tiles(plan.tiles.begin(), plan.tiles.end());
    const std::vector<uint32_t> entries(plan.entries.begin(), plan.entries.end());
    REQUIRE(tiles.size() == (size_t)kMixedRecords * T * kMixedTileDwords);
    uint32_t next = 0;
    int max_rows = 0, max_out = -1;
    for (int id = 0; id < kMixedRecords; ++id)
        for (int t = 0; t < T; ++t) {
            const uint32_t *tile = tiles.data() + ((size_t)id * T + t) * kMixedTileDwords;
            const bool own = id < (int)maps.size() && t < maps[(size_t)id].n_tiles;
            if (!own) {
                // (a map without rows keeps one record of zeros, which is not its "own" tile here)
                REQUIRE(tile[1] == 0 && tile[2] == 0);
                continue;
            }
            const Map &m = maps[(size_t)id];
            const uint32_t count = (uint32_t)m.counts[(size_t)t];
            const uint32_t padded = (count + (uint32_t)depth - 1) / (uint32_t)depth * (uint32_t)depth;
            REQUIRE(tile[0] == next && tile[1] == padded);
            REQUIRE(tile[2] == m.tiles[(size_t)t * kMixedTileDwords + 2]);
            REQUIRE(((size_t)tile[0] + tile[1]) * kMixedEntryDwords <= entries.size());
            const uint32_t src0 = m.tiles[(size_t)t * kMixedTileDwords];
            for (uint32_t e = 0; e < padded; ++e) {
                const uint32_t *rec = entries.data() + ((size_t)tile[0] + e) * kMixedEntryDwords;
                if (e < count) {
                    REQUIRE(rec[0] != kMixedDummySlot);
                    REQUIRE(std::equal(rec, rec + kMixedEntryDwords,
                                       m.entries.data() + ((size_t)src0 + e) * kMixedEntryDwords));
                } else {
                    REQUIRE(rec[0] == kMixedDummySlot);
                    for (int d = 1; d < kMixedEntryDwords; ++d) REQUIRE(rec[d] == 0);
                }
            }
            next += padded;
            max_rows = std::max(max_rows, (int)tile[2]);
            for (uint32_t r = 0; r < tile[2]; ++r) max_out = std::max(max_out, (int)tile[4 + r]);
        }
    REQUIRE(entries.size() == (size_t)std::max<uint32_t>(next, 1) * kMixedEntryDwords);
    REQUIRE(plan.max_rows == max_rows && plan.max_out_slot == max_out);

    // the interpreter, out of place, for every id byte
    const int64_t len = 37;
    const int out_slots = std::max(max_out + 1, 1);
    std::vector<uint8_t> in((size_t)kIn * len), in0;
    for (uint8_t &b : in) b = (uint8_t)rng();
    in0 = in;
    for (int id = 0; id < kMixedRecords; ++id) {
        std::vector<uint8_t> out((size_t)out_slots * len, 0x5A), want((size_t)out_slots * len, 0x5A);
        REQUIRE(emulate_tiled(plan, (uint8_t)id, in.data(), out.data(), len));
        if (id < (int)maps.size()) direct(maps[(size_t)id], in.data(), want.data(), len);
        REQUIRE(out == want);  // also: slots past the pattern's own rows keep the sentinel
        REQUIRE(in == in0);
    }
}

int main() {
    std::mt19937_64 rng(20240607);
    const Map empty = make_map(0, {}, 0, rng);
    const Map one20 = make_map(8, {20}, 3, rng);
    const Map one20b = make_map(8, {20}, 0, rng);
    const Map small = make_map(3, {5}, 1, rng);
    const Map two = make_map(16, {20, 20}, 2, rng);
    const Map ragged = make_map(9, {12, 1}, 0, rng);  // the last tile has one row (and one entry)
    const Map four = make_map(32, {7, 13, 24, 4}, 5, rng);
    const Map three = make_map(20, {9, 17, 3}, 0, rng);
    const Map eight = make_map(64, {24, 1, 8, 20, 21, 12, 4, 16}, 1, rng);
    const Map seven = make_map(50, {3, 3, 3, 3, 3, 3, 2}, 0, rng);

    for (int depth : {4, 8, 20}) {
        // T = 1: one record per id, the interpreter over single-tile maps
        {
            const std::vector<Map> maps = {one20, empty, small, one20b, small};
            std::vector<TiledPatternIn> tin;
            for (const Map &m : maps)
                tin.push_back(TiledPatternIn{m.entries.data(), m.tiles.data(), std::max(1, m.n_tiles)});
            TiledPlan tp;
            REQUIRE(build_tiled_plan(tin.data(), (int)tin.size(), depth, &tp));
            REQUIRE(tp.tiles_per_pattern == 1 && tp.tiles.size() == (size_t)kMixedRecords * kMixedTileDwords);
            REQUIRE(tp.max_rows == 8 && tp.npatterns == (int)maps.size());
            std::vector<uint8_t> in((size_t)kIn * 16), a((size_t)8 * 16, 1), b((size_t)8 * 16, 1);
            for (uint8_t &x : in) x = (uint8_t)rng();
            for (int id : {0, 1, 2, 3, 4, 5, 255}) {
                REQUIRE(emulate_tiled(tp, (uint8_t)id, in.data(), a.data(), 16));
                std::fill(b.begin(), b.end(), 1);
                if (id < (int)maps.size()) direct(maps[(size_t)id], in.data(), b.data(), 16);
                REQUIRE(a == b);
                std::fill(a.begin(), a.end(), 1);
            }
        }
        check_set({one20, one20b, one20}, 1, depth, rng);
        check_set({one20, empty, small}, 1, depth, rng);
        check_set({one20, two, empty, one20b}, 2, depth, rng);
        check_set({ragged, small, ragged}, 2, depth, rng);
        check_set({four, ragged, one20, empty, three, two}, 4, depth, rng);
        check_set({eight, small, seven, ragged, four, empty}, 8, depth, rng);
    }
    {  // 256 patterns, every id byte used
        std::vector<Map> maps;
        for (int i = 0; i < kMixedRecords; ++i) maps.push_back(i % 3 ? one20 : two);
        check_set(maps, 2, 4, rng);
    }
    {  // the depth rule, and a tile of exactly the depth takes no padding
        std::vector<TiledPatternIn> ins = {one20.in(), one20b.in(), empty.in()};
        TiledPlan p;
        REQUIRE(build_tiled_plan(ins.data(), 3, 20, &p));
        for (int id = 0; id < 2; ++id) REQUIRE(p.tiles[(size_t)id * kMixedTileDwords + 1] == 20);  // no padding
        REQUIRE(tiled_depth(ins.data(), 3) == 8);
        ins.push_back(two.in());
        REQUIRE(build_tiled_plan(ins.data(), 4, 4, &p) && p.tiles_per_pattern == 2);
        REQUIRE(tiled_depth(ins.data(), 4) == 8);
        ins.push_back(ragged.in());
        REQUIRE(build_tiled_plan(ins.data(), 5, 4, &p));
        REQUIRE(tiled_depth(ins.data(), 5) == 4);  // a tile of one entry
        ins = {empty.in()};
        REQUIRE(tiled_depth(ins.data(), 1) == 4);
        REQUIRE(build_tiled_plan(ins.data(), 1, 8, &p) && p.max_rows == 0 && p.max_out_slot == -1);
        REQUIRE(p.entries.size() == (size_t)kMixedEntryDwords && p.tiles_per_pattern == 1);
    }
    {  // the refusals leave *out untouched
        TiledPlan p;
        p.npatterns = 77;
        std::vector<TiledPatternIn> ins = {one20.in()};
        REQUIRE(!build_tiled_plan(nullptr, 1, 4, &p));
        REQUIRE(!build_tiled_plan(ins.data(), 1, 4, nullptr));
        REQUIRE(!build_tiled_plan(ins.data(), 0, 4, &p));
        REQUIRE(!build_tiled_plan(ins.data(), 1, 0, &p));
        std::vector<TiledPatternIn> many((size_t)kMixedRecords + 1, one20.in());
        REQUIRE(!build_tiled_plan(many.data(), kMixedRecords + 1, 4, &p));
        const Map nine = make_map(72, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 0, rng);
        ins = {nine.in()};
        REQUIRE(!build_tiled_plan(ins.data(), 1, 4, &p));
        Map tall = one20;
        tall.tiles[2] = kMixedTileRows + 1;
        ins = {tall.in()};
        REQUIRE(!build_tiled_plan(ins.data(), 1, 4, &p));
        ins = {TiledPatternIn{nullptr, one20.tiles.data(), 1}};
        REQUIRE(!build_tiled_plan(ins.data(), 1, 4, &p));
        REQUIRE(p.npatterns == 77);
        // a plan that breaks its invariants is refused by the interpreter
        ins = {two.in()};
        REQUIRE(build_tiled_plan(ins.data(), 1, 4, &p));
        std::vector<uint8_t> in((size_t)kIn * 8, 3), out((size_t)16 * 8);
        REQUIRE(emulate_tiled(p, 0, in.data(), out.data(), 8));
        TiledPlan bad = p;
        bad.tiles[kMixedTileDwords + 1] += 1;  // tile 1: not a multiple of the depth
        REQUIRE(!emulate_tiled(bad, 0, in.data(), out.data(), 8));
        bad = p;
        bad.tiles.pop_back();
        REQUIRE(!emulate_tiled(bad, 0, in.data(), out.data(), 8));
        bad = p;
        bad.tiles[kMixedTileDwords] = (uint32_t)(p.entries.size() / kMixedEntryDwords);  // entries outside the array
        REQUIRE(!emulate_tiled(bad, 0, in.data(), out.data(), 8));
    }
    std::printf("tiled_plan_check: ok (%ld checks)\n", g_checks);
    return 0;
}
