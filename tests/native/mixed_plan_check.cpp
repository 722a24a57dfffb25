// mixed_plan_check.cpp -- the device plan of a pattern set (csrc/mixed_plan.cpp) with one tile per
// pattern, the form the in-place RS kernels read, on the CPU: built from that file and csrc/gf.cpp
// (the field's tables) with no ROCm include path (tests/test_mixed_plan_native.py;
// tests/native/tiled_plan_check.cpp has the plans of several tiles).
//
// Synthetic single-tile maps of 1, 3, 4, 12 and 17 entries (and one with no rows) are compiled
// into sets at load-ring depths 4 and 8.  Asserted: every record's rebased first index and padded
// count; that padding entries name kDummySlot with zero masks and nothing else does; that the
// records past npatterns are empty; that the interpreter over pattern id p equals both the
// interpreter over that pattern's own padded plan and the map computed directly in GF(2^8); that
// an id without a pattern, and an empty pattern, write nothing; duplicates; 256 patterns; the
// depth rule; and the refusals.
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

// A synthetic single-tile map: `count` inputs in slots chosen from [0, kSlots), `rows` outputs in
// other slots, random coefficients (0, 1 and general).  Its entry array starts `lead` junk
// entries in, so the record's first-entry index is not 0 before it is rebased.
constexpr int kSlots = 32;
struct Pattern {
    int count = 0, rows = 0, lead = 0;
    std::vector<int> in_slot, out_slot;
    std::vector<uint8_t> coef;  // [rows][count]
    std::vector<uint32_t> entries;
    uint32_t tile[kMixedTileDwords] = {0};
    // (a map without rows still has one record, of zeros)
    TiledPatternIn in() const { return TiledPatternIn{entries.data(), tile, 1}; }
};

static Pattern make_pattern(int count, int rows, int lead, std::mt19937_64 &rng) {
    Pattern p;
    p.count = count;
    p.rows = rows;
    p.lead = lead;
    std::vector<int> slots(kSlots);
    for (int i = 0; i < kSlots; ++i) slots[i] = i;
    for (int i = kSlots - 1; i > 0; --i) std::swap(slots[i], slots[rng() % (uint64_t)(i + 1)]);
    p.in_slot.assign(slots.begin(), slots.begin() + count);
    p.out_slot.assign(slots.begin() + count, slots.begin() + count + rows);
    p.coef.resize((size_t)rows * count);
    p.entries.assign((size_t)lead * kMixedEntryDwords, 0xDEADBEEFu);
    for (int j = 0; j < count; ++j) {
        uint32_t rec[kMixedEntryDwords] = {0};
        rec[0] = (uint32_t)p.in_slot[j];
        for (int r = 0; r < rows; ++r) {
            const uint64_t pick = rng() % 8;
            // every input keeps a coefficient in row 0, so no entry is all zero
            uint8_t c = pick == 0 && r > 0 ? 0 : (pick == 1 ? 1 : (uint8_t)(2 + rng() % 254));
            p.coef[(size_t)r * count + j] = c;
            if (c == 1) rec[2] |= 1u << r;
            else if (c) {
                rec[1] |= 1u << r;
                split_tables(c, rec + 4 + 5 * r);
            }
        }
        p.entries.insert(p.entries.end(), rec, rec + kMixedEntryDwords);
    }
    if (p.entries.empty()) p.entries.assign(kMixedEntryDwords, 0u);  // as CompiledMap keeps an empty map
    p.tile[0] = rows ? (uint32_t)lead : 0u;
    p.tile[1] = (uint32_t)count;
    p.tile[2] = (uint32_t)rows;
    p.tile[3] = (uint32_t)count;
    for (int r = 0; r < rows; ++r) p.tile[4 + r] = (uint32_t)p.out_slot[r];
    return p;
}

// the map computed directly in GF(2^8) over a [slot][len] stripe, outputs into `out`
static void direct(const Pattern &p, const uint8_t *in, uint8_t *out, int64_t len) {
    const Field &f = Field::get();
    std::vector<uint8_t> acc((size_t)p.rows * len, 0);
    for (int r = 0; r < p.rows; ++r)
        for (int j = 0; j < p.count; ++j)
            for (int64_t i = 0; i < len; ++i)
                acc[(size_t)r * len + i] ^= f.mul(p.coef[(size_t)r * p.count + j], in[(int64_t)p.in_slot[j] * len + i]);
    for (int r = 0; r < p.rows; ++r)
        for (int64_t i = 0; i < len; ++i) out[(int64_t)p.out_slot[r] * len + i] = acc[(size_t)r * len + i];
}

static void check_set(const std::vector<Pattern> &pats, int depth, std::mt19937_64 &rng) {
    std::vector<TiledPatternIn> ins;
    for (const Pattern &p : pats) ins.push_back(p.in());
    TiledPlan plan;
    REQUIRE(build_tiled_plan(ins.data(), (int)ins.size(), depth, &plan));
    REQUIRE(plan.npatterns == (int)pats.size() && plan.depth == depth && plan.tiles_per_pattern == 1);
    REQUIRE(plan.tiles.size() == (size_t)kMixedRecords * kMixedTileDwords);
    REQUIRE(plan.entries.size() % kMixedEntryDwords == 0 && !plan.entries.empty());

    // records: rebased first index, padded count, rows and output slots; padding entries
    uint32_t next = 0;
    int max_rows = 0;
    std::vector<char> is_padding(plan.entries.size() / kMixedEntryDwords, 0);
    for (size_t p = 0; p < pats.size(); ++p) {
        const uint32_t *tile = plan.tiles.data() + p * kMixedTileDwords;
        const uint32_t padded = (uint32_t)((pats[p].count + depth - 1) / depth * depth);
        REQUIRE(tile[0] == next);
        REQUIRE(tile[1] == padded && tile[1] % (uint32_t)depth == 0);
        REQUIRE(tile[2] == (uint32_t)pats[p].rows);
        for (int r = 0; r < pats[p].rows; ++r) REQUIRE(tile[4 + r] == (uint32_t)pats[p].out_slot[r]);
        REQUIRE(((size_t)tile[0] + tile[1]) * kMixedEntryDwords <= plan.entries.size());
        for (uint32_t e = 0; e < padded; ++e) {
            const uint32_t *rec = plan.entries.data() + ((size_t)next + e) * kMixedEntryDwords;
            if (e < (uint32_t)pats[p].count) {
                const uint32_t *src = pats[p].entries.data() + ((size_t)pats[p].lead + e) * kMixedEntryDwords;
                for (int d = 0; d < kMixedEntryDwords; ++d) REQUIRE(rec[d] == src[d]);
                REQUIRE(rec[0] != kMixedDummySlot);
            } else {
                is_padding[next + e] = 1;
                REQUIRE(rec[0] == kMixedDummySlot);
                for (int d = 1; d < kMixedEntryDwords; ++d) REQUIRE(rec[d] == 0u);
            }
        }
        next += padded;
        max_rows = pats[p].rows > max_rows ? pats[p].rows : max_rows;
    }
    REQUIRE(plan.max_rows == max_rows);
    REQUIRE(plan.entries.size() == (size_t)(next ? next : 1) * kMixedEntryDwords);
    for (size_t e = 0; e < is_padding.size(); ++e)
        if (!is_padding[e] && next) REQUIRE(plan.entries[e * kMixedEntryDwords] != kMixedDummySlot);
    for (size_t p = pats.size(); p < (size_t)kMixedRecords; ++p)
        for (int d = 0; d < kMixedTileDwords; ++d) REQUIRE(plan.tiles[p * kMixedTileDwords + d] == 0u);

    // the interpreter, per id, over an odd length
    const int64_t len = 37;
    std::vector<uint8_t> stripe((size_t)kSlots * len);
    for (uint8_t &b : stripe) b = (uint8_t)rng();
    for (int id = 0; id < kMixedRecords; ++id) {
        if (id >= (int)pats.size() && id != (int)pats.size() && id != 255) continue;  // the first empty id and 255
        std::vector<uint8_t> got = stripe;
        REQUIRE(emulate_tiled(plan, (uint8_t)id, stripe.data(), got.data(), len));
        std::vector<uint8_t> want = stripe;
        if (id < (int)pats.size()) {
            direct(pats[id], stripe.data(), want.data(), len);
            // the pattern's own padded plan: a set of that one pattern, record 0
            TiledPlan own;
            const TiledPatternIn one = pats[id].in();
            REQUIRE(build_tiled_plan(&one, 1, depth, &own));
            std::vector<uint8_t> alone = stripe;
            REQUIRE(emulate_tiled(own, 0, stripe.data(), alone.data(), len));
            REQUIRE(alone == got);
        }
        REQUIRE(got == want);  // inputs and every other slot untouched, outputs as computed
    }
}

int main() {
    std::mt19937_64 rng(20240611);
    const int counts[] = {1, 3, 4, 12, 17};
    for (int depth : {4, 8}) {
        // each count alone, over 1..8 rows
        for (int c : counts)
            for (int rows : {1, 2, 4, 8}) check_set({make_pattern(c, rows, 0, rng)}, depth, rng);
        // all of them in one set, with an empty pattern in the middle and non-zero first indices
        std::vector<Pattern> all;
        int lead = 0;
        for (int c : counts) {
            all.push_back(make_pattern(c, 1 + (int)(rng() % 8), lead++, rng));
            if (c == 4) all.push_back(make_pattern(0, 0, 0, rng));
        }
        check_set(all, depth, rng);
        // duplicates: the same pattern listed twice (and a third time at the end)
        std::vector<Pattern> dup = {all[0], all[4], all[4], all[1], all[0]};
        check_set(dup, depth, rng);
        // 256 patterns: every record taken
        std::vector<Pattern> full;
        for (int p = 0; p < kMixedRecords; ++p) full.push_back(make_pattern(counts[p % 5], 1 + p % 8, p % 3, rng));
        check_set(full, depth, rng);
    }

    // the depth rule: 8 only if every non-empty pattern has at least 12 entries
    {
        const Pattern p1 = make_pattern(1, 1, 0, rng), p12 = make_pattern(12, 4, 0, rng), p17 = make_pattern(17, 3, 2, rng),
                      p11 = make_pattern(11, 2, 0, rng), p0 = make_pattern(0, 0, 0, rng);
        auto depth_of = [](std::vector<const Pattern *> v) {
            std::vector<TiledPatternIn> ins;
            for (const Pattern *p : v) ins.push_back(p->in());
            return tiled_depth(ins.data(), (int)ins.size());
        };
        REQUIRE(depth_of({&p12, &p17}) == 8);
        REQUIRE(depth_of({&p12, &p0, &p17}) == 8);
        REQUIRE(depth_of({&p12, &p11}) == 4);
        REQUIRE(depth_of({&p1, &p17}) == 4);
        REQUIRE(depth_of({&p0}) == 4);
    }

    // refusals leave *out untouched
    {
        const Pattern p = make_pattern(3, 2, 0, rng);
        const TiledPatternIn one = p.in();
        TiledPlan plan;
        plan.npatterns = -7;
        REQUIRE(!build_tiled_plan(&one, 0, 4, &plan));
        REQUIRE(!build_tiled_plan(&one, kMixedRecords + 1, 4, &plan));
        REQUIRE(!build_tiled_plan(&one, 1, 0, &plan));
        REQUIRE(!build_tiled_plan(nullptr, 1, 4, &plan));
        const TiledPatternIn no_tiles{p.entries.data(), nullptr, 1};
        REQUIRE(!build_tiled_plan(&no_tiles, 1, 4, &plan));
        Pattern wide = p;
        wide.tile[2] = kMixedTileRows + 1;
        const TiledPatternIn w = wide.in();
        REQUIRE(!build_tiled_plan(&w, 1, 4, &plan));
        REQUIRE(plan.npatterns == -7 && plan.tiles.empty());
        // the interpreter refuses a record that is not padded to the plan's depth
        REQUIRE(build_tiled_plan(&one, 1, 4, &plan));
        plan.depth = 8;
        std::vector<uint8_t> s((size_t)kSlots * 4, 1), o = s;
        REQUIRE(!emulate_tiled(plan, 0, s.data(), o.data(), 4));
        REQUIRE(emulate_tiled(plan, 9, s.data(), o.data(), 4) && o == s);
    }
    std::printf("mixed_plan_check: ok (%ld checks)\n", g_checks);
    return 0;
}
