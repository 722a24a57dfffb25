// clay_partial_plan_check.cpp -- the partial-sum plan of a Clay pattern set
// (csrc/clay_partial_plan.cpp), on the CPU: built from that file, csrc/mixed_plan.cpp,
// csrc/codes.cpp and csrc/gf.cpp with no ROCm include path (tests/test_clay_partial_plan_native.py).
//
// Sets over Clay(4,2) (all 21 one- and two-node lists plus the empty list), Clay(2,2), Clay(3,3)
// and Clay(6,2) (single nodes, pairs, the empty list) are compiled from the planner's
// standard-null-pattern performCoding maps: tiled here as CompiledMap tiles them (engine.cpp: rows
// grouped greedily by shared inputs into tiles of 8, a tile's entries its non-zero columns in
// ascending order -- the order within a tile does not matter to anything checked here), through
// build_tiled_plan, then cut by node at depths 4 and 8.  Asserted: the plan's sizes; that every
// record keeps its tile's rows and output slots, has a padded count that is a multiple of the
// depth, plane numbers below alpha in its entries and kDummySlot with zero masks in its padding;
// that a list's records hold each entry of its tiles exactly once; that for every (list, node)
// the interpreter over random planes and a random accumulator equals the list's map restricted to
// that node's columns computed here directly in GF(2^8), assigning and accumulating, with guard
// bytes, gaps and the rows past the list's own left alone; that the XOR over all nodes equals the
// full map's output (emulate_tiled and the direct product); that every (id byte, node byte) pair
// stays inside exact-size arrays and writes nothing where nothing is to be written; and the
// refusals.  Printed per geometry: the largest per-record entry count.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../repair-pipelining_amd/csrc/clay_partial_plan.hpp"
#include "../../repair-pipelining_amd/csrc/codes.hpp"
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

// engine.cpp group_rows: seed each tile with the lowest unassigned row, then add the row with the
// most shared inputs (ties: fewest new inputs, then lowest index)
static std::vector<int> group_rows(const LinearMap &m) {
    std::vector<int> order;
    if (m.n_out <= kMixedTileRows) {
        for (int r = 0; r < m.n_out; ++r) order.push_back(r);
        return order;
    }
    std::vector<std::vector<int>> sup((size_t)m.n_out);
    for (int r = 0; r < m.n_out; ++r)
        for (int j = 0; j < m.n_in; ++j)
            if (m.at(r, j)) sup[(size_t)r].push_back(j);
    std::vector<char> used((size_t)m.n_out, 0), in_tile((size_t)m.n_in, 0);
    for (int seed = 0; seed < m.n_out; ++seed) {
        if (used[(size_t)seed]) continue;
        std::vector<int> tile = {seed};
        used[(size_t)seed] = 1;
        std::fill(in_tile.begin(), in_tile.end(), 0);
        for (int j : sup[(size_t)seed]) in_tile[(size_t)j] = 1;
        while ((int)tile.size() < kMixedTileRows) {
            int best = -1, best_shared = -1, best_new = 0;
            for (int r = 0; r < m.n_out; ++r) {
                if (used[(size_t)r]) continue;
                int shared = 0;
                for (int j : sup[(size_t)r]) shared += in_tile[(size_t)j];
                const int fresh = (int)sup[(size_t)r].size() - shared;
                if (shared - fresh > best_shared - best_new || best < 0) {
                    best = r;
                    best_shared = shared;
                    best_new = fresh;
                }
            }
            if (best < 0) break;
            used[(size_t)best] = 1;
            tile.push_back(best);
            for (int j : sup[(size_t)best]) in_tile[(size_t)j] = 1;
        }
        order.insert(order.end(), tile.begin(), tile.end());
    }
    return order;
}

// One list's map and its tile records and entries, as CompiledMap holds them.
struct Tiled {
    LinearMap map;
    std::vector<uint32_t> entries, tiles;
    int n_tiles = 0;
    TiledPatternIn in() const { return TiledPatternIn{entries.data(), tiles.data(), std::max(1, n_tiles)}; }
};

static Tiled tile_map(LinearMap lm) {
    Tiled t;
    t.map = std::move(lm);
    const LinearMap &m = t.map;
    const std::vector<int> order = group_rows(m);
    for (int r0 = 0; r0 < m.n_out; r0 += kMixedTileRows) {
        const int rows = std::min(kMixedTileRows, m.n_out - r0);
        uint32_t tile[kMixedTileDwords] = {0};
        tile[0] = (uint32_t)(t.entries.size() / kMixedEntryDwords);
        for (int j = 0; j < m.n_in; ++j) {
            uint32_t rec[kMixedEntryDwords] = {0};
            rec[0] = (uint32_t)m.in_slot[(size_t)j];
            for (int r = 0; r < rows; ++r) {
                const uint8_t c = m.at(order[(size_t)(r0 + r)], j);
                if (c == 1) rec[2] |= 1u << r;
                else if (c) {
                    rec[1] |= 1u << r;
                    split_tables(c, rec + 4 + 5 * r);
                }
            }
            if ((rec[1] | rec[2]) == 0) continue;
            t.entries.insert(t.entries.end(), rec, rec + kMixedEntryDwords);
            ++tile[1];
        }
        tile[2] = (uint32_t)rows;
        tile[3] = tile[1];
        for (int r = 0; r < rows; ++r) tile[4 + r] = (uint32_t)m.out_slot[(size_t)order[(size_t)(r0 + r)]];
        t.tiles.insert(t.tiles.end(), tile, tile + kMixedTileDwords);
        ++t.n_tiles;
    }
    if (t.entries.empty()) t.entries.assign(kMixedEntryDwords, 0u);
    if (t.tiles.empty()) t.tiles.assign(kMixedTileDwords, 0u);  // as CompiledMap keeps an empty map
    return t;
}

// The list's repair map for the standard null pattern (ecx_api.cpp clay_standard_map): the erased
// nodes' sub-chunks absent, every other one present; input slot z*n + node, output slot z*|E| + j.
static Tiled list_map(int k, int m, const std::vector<int> &erased) {
    if (erased.empty()) return tile_map(LinearMap());
    const ClayPlanner pl(k, m, erased);
    const int n = pl.n_real(), a = pl.alpha();
    std::vector<bool> present((size_t)n * a, true);
    for (int z = 0; z < a; ++z)
        for (int e : erased) present[(size_t)z * n + e] = false;
    return tile_map(pl.perform_coding_map(present));
}

static void check_geometry(int k, int m, const std::vector<std::vector<int>> &lists, std::mt19937_64 &rng) {
    const Field &f = Field::get();
    const int n = k + m, np = (int)lists.size();
    int alpha = 1;
    for (int i = 0; i < n / m; ++i) alpha *= m;
    std::vector<Tiled> maps;
    for (const std::vector<int> &e : lists) maps.push_back(list_map(k, m, e));
    std::vector<TiledPatternIn> ins;
    for (const Tiled &t : maps) ins.push_back(t.in());
    int max_rows_total = 0;
    for (const std::vector<int> &e : lists) max_rows_total = std::max(max_rows_total, (int)e.size() * alpha);
    int largest = 0;

    for (int depth : {4, 8}) {
        TiledPlan tiled;
        REQUIRE(build_tiled_plan(ins.data(), np, depth == 4 ? 8 : 4, &tiled));  // any depth: its padding is dropped
        ClayPartialPlan built;
        REQUIRE(build_clay_partial_plan(tiled, n, depth, &built));
        // exact-size copies: under AddressSanitizer a record or entry past the plan is a fault
        ClayPartialPlan plan = built;
        plan.tiles = std::vector<uint32_t>(built.tiles.begin(), built.tiles.end());
        plan.entries = std::vector<uint32_t>(built.entries.begin(), built.entries.end());
        const int T = plan.tiles_per_pattern;
        REQUIRE(T == tiled.tiles_per_pattern && plan.n == n && plan.npatterns == np && plan.depth == depth);
        REQUIRE(plan.tiles.size() == (size_t)kMixedRecords * n * T * kMixedTileDwords);  // 64 B per record
        REQUIRE(plan.max_rows == tiled.max_rows);
        int max_entries = 0, min_entries = 0x7FFFFFFF;
        for (int id = 0; id < kMixedRecords; ++id)
            for (int t = 0; t < T; ++t) {
                const uint32_t *src = tiled.tiles.data() + ((size_t)id * T + t) * kMixedTileDwords;
                uint32_t kept_sum = 0, real_in_tile = 0;
                for (uint32_t e = 0; e < src[1]; ++e)
                    real_in_tile += tiled.entries[((size_t)src[0] + e) * kMixedEntryDwords] != kMixedDummySlot;
                for (int i = 0; i < n; ++i) {
                    const uint32_t *tile = plan.tiles.data() + (((size_t)id * n + i) * T + t) * kMixedTileDwords;
                    if (src[2] == 0) {
                        REQUIRE(tile[1] == 0 && tile[2] == 0);
                        continue;
                    }
                    REQUIRE(id < np);
                    REQUIRE(tile[2] == src[2] && std::equal(tile + 4, tile + kMixedTileDwords, src + 4));
                    REQUIRE(tile[1] % (uint32_t)depth == 0 && tile[3] <= tile[1] && tile[1] - tile[3] < (uint32_t)depth);
                    REQUIRE(((size_t)tile[0] + tile[1]) * kMixedEntryDwords <= plan.entries.size());
                    for (uint32_t e = 0; e < tile[1]; ++e) {
                        const uint32_t *rec = plan.entries.data() + ((size_t)tile[0] + e) * kMixedEntryDwords;
                        if (e < tile[3]) {
                            REQUIRE(rec[0] < (uint32_t)alpha && ((rec[1] | rec[2]) >> tile[2]) == 0);
                        } else {
                            REQUIRE(rec[0] == kMixedDummySlot);
                            for (int d = 1; d < kMixedEntryDwords; ++d) REQUIRE(rec[d] == 0);
                        }
                    }
                    kept_sum += tile[3];
                    max_entries = std::max(max_entries, (int)tile[3]);
                    if (tile[3] > 0) min_entries = std::min(min_entries, (int)tile[3]);
                    const bool reads = std::find(lists[(size_t)id].begin(), lists[(size_t)id].end(), i) == lists[(size_t)id].end();
                    if (!reads) REQUIRE(tile[3] == 0);  // an erased node is never read
                }
                REQUIRE(kept_sum == real_in_tile);  // every entry of the tile in exactly one node's record
            }
        REQUIRE(plan.max_entries == max_entries);
        REQUIRE(plan.min_entries == (min_entries == 0x7FFFFFFF ? 0 : min_entries));
        REQUIRE(clay_partial_depth(plan) == (plan.min_entries >= 12 ? 8 : 4));
        largest = max_entries;

        // every (list, node): the interpreter against the node's columns computed directly, over an
        // odd length, planes and rows a stride apart, with guards and the rows past the list's own
        const int64_t len = 37, in_stride = 41, acc_stride = 43, guard = 5;
        const int acc_rows = std::max(max_rows_total, 1);
        std::vector<uint8_t> in((size_t)((alpha - 1) * in_stride + len));
        for (int p = 0; p < np; ++p) {
            const LinearMap &lm = maps[(size_t)p].map;
            const int rows = (int)lists[(size_t)p].size() * alpha;
            REQUIRE(lm.n_out == rows);
            // full input of one stripe, plane-major, for the sum over the nodes
            std::vector<uint8_t> full((size_t)n * alpha * len);
            for (uint8_t &b : full) b = (uint8_t)rng();
            std::vector<uint8_t> sum_first((size_t)(2 * guard + (acc_rows - 1) * acc_stride + len), 0xC3), sum_acc;
            for (int first = 1; first >= 0; --first) {
                std::vector<uint8_t> running((size_t)(2 * guard + (acc_rows - 1) * acc_stride + len));
                for (uint8_t &b : running) b = (uint8_t)rng();
                const std::vector<uint8_t> start = running;
                for (int i = 0; i < n; ++i) {
                    for (int z = 0; z < alpha; ++z)
                        std::copy(full.begin() + ((size_t)z * n + i) * len, full.begin() + ((size_t)z * n + i + 1) * len,
                                  in.begin() + (size_t)z * in_stride);
                    // this (list, node) alone, over a random accumulator
                    std::vector<uint8_t> acc((size_t)(2 * guard + (acc_rows - 1) * acc_stride + len));
                    for (uint8_t &b : acc) b = (uint8_t)rng();
                    std::vector<uint8_t> want = acc;
                    for (int r = 0; r < rows; ++r) {
                        const int slot = lm.out_slot[(size_t)r];
                        for (int64_t b = 0; b < len; ++b) {
                            uint8_t v = 0;
                            for (int j = 0; j < lm.n_in; ++j)
                                if (lm.in_slot[(size_t)j] % n == i)
                                    v ^= f.mul(lm.at(r, j), in[(size_t)(lm.in_slot[(size_t)j] / n * in_stride + b)]);
                            uint8_t &w = want[(size_t)(guard + slot * acc_stride + b)];
                            w = first ? v : (uint8_t)(w ^ v);
                        }
                    }
                    REQUIRE(emulate_clay_partial(plan, (uint8_t)p, (uint8_t)i, in.data(), in_stride, acc.data() + guard,
                                                 acc_stride, len, first != 0));
                    REQUIRE(acc == want);
                    // the chain: node 0 assigns (first) or accumulates, the others accumulate
                    REQUIRE(emulate_clay_partial(plan, (uint8_t)p, (uint8_t)i, in.data(), in_stride, running.data() + guard,
                                                 acc_stride, len, first != 0 && i == 0));
                }
                // the XOR over all nodes is the full map's output: the tiled plan's interpreter and the direct product
                std::vector<uint8_t> whole((size_t)acc_rows * len, 0), direct((size_t)acc_rows * len, 0);
                REQUIRE(emulate_tiled(tiled, (uint8_t)p, full.data(), whole.data(), len));
                for (int r = 0; r < rows; ++r)
                    for (int64_t b = 0; b < len; ++b) {
                        uint8_t v = 0;
                        for (int j = 0; j < lm.n_in; ++j) v ^= f.mul(lm.at(r, j), full[(size_t)lm.in_slot[(size_t)j] * len + b]);
                        direct[(size_t)lm.out_slot[(size_t)r] * len + b] = v;
                    }
                REQUIRE(whole == direct);
                std::vector<uint8_t> want = start;
                for (int r = 0; r < rows; ++r)
                    for (int64_t b = 0; b < len; ++b) {
                        uint8_t &w = want[(size_t)(guard + r * acc_stride + b)];
                        w = first ? whole[(size_t)r * len + b] : (uint8_t)(w ^ whole[(size_t)r * len + b]);
                    }
                REQUIRE(running == want);
            }
        }
        // every id byte and every node byte: nothing past npatterns or n is read or written
        for (int id = 0; id < 256; ++id)
            for (int nd = 0; nd < 256; ++nd) {
                if (id < np && nd < n && !lists[(size_t)id].empty()) continue;  // covered above
                std::vector<uint8_t> acc((size_t)((acc_rows - 1) * acc_stride + len), 0xA5);
                const std::vector<uint8_t> before = acc;
                REQUIRE(emulate_clay_partial(plan, (uint8_t)id, (uint8_t)nd, in.data(), in_stride, acc.data(), acc_stride, len,
                                             true));
                REQUIRE(acc == before);
                if (nd < n) REQUIRE((((size_t)id * n + nd) * T + T) * kMixedTileDwords <= plan.tiles.size());
            }
    }
    std::printf("clay_partial_plan_check: Clay(%d,%d) n=%d alpha=%d lists=%d: largest (list, node, tile) record %d entries\n", k, m,
                n, alpha, np, largest);
}

static void subsets(int n, int size, int from, std::vector<int> &cur, std::vector<std::vector<int>> &out) {
    if ((int)cur.size() == size) {
        out.push_back(cur);
        return;
    }
    for (int i = from; i < n; ++i) {
        cur.push_back(i);
        subsets(n, size, i + 1, cur, out);
        cur.pop_back();
    }
}

int main() {
    std::mt19937_64 rng(20241021);
    std::vector<int> cur;
    {  // Clay(4,2): every single node, every pair, the empty list
        std::vector<std::vector<int>> lists;
        subsets(6, 1, 0, cur, lists);
        subsets(6, 2, 0, cur, lists);
        REQUIRE(lists.size() == 21);
        lists.push_back({});
        check_geometry(4, 2, lists, rng);
    }
    {  // Clay(4,2), single nodes only: one tile per list
        std::vector<std::vector<int>> lists;
        subsets(6, 1, 0, cur, lists);
        check_geometry(4, 2, lists, rng);
    }
    check_geometry(2, 2, {{0}, {1}, {2}, {3}, {0, 3}, {1, 2}, {}}, rng);   // alpha 4: the 4-row instance
    check_geometry(3, 3, {{0}, {1}, {2}, {3}, {4}, {5}, {1, 4}, {0, 5}}, rng);  // alpha 9: a second tile of one row
    check_geometry(6, 2, {{0}, {3}, {7}, {0, 1}, {2, 7}, {}}, rng);        // alpha 16: ragged tile counts, T = 4
    {  // the refusals leave *out untouched; the interpreter refuses a plan that breaks its invariants
        const Tiled one = list_map(4, 2, {1});
        std::vector<TiledPatternIn> ins = {one.in()};
        TiledPlan tiled;
        REQUIRE(build_tiled_plan(ins.data(), 1, 4, &tiled));
        ClayPartialPlan plan;
        plan.npatterns = -7;
        REQUIRE(!build_clay_partial_plan(tiled, 0, 4, &plan));
        REQUIRE(!build_clay_partial_plan(tiled, 256, 4, &plan));
        REQUIRE(!build_clay_partial_plan(tiled, 6, 0, &plan));
        REQUIRE(!build_clay_partial_plan(tiled, 6, 4, nullptr));
        TiledPlan bad_tiled = tiled;
        bad_tiled.tiles.pop_back();
        REQUIRE(!build_clay_partial_plan(bad_tiled, 6, 4, &plan));
        bad_tiled = tiled;
        bad_tiled.tiles[0] = (uint32_t)(tiled.entries.size() / kMixedEntryDwords);  // entries outside the array
        REQUIRE(!build_clay_partial_plan(bad_tiled, 6, 4, &plan));
        REQUIRE(plan.npatterns == -7 && plan.entries.empty() && plan.tiles.empty());
        REQUIRE(build_clay_partial_plan(tiled, 6, 4, &plan));
        std::vector<uint8_t> in((size_t)8 * 4, 1), acc((size_t)8 * 4, 0);
        REQUIRE(emulate_clay_partial(plan, 0, 0, in.data(), 4, acc.data(), 4, 4, true));
        ClayPartialPlan bad = plan;
        bad.tiles[1] += 1;  // not a multiple of the depth
        REQUIRE(!emulate_clay_partial(bad, 0, 0, in.data(), 4, acc.data(), 4, 4, true));
        bad = plan;
        bad.tiles.pop_back();
        REQUIRE(!emulate_clay_partial(bad, 0, 0, in.data(), 4, acc.data(), 4, 4, true));
        bad = plan;
        bad.tiles[0] = (uint32_t)(plan.entries.size() / kMixedEntryDwords);  // entries outside the array
        REQUIRE(!emulate_clay_partial(bad, 0, 0, in.data(), 4, acc.data(), 4, 4, true));
        bad = plan;
        bad.tiles[2] = kMixedTileRows + 1;
        REQUIRE(!emulate_clay_partial(bad, 0, 0, in.data(), 4, acc.data(), 4, 4, true));
    }
    std::printf("clay_partial_plan_check: ok (%ld checks)\n", g_checks);
    return 0;
}
