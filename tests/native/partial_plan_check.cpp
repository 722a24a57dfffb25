// partial_plan_check.cpp -- the partial-sum plan of a pattern set (csrc/partial_plan.cpp), on the
// CPU: built from that file, csrc/codes.cpp and csrc/gf.cpp with no ROCm include path
// (tests/test_partial_plan_native.py).
//
// Sets over RS(4,2) (every pattern of up to two missing shards), RS(12,4) (all 120 pairs, nothing
// missing, a duplicate, three and four missing) and RS(17,3) (up to three missing) are compiled
// from the codec's decodeMissing maps, as the library compiles them.  Asserted: the plan's sizes;
// that the row-count table is the patterns' missing counts and zero past npatterns; that every
// entry has slot 0 and no mask bit at or above its row count; that the interpreter over (p, i)
// equals column i of pattern p's decode matrix computed here directly in GF(2^8) -- the inverse of
// the first k present generator rows for a data row, a parity row times that for a parity row,
// zero for a shard the pattern does not read -- assigning and accumulating, with bytes around the
// rows left alone; that every (id byte, shard byte) pair, also those without a pattern or a shard,
// stays inside the arrays (the interpreter is handed exact-size buffers: the sanitizer build checks
// them) and writes nothing where nothing is to be written; and the refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../repair-pipelining_amd/csrc/codes.hpp"
#include "../../repair-pipelining_amd/csrc/gf.hpp"
#include "../../repair-pipelining_amd/csrc/partial_plan.hpp"

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

// D[o][i] for the o-th missing shard (ascending) of `present`, directly: data shards come from the
// inverse of the first k present rows of the generator matrix, parity shards from their parity row
// times the decoded data (ReedSolomon.java:224-283).
static std::vector<std::vector<uint8_t>> direct_matrix(const RsCode &c, const std::vector<bool> &present) {
    const Field &f = Field::get();
    const int k = c.k(), n = c.n();
    std::vector<int> used;
    for (int i = 0; i < n && (int)used.size() < k; ++i)
        if (present[i]) used.push_back(i);
    Matrix sub(k, k);
    for (int r = 0; r < k; ++r)
        for (int j = 0; j < k; ++j) sub.at(r, j) = c.matrix().at(used[r], j);
    const Matrix inv = sub.inverse();
    // data[d][i]: coefficient of shard i in data shard d (identity for a present data shard)
    std::vector<std::vector<uint8_t>> data(k, std::vector<uint8_t>(n, 0));
    for (int d = 0; d < k; ++d) {
        if (present[d]) data[d][d] = 1;
        else
            for (int j = 0; j < k; ++j) data[d][used[j]] = inv.at(d, j);
    }
    std::vector<std::vector<uint8_t>> rows;
    for (int o = 0; o < n; ++o) {
        if (present[o]) continue;
        if (o < k) {
            rows.push_back(data[o]);
            continue;
        }
        std::vector<uint8_t> row(n, 0);
        for (int d = 0; d < k; ++d)
            for (int i = 0; i < n; ++i) row[i] ^= f.mul(c.matrix().at(o, d), data[d][i]);
        rows.push_back(row);
    }
    return rows;
}

static void check_code(int k, int m, const std::vector<std::vector<int>> &missing_sets, std::mt19937_64 &rng) {
    const Field &f = Field::get();
    const RsCode code(k, m);
    const int n = k + m, np = (int)missing_sets.size();
    std::vector<std::vector<bool>> present;
    std::vector<LinearMap> maps;
    std::vector<PartialPatternIn> ins;
    for (const std::vector<int> &miss : missing_sets) {
        std::vector<bool> pr(n, true);
        for (int i : miss) pr[i] = false;
        present.push_back(pr);
        maps.push_back(code.decode_map(pr));
    }
    for (const LinearMap &lm : maps) ins.push_back(PartialPatternIn{lm.n_out, lm.n_in, lm.a.data(), lm.in_slot.data()});
    PartialPlan plan;
    REQUIRE(build_partial_plan(ins.data(), np, n, &plan));
    REQUIRE(plan.npatterns == np && plan.n == n);
    REQUIRE(plan.entries.size() == (size_t)np * n * kPartialEntryDwords);  // 192 B per (pattern, shard)
    REQUIRE(plan.rows.size() == (size_t)kPartialRecords);
    int max_rows = 0;
    for (int p = 0; p < kPartialRecords; ++p) {
        const uint32_t want = p < np ? (uint32_t)missing_sets[p].size() : 0u;
        REQUIRE(plan.rows[p] == want);
        max_rows = (int)want > max_rows ? (int)want : max_rows;
    }
    REQUIRE(plan.max_rows == max_rows);
    for (int p = 0; p < np; ++p)
        for (int i = 0; i < n; ++i) {
            const uint32_t *rec = plan.entries.data() + ((size_t)p * n + i) * kPartialEntryDwords;
            REQUIRE(rec[0] == 0u && rec[3] == 0u);
            REQUIRE(((rec[1] | rec[2]) >> plan.rows[p]) == 0u && (rec[1] & rec[2]) == 0u);
        }

    // every (p, i) against the matrix computed directly, over an odd length, rows a stride apart
    const int64_t len = 37, stride = 41, guard = 5;
    std::vector<uint8_t> in((size_t)len);
    for (int p = 0; p < np; ++p) {
        const int rows = (int)missing_sets[p].size();
        const auto D = direct_matrix(code, present[p]);
        REQUIRE((int)D.size() == rows);
        for (int i = 0; i < n; ++i) {
            for (uint8_t &b : in) b = (uint8_t)rng();
            for (int first = 0; first < 2; ++first) {
                // exactly the bytes the rows span, plus guards: an access outside is the sanitizer's to find
                std::vector<uint8_t> acc((size_t)(guard + (rows ? (rows - 1) * stride + len : 0) + guard));
                for (uint8_t &b : acc) b = (uint8_t)rng();
                std::vector<uint8_t> want = acc;
                for (int o = 0; o < rows; ++o)
                    for (int64_t b = 0; b < len; ++b) {
                        uint8_t &w = want[(size_t)(guard + o * stride + b)];
                        const uint8_t v = f.mul(D[o][i], in[(size_t)b]);
                        w = first ? v : (uint8_t)(w ^ v);
                    }
                REQUIRE(emulate_partial(plan, (uint8_t)p, (uint8_t)i, in.data(), acc.data() + guard, stride, len, first != 0));
                REQUIRE(acc == want);
            }
        }
    }
    // every id byte and every shard byte: nothing past npatterns or n is read or written
    for (int id = 0; id < 256; ++id)
        for (int sh = 0; sh < 256; ++sh) {
            if (id < np && sh < n) continue;  // covered above
            const int rows = id < np ? (int)missing_sets[id].size() : 0;
            std::vector<uint8_t> acc((size_t)(rows ? (rows - 1) * stride + len : 1), 0xA5);
            const std::vector<uint8_t> before = acc;
            REQUIRE(emulate_partial(plan, (uint8_t)id, (uint8_t)sh, in.data(), acc.data(), stride, len, true));
            REQUIRE(acc == before);
            // the index the kernel would form is only formed for a row count above zero and sh < n
            if (plan.rows[id] != 0 && sh < n) REQUIRE(((size_t)id * n + sh + 1) * kPartialEntryDwords <= plan.entries.size());
        }
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
    std::mt19937_64 rng(20240921);
    std::vector<int> cur;
    {  // RS(4,2): nothing, every single shard, every pair
        std::vector<std::vector<int>> sets;
        for (int size = 0; size <= 2; ++size) subsets(6, size, 0, cur, sets);
        REQUIRE(sets.size() == 22);
        check_code(4, 2, sets, rng);
    }
    {  // RS(12,4): all 120 pairs, nothing missing, a duplicate pair, three and four missing
        std::vector<std::vector<int>> sets;
        subsets(16, 2, 0, cur, sets);
        REQUIRE(sets.size() == 120);
        sets.push_back({});
        sets.push_back({0, 11});
        sets.push_back({1, 12, 15});
        sets.push_back({0, 5, 13, 14});
        sets.push_back({12, 13, 14, 15});
        check_code(12, 4, sets, rng);
    }
    {  // RS(17,3): a single shard, pairs and triples over data and parity
        std::vector<std::vector<int>> sets = {{3}, {19}, {0, 16}, {17, 18}, {0, 1, 2}, {5, 17, 19}, {17, 18, 19}, {}};
        check_code(17, 3, sets, rng);
    }
    {  // 256 patterns: the whole table taken
        std::vector<std::vector<int>> sets;
        subsets(16, 2, 0, cur, sets);
        subsets(16, 3, 0, cur, sets);
        sets.resize(256);
        check_code(12, 4, sets, rng);
    }
    // refusals leave *out untouched; the interpreter refuses a plan that breaks its invariants
    {
        const RsCode code(4, 2);
        const LinearMap lm = code.decode_map({true, false, true, true, false, true});
        const PartialPatternIn one{lm.n_out, lm.n_in, lm.a.data(), lm.in_slot.data()};
        PartialPlan plan;
        plan.npatterns = -7;
        REQUIRE(!build_partial_plan(&one, 0, 6, &plan));
        REQUIRE(!build_partial_plan(&one, kPartialRecords + 1, 6, &plan));
        REQUIRE(!build_partial_plan(&one, 1, 0, &plan));
        REQUIRE(!build_partial_plan(nullptr, 1, 6, &plan));
        PartialPatternIn wide = one;
        wide.rows = kPartialRows + 1;
        REQUIRE(!build_partial_plan(&wide, 1, 6, &plan));
        PartialPatternIn null_matrix = one;
        null_matrix.matrix = nullptr;
        REQUIRE(!build_partial_plan(&null_matrix, 1, 6, &plan));
        REQUIRE(plan.npatterns == -7 && plan.entries.empty() && plan.rows.empty());
        REQUIRE(build_partial_plan(&one, 1, 6, &plan));
        std::vector<uint8_t> in(4, 1), acc(8, 0);
        REQUIRE(emulate_partial(plan, 0, 0, in.data(), acc.data(), 4, 4, true));
        PartialPlan bad = plan;
        bad.rows[1] = 2;  // a row count past npatterns would index outside the entries
        REQUIRE(!emulate_partial(bad, 1, 0, in.data(), acc.data(), 4, 4, true));
        bad = plan;
        bad.rows[0] = kPartialRows + 1;
        REQUIRE(!emulate_partial(bad, 0, 0, in.data(), acc.data(), 4, 4, true));
        bad = plan;
        bad.entries[0] = 1;  // the kernel has one input: slot 0
        REQUIRE(!emulate_partial(bad, 0, 0, in.data(), acc.data(), 4, 4, true));
        bad = plan;
        bad.entries.resize(bad.entries.size() - 1);
        REQUIRE(!emulate_partial(bad, 0, 0, in.data(), acc.data(), 4, 4, true));
    }
    std::printf("partial_plan_check: ok (%ld checks)\n", g_checks);
    return 0;
}
