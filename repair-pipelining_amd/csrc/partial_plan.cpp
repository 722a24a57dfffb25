// partial_plan.cpp -- the partial-sum plan of a pattern set and its host interpreter
// (partial_plan.hpp).  Plain C++: built by the host compiler alone, like mixed_plan.cpp.
#include "partial_plan.hpp"

#include <algorithm>

#include "gf.hpp"

namespace ecx {

namespace {
uint32_t pack4(const uint8_t *t) {
    return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
}

// the five split-table dwords of coefficient c (engine.hpp: T0a T0b T1a T1b T2)
void split_tables(uint8_t c, uint32_t *out) {
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
}  // namespace

bool build_partial_plan(const PartialPatternIn *patterns, int npatterns, int n, PartialPlan *out) {
    if (!patterns || !out || npatterns < 1 || npatterns > kPartialRecords || n < 1) return false;
    for (int p = 0; p < npatterns; ++p) {
        const PartialPatternIn &in = patterns[p];
        if (in.rows < 0 || in.rows > kPartialRows || in.n_in < 0) return false;
        if (in.rows > 0 && in.n_in > 0 && (!in.matrix || !in.in_slot)) return false;
    }
    PartialPlan m;
    m.npatterns = npatterns;
    m.n = n;
    m.rows.assign(kPartialRecords, 0u);
    m.entries.assign((size_t)npatterns * n * kPartialEntryDwords, 0u);
    for (int p = 0; p < npatterns; ++p) {
        const PartialPatternIn &in = patterns[p];
        m.rows[(size_t)p] = (uint32_t)in.rows;
        m.max_rows = std::max(m.max_rows, in.rows);
        for (int j = 0; j < in.n_in && in.rows > 0; ++j) {
            const int shard = in.in_slot[j];
            if (shard < 0 || shard >= n) continue;  // not a shard of this code: no helper holds it
            uint32_t *rec = m.entries.data() + ((size_t)p * n + shard) * kPartialEntryDwords;
            for (int r = 0; r < in.rows; ++r) {
                const uint8_t c = in.matrix[(size_t)r * in.n_in + j];
                if (c == 1) rec[2] |= 1u << r;
                else if (c) {
                    rec[1] |= 1u << r;
                    split_tables(c, rec + 4 + 5 * r);
                }
            }
        }
    }
    *out = std::move(m);
    return true;
}

bool emulate_partial(const PartialPlan &p, uint8_t id, uint8_t shard, const uint8_t *in, uint8_t *acc,
                     int64_t row_stride, int64_t len, bool is_first) {
    auto table_byte = [](uint32_t lo, uint32_t hi, int idx) {
        return (uint8_t)((idx < 4 ? lo : hi) >> (8 * (idx & 3)));
    };
    if (p.rows.size() != (size_t)kPartialRecords || p.n < 1 || p.npatterns < 1 || p.npatterns > kPartialRecords)
        return false;
    if (p.entries.size() != (size_t)p.npatterns * p.n * kPartialEntryDwords) return false;
    const uint32_t rows = p.rows[id];
    if (rows > (uint32_t)kPartialRows) return false;
    if (rows == 0 || (int)shard >= p.n) return true;  // the kernel leaves before it forms an entry index
    if ((int)id >= p.npatterns) return false;         // a row count past npatterns would index outside the entries
    const uint32_t *rec = p.entries.data() + ((size_t)id * p.n + shard) * kPartialEntryDwords;
    if (rec[0] != 0u || ((rec[1] | rec[2]) >> rows) != 0u || (rec[1] & rec[2]) != 0u) return false;
    for (uint32_t r = 0; r < rows; ++r) {
        uint8_t *a = acc + (int64_t)r * row_stride;
        const uint32_t *tb = rec + 4 + 5 * r;
        for (int64_t i = 0; i < len; ++i) {
            uint8_t v = 0;
            if (rec[2] & (1u << r)) v = in[i];
            if (rec[1] & (1u << r))
                v = table_byte(tb[0], tb[1], in[i] & 7) ^ table_byte(tb[2], tb[3], (in[i] >> 3) & 7) ^
                    table_byte(tb[4], tb[4], in[i] >> 6);
            a[i] = is_first ? v : (uint8_t)(a[i] ^ v);
        }
    }
    return true;
}

}  // namespace ecx
