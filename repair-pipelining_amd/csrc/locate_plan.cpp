// locate_plan.cpp -- the locate plan of an RS code and its host interpreter (locate_plan.hpp).
// Plain C++: built by the host compiler alone, like partial_plan.cpp.
#include "locate_plan.hpp"

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

void locate_set_coefficient(uint32_t *rec, int r, uint8_t c) {
    if (c == 1) rec[2] |= 1u << r;
    else if (c) {
        rec[1] |= 1u << r;
        split_tables(c, rec + 4 + 5 * r);
    }
}

uint8_t locate_row_or(const uint32_t *ent, int m, uint32_t r, const uint8_t *syn, int64_t syn_stride, int64_t b0,
                      int64_t b1) {
    auto table_byte = [](uint32_t lo, uint32_t hi, int idx) {
        return (uint8_t)((idx < 4 ? lo : hi) >> (8 * (idx & 3)));
    };
    uint8_t nz = 0;
    for (int64_t b = b0; b < b1; ++b) {
        uint8_t v = 0;
        for (int q = 0; q < m; ++q) {
            const uint32_t *rec = ent + (size_t)q * kLocateEntryDwords;
            const uint32_t *tb = rec + 4 + 5 * r;
            const uint8_t x = syn[q * syn_stride + b];
            if (rec[2] & (1u << r)) v ^= x;
            if (rec[1] & (1u << r))
                v ^= table_byte(tb[0], tb[1], x & 7) ^ table_byte(tb[2], tb[3], (x >> 3) & 7) ^
                     table_byte(tb[4], tb[4], x >> 6);
        }
        nz |= v;
    }
    return nz;
}

bool build_locate_plan(const uint8_t *parity, int k, int m, LocatePlan *out) {
    if (!parity || !out || k < 1 || m < 2 || m > kLocateMaxParity || k + m > 256) return false;
    for (int j = 0; j < k; ++j)
        if (parity[j] == 0) return false;
    const Field &f = Field::get();
    const int n = k + m, rows = n * (m - 1);
    LocatePlan pl;
    pl.k = k;
    pl.m = m;
    pl.n_tiles = (rows + kLocateTileRows - 1) / kLocateTileRows;
    pl.entries.assign((size_t)pl.n_tiles * m * kLocateEntryDwords, 0u);
    pl.tiles.assign((size_t)pl.n_tiles * kLocateTileDwords, 0u);
    pl.candidate.reserve((size_t)rows);
    // coefficient c of syndrome p in test row `row`
    auto put = [&](int row, int p, uint8_t c) {
        const int t = row / kLocateTileRows, r = row % kLocateTileRows;
        locate_set_coefficient(pl.entries.data() + ((size_t)t * m + p) * kLocateEntryDwords, r, c);
    };
    for (int j = 0; j < n; ++j) {
        for (int i = 0; i < m - 1; ++i) {
            const int row = (int)pl.candidate.size();
            if (j < k) {  // S_q ^ (H[q][j] / H[0][j]) * S_0, q = i + 1
                const int q = i + 1;
                put(row, q, 1);
                put(row, 0, f.div(parity[(size_t)q * k + j], parity[j]));
            } else {  // S_q for the i-th q != p
                const int p = j - k;
                put(row, i < p ? i : i + 1, 1);
            }
            pl.candidate.push_back(j);
        }
    }
    for (int t = 0; t < pl.n_tiles; ++t) {
        uint32_t *tile = pl.tiles.data() + (size_t)t * kLocateTileDwords;
        const int r0 = t * kLocateTileRows, nr = std::min(kLocateTileRows, rows - r0);
        tile[0] = (uint32_t)(t * m);
        tile[1] = (uint32_t)m;
        tile[2] = (uint32_t)nr;
        for (int r = 0; r < nr; ++r) tile[4 + r] = (uint32_t)pl.candidate[(size_t)(r0 + r)];
        for (int p = 0; p < m; ++p) pl.entries[((size_t)t * m + p) * kLocateEntryDwords] = (uint32_t)p;
    }
    *out = std::move(pl);
    return true;
}

bool emulate_locate(const LocatePlan &p, const uint8_t *syn, int64_t syn_stride, int64_t len, uint8_t *suspect) {
    if (p.k < 1 || p.m < 2 || p.m > kLocateMaxParity || p.k + p.m > 256) return false;
    const int n = p.k + p.m, rows = n * (p.m - 1);
    if (p.n_tiles != (rows + kLocateTileRows - 1) / kLocateTileRows) return false;
    if (p.entries.size() != (size_t)p.n_tiles * p.m * kLocateEntryDwords) return false;
    if (p.tiles.size() != (size_t)p.n_tiles * kLocateTileDwords || p.candidate.size() != (size_t)rows) return false;
    std::fill(suspect, suspect + n, (uint8_t)1);  // k_set_suspects; the passes only ever clear
    for (int t = 0; t < p.n_tiles; ++t) {
        const uint32_t *tile = p.tiles.data() + (size_t)t * kLocateTileDwords;
        const uint32_t nr = tile[2];
        if (tile[0] != (uint32_t)(t * p.m) || tile[1] != (uint32_t)p.m || nr < 1 || nr > (uint32_t)kLocateTileRows)
            return false;
        const uint32_t *ent = p.entries.data() + (size_t)tile[0] * kLocateEntryDwords;
        for (int q = 0; q < p.m; ++q) {
            const uint32_t *rec = ent + (size_t)q * kLocateEntryDwords;
            if (rec[0] != (uint32_t)q || ((rec[1] | rec[2]) >> nr) != 0u || (rec[1] & rec[2]) != 0u) return false;
        }
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t cand = tile[4 + r];
            if (cand >= (uint32_t)n || (int)cand != p.candidate[(size_t)t * kLocateTileRows + r]) return false;
            if (locate_row_or(ent, p.m, r, syn, syn_stride, 0, len)) suspect[cand] = 0;
        }
    }
    return true;
}

}  // namespace ecx
