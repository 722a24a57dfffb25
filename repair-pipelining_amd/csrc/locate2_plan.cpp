// locate2_plan.cpp -- the pair plan of an RS code and its host interpreter (locate2_plan.hpp).
// Plain C++: built by the host compiler alone, like locate_plan.cpp.
#include "locate2_plan.hpp"

#include <algorithm>
#include <array>

#include "gf.hpp"

namespace ecx {

namespace {
using Vec = std::array<uint8_t, kLocateMaxParity>;

// H[q][j] of H = [parity | I]
uint8_t h_at(const uint8_t *parity, int k, int q, int j) {
    return j < k ? parity[(size_t)q * k + j] : (uint8_t)(j - k == q ? 1 : 0);
}

// A basis of the left null space of [H_i H_j]: [H_i H_j | I] row-reduced, the I part of the rows
// whose first two columns came out zero.  False when the two columns are dependent.
bool null_rows(const uint8_t *parity, int k, int m, int i, int j, std::vector<Vec> *rows) {
    const Field &f = Field::get();
    uint8_t a[kLocateMaxParity][2 + kLocateMaxParity] = {};
    for (int q = 0; q < m; ++q) {
        a[q][0] = h_at(parity, k, q, i);
        a[q][1] = h_at(parity, k, q, j);
        a[q][2 + q] = 1;
    }
    for (int c = 0; c < 2; ++c) {
        int piv = c;
        while (piv < m && a[piv][c] == 0) ++piv;
        if (piv == m) return false;
        std::swap_ranges(a[piv], a[piv] + 2 + m, a[c]);
        const uint8_t inv = f.div(1, a[c][c]);
        for (int x = 0; x < 2 + m; ++x) a[c][x] = f.mul(a[c][x], inv);
        for (int q = 0; q < m; ++q) {
            const uint8_t g = a[q][c];
            if (q == c || g == 0) continue;
            for (int x = 0; x < 2 + m; ++x) a[q][x] ^= f.mul(g, a[c][x]);
        }
    }
    rows->clear();
    for (int q = 2; q < m; ++q) {
        Vec v{};
        std::copy(a[q] + 2, a[q] + 2 + m, v.begin());
        rows->push_back(v);
    }
    return true;
}

bool sizes_hold(const Locate2Plan &p) {
    if (p.k < 1 || p.m < kLocate2MinParity || p.m > kLocateMaxParity || p.k + p.m > kLocate2MaxShards) return false;
    const int n = p.k + p.m, rows = p.n_pairs * (p.m - 2);
    return p.n_pairs == n * (n - 1) / 2 && p.n_tiles == (rows + kLocateTileRows - 1) / kLocateTileRows &&
           p.entries.size() == (size_t)p.n_tiles * p.m * kLocateEntryDwords &&
           p.tiles.size() == (size_t)p.n_tiles * kLocateTileDwords && p.suspect.size() == (size_t)rows &&
           p.members.size() == (size_t)p.n_pairs * 2;
}
}  // namespace

bool build_locate2_plan(const uint8_t *parity, int k, int m, Locate2Plan *out) {
    if (!parity || !out || k < 1 || m < kLocate2MinParity || m > kLocateMaxParity || k + m > kLocate2MaxShards)
        return false;
    const Field &f = Field::get();
    const int n = k + m;
    Locate2Plan pl;
    pl.k = k;
    pl.m = m;
    pl.n_pairs = n * (n - 1) / 2;
    const int rows = pl.n_pairs * (m - 2);
    pl.n_tiles = (rows + kLocateTileRows - 1) / kLocateTileRows;
    pl.entries.assign((size_t)pl.n_tiles * m * kLocateEntryDwords, 0u);
    pl.tiles.assign((size_t)pl.n_tiles * kLocateTileDwords, 0u);
    pl.suspect.reserve((size_t)rows);
    pl.members.reserve((size_t)pl.n_pairs * 2);
    std::vector<Vec> basis;
    for (int i = 0; i < n; ++i) {
        for (int j = i + 1; j < n; ++j) {
            if (!null_rows(parity, k, m, i, j, &basis)) return false;
            // the shortcut's ground: no third column lies in span(H_i, H_j) (each triple once)
            for (int c = j + 1; c < n; ++c) {
                bool outside = false;
                for (const Vec &v : basis) {
                    uint8_t dot = 0;
                    for (int q = 0; q < m; ++q) dot ^= f.mul(v[(size_t)q], h_at(parity, k, q, c));
                    outside = outside || dot != 0;
                }
                if (!outside) return false;
            }
            for (const Vec &v : basis) {
                const int row = (int)pl.suspect.size(), t = row / kLocateTileRows, r = row % kLocateTileRows;
                for (int q = 0; q < m; ++q)
                    locate_set_coefficient(pl.entries.data() + ((size_t)t * m + q) * kLocateEntryDwords, r, v[(size_t)q]);
                pl.suspect.push_back(n + pair_index(n, i, j));
            }
            pl.members.push_back((uint8_t)i);
            pl.members.push_back((uint8_t)j);
        }
    }
    for (int t = 0; t < pl.n_tiles; ++t) {
        uint32_t *tile = pl.tiles.data() + (size_t)t * kLocateTileDwords;
        const int r0 = t * kLocateTileRows, nr = std::min(kLocateTileRows, rows - r0);
        tile[0] = (uint32_t)(t * m);
        tile[1] = (uint32_t)m;
        tile[2] = (uint32_t)nr;
        for (int r = 0; r < nr; ++r) tile[4 + r] = (uint32_t)pl.suspect[(size_t)(r0 + r)];
        for (int q = 0; q < m; ++q) pl.entries[((size_t)t * m + q) * kLocateEntryDwords] = (uint32_t)q;
    }
    *out = std::move(pl);
    return true;
}

bool emulate_locate2(const Locate2Plan &p, const LocatePlan &single, const uint8_t *syn, int64_t syn_stride,
                     int64_t len, uint8_t *suspect, bool shortcut) {
    if (!sizes_hold(p) || single.k != p.k || single.m != p.m) return false;
    const int n = p.k + p.m, m = p.m, width = n + p.n_pairs;
    for (int t = 0; t < p.n_tiles; ++t) {
        const uint32_t *tile = p.tiles.data() + (size_t)t * kLocateTileDwords;
        const uint32_t nr = tile[2];
        if (tile[0] != (uint32_t)(t * m) || tile[1] != (uint32_t)m || nr < 1 || nr > (uint32_t)kLocateTileRows) return false;
        for (int q = 0; q < m; ++q) {
            const uint32_t *rec = p.entries.data() + ((size_t)tile[0] + q) * kLocateEntryDwords;
            if (rec[0] != (uint32_t)q || ((rec[1] | rec[2]) >> nr) != 0u || (rec[1] & rec[2]) != 0u) return false;
        }
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t idx = tile[4 + r];
            if (idx < (uint32_t)n || idx >= (uint32_t)width || (int)idx != p.suspect[(size_t)t * kLocateTileRows + r])
                return false;
        }
    }
    for (int q = 0; q < p.n_pairs; ++q)
        if (p.members[(size_t)2 * q] >= p.members[(size_t)2 * q + 1] || p.members[(size_t)2 * q + 1] >= n) return false;
    std::vector<uint8_t> one((size_t)n);
    if (!emulate_locate(single, syn, syn_stride, 0, one.data())) return false;  // the single plan's invariants
    std::fill(suspect, suspect + width, (uint8_t)1);  // k_set_suspects; the passes only ever clear
    for (int64_t b0 = 0; b0 < len; b0 += kLocate2SpanBytes) {
        const int64_t b1 = std::min<int64_t>(len, b0 + kLocate2SpanBytes);
        uint8_t any = 0;
        for (int q = 0; q < m; ++q)
            for (int64_t b = b0; b < b1; ++b) any |= syn[q * syn_stride + b];
        if (!any) continue;  // the wave leaves after stage one
        uint64_t cleared = 0;  // stage two-a: the single plan
        for (int t = 0; t < single.n_tiles; ++t) {
            const uint32_t *tile = single.tiles.data() + (size_t)t * kLocateTileDwords;
            const uint32_t *ent = single.entries.data() + (size_t)tile[0] * kLocateEntryDwords;
            for (uint32_t r = 0; r < tile[2]; ++r) {
                if (!locate_row_or(ent, m, r, syn, syn_stride, b0, b1)) continue;
                suspect[tile[4 + r]] = 0;
                cleared |= (uint64_t)1 << tile[4 + r];
            }
        }
        const uint64_t alive = ~cleared & (n == 64 ? ~(uint64_t)0 : (((uint64_t)1 << n) - 1));
        if (shortcut && alive != 0 && (alive & (alive - 1)) == 0) {  // stage two-b
            int i = 0;
            while (!((alive >> i) & 1)) ++i;
            for (int q = 0; q < p.n_pairs; ++q)
                if (p.members[(size_t)2 * q] != i && p.members[(size_t)2 * q + 1] != i) suspect[n + q] = 0;
            continue;
        }
        for (int t = 0; t < p.n_tiles; ++t) {  // stage two-c: the pair tiles
            const uint32_t *tile = p.tiles.data() + (size_t)t * kLocateTileDwords;
            const uint32_t *ent = p.entries.data() + (size_t)tile[0] * kLocateEntryDwords;
            for (uint32_t r = 0; r < tile[2]; ++r)
                if (locate_row_or(ent, m, r, syn, syn_stride, b0, b1)) suspect[tile[4 + r]] = 0;
        }
    }
    return true;
}

}  // namespace ecx
