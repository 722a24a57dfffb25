// clay_partial_plan.cpp -- the partial-sum plan of a Clay pattern set and its host interpreter
// (clay_partial_plan.hpp).  Plain C++: built by the host compiler alone, like mixed_plan.cpp.
#include "clay_partial_plan.hpp"

#include <algorithm>

namespace ecx {

int clay_partial_depth(const ClayPartialPlan &p) { return p.min_entries >= 12 ? 8 : 4; }

bool build_clay_partial_plan(const TiledPlan &tiled, int n, int depth, ClayPartialPlan *out) {
    const int T = tiled.tiles_per_pattern;
    if (!out || n < 1 || n > 255 || depth <= 0 || T < 1 || T > kMixedMaxTiles) return false;
    if (tiled.npatterns < 1 || tiled.npatterns > kMixedRecords) return false;
    if (tiled.tiles.size() != (size_t)kMixedRecords * T * kMixedTileDwords) return false;
    ClayPartialPlan m;
    m.npatterns = tiled.npatterns;
    m.n = n;
    m.tiles_per_pattern = T;
    m.depth = depth;
    m.tiles.assign((size_t)kMixedRecords * n * T * kMixedTileDwords, 0u);
    int min_entries = 0x7FFFFFFF;
    for (int p = 0; p < tiled.npatterns; ++p)
        for (int t = 0; t < T; ++t) {
            const uint32_t *src = tiled.tiles.data() + ((size_t)p * T + t) * kMixedTileDwords;
            const uint32_t begin = src[0], count = src[1], rows = src[2];
            if (rows == 0) continue;  // an empty list, or a tile the list does not have: n empty records
            if (rows > (uint32_t)kMixedTileRows) return false;
            if (((size_t)begin + count) * kMixedEntryDwords > tiled.entries.size()) return false;
            m.max_rows = std::max(m.max_rows, (int)rows);
            for (int i = 0; i < n; ++i) {
                uint32_t *tile = m.tiles.data() + (((size_t)p * n + i) * T + t) * kMixedTileDwords;
                std::copy(src, src + kMixedTileDwords, tile);  // rows and output slots unchanged
                tile[0] = (uint32_t)(m.entries.size() / kMixedEntryDwords);
                uint32_t kept = 0;
                for (uint32_t e = 0; e < count; ++e) {
                    const uint32_t *rec = tiled.entries.data() + ((size_t)begin + e) * kMixedEntryDwords;
                    if (rec[0] == kMixedDummySlot || rec[0] % (uint32_t)n != (uint32_t)i) continue;
                    m.entries.insert(m.entries.end(), rec, rec + kMixedEntryDwords);
                    m.entries[m.entries.size() - kMixedEntryDwords] = rec[0] / (uint32_t)n;  // the plane
                    ++kept;
                }
                const uint32_t padded = (kept + (uint32_t)depth - 1) / (uint32_t)depth * (uint32_t)depth;
                for (uint32_t d = kept; d < padded; ++d) {
                    uint32_t rec[kMixedEntryDwords] = {0};
                    rec[0] = kMixedDummySlot;
                    m.entries.insert(m.entries.end(), rec, rec + kMixedEntryDwords);
                }
                tile[1] = padded;
                tile[3] = kept;
                m.max_entries = std::max(m.max_entries, (int)kept);
                if (kept > 0) min_entries = std::min(min_entries, (int)kept);
            }
        }
    m.min_entries = min_entries == 0x7FFFFFFF ? 0 : min_entries;
    if (m.entries.empty()) m.entries.assign(kMixedEntryDwords, 0u);
    *out = std::move(m);
    return true;
}

bool emulate_clay_partial(const ClayPartialPlan &p, uint8_t id, uint8_t node, const uint8_t *in, int64_t in_sub_stride,
                          uint8_t *acc, int64_t acc_sub_stride, int64_t len, bool is_first) {
    auto table_byte = [](uint32_t lo, uint32_t hi, int idx) {
        return (uint8_t)((idx < 4 ? lo : hi) >> (8 * (idx & 3)));
    };
    const int T = p.tiles_per_pattern;
    if (T < 1 || T > kMixedMaxTiles || p.depth <= 0 || p.n < 1 || p.n > 255) return false;
    if (p.tiles.size() != (size_t)kMixedRecords * p.n * T * kMixedTileDwords) return false;
    if ((int)node >= p.n) return true;  // the kernel leaves before it forms a record index
    for (int t = 0; t < T; ++t) {
        const uint32_t *tile = p.tiles.data() + (((size_t)id * p.n + node) * T + t) * kMixedTileDwords;
        const uint32_t rows = tile[2];
        if (rows == 0) continue;
        if (rows > (uint32_t)kMixedTileRows || tile[1] % (uint32_t)p.depth) return false;
        if (((size_t)tile[0] + tile[1]) * kMixedEntryDwords > p.entries.size()) return false;
        if (!is_first && tile[1] == 0) continue;
        std::vector<uint8_t> sum((size_t)rows * len, 0);
        for (uint32_t e = 0; e < tile[1]; ++e) {
            const uint32_t *rec = p.entries.data() + ((size_t)tile[0] + e) * kMixedEntryDwords;
            if (rec[0] == kMixedDummySlot) {
                if (rec[1] | rec[2]) return false;
                continue;  // reads the zero page: contributes nothing
            }
            const uint8_t *x = in + (int64_t)rec[0] * in_sub_stride;
            for (uint32_t r = 0; r < rows; ++r) {
                uint8_t *a = sum.data() + (size_t)r * len;
                if (rec[2] & (1u << r))
                    for (int64_t i = 0; i < len; ++i) a[i] ^= x[i];
                if (rec[1] & (1u << r)) {
                    const uint32_t *tb = rec + 4 + 5 * r;
                    for (int64_t i = 0; i < len; ++i)
                        a[i] ^= table_byte(tb[0], tb[1], x[i] & 7) ^ table_byte(tb[2], tb[3], (x[i] >> 3) & 7) ^
                                table_byte(tb[4], tb[4], x[i] >> 6);
                }
            }
        }
        for (uint32_t r = 0; r < rows; ++r) {
            uint8_t *dst = acc + (int64_t)tile[4 + r] * acc_sub_stride;
            const uint8_t *a = sum.data() + (size_t)r * len;
            for (int64_t i = 0; i < len; ++i) dst[i] = is_first ? a[i] : (uint8_t)(dst[i] ^ a[i]);
        }
    }
    return true;
}

}  // namespace ecx
