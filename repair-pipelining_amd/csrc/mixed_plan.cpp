// mixed_plan.cpp -- the device plan of a pattern set and its host interpreter (mixed_plan.hpp).
// Plain C++: built by the host compiler alone, like blocked_layout.cpp.
#include "mixed_plan.hpp"

#include <algorithm>

namespace ecx {

namespace {

// One record of a plan applied to one stripe, as apply_tile reads it: `in` is only read, the
// record's output slots of `out` are written.
bool emulate_record(const std::vector<uint32_t> &entries, const uint32_t *tile, int depth, const uint8_t *in,
                    uint8_t *out, int64_t len) {
    auto table_byte = [](uint32_t lo, uint32_t hi, int idx) {
        return (uint8_t)((idx < 4 ? lo : hi) >> (8 * (idx & 3)));
    };
    const uint32_t rows = tile[2];
    if (rows == 0) return true;  // the kernel returns before it reads anything else
    if (rows > (uint32_t)kMixedTileRows || tile[1] % (uint32_t)depth) return false;
    if (((size_t)tile[0] + tile[1]) * kMixedEntryDwords > entries.size()) return false;
    std::vector<uint8_t> acc((size_t)rows * len, 0);
    for (uint32_t e = 0; e < tile[1]; ++e) {
        const uint32_t *rec = entries.data() + ((size_t)tile[0] + e) * kMixedEntryDwords;
        if (rec[0] == kMixedDummySlot) {
            if (rec[1] | rec[2]) return false;
            continue;  // reads the zero page: contributes nothing
        }
        const uint8_t *x = in + (int64_t)rec[0] * len;
        for (uint32_t r = 0; r < rows; ++r) {
            uint8_t *a = acc.data() + (size_t)r * len;
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
    for (uint32_t r = 0; r < rows; ++r)
        std::copy(acc.begin() + (size_t)r * len, acc.begin() + (size_t)(r + 1) * len, out + (int64_t)tile[4 + r] * len);
    return true;
}

}  // namespace

int tiled_depth(const TiledPatternIn *patterns, int npatterns) {
    uint32_t min_count = 0xFFFFFFFFu;
    for (int p = 0; p < npatterns; ++p)
        for (int t = 0; t < patterns[p].n_tiles; ++t) {
            const uint32_t c = patterns[p].tiles[(size_t)t * kMixedTileDwords + 1];
            if (c > 0) min_count = std::min(min_count, c);
        }
    return min_count != 0xFFFFFFFFu && min_count >= 12 ? 8 : 4;
}

bool build_tiled_plan(const TiledPatternIn *patterns, int npatterns, int depth, TiledPlan *out) {
    if (!patterns || !out || npatterns < 1 || npatterns > kMixedRecords || depth <= 0) return false;
    int T = 1;
    for (int p = 0; p < npatterns; ++p) {
        const TiledPatternIn &in = patterns[p];
        if (in.n_tiles < 0 || in.n_tiles > kMixedMaxTiles) return false;
        if (in.n_tiles > 0 && (!in.tiles || !in.entries)) return false;
        for (int t = 0; t < in.n_tiles; ++t)
            if (in.tiles[(size_t)t * kMixedTileDwords + 2] > (uint32_t)kMixedTileRows) return false;
        T = std::max(T, in.n_tiles);
    }
    TiledPlan m;
    m.npatterns = npatterns;
    m.tiles_per_pattern = T;
    m.depth = depth;
    m.tiles.assign((size_t)kMixedRecords * T * kMixedTileDwords, 0u);
    for (int p = 0; p < npatterns; ++p)
        for (int t = 0; t < patterns[p].n_tiles; ++t) {
            const uint32_t *src = patterns[p].tiles + (size_t)t * kMixedTileDwords;
            uint32_t *tile = m.tiles.data() + ((size_t)p * T + t) * kMixedTileDwords;
            const uint32_t begin = src[0], count = src[1], rows = src[2];
            std::copy(src, src + kMixedTileDwords, tile);
            tile[0] = (uint32_t)(m.entries.size() / kMixedEntryDwords);
            m.entries.insert(m.entries.end(), patterns[p].entries + (size_t)begin * kMixedEntryDwords,
                             patterns[p].entries + (size_t)(begin + count) * kMixedEntryDwords);
            const uint32_t padded = (count + (uint32_t)depth - 1) / (uint32_t)depth * (uint32_t)depth;
            for (uint32_t d = count; d < padded; ++d) {
                uint32_t rec[kMixedEntryDwords] = {0};
                rec[0] = kMixedDummySlot;
                m.entries.insert(m.entries.end(), rec, rec + kMixedEntryDwords);
            }
            tile[1] = padded;
            m.max_rows = std::max(m.max_rows, (int)rows);
            for (uint32_t r = 0; r < rows; ++r) m.max_out_slot = std::max(m.max_out_slot, (int)src[4 + r]);
        }
    if (m.entries.empty()) m.entries.assign(kMixedEntryDwords, 0u);
    *out = std::move(m);
    return true;
}

bool emulate_tiled(const TiledPlan &p, uint8_t id, const uint8_t *in, uint8_t *out, int64_t len) {
    const int T = p.tiles_per_pattern;
    if (T < 1 || T > kMixedMaxTiles || p.depth <= 0) return false;
    if (p.tiles.size() != (size_t)kMixedRecords * T * kMixedTileDwords) return false;
    for (int t = 0; t < T; ++t)
        if (!emulate_record(p.entries, p.tiles.data() + ((size_t)id * T + t) * kMixedTileDwords, p.depth, in, out, len))
            return false;
    return true;
}

}  // namespace ecx
