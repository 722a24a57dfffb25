// mixed_plan.hpp -- the device plan of a pattern set (include/ecx.h ecx_rs_pattern_set,
// ecx_clay_pattern_set; DESIGN.md sections 4.7 and 4.7.3): several maps of one codec, one per
// erasure pattern, concatenated so that one launch runs stripes that each name their own.
//
// The plan is the one k_gf_apply reads (engine.hpp: entries of kEntryDwords, tile records of
// kTileDwords), with two differences:
//   * the entry arrays of the patterns' tiles lie back to back in (pattern, tile) order, each
//     padded to a multiple of the set's load-ring depth with zero-coefficient kDummySlot entries,
//     and every record's first-entry index is rebased into that array;
//   * the record array is [kMixedRecords][T], T the largest tile count among the set's maps
//     (1..kMixedMaxTiles): record (id, t) at (id * T + t) * kMixedTileDwords is tile t of pattern
//     id.  Every record past a pattern's own tile count and every record of an id >= npatterns is
//     empty (0 entries, 0 rows).  A stripe names its pattern with one byte, so every
//     (id byte, tile < T) pair selects a record inside the plan: the kernels need no bounds
//     branch, and an id without a pattern does nothing.
// A set of single-tile maps (the RS decodes) has T == 1 and 256 records: k_gf_apply_mixed
// (apply_mixed.hip) reads record `id`, in place.  A set with a map of several tiles (Clay repair
// of two nodes: 16 rows) runs out of place only (apply_map_mixed.hip k_gf_map_mixed).
//
// No HIP header and no other unit of the engine: the plan and its interpreter run -- and are
// tested -- on the CPU (tests/native/mixed_plan_check.cpp, tiled_plan_check.cpp).  The constants
// repeat engine.hpp's; pattern_set.hpp asserts that they agree.
#pragma once

#include <cstdint>
#include <vector>

namespace ecx {

constexpr int kMixedRecords = 256;
constexpr int kMixedEntryDwords = 48;
constexpr int kMixedTileDwords = 16;
constexpr int kMixedTileRows = 8;
constexpr uint32_t kMixedDummySlot = 0xFFFFFFFFu;
constexpr int kMixedMaxTiles = 8;

// One pattern's map as CompiledMap holds it: `tiles` are its n_tiles tile records (kTileDwords
// each) and `entries` the unpadded entry array they index.  Nothing else of a multi-tile map is
// read.  n_tiles 0 is a map with no rows.
struct TiledPatternIn {
    const uint32_t *entries = nullptr;
    const uint32_t *tiles = nullptr;
    int n_tiles = 0;
};

struct TiledPlan {
    std::vector<uint32_t> entries;  // padded, concatenated; never empty
    std::vector<uint32_t> tiles;    // kMixedRecords * tiles_per_pattern * kMixedTileDwords
    int npatterns = 0;
    int tiles_per_pattern = 1;
    int depth = 4;
    int max_rows = 0;      // the largest row count of any tile
    int max_out_slot = -1;  // the largest output slot of any tile
};

// The load-ring depth of a set, by CompiledMap::preferred_depth's rule: 8 only if every
// non-empty tile of the set has at least 12 entries, else 4.
int tiled_depth(const TiledPatternIn *patterns, int npatterns);

// Builds the plan for `depth`.  False -- and *out untouched -- when npatterns is outside
// 1..kMixedRecords, depth is not positive, a pointer is null, a pattern has more than
// kMixedMaxTiles tiles or a tile more than kMixedTileRows rows.
bool build_tiled_plan(const TiledPatternIn *patterns, int npatterns, int depth, TiledPlan *out);

// The plan applied to one stripe as k_gf_map_mixed reads it for pattern id `id` (any byte), out of
// place: `in` is [slot][len] and is only read, `out` is [slot][len] and only the output slots of
// the id's records are written; padding entries read zeros.  With T == 1, `in` and `out` may be
// two copies of one stripe: that is k_gf_apply_mixed.  False when a record breaks the plan's
// invariants (entry count not a multiple of the depth, a padding entry with coefficients, entries
// outside the array).
bool emulate_tiled(const TiledPlan &p, uint8_t id, const uint8_t *in, uint8_t *out, int64_t len);

}  // namespace ecx
