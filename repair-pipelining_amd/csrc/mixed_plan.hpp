// mixed_plan.hpp -- the device plan of a pattern set (include/ecx.h ecx_rs_pattern_set,
// DESIGN.md section 4.7): several single-tile maps of one codec, one per erasure pattern,
// concatenated so that one launch decodes stripes that miss different shards.
//
// The plan is the one k_gf_apply reads (engine.hpp: entries of kEntryDwords, tile records of
// kTileDwords), with two differences:
//   * the entry arrays of the patterns lie back to back, each padded to a multiple of the set's
//     load-ring depth with zero-coefficient kDummySlot entries, and record p's first-entry
//     index is rebased into that array;
//   * there are always kMixedRecords (256) tile records.  Record p < npatterns is pattern p's;
//     the rest are empty (0 entries, 0 rows).  A stripe names its pattern with one byte, so
//     every value that byte can hold selects a record inside the plan: k_gf_apply_mixed
//     (apply_mixed.hip) needs no bounds branch, and an id without a pattern does nothing.
//
// No HIP header and no other unit of the engine: the plan and its interpreter run -- and are
// tested -- on the CPU (tests/native/mixed_plan_check.cpp).  The constants repeat engine.hpp's;
// engine.cpp asserts that they agree.
#pragma once

#include <cstdint>
#include <vector>

namespace ecx {

constexpr int kMixedRecords = 256;
constexpr int kMixedEntryDwords = 48;
constexpr int kMixedTileDwords = 16;
constexpr int kMixedTileRows = 8;
constexpr uint32_t kMixedDummySlot = 0xFFFFFFFFu;

// One pattern's single-tile map as CompiledMap holds it: `tile` is its tile record (kTileDwords:
// [0] first entry [1] entry count [2] rows [4..4+rows) output slots) and `entries` the entry
// array that record indexes, unpadded.  A map with no rows has a record of zeros.
struct MixedPatternIn {
    const uint32_t *entries = nullptr;
    const uint32_t *tile = nullptr;
};

struct MixedPlan {
    std::vector<uint32_t> entries;  // padded, concatenated; never empty (one zero entry at least)
    std::vector<uint32_t> tiles;    // kMixedRecords * kMixedTileDwords
    int npatterns = 0;
    int depth = 4;     // every record's entry count is a multiple of it
    int max_rows = 0;  // the largest row count of the set: which ROWS instance can run it
};

// The load-ring depth of a set, by CompiledMap::preferred_depth's rule: 8 only if every
// non-empty pattern has at least 12 entries, else 4.
int mixed_depth(const MixedPatternIn *patterns, int npatterns);

// Builds the plan for `depth`.  False -- and *out untouched -- when npatterns is outside
// 1..kMixedRecords, depth is not positive, a pointer is null or a record has more than
// kMixedTileRows rows.
bool build_mixed_plan(const MixedPatternIn *patterns, int npatterns, int depth, MixedPlan *out);

// The plan applied to one stripe as k_gf_apply_mixed reads it for pattern id `id` (any byte):
// `in` and `out` are [slot][len]; padding entries read zeros; only the record's output slots are
// written.  False when the record breaks the plan's invariants (entry count not a multiple of
// the depth, a padding entry with coefficients, entries outside the array).
bool emulate_mixed(const MixedPlan &p, uint8_t id, const uint8_t *in, uint8_t *out, int64_t len);

// ---- the tiled form (apply_map_mixed.hip k_gf_map_mixed) ----
//
// A set whose maps have several tiles (Clay repair of two nodes: 16 rows).  T, the tiles per
// pattern, is the largest tile count among the set's maps, 1..kMixedMaxTiles.  The record array is
// [kMixedRecords][T]: record (id, t) at (id * T + t) * kMixedTileDwords is tile t of pattern id;
// every record past a pattern's own tile count and every record of an id >= npatterns is empty, so
// every (id byte, tile < T) pair selects a record inside the plan.  The entries are those of the
// mixed plan: each tile's padded to the depth, back to back in (pattern, tile) order, first-entry
// indices rebased.  With T == 1 the arrays are build_mixed_plan's bit for bit.
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

// mixed_depth's rule over every non-empty tile of the set.
int tiled_depth(const TiledPatternIn *patterns, int npatterns);

// Builds the tiled plan for `depth`.  False -- and *out untouched -- when npatterns is outside
// 1..kMixedRecords, depth is not positive, a pointer is null, a pattern has more than
// kMixedMaxTiles tiles or a tile more than kMixedTileRows rows.
bool build_tiled_plan(const TiledPatternIn *patterns, int npatterns, int depth, TiledPlan *out);

// The tiled plan applied to one stripe as k_gf_map_mixed reads it for pattern id `id` (any byte),
// out of place: `in` is [slot][len] and is only read, `out` is [slot][len] and only the output
// slots of the id's records are written.  False when a record breaks the plan's invariants.
bool emulate_tiled(const TiledPlan &p, uint8_t id, const uint8_t *in, uint8_t *out, int64_t len);

}  // namespace ecx
