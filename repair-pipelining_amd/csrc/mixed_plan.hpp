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

}  // namespace ecx
