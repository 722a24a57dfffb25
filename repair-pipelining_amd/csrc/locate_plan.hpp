// locate_plan.hpp -- the locate plan of an RS code (include/ecx.h ecx_rs_locate_corrupt_batch,
// DESIGN.md section 4.8): which single shard, replaced alone, can make a stripe that fails
// isParityCorrect (ReedSolomon.java:129-178) pass again.
//
// Write H = [P | I] for the m x n check matrix of the code (P the parity rows, ecx_api.cpp
// rs_check_map) and S(b) = H * x(b) for the m syndromes at byte position b.  Shard j alone explains
// the stripe exactly when S(b) is a multiple of column H_j at every b.  The plan turns that into
// m - 1 TEST ROWS per candidate shard, linear in the syndromes, that are all zero exactly then:
//   data shard j:        S_q ^ (H[q][j] / H[0][j]) * S_0   for q = 1..m-1
//   parity shard k + p:  S_q                               for q != p
// The n * (m - 1) rows, candidate after candidate, are cut into tiles of at most kLocateTileRows
// rows.  Every tile holds exactly m entry records in the engine's entry format (engine.hpp:
// kEntryDwords; [0] input slot -- here the syndrome index, [1] rows with a general coefficient,
// [2] rows with coefficient 1, [4 + 5r ..) the split tables of row r), in syndrome order: record p
// of a tile is the record of S_p whether or not the tile uses S_p (an unused one has empty masks),
// so k_gf_locate (apply_locate.hip) unrolls its loop over p across the syndrome registers -- no
// ring, no padding entry, no dynamic register index.  A tile record is the engine's (kTileDwords:
// [0] first entry [1] entry count = m [2] rows [4 + r] the candidate shard of row r); `candidate`
// repeats the row -> candidate table for the host.
//
// No HIP header and no other unit of the engine but the field (gf.hpp): the plan and its
// interpreter run -- and are tested -- on the CPU (tests/native/locate_plan_check.cpp).  The
// constants repeat engine.hpp's; locate.hpp asserts that they agree.
#pragma once

#include <cstdint>
#include <vector>

namespace ecx {

constexpr int kLocateEntryDwords = 48;
constexpr int kLocateTileDwords = 16;
constexpr int kLocateTileRows = 8;
constexpr int kLocateMaxParity = 8;  // the check map is one tile up to here: m syndrome registers

struct LocatePlan {
    std::vector<uint32_t> entries;  // n_tiles * m entries of kLocateEntryDwords
    std::vector<uint32_t> tiles;    // n_tiles records of kLocateTileDwords
    std::vector<int> candidate;     // n * (m - 1): the candidate shard of each test row
    int k = 0, m = 0;
    int n_tiles = 0;
};

// `parity` is the code's m x k parity rows, row-major (H = [parity | I]).  False -- and *out
// untouched -- when k < 1, m is outside 2..kLocateMaxParity (m < 2: every column matches every
// syndrome; m > 8: the check map is no longer one tile), k + m > 256, a pointer is null, or
// parity[0][j] is zero for some j (no MDS code has such a row).
bool build_locate_plan(const uint8_t *parity, int k, int m, LocatePlan *out);

// The plan applied to one stripe as k_gf_locate reads it: `syn` holds the m syndromes, syndrome p
// at syn + p * syn_stride, len bytes each; suspect[j] (n = k + m bytes) becomes 1 when every test
// row of candidate j is zero at every byte, else 0.  False when the plan breaks its invariants
// (arrays of the wrong size, a tile without exactly m records in syndrome order, a row count
// outside 1..kLocateTileRows, mask bits at or above the row count, a candidate outside 0..n-1).
bool emulate_locate(const LocatePlan &p, const uint8_t *syn, int64_t syn_stride, int64_t len, uint8_t *suspect);

// What both this plan and the pair plan (locate2_plan.hpp) are written and read with: coefficient c
// of a record's syndrome in test row r of its tile (mask bit, and the split tables of a general c);
// and the OR over bytes [b0, b1) of row r of the tile whose m records start at `ent`.
void locate_set_coefficient(uint32_t *rec, int r, uint8_t c);
uint8_t locate_row_or(const uint32_t *ent, int m, uint32_t r, const uint8_t *syn, int64_t syn_stride, int64_t b0,
                      int64_t b1);

}  // namespace ecx
