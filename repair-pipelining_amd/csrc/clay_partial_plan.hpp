// clay_partial_plan.hpp -- the partial-sum plan of a Clay pattern set (include/ecx.h
// ecx_clay_partial_batch_mixed): one hop of the pipelined repair chain
// (ClayCoordinator.kt:265-319, ClayCodeNode.kt:165-233: every helper adds its own sub-chunks'
// share of the erased nodes to a running sum and forwards it) over stripes that name their
// erased-node list AND the node this helper holds with one byte each.
//
// The plan is the set's tiled plan (mixed_plan.hpp TiledPlan) cut by input node.  A list's map
// reads input slot z * n + node (plane z of node `node`) and writes output slot z * |E| + j.  For
// every (list p, node i < n, tile t < T) the plan holds ONE tile record, record
// ((p * n + i) * T + t), and its entries: the entries of tile t of list p whose input slot is
// i (mod n), in their order, their slot rewritten to the plane z = slot / n -- the kernel's input
// is the helper's own planes, z the slot index -- and padded to the load-ring depth with
// zero-coefficient kDummySlot entries.  Rows and output slots are the tile's own, so the hops of
// all n nodes sum to the tile.  A node the list does not read (an erased node, or one whose planes
// a tile happens not to need) has a record with the tile's rows and NO entries: it adds nothing
// to a running sum and assigns zeros as a chain's first hop.
//
// There are always kMixedRecords * n * T records: those of an id >= npatterns, of an empty list
// and of a tile a list does not have are empty (0 rows), so every (id byte, node < n, tile < T)
// selects a record inside the plan -- k_gf_map_partial_mixed (apply_clay_partial_mixed.hip) has no
// bounds branch on the id, and one compare of the node byte against n.
//
// Size: 64 B per record, 256 * n * T records, and 192 B per padded entry.  The six single-node
// lists of Clay(4,2) (n = 6, T = 1): 96 KiB of records and 6 lists x 5 helper nodes x 4 planes =
// 120 entries, 22.5 KiB, at depth 4.  With the 15 pair lists as well (T = 2): 192 KiB of records.
// Clay(6,2) with pair lists (n = 8, T = 4): 512 KiB of records.
//
// No HIP header and no other unit of the engine but mixed_plan.hpp: the plan and its interpreter
// run -- and are tested -- on the CPU (tests/native/clay_partial_plan_check.cpp).
#pragma once

#include <cstdint>
#include <vector>

#include "mixed_plan.hpp"

namespace ecx {

struct ClayPartialPlan {
    std::vector<uint32_t> entries;  // padded, concatenated in (list, node, tile) order; never empty
    std::vector<uint32_t> tiles;    // kMixedRecords * n * tiles_per_pattern * kMixedTileDwords
    int npatterns = 0;
    int n = 0;  // nodes per stripe
    int tiles_per_pattern = 1;
    int depth = 4;        // every record's entry count is a multiple of it
    int max_rows = 0;     // the largest row count of any record: which ROWS instance can run it
    int max_entries = 0;  // the largest unpadded entry count of any record
    int min_entries = 0;  // the smallest unpadded entry count of a record that has entries (0: none has)
};

// The load-ring depth of a plan by CompiledMap::preferred_depth's rule over its records: 8 only
// if every record that has entries has at least 12, else 4.
int clay_partial_depth(const ClayPartialPlan &p);

// Cuts `tiled` (of any depth: its padding entries are dropped) by node for a code of n nodes and
// pads for `depth`.  False -- and *out untouched -- when n is outside 1..255, depth is not
// positive, out is null or `tiled` breaks its own invariants (array sizes, entries outside the
// array).
bool build_clay_partial_plan(const TiledPlan &tiled, int n, int depth, ClayPartialPlan *out);

// The plan applied to one stripe as k_gf_map_partial_mixed reads it for id byte `id` and node byte
// `node` (any bytes): plane z of the helper's node lies at in + z * in_sub_stride, row r of the
// running sum at acc + r * acc_sub_stride, `len` bytes each.  The output slots of the T records
// are assigned (is_first) or XOR-accumulated; a record without rows, and when accumulating one
// without entries, touches nothing, and node >= n touches nothing at all.  Padding entries read
// nothing.  False when a record breaks the plan's invariants (array sizes, an entry count that is
// no multiple of the depth, entries outside the array, a padding entry with coefficients).
bool emulate_clay_partial(const ClayPartialPlan &p, uint8_t id, uint8_t node, const uint8_t *in, int64_t in_sub_stride,
                          uint8_t *acc, int64_t acc_sub_stride, int64_t len, bool is_first);

}  // namespace ecx
