// pattern_set.hpp -- the HIP side of a pattern set (include/ecx.h ecx_rs_pattern_set,
// ecx_clay_pattern_set): several maps of one codec compiled into one device plan (mixed_plan.hpp
// has the format and is HIP-free), uploaded lazily per device, and the launches that run a batch
// whose stripes name their pattern with one byte each: in place over single-tile maps
// (apply_mixed.hip, the RS decodes) and out of place over maps of up to kMixedMaxTiles tiles
// (apply_map_mixed.hip, the Clay repair), and the partial-sum hops of both
// (apply_partial_mixed.hip, apply_clay_partial_mixed.hip).
#pragma once

#include <tuple>

#include "blocked_layout.hpp"
#include "clay_partial_plan.hpp"
#include "engine.hpp"
#include "mixed_plan.hpp"
#include "partial_plan.hpp"

namespace ecx {

// mixed_plan.hpp repeats the plan format's constants so that it needs no HIP header
static_assert(kMixedEntryDwords == kEntryDwords && kMixedTileDwords == kTileDwords && kMixedTileRows == kTileRows &&
                  kMixedDummySlot == kDummySlot,
              "mixed_plan.hpp and engine.hpp describe one plan format");
static_assert(kPartialEntryDwords == kEntryDwords && kPartialRows == kTileRows && kPartialRecords == kMixedRecords,
              "partial_plan.hpp and engine.hpp describe one plan format");

// A plan of a set on one device: its entries and its records -- tile records (kTileDwords each),
// or the row counts of the RS partial-sum plan.
struct PatternDevicePlan {
    uint32_t *entries = nullptr;
    uint32_t *records = nullptr;
};

// The maps are read while the set is built, and once more when its partial-sum plan is (the first
// ecx_rs_decode_partial_batch_mixed with the set): they must live as long as the set does.  The
// codec a set holds a reference on keeps them.
class PatternSet {
public:
    // Throws ECX_E_ILLEGAL_ARGUMENT for an empty list, more than kMixedRecords maps or a map of
    // more than kMixedMaxTiles tiles.
    explicit PatternSet(const std::vector<const CompiledMap *> &maps);
    ~PatternSet();
    PatternSet(const PatternSet &) = delete;
    PatternSet &operator=(const PatternSet &) = delete;
    // The set's load-ring depth (tiled_depth's rule), and the host plan (mixed_plan.hpp) padded for
    // depth 4 or 8 (anything else is 4; the other one only runs when ecx_tune "depth" forces it,
    // as for a CompiledMap).
    int preferred_depth() const { return depth_; }
    const TiledPlan &plan(int depth) const { return depth == 8 ? plan8_ : plan4_; }
    // Tiles per pattern, and the largest output slot of any pattern (-1: no pattern writes anything).
    int tiles_per_pattern() const { return plan4_.tiles_per_pattern; }
    int max_out_slot() const { return plan4_.max_out_slot; }
    // The largest row count of the set when every map has one tile, 0 when a map has several: the
    // in-place launches and the RS partial hop read record `id` alone, and do nothing with such a
    // set (plan(4).max_rows is the largest tile's, whatever T).
    int max_rows() const { return plan4_.tiles_per_pattern == 1 ? plan4_.max_rows : 0; }
    // What an out-of-place host batch moves (host_pipe.cpp run_host_map_mixed_batch), sorted:
    // in_slots is the union of the patterns' input slots, out_slots every slot 0..max_out_slot().
    const std::vector<int> &in_slots() const { return in_slots_; }
    const std::vector<int> &out_slots() const { return out_slots_; }
    // What a host batch moves (host_pipe.cpp run_host_mixed_batch), sorted: down_slots is the union
    // of the patterns' output slots, up_slots the union of every pattern's input AND output slots.
    // A stripe gets every down slot back, also one its own pattern leaves alone, so each of them
    // must have gone up for every stripe even where no pattern reads it.
    const std::vector<int> &up_slots() const { return up_slots_; }
    const std::vector<int> &down_slots() const { return down_slots_; }
    // plan(depth) uploaded for the current device, lazily, like CompiledMap::plan_for_current_device.
    // A first-use site: refused on a capturing stream (engine.hpp refuse_if_capturing) as `what`.
    const PatternDevicePlan &plan_for_current_device(int depth, const char *what);
    // The partial-sum plan (partial_plan.hpp) for a code of n shards, built on the first call --
    // creating a set costs nothing for it -- and its upload for the current device, lazily, a
    // first-use site like plan_for_current_device.
    const PartialPlan &partial_plan(int n);
    const PatternDevicePlan &partial_plan_for_current_device(int n);
    // The Clay partial-sum plan (clay_partial_plan.hpp: the plan cut by input node) for a code of
    // n nodes, padded for depth 4 or 8 (anything else is 4); both are built on the first call,
    // and uploaded for the current device lazily, a first-use site like the others.
    const ClayPartialPlan &clay_partial_plan(int n, int depth);
    const PatternDevicePlan &clay_partial_plan_for_current_device(int n, int depth);

private:
    enum PlanKind { kPlan, kPartial, kClayPartial };
    // The one upload path: the two host arrays of a plan on the current device, cached by (kind,
    // device, depth).  Refuses a first use under capture as `what`; a half-uploaded plan is
    // never published.
    const PatternDevicePlan &resident(PlanKind kind, int depth, const std::vector<uint32_t> &entries,
                                      const std::vector<uint32_t> &records, const char *what);

    std::vector<const CompiledMap *> maps_;
    PartialPlan partial_;  // npatterns == 0: not built yet
    ClayPartialPlan clay_partial4_, clay_partial8_;  // npatterns == 0: not built yet
    TiledPlan plan4_, plan8_;
    int depth_ = 4;
    std::vector<int> up_slots_, down_slots_, in_slots_, out_slots_;
    std::mutex mu_;
    std::map<std::tuple<int, int, int>, PatternDevicePlan> dev_;  // (kind, device, depth)
};

// decodeMissing with a pattern per stripe, in place (apply_mixed.hip k_gf_apply_mixed): stripe s
// of [stripe][slot][bytes] at `base` is run through record ids[s] of the set's plan over bytes
// [0, nbytes) of each slot; `ids` is a device byte array of nstripes.  A record with no rows
// leaves its stripe untouched.
void launch_apply_mixed(PatternSet &set, const uint8_t *ids, uint8_t *base, int64_t stripe_stride,
                        int64_t slot_stride, int64_t nstripes, int64_t nbytes, hipStream_t stream);
// The general form: `units` units of [unit][slot][bytes] at `base`, `divisor` consecutive ones per
// caller stripe (a pass of a blocked batch, blocked_layout.hpp), the first of them unit
// `first_unit` of the whole pass -- a chunk of the host pipeline may begin mid-stripe.  `ids` is
// the id of the whole pass's first stripe: unit u runs record ids[(first_unit + u) / divisor].
// Divisor 1 is launch_apply_mixed's kernel; above it k_gf_apply_mixed_blocked divides on the
// device (mixed_launch.hpp has the split into launches).
void launch_apply_mixed_units(PatternSet &set, const uint8_t *ids, uint8_t *base, int64_t stripe_stride,
                              int64_t slot_stride, int64_t units, int64_t nbytes, int64_t divisor,
                              int64_t first_unit, hipStream_t stream);
// Every pass of a blocked batch at `base`, in place; `ids` is a device byte array of the batch's
// caller stripes.
void launch_apply_mixed_blocked(PatternSet &set, const uint8_t *ids, uint8_t *base, const BlockedPlan &plan,
                                hipStream_t stream);

// One hop of the partial-sum chain with a pattern and a helper shard per stripe
// (apply_partial_mixed.hip k_gf_partial_mixed; ecx.h ecx_rs_decode_partial_batch_mixed has the
// meaning): `ids` and `shards` are device byte arrays of nstripes, n the code's shard count.
void launch_partial_mixed(PatternSet &set, int n, const uint8_t *ids, const uint8_t *shards, const uint8_t *in,
                          int64_t in_stripe_stride, int64_t in_shard_stride, uint8_t *acc, int64_t acc_stripe_stride,
                          int64_t acc_row_stride, int64_t nstripes, int64_t nbytes, bool is_first, hipStream_t stream);

// One hop of the Clay partial-sum chain with a list and a helper node per stripe
// (apply_clay_partial_mixed.hip k_gf_map_partial_mixed; ecx.h ecx_clay_partial_batch_mixed has the
// meaning): `ids` and `nodes` are device byte arrays of nstripes, n the code's node count.
void launch_clay_partial_mixed(PatternSet &set, int n, const uint8_t *ids, const uint8_t *nodes, const uint8_t *in,
                               int64_t in_stripe_stride, int64_t in_node_stride, int64_t in_sub_stride, uint8_t *acc,
                               int64_t acc_stripe_stride, int64_t acc_sub_stride, int64_t nstripes, int64_t nbytes,
                               bool is_first, hipStream_t stream);

// A map with a pattern per stripe, out of place (apply_map_mixed.hip k_gf_map_mixed): unit u of
// [unit][slot][bytes] at `in` is run through records (ids[first_unit + u], 0..T) of the set's
// plan over bytes [0, nbytes) of each slot, into [unit][slot][bytes] at `out`; `ids` is a
// device byte array.  Only a record's own output slots are written; a unit whose id has no rows
// is left untouched.  `in` and `out` must not overlap.
void launch_map_mixed(PatternSet &set, const uint8_t *ids, const uint8_t *in, int64_t in_stripe_stride,
                      int64_t in_slot_stride, uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride,
                      int64_t units, int64_t nbytes, int64_t first_unit, hipStream_t stream);

}  // namespace ecx
