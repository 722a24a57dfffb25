// pattern_set.hpp -- the HIP side of a pattern set (include/ecx.h ecx_rs_pattern_set): several
// single-tile maps of one codec compiled into one device plan (mixed_plan.hpp has the format and
// is HIP-free), uploaded lazily per device, and the launch that decodes a batch whose stripes
// name their pattern with one byte each (apply_mixed.hip).
#pragma once

#include "engine.hpp"
#include "mixed_plan.hpp"

namespace ecx {

// mixed_plan.hpp repeats the plan format's constants so that it needs no HIP header
static_assert(kMixedEntryDwords == kEntryDwords && kMixedTileDwords == kTileDwords && kMixedTileRows == kTileRows &&
                  kMixedDummySlot == kDummySlot,
              "mixed_plan.hpp and engine.hpp describe one plan format");

struct MixedDevicePlan {
    uint32_t *entries = nullptr;
    uint32_t *tiles = nullptr;  // kMixedRecords records
};

// The maps are only read while the set is built.
class PatternSet {
public:
    // Throws ECX_E_ILLEGAL_ARGUMENT for an empty list, more than kMixedRecords maps or a map of
    // more than one tile.
    explicit PatternSet(const std::vector<const CompiledMap *> &maps);
    ~PatternSet();
    PatternSet(const PatternSet &) = delete;
    PatternSet &operator=(const PatternSet &) = delete;
    // The set's load-ring depth (mixed_depth's rule), and the host plan padded for depth 4 or 8
    // (the other one only runs when ecx_tune "depth" forces it, as for a CompiledMap).
    int preferred_depth() const { return preferred_depth_; }
    const MixedPlan &plan(int depth) const { return depth == 8 ? plan8_ : plan4_; }
    int max_rows() const { return plan4_.max_rows; }
    // The plan uploaded for the current device, lazily, like CompiledMap::plan_for_current_device.
    // A first-use site: refused on a capturing stream (engine.hpp refuse_if_capturing).
    const MixedDevicePlan &plan_for_current_device(int depth);

private:
    MixedPlan plan4_, plan8_;
    int preferred_depth_ = 4;
    std::mutex mu_;
    std::map<std::pair<int, int>, MixedDevicePlan> dev_;  // (device, depth)
};

// decodeMissing with a pattern per stripe, in place (apply_mixed.hip k_gf_apply_mixed): stripe s
// of [stripe][slot][bytes] at `base` is run through record ids[s] of the set's plan over bytes
// [0, nbytes) of each slot; `ids` is a device byte array of nstripes.  A record with no rows
// leaves its stripe untouched.
void launch_apply_mixed(PatternSet &set, const uint8_t *ids, uint8_t *base, int64_t stripe_stride,
                        int64_t slot_stride, int64_t nstripes, int64_t nbytes, hipStream_t stream);

}  // namespace ecx
