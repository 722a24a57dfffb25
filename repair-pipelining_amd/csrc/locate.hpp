// locate.hpp -- the HIP side of the locate plan (locate_plan.hpp; include/ecx.h
// ecx_rs_locate_corrupt_batch): the plan uploaded lazily per device, and the
// launches that name the corrupt shard of every stripe that fails the parity check
// (apply_locate.hip).
#pragma once

#include "blocked_layout.hpp"
#include "engine.hpp"
#include "locate_plan.hpp"

namespace ecx {

// locate_plan.hpp repeats the plan format's constants so that it needs no HIP header
static_assert(kLocateEntryDwords == kEntryDwords && kLocateTileDwords == kTileDwords && kLocateTileRows == kTileRows,
              "locate_plan.hpp and engine.hpp describe one plan format");

struct LocateDevicePlan {
    uint32_t *entries = nullptr;
    uint32_t *tiles = nullptr;
};

// A code's locate plan and its device copies; lives as long as the codec (ecx_api.cpp).
class LocateSet {
public:
    explicit LocateSet(LocatePlan p) : plan_(std::move(p)) {}
    ~LocateSet();
    LocateSet(const LocateSet &) = delete;
    LocateSet &operator=(const LocateSet &) = delete;
    const LocatePlan &plan() const { return plan_; }
    // The plan uploaded for the current device, lazily, like CompiledMap::plan_for_current_device.
    // A first-use site: refused on a capturing stream (engine.hpp refuse_if_capturing).
    const LocateDevicePlan &plan_for_current_device();

private:
    LocatePlan plan_;
    std::mutex mu_;
    std::map<int, LocateDevicePlan> dev_;  // by device
};

// For stripe s of [stripe][shard][bytes] at `in`, over bytes [0, nbytes) of each shard: suspect[s][j]
// (device bytes, n per stripe) = 1 when replacing shard j alone can make the stripe pass the
// parity check, else 0; culprit[s] (device int32) = -1 for a clean stripe (all n suspects), j for
// exactly one suspect, -2 otherwise; heal_id[s] (device bytes, or null) = j when culprit[s] == j,
// else 255.  `cm` is the code's check map (one tile: m <= 8), `ls` its locate plan.  Read-only on
// the stripes.
void launch_locate(CompiledMap &cm, LocateSet &ls, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                   uint8_t *suspect, int32_t *culprit, uint8_t *heal_id, int64_t nstripes, int64_t nbytes,
                   hipStream_t stream);
// The same over a blocked batch of n-shard stripes (blocked_layout.hpp), from the layout's body
// and tail passes: both only ever clear suspects, so a shard stays one when it explains every
// block of its stripe and the tail.
void launch_locate_blocked(CompiledMap &cm, LocateSet &ls, const uint8_t *base, int n, int64_t nstripes,
                           int64_t byte_count, int64_t block, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id,
                           hipStream_t stream);

// suspect[i] = 1 for all nstripes * n bytes (k_set_suspects): what every locate starts with, n being
// the bytes of a stripe's suspect row.
void set_suspects(uint8_t *suspect, int64_t nstripes, int n, hipStream_t stream);

}  // namespace ecx
