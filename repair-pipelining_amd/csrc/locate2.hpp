// locate2.hpp -- the HIP side of the pair plan (locate2_plan.hpp; include/ecx.h
// ecx_rs_locate_corrupt2_batch): the plan uploaded lazily per device, and
// the launches that name up to two corrupt shards of every stripe that fails the parity check
// (apply_locate2.hip).
#pragma once

#include "locate.hpp"
#include "locate2_plan.hpp"

namespace ecx {

struct Locate2DevicePlan {
    uint32_t *entries = nullptr;
    uint32_t *tiles = nullptr;
    uint16_t *members = nullptr;  // pair p: i in the low byte, j in the high one
};

// A code's pair plan and its device copies; lives as long as the codec (ecx_api.cpp).
class Locate2Set {
public:
    explicit Locate2Set(Locate2Plan p) : plan_(std::move(p)) {}
    ~Locate2Set();
    Locate2Set(const Locate2Set &) = delete;
    Locate2Set &operator=(const Locate2Set &) = delete;
    const Locate2Plan &plan() const { return plan_; }
    // As LocateSet::plan_for_current_device: a first-use site, refused on a capturing stream.
    const Locate2DevicePlan &plan_for_current_device();

private:
    Locate2Plan plan_;
    std::mutex mu_;
    std::map<int, Locate2DevicePlan> dev_;  // by device
};

// launch_locate's arguments and layout, with suspect rows of n + C(n,2) bytes (the n single
// suspects, then the pair suspects in lexicographic pair order), culprit[s][0..1] and heal_id[s]
// (or null):
//   all n singles set                     (-1, -1)   255
//   exactly one single, j                 (j, -1)    j
//   no single, exactly one pair p = {i,j} (i, j)     n + p
//   anything else                         (-2, -2)   255
// `cm` is the code's check map, `ls` its locate plan, `l2` its pair plan.  Read-only on the stripes.
void launch_locate2(CompiledMap &cm, LocateSet &ls, Locate2Set &l2, const uint8_t *in, int64_t in_stripe_stride,
                    int64_t in_slot_stride, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id, int64_t nstripes,
                    int64_t nbytes, hipStream_t stream);
// The same over a blocked batch of n-shard stripes, as launch_locate_blocked.
void launch_locate2_blocked(CompiledMap &cm, LocateSet &ls, Locate2Set &l2, const uint8_t *base, int n,
                            int64_t nstripes, int64_t byte_count, int64_t block, uint8_t *suspect, int32_t *culprit,
                            uint8_t *heal_id, hipStream_t stream);

}  // namespace ecx
