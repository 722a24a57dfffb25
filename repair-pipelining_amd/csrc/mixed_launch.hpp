// mixed_launch.hpp -- how a mixed decode over one pass of units is cut into launches
// (apply_mixed.hip launch_apply_mixed_units).
//
// A pass is `units` units of n equal slots (blocked_layout.hpp: the block rows of a blocked
// batch's body, its tails, or the stripes of a natural batch), `divisor` consecutive ones per
// caller stripe, and the ids name a pattern per caller stripe.  The pass handed to the launcher
// may begin mid-stripe -- the host pipeline (host_pipe.cpp run_host_mixed_batch) streams chunks
// of units -- so it says which unit of the whole pass its first one is (`first_unit`).  A grid
// is capped in workgroups, so a launch covers at most cap / (workgroups per unit) units, one at
// least.  Launch l then covers units [unit_begin, unit_begin + unit_count) of the handed pass,
// reads its ids from id_begin on -- the caller stripe of its first unit, relative to the stripe
// of the WHOLE pass's unit 0 -- and finds the stripe of its local unit u as
// id_begin + verdict_quot(vd, u), vd.rem being the first unit's place in its stripe.
//
// No HIP header: the split is walked on the CPU with a tiny cap
// (tests/native/mixed_launch_check.cpp).
#pragma once

#include <cstdint>

#include "blocked_layout.hpp"

namespace ecx {

constexpr int64_t kMixedMaxBlocks = (int64_t)1 << 30;  // workgroups of one launch

struct MixedLaunch {
    int64_t unit_begin = 0;  // in the handed pass
    int64_t unit_count = 0;
    int64_t id_begin = 0;    // (first_unit + unit_begin) / divisor
    VerdictDiv vd;           // divisor 1: unused (the unit is the stripe)
};

// Units per launch of a pass whose units take blocks_per_unit workgroups each.
inline int64_t mixed_units_per_launch(int64_t blocks_per_unit, int64_t max_blocks) {
    const int64_t per = blocks_per_unit > 0 ? max_blocks / blocks_per_unit : max_blocks;
    return per < 1 ? 1 : per;
}

// f(const MixedLaunch &) for each launch of the pass, in unit order.  divisor >= 1,
// first_unit >= 0; nothing is called for units <= 0.
template <class F>
void for_mixed_launches(int64_t units, int64_t blocks_per_unit, int64_t divisor, int64_t first_unit,
                        int64_t max_blocks, F &&f) {
    const int64_t per = mixed_units_per_launch(blocks_per_unit, max_blocks);
    for (int64_t u0 = 0; u0 < units; u0 += per) {
        MixedLaunch l;
        l.unit_begin = u0;
        l.unit_count = units - u0 < per ? units - u0 : per;
        l.id_begin = (first_unit + u0) / divisor;
        if (divisor > 1) l.vd = verdict_div(divisor, first_unit + u0);
        f(l);
    }
}

}  // namespace ecx
