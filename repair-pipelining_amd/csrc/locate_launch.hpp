// locate_launch.hpp -- the launch skeleton that k_gf_locate (apply_locate.hip) and k_gf_locate2
// (apply_locate2.hip) share: launch_check_core's (apply_check.hip) at ring depth 4, over suspect
// rows of `row_bytes` bytes per stripe.  The vectorised kernel takes the full chunks and, as a
// shifted full window, a partial last chunk that is a multiple of 16 B; the byte-safe kernel takes
// what is left; a launch holds at most 2^30 workgroups.  launch_k(safe, rows, grid, a, vd) launches
// one instance.
#pragma once

#include <algorithm>
#include <string>

#include "apply.hpp"
#include "blocked_layout.hpp"

namespace ecx {

// Clears suspect[s / divisor][...] from bytes [0, nbytes) of stripe (unit) s.
template <class LaunchK>
void launch_locate_passes(CompiledMap &cm, int row_bytes, const uint8_t *in, int64_t in_stripe_stride,
                          int64_t in_slot_stride, uint8_t *suspect, int64_t nstripes, int64_t nbytes, int64_t divisor,
                          const char *what, LaunchK &&launch_k) {
    const Tuning &tu = tuning();
    const int rows = cm.max_tile_rows() <= 4 ? 4 : kTileRows;
    const bool aligned = aligned16(in) && in_stripe_stride % 16 == 0 && in_slot_stride % 16 == 0;
    const int64_t full = aligned ? nbytes / kChunkBytes : 0;
    const int64_t tail = nbytes - full * kChunkBytes;
    // the partial last chunk as a shifted full window (read-only: overlap is re-checked)
    const bool fuse_tail = aligned && full >= 1 && tail > 0 && tail % 16 == 0;
    const DevicePlan &plan = cm.plan_for_current_device(4);

    ApplyArgs a{};
    a.in = in;
    a.out = suspect;
    a.zero_page = zero_page_for_current_device();
    a.in_stripe_stride = in_stripe_stride;
    a.in_slot_stride = in_slot_stride;
    a.out_stripe_stride = row_bytes;
    a.out_slot_stride = 1;
    a.nbytes = nbytes;
    a.n_tiles = cm.n_tiles();
    a.stagger = tu.stagger;
    const bool misaligned128 = ((uintptr_t)in % 128) != 0 || in_stripe_stride % 128 != 0 || in_slot_stride % 128 != 0;
    a.xcd_group = tu.xcd_group == 3 ? 3 : (tu.xcd_misaligned && misaligned128 ? 3 : 0);
    a.xcd_run = tu.xcd_run;
    a.tail_chunk = fuse_tail ? full : -1;
    a.entries = plan.entries;
    a.tiles = plan.tiles;
    auto run = [&](bool safe, int64_t chunk_begin, int64_t n_chunks) {
        if (n_chunks <= 0) return;
        a.chunk_begin = chunk_begin;
        a.n_chunks = n_chunks;
        const int64_t per_stripe = n_chunks * a.n_tiles;
        const int64_t stripes_per_launch = std::max<int64_t>(1, ((int64_t)1 << 30) / per_stripe);
        for (int64_t s0 = 0; s0 < nstripes; s0 += stripes_per_launch) {
            a.stripe_begin = s0;
            const dim3 grid((unsigned)(std::min(stripes_per_launch, nstripes - s0) * per_stripe));
            // blocked: the launch's suspect rows start at its first unit's stripe (launch_check_core)
            const VerdictDiv vdiv = divisor > 1 ? verdict_div(divisor, s0) : VerdictDiv{};
            a.out = divisor > 1 ? suspect + (s0 / divisor) * row_bytes : suspect;
            launch_k(safe, rows, grid, a, divisor > 1 ? &vdiv : nullptr);
        }
    };
    const uint64_t notes0 = kernel_notes();
    if (fuse_tail) {
        run(false, 0, full + 1);
    } else {
        run(false, 0, full);
        a.tail_chunk = -1;
        run(true, full, (tail + kChunkBytes - 1) / kChunkBytes);  // (not noted: byte-safe)
    }
    if (kernel_notes() != notes0)
        set_last_shape_order("stagger=" + std::to_string(a.stagger) + " xcd_group=" + std::to_string(a.xcd_group) +
                             " xcd_run=" + std::to_string(a.xcd_group == 3 ? a.xcd_run : 0));
    check_hip(hipGetLastError(), what);
}

}  // namespace ecx
