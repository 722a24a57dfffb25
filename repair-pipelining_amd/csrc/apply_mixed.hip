// apply_mixed.hip -- k_gf_apply_mixed: ReedSolomon.decodeMissing (ReedSolomon.java:189-286) over
// device-resident stripes that miss different shards, in one launch.
//
// A pattern set (mixed_plan.hpp, pattern_set.hpp) holds the decode maps of up to 256 erasure patterns
// of one codec as one plan: the patterns' padded entry arrays back to back and, every map having
// one tile, 256 tile records.
// One workgroup covers one (stripe, 4 KiB chunk), stripe-major.  It reads its stripe's pattern id
// -- one byte of a device array the caller wrote -- makes it wave-uniform, and runs apply_tile
// (apply.hpp, through mixed_pass.hpp mixed_tile) on record `id` exactly as k_gf_apply runs a single-tile map: the inner loop, the
// load ring and the split-table arithmetic are the same code.  Every byte value names a record of
// the plan (the unused ones have no rows), so there is no bounds branch: a stripe whose record has
// no rows -- nothing missing, or an id without a pattern -- returns before it touches the shards.
//
// The id array is device memory written by an earlier kernel or copy of the caller's stream, so
// it is read with an ordinary global load, not through the constant address space the plan uses.
//
// Over the blocked RS layout (blocked_layout.hpp) the same body runs as
// k_gf_apply_mixed_blocked: a launch's units are the block rows of the layout's body pass, `full`
// consecutive ones per caller stripe, and a unit takes the id of stripe unit / full
// (launch_apply_mixed_units; mixed_launch.hpp cuts a pass into launches).
#include <algorithm>

#include "mixed_pass.hpp"

namespace ecx {

template <bool SAFE, int DEPTH, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_APPLY_BOUNDS(ROWS, DEPTH)) k_gf_apply_mixed(ApplyArgs a,
                                                                                                const uint8_t *ids) {
    // (a launch covers whole stripes: gridDim.x = stripes x n_chunks)
    const uint32_t nc = (uint32_t)a.n_chunks;
    const int64_t s = (int64_t)(blockIdx.x / nc) + a.stripe_begin;
    const int64_t c = (int64_t)(blockIdx.x % nc) + a.chunk_begin;
    const uint32_t id = __builtin_amdgcn_readfirstlane((uint32_t)((const gu8 *)ids)[s]);
    mixed_tile<SAFE, DEPTH, ROWS>(a, plan_ptr(a.tiles) + id * kTileDwords, s, c, 0);
}

// The same body over one pass of a blocked batch (blocked_layout.hpp, mixed_launch.hpp): the
// launch's units are block rows, vd.divisor consecutive ones per caller stripe, so the pattern id
// of a unit is that of stripe unit / divisor.  `ids` points at the id of the launch's first
// unit's stripe and vd.rem is that unit's place in it.  The unit comes from the block index and is
// made wave-uniform first, so the quotient is two scalar multiplies (verdict_quot; gfx950 has no
// scalar divide) ahead of the id load.  A kernel of its own, as k_gf_check_blocked is: the
// natural layout's instances stay what they were.
template <bool SAFE, int DEPTH, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_APPLY_BOUNDS(ROWS, DEPTH))
    k_gf_apply_mixed_blocked(ApplyArgs a, const uint8_t *ids, VerdictDiv vd) {
    const uint32_t nc = (uint32_t)a.n_chunks;
    const uint32_t local_unit = __builtin_amdgcn_readfirstlane(blockIdx.x / nc);
    const int64_t s = (int64_t)local_unit + a.stripe_begin;
    const int64_t c = (int64_t)(blockIdx.x % nc) + a.chunk_begin;
    const uint32_t id = __builtin_amdgcn_readfirstlane((uint32_t)((const gu8 *)ids)[verdict_quot(vd, local_unit)]);
    mixed_tile<SAFE, DEPTH, ROWS>(a, plan_ptr(a.tiles) + id * kTileDwords, s, c, 0);
}

// The instances are with_mixed_instance's (mixed_pass.hpp); the byte-safe one reads the same plan
// as the full chunks (a record padded to a multiple of 8 is padded to a multiple of 4).
//
// The pass is `units` units of which `divisor` consecutive ones are one caller stripe, and its
// first unit is unit `first_unit` of the whole pass `ids` describes: ids[(first_unit + u) / divisor]
// is unit u's pattern.  Divisor 1 (a natural batch, a blocked batch's tails, a body of one block
// per stripe) runs k_gf_apply_mixed, anything else k_gf_apply_mixed_blocked; mixed_launch.hpp
// cuts the pass into launches.
void launch_apply_mixed_units(PatternSet &set, const uint8_t *ids, uint8_t *base, int64_t stripe_stride,
                              int64_t slot_stride, int64_t units, int64_t nbytes, int64_t divisor,
                              int64_t first_unit, hipStream_t stream) {
    if (units <= 0 || nbytes <= 0 || set.max_rows() == 0) return;
    if (divisor < 1 || first_unit < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "bad unit divisor");
    // in place: the alignment conditions of a full-chunk launch are launch_rules' (BatchLayout)
    const BatchLayout b{(uintptr_t)base, (uintptr_t)base, stripe_stride, slot_stride, stripe_stride,
                        slot_stride,     units,           nbytes,        false};
    MixedPass pass{units, nbytes, divisor, first_unit, 1, b.aligned16(), set.max_rows(), set.preferred_depth()};
    pass.too_large = "byte_count is too large for one launch";
    pass.what = "k_gf_apply_mixed launch";
    // (input bytes, for the launch registry: as if every stripe read its longest pattern)
    const TiledPlan &hp = set.plan(4);
    uint32_t inputs = 0;
    for (int p = 0; p < hp.npatterns; ++p) inputs = std::max(inputs, hp.tiles[(size_t)p * kTileDwords + 3]);
    pass.inputs = inputs;

    ApplyArgs a = mixed_apply_args(base, stripe_stride, slot_stride, base, stripe_stride, slot_stride, nbytes, 1, false);
    const PatternDevicePlan *plan = nullptr;
    run_mixed_pass(
        pass, stream,
        [&](int depth, int64_t, int64_t) {
            plan = &set.plan_for_current_device(depth, "the pattern set's device plan");
            a.tiles = plan->records;
            a.zero_page = zero_page_for_current_device();
        },
        [&](auto safe, auto depth, auto rows, const MixedStep &st) {
            constexpr bool SAFE = decltype(safe)::value;
            constexpr int D = decltype(depth)::value, R = decltype(rows)::value;
            st.aim(a, *plan);
            if (divisor > 1) {
                if (!SAFE) note_kernel("k_gf_apply_mixed_blocked", SAFE, D, R);
                hipLaunchKernelGGL((k_gf_apply_mixed_blocked<SAFE, D, R>), st.grid, dim3(kBlockThreads), 0, stream, a,
                                   ids + st.l.id_begin, st.l.vd);
                return;
            }
            // divisor 1: k_gf_apply_mixed indexes its ids by unit_begin + the local unit itself
            if (!SAFE) note_kernel("k_gf_apply_mixed", SAFE, D, R);
            hipLaunchKernelGGL((k_gf_apply_mixed<SAFE, D, R>), st.grid, dim3(kBlockThreads), 0, stream, a, ids + first_unit);
        });
}

void launch_apply_mixed(PatternSet &set, const uint8_t *ids, uint8_t *base, int64_t stripe_stride,
                        int64_t slot_stride, int64_t nstripes, int64_t nbytes, hipStream_t stream) {
    launch_apply_mixed_units(set, ids, base, stripe_stride, slot_stride, nstripes, nbytes, 1, 0, stream);
}

// A mixed decode over a blocked batch: the layout's passes in order, each with its divisor.  The
// first pass makes the set's plan resident before it enqueues anything, so a first use refused
// under capture leaves no node of either pass behind.
void launch_apply_mixed_blocked(PatternSet &set, const uint8_t *ids, uint8_t *base, const BlockedPlan &plan,
                                hipStream_t stream) {
    std::string body_kernel;
    for (int i = 0; i < plan.count; ++i) {
        const BlockedPass &p = plan.pass[i];
        const uint64_t notes0 = kernel_notes();
        launch_apply_mixed_units(set, ids, base + p.offset, p.stripe_stride, p.slot_bytes, p.units, p.slot_bytes,
                                 p.divisor, 0, stream);
        if (i == 0 && kernel_notes() != notes0) body_kernel = last_kernel();
    }
    // the launch of record is the first pass's (the body, nearly all of the bytes), not the tails'
    if (plan.count > 1 && !body_kernel.empty()) set_last_kernel(body_kernel);
}

}  // namespace ecx
