// apply_map_mixed.hip -- k_gf_map_mixed: ClayCodeErasureDecodingStep.performCoding
// (ClayCodeErasureDecodingStep.java:53-107) over device-resident stripes that lost different
// nodes, out of place and in one launch.
//
// The plan of a pattern set (mixed_plan.hpp TiledPlan) holds the repair maps of up to 256
// erased-node lists as [256][T] tile records over one entry array.  One workgroup covers one
// (stripe, 4 KiB chunk, tile), the tile index fastest: the T workgroups of a (stripe, chunk) are
// neighbours in the grid and run at about the same time.  Under MI355X's round-robin dispatch
// neighbouring workgroups sit on different XCDs (apply.hpp logical_block), so the inputs that
// several tiles read meet in the memory-side cache, not in one XCD's L2; keeping a unit's tiles on
// one XCD, as k_gf_apply's xcd_group 2 does, is not done here.  A
// workgroup reads its stripe's pattern id -- one byte of a device array the caller wrote, an
// ordinary global load as in apply_mixed.hip -- makes it wave-uniform and runs mixed_tile
// (mixed_pass.hpp) on record id * T + tile with separate input and output bases, strides and slot
// strides.  Every (id byte, tile < T) pair names a record inside the plan and the ones without a
// tile have no rows, so there is no bounds branch: such a workgroup leaves before it touches any
// data.
#include <algorithm>

#include "mixed_pass.hpp"

namespace ecx {

template <bool SAFE, int DEPTH, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_APPLY_BOUNDS(ROWS, DEPTH)) k_gf_map_mixed(ApplyArgs a,
                                                                                              const uint8_t *ids) {
    // (a launch covers whole stripes: gridDim.x = stripes x n_chunks x T)
    const uint32_t T = (uint32_t)a.n_tiles, nc = (uint32_t)a.n_chunks;
    const uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x % T);
    const uint32_t unit = blockIdx.x / T;
    const int64_t s = (int64_t)(unit / nc) + a.stripe_begin;
    const int64_t c = (int64_t)(unit % nc) + a.chunk_begin;
    const uint32_t id = __builtin_amdgcn_readfirstlane((uint32_t)((const gu8 *)ids)[s]);
    mixed_tile<SAFE, DEPTH, ROWS>(a, plan_ptr(a.tiles) + (id * T + t) * kTileDwords, s, c, 0);
}

// The instances are with_mixed_instance's (mixed_pass.hpp).  The byte-safe launch reads the
// depth-4 plan whatever the full chunks run with.
// (A depth-20 instance for sets whose records all have exactly 20 entries -- Clay(4,2), where the
// uniform kernel runs at depth 20 -- was measured and did not beat depth 4 or 8: DESIGN.md 4.7.3.)
void launch_map_mixed(PatternSet &set, const uint8_t *ids, const uint8_t *in, int64_t in_stripe_stride,
                      int64_t in_slot_stride, uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride,
                      int64_t units, int64_t nbytes, int64_t first_unit, hipStream_t stream) {
    const TiledPlan &hp = set.plan(4);
    if (units <= 0 || nbytes <= 0 || hp.max_rows == 0) return;
    if (first_unit < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "bad first unit");
    const int T = hp.tiles_per_pattern;
    const BatchLayout b{(uintptr_t)in, (uintptr_t)out, in_stripe_stride, in_slot_stride, out_stripe_stride,
                        out_slot_stride, units,         nbytes,           false};
    MixedPass pass{units, nbytes, 1, first_unit, T, b.aligned16(), hp.max_rows, set.preferred_depth()};
    pass.too_large = "buf_size is too large for one launch";
    pass.what = "k_gf_map_mixed launch";
    // (input bytes, for the launch registry: as if every stripe read its longest pattern)
    uint32_t inputs = 0;
    for (int p = 0; p < hp.npatterns; ++p) {
        uint32_t sum = 0;
        for (int t = 0; t < T; ++t) sum += hp.tiles[((size_t)p * T + t) * kTileDwords + 3];
        inputs = std::max(inputs, sum);
    }
    pass.inputs = inputs;

    ApplyArgs a = mixed_apply_args(in, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nbytes, T,
                                   false);
    const PatternDevicePlan *plan = nullptr, *plan_safe = nullptr;
    run_mixed_pass(
        pass, stream,
        [&](int depth, int64_t full, int64_t rest) {
            if (full > 0) plan = &set.plan_for_current_device(depth, "the pattern set's tiled device plan");
            if (rest > 0) plan_safe = &set.plan_for_current_device(4, "the pattern set's tiled device plan");
            a.zero_page = zero_page_for_current_device();
        },
        [&](auto safe, auto depth, auto rows, const MixedStep &st) {
            constexpr bool SAFE = decltype(safe)::value;
            constexpr int D = decltype(depth)::value, R = decltype(rows)::value;
            st.aim(a, SAFE ? *plan_safe : *plan);
            a.tiles = (SAFE ? plan_safe : plan)->records;
            if (!SAFE) note_kernel("k_gf_map_mixed", SAFE, D, R);
            // (the kernel indexes its ids by unit_begin + the local unit)
            hipLaunchKernelGGL((k_gf_map_mixed<SAFE, D, R>), st.grid, dim3(kBlockThreads), 0, stream, a, ids + first_unit);
        });
}

}  // namespace ecx
