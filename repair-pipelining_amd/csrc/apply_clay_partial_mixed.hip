// apply_clay_partial_mixed.hip -- k_gf_map_partial_mixed: one hop of the pipelined Clay repair
// chain (ClayCoordinator.kt:265-319, ClayCodeNode.kt:165-233) over device-resident stripes that
// each name their erased-node list and the node this helper holds for them (DESIGN.md section
// 4.7.4).
//
// A Clay pattern set's partial plan (clay_partial_plan.hpp) holds one tile record per (list, node,
// tile), [256][n][T] over one entry array.  One workgroup covers one (stripe, 4 KiB chunk, tile),
// the tile index fastest, as in k_gf_map_mixed.  It reads its stripe's list id and node byte --
// two independent bytes of device arrays the caller wrote, ordinary global loads, not the constant
// path the plan goes through: the caller may rewrite them between two replays of a graph -- makes
// both wave-uniform and leaves when the node byte is no node.  Otherwise record
// (id * n + node) * T + tile lies inside the plan whatever the two arrays hold; the workgroup
// leaves when the record has no rows, or when the hop accumulates and the record has no entries (a
// node the list does not read adds nothing).  What remains is mixed_tile (mixed_pass.hpp) over the
// node's own planes -- the entry's slot is the plane -- with ApplyArgs::accumulate: the load ring,
// then the old rows XORed in when the hop accumulates, then the stores.  A first hop whose record
// has no entries stores zeros to the tile's rows.
#include "mixed_pass.hpp"

namespace ecx {

struct ClayPartialSel {
    const uint8_t *ids;    // per stripe: the erased-node list
    const uint8_t *nodes;  // per stripe: the node this helper holds
    int64_t in_node_stride;
    uint32_t n;  // nodes per stripe
};

template <bool SAFE, int DEPTH, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_APPLY_BOUNDS(ROWS, DEPTH)) k_gf_map_partial_mixed(ApplyArgs a,
                                                                                                      ClayPartialSel q) {
    // (a launch covers whole stripes: gridDim.x = stripes x n_chunks x T)
    const uint32_t T = (uint32_t)a.n_tiles, nc = (uint32_t)a.n_chunks;
    const uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x % T);
    const uint32_t unit = blockIdx.x / T;
    const int64_t s = (int64_t)(unit / nc) + a.stripe_begin;
    const int64_t c = (int64_t)(unit % nc) + a.chunk_begin;
    const uint32_t idb = ((const gu8 *)q.ids)[s], ndb = ((const gu8 *)q.nodes)[s];  // both in flight
    const uint32_t id = __builtin_amdgcn_readfirstlane(idb);
    const uint32_t node = __builtin_amdgcn_readfirstlane(ndb);
    if (node >= q.n) return;  // wave-uniform: the whole workgroup leaves
    // id < 256 and node < n: the record is inside the plan
    cu32 *tile = plan_ptr(a.tiles) + ((id * q.n + node) * T + t) * kTileDwords;
    if (a.accumulate && tile[1] == 0) return;  // a node the list does not read adds nothing
    mixed_tile<SAFE, DEPTH, ROWS>(a, tile, s, c, (int64_t)node * q.in_node_stride);
}

// The instances are with_mixed_instance's (mixed_pass.hpp), as launch_map_mixed's; the byte-safe
// launch reads the depth-4 plan.
void launch_clay_partial_mixed(PatternSet &set, int n, const uint8_t *ids, const uint8_t *nodes, const uint8_t *in,
                               int64_t in_stripe_stride, int64_t in_node_stride, int64_t in_sub_stride, uint8_t *acc,
                               int64_t acc_stripe_stride, int64_t acc_sub_stride, int64_t nstripes, int64_t nbytes,
                               bool is_first, hipStream_t stream) {
    if (nstripes <= 0 || nbytes <= 0 || set.plan(4).max_rows == 0) return;
    const ClayPartialPlan &hp = set.clay_partial_plan(n, 4);
    const int T = hp.tiles_per_pattern;
    // (the node stride moves the base only: a multiple of 16 keeps every lane's loads aligned)
    const BatchLayout b{(uintptr_t)in,  (uintptr_t)acc, in_stripe_stride, in_sub_stride, acc_stripe_stride,
                        acc_sub_stride, nstripes,       nbytes,           !is_first};
    MixedPass pass{nstripes,    nbytes, 1, 0, T, b.aligned16() && in_node_stride % 16 == 0,
                   hp.max_rows, clay_partial_depth(hp)};
    pass.too_large = "buf_size is too large for one launch";
    pass.what = "k_gf_map_partial_mixed launch";
    // (input bytes, for the launch registry: as if every stripe read its node's longest record)
    pass.inputs = hp.max_entries;

    ApplyArgs a = mixed_apply_args(in, in_stripe_stride, in_sub_stride, acc, acc_stripe_stride, acc_sub_stride, nbytes, T,
                                   !is_first);
    const ClayPartialSel q{ids, nodes, in_node_stride, (uint32_t)n};
    const PatternDevicePlan *plan = nullptr, *plan_safe = nullptr;
    run_mixed_pass(
        pass, stream,
        [&](int depth, int64_t full, int64_t rest) {
            if (full > 0) plan = &set.clay_partial_plan_for_current_device(n, depth);
            if (rest > 0) plan_safe = &set.clay_partial_plan_for_current_device(n, 4);
            a.zero_page = zero_page_for_current_device();
        },
        [&](auto safe, auto depth, auto rows, const MixedStep &st) {
            constexpr bool SAFE = decltype(safe)::value;
            constexpr int D = decltype(depth)::value, R = decltype(rows)::value;
            st.aim(a, SAFE ? *plan_safe : *plan);
            a.tiles = (SAFE ? plan_safe : plan)->records;
            if (!SAFE) note_kernel("k_gf_map_partial_mixed", SAFE, D, R);
            hipLaunchKernelGGL((k_gf_map_partial_mixed<SAFE, D, R>), st.grid, dim3(kBlockThreads), 0, stream, a, q);
        });
}

}  // namespace ecx
