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
// node the list does not read adds nothing).  What remains is apply_tile (apply.hpp) over the
// node's own planes -- the entry's slot is the plane -- with ApplyArgs::accumulate: the load ring,
// then the old rows XORed in when the hop accumulates, then the stores.  A first hop whose record
// has no entries stores zeros to the tile's rows.
#include <algorithm>

#include "apply.hpp"
#include "layout_probe.hpp"  // note_device_launch
#include "mixed_launch.hpp"
#include "pattern_set.hpp"

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
    if (tile[2] == 0) return;
    if (a.accumulate && tile[1] == 0) return;  // a node the list does not read adds nothing
    const int64_t cbase = c * kChunkBytes;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)threadIdx.x * 16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    apply_tile<SAFE, true, SAFE ? 0 : 1, DEPTH, false, kBlockThreads, ROWS>(
        a, tile, uniform64((uint64_t)(a.in + s * a.in_stripe_stride + (int64_t)node * q.in_node_stride + cbase)),
        uniform64((uint64_t)(a.out + s * a.out_stripe_stride + cbase)), threadIdx.x * 16, valid, nullptr);
}

namespace {
template <bool SAFE, int D, int R>
void launch_clay_partial_k(dim3 grid, hipStream_t stream, const ApplyArgs &a, const ClayPartialSel &q) {
    if (!SAFE) note_kernel("k_gf_map_partial_mixed", SAFE, D, R);
    hipLaunchKernelGGL((k_gf_map_partial_mixed<SAFE, D, R>), grid, dim3(kBlockThreads), 0, stream, a, q);
}
}  // namespace

// Instances, as launch_map_mixed's: 4 or 8 accumulator rows (the set's largest tile decides) at
// ring depth 4 or 8 for the full chunks of 16-B aligned layouts; one byte-safe instance (depth 4,
// 8 rows) for the partial last chunk and every other layout, over the depth-4 plan.
void launch_clay_partial_mixed(PatternSet &set, int n, const uint8_t *ids, const uint8_t *nodes, const uint8_t *in,
                               int64_t in_stripe_stride, int64_t in_node_stride, int64_t in_sub_stride, uint8_t *acc,
                               int64_t acc_stripe_stride, int64_t acc_sub_stride, int64_t nstripes, int64_t nbytes,
                               bool is_first, hipStream_t stream) {
    if (nstripes <= 0 || nbytes <= 0 || set.tiled_max_rows() == 0) return;
    const ClayPartialPlan &hp = set.clay_partial_plan(n, 4);
    // the plan's own ring depth, or the one ecx_tune "depth" forces (4 / 8; others have no instance)
    const Tuning tu = tuning();
    const int depth = tu.depth == 4 || tu.depth == 8 ? tu.depth : clay_partial_depth(hp);
    const int T = hp.tiles_per_pattern;
    const int rows = hp.max_rows <= 4 ? 4 : kTileRows;
    // (the node stride moves the base only: a multiple of 16 keeps every lane's loads aligned)
    const BatchLayout b{(uintptr_t)in,  (uintptr_t)acc, in_stripe_stride, in_sub_stride, acc_stripe_stride,
                        acc_sub_stride, nstripes,       nbytes,           !is_first};
    const int64_t full = b.aligned16() && in_node_stride % 16 == 0 ? nbytes / kChunkBytes : 0;
    const int64_t rest = (nbytes - full * kChunkBytes + kChunkBytes - 1) / kChunkBytes;
    if ((full + rest) * T > kMixedMaxBlocks) throw Error(ECX_E_ILLEGAL_ARGUMENT, "buf_size is too large for one launch");

    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    // resident before anything is enqueued: a first use refused on a capturing stream leaves no node behind
    const MixedDevicePlan *plan = full > 0 ? &set.clay_partial_plan_for_current_device(n, depth) : nullptr;
    const MixedDevicePlan *plan_safe = rest > 0 ? &set.clay_partial_plan_for_current_device(n, 4) : nullptr;
    const uint8_t *zero_page = zero_page_for_current_device();

    ApplyArgs a{};
    a.in = in;
    a.out = acc;
    a.zero_page = zero_page;
    a.in_stripe_stride = in_stripe_stride;
    a.in_slot_stride = in_sub_stride;
    a.out_stripe_stride = acc_stripe_stride;
    a.out_slot_stride = acc_sub_stride;
    a.nbytes = nbytes;
    a.n_tiles = T;
    a.accumulate = is_first ? 0 : 1;
    a.tail_chunk = -1;
    const ClayPartialSel q{ids, nodes, in_node_stride, (uint32_t)n};
    auto run = [&](bool safe, const MixedDevicePlan *p, int64_t chunk_begin, int64_t n_chunks) {
        if (n_chunks <= 0) return;
        a.entries = p->entries;
        a.tiles = p->tiles;
        a.chunk_begin = chunk_begin;
        a.n_chunks = n_chunks;
        for_mixed_launches(nstripes, n_chunks * T, 1, 0, kMixedMaxBlocks, [&](const MixedLaunch &l) {
            a.stripe_begin = l.unit_begin;
            const dim3 grid((unsigned)(l.unit_count * n_chunks * T));
            if (safe) launch_clay_partial_k<true, 4, kTileRows>(grid, stream, a, q);
            else if (rows == 4 && depth == 8) launch_clay_partial_k<false, 8, 4>(grid, stream, a, q);
            else if (rows == 4) launch_clay_partial_k<false, 4, 4>(grid, stream, a, q);
            else if (depth == 8) launch_clay_partial_k<false, 8, kTileRows>(grid, stream, a, q);
            else launch_clay_partial_k<false, 4, kTileRows>(grid, stream, a, q);
        });
    };
    run(false, plan, 0, full);
    run(true, plan_safe, full, rest);
    check_hip(hipGetLastError(), "k_gf_map_partial_mixed launch");
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    // (input bytes, for the launch registry: as if every stripe read its node's longest record)
    note_device_launch(dev, stream, nstripes * nbytes * (int64_t)hp.max_entries);
}

}  // namespace ecx
