// apply_map_mixed.hip -- k_gf_map_mixed: ClayCodeErasureDecodingStep.performCoding
// (ClayCodeErasureDecodingStep.java:53-107) over device-resident stripes that lost different
// nodes, out of place and in one launch.
//
// The tiled plan of a pattern set (mixed_plan.hpp TiledPlan) holds the repair maps of up to 256
// erased-node lists as [256][T] tile records over one entry array.  One workgroup covers one
// (stripe, 4 KiB chunk, tile), the tile index fastest: the T workgroups of a (stripe, chunk) are
// neighbours in the grid and run at about the same time.  Under MI355X's round-robin dispatch
// neighbouring workgroups sit on different XCDs (apply.hpp logical_block), so the inputs that
// several tiles read meet in the memory-side cache, not in one XCD's L2; keeping a unit's tiles on
// one XCD, as k_gf_apply's xcd_group 2 does, is not done here.  A
// workgroup reads its stripe's pattern id -- one byte of a device array the caller wrote, an
// ordinary global load as in apply_mixed.hip -- makes it wave-uniform and runs apply_tile
// (apply.hpp) on record id * T + tile with separate input and output bases, strides and slot
// strides.  Every (id byte, tile < T) pair names a record inside the plan and the ones without a
// tile have no rows, so there is no bounds branch: such a workgroup leaves before it touches any
// data.
#include <algorithm>

#include "apply.hpp"
#include "layout_probe.hpp"  // note_device_launch
#include "mixed_launch.hpp"
#include "pattern_set.hpp"

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
    cu32 *tile = plan_ptr(a.tiles) + (id * T + t) * kTileDwords;
    if (tile[2] == 0) return;  // wave-uniform: the whole workgroup leaves
    const int64_t cbase = c * kChunkBytes;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)threadIdx.x * 16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    apply_tile<SAFE, true, SAFE ? 0 : 1, DEPTH, false, kBlockThreads, ROWS>(
        a, tile, uniform64((uint64_t)(a.in + s * a.in_stripe_stride + cbase)),
        uniform64((uint64_t)(a.out + s * a.out_stripe_stride + cbase)), threadIdx.x * 16, valid, nullptr);
}

namespace {
template <bool SAFE, int D, int R>
void launch_map_mixed_k(dim3 grid, hipStream_t stream, const ApplyArgs &a, const uint8_t *ids) {
    if (!SAFE) note_kernel("k_gf_map_mixed", SAFE, D, R);
    hipLaunchKernelGGL((k_gf_map_mixed<SAFE, D, R>), grid, dim3(kBlockThreads), 0, stream, a, ids);
}
}  // namespace

// Instances: 4 or 8 accumulator rows (the set's largest tile decides) at ring depth 4 or 8 for the
// full chunks of 16-B aligned layouts; one byte-safe instance (depth 4 -- every record of the
// depth-4 plan is a multiple of it -- and 8 rows) for the partial last chunk and every other
// layout.  The byte-safe launch reads the depth-4 plan whatever the full chunks run with.
// (A depth-20 instance for sets whose records all have exactly 20 entries -- Clay(4,2), where the
// uniform kernel runs at depth 20 -- was measured and did not beat depth 4 or 8: DESIGN.md 4.7.3.)
void launch_map_mixed(PatternSet &set, const uint8_t *ids, const uint8_t *in, int64_t in_stripe_stride,
                      int64_t in_slot_stride, uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride,
                      int64_t units, int64_t nbytes, int64_t first_unit, hipStream_t stream) {
    if (units <= 0 || nbytes <= 0 || set.tiled_max_rows() == 0) return;
    if (first_unit < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "bad first unit");
    // the set's own ring depth, or the one ecx_tune "depth" forces (4 / 8; others have no instance)
    const Tuning tu = tuning();
    const int depth = tu.depth == 4 || tu.depth == 8 ? tu.depth : set.tiled_preferred_depth();
    const int T = set.tiles_per_pattern();
    const int rows = set.tiled_max_rows() <= 4 ? 4 : kTileRows;
    const BatchLayout b{(uintptr_t)in, (uintptr_t)out, in_stripe_stride, in_slot_stride, out_stripe_stride,
                        out_slot_stride, units,         nbytes,           false};
    const int64_t full = b.aligned16() ? nbytes / kChunkBytes : 0;
    const int64_t rest = (nbytes - full * kChunkBytes + kChunkBytes - 1) / kChunkBytes;
    if ((full + rest) * T > kMixedMaxBlocks) throw Error(ECX_E_ILLEGAL_ARGUMENT, "buf_size is too large for one launch");

    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    // resident before anything is enqueued: a first use refused on a capturing stream leaves no node behind
    const MixedDevicePlan *plan = full > 0 ? &set.tiled_plan_for_current_device(depth) : nullptr;
    const MixedDevicePlan *plan_safe = rest > 0 ? &set.tiled_plan_for_current_device(4) : nullptr;
    const uint8_t *zero_page = zero_page_for_current_device();

    ApplyArgs a{};
    a.in = in;
    a.out = out;
    a.zero_page = zero_page;
    a.in_stripe_stride = in_stripe_stride;
    a.in_slot_stride = in_slot_stride;
    a.out_stripe_stride = out_stripe_stride;
    a.out_slot_stride = out_slot_stride;
    a.nbytes = nbytes;
    a.n_tiles = T;
    a.tail_chunk = -1;
    auto run = [&](bool safe, const MixedDevicePlan *p, int64_t chunk_begin, int64_t n_chunks) {
        if (n_chunks <= 0) return;
        a.entries = p->entries;
        a.tiles = p->tiles;
        a.chunk_begin = chunk_begin;
        a.n_chunks = n_chunks;
        for_mixed_launches(units, n_chunks * T, 1, first_unit, kMixedMaxBlocks, [&](const MixedLaunch &l) {
            a.stripe_begin = l.unit_begin;
            const dim3 grid((unsigned)(l.unit_count * n_chunks * T));
            const uint8_t *lids = ids + first_unit;  // the kernel indexes by unit_begin + the local unit
            if (safe) launch_map_mixed_k<true, 4, kTileRows>(grid, stream, a, lids);
            else if (rows == 4 && depth == 8) launch_map_mixed_k<false, 8, 4>(grid, stream, a, lids);
            else if (rows == 4) launch_map_mixed_k<false, 4, 4>(grid, stream, a, lids);
            else if (depth == 8) launch_map_mixed_k<false, 8, kTileRows>(grid, stream, a, lids);
            else launch_map_mixed_k<false, 4, kTileRows>(grid, stream, a, lids);
        });
    };
    run(false, plan, 0, full);
    run(true, plan_safe, full, rest);
    check_hip(hipGetLastError(), "k_gf_map_mixed launch");
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    // (input bytes, for the launch registry: as if every stripe read its longest pattern)
    const TiledPlan &hp = set.tiled_plan(4);
    uint32_t inputs = 0;
    for (int p = 0; p < hp.npatterns; ++p) {
        uint32_t sum = 0;
        for (int t = 0; t < T; ++t) sum += hp.tiles[((size_t)p * T + t) * kTileDwords + 3];
        inputs = std::max(inputs, sum);
    }
    note_device_launch(dev, stream, units * nbytes * (int64_t)inputs);
}

}  // namespace ecx
