// mixed_pass.hpp -- what the pattern-set kernels share: the device body
// of the four load-ring kernels (k_gf_apply_mixed, k_gf_apply_mixed_blocked, k_gf_map_mixed,
// k_gf_map_partial_mixed) and the launch skeleton of all five (k_gf_partial_mixed too).  A kernel
// keeps what is its own -- how it finds its stripe, chunk and record -- and a launcher its plans,
// its arguments and its template's name; the rules of a pass are written here, once.
#pragma once

#include <type_traits>

#include "apply.hpp"
#include "layout_probe.hpp"  // note_device_launch
#include "mixed_launch.hpp"
#include "pattern_set.hpp"

namespace ecx {

// Tile record `tile` over chunk c of stripe s, as k_gf_apply runs a single-tile map: the inner
// loop, the load ring and the split-table arithmetic are apply_tile's (apply.hpp).  A record with
// no rows returns before it touches any data (wave-uniform: the whole workgroup leaves).
// `in_offset` moves the input base only (a helper's node; 0 elsewhere).
template <bool SAFE, int DEPTH, int ROWS>
__device__ __forceinline__ void mixed_tile(const ApplyArgs &a, cu32 *tile, int64_t s, int64_t c, int64_t in_offset) {
    if (tile[2] == 0) return;
    const int64_t cbase = c * kChunkBytes;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)threadIdx.x * 16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    apply_tile<SAFE, true, SAFE ? 0 : 1, DEPTH, false, kBlockThreads, ROWS>(
        a, tile, uniform64((uint64_t)(a.in + s * a.in_stripe_stride + in_offset + cbase)),
        uniform64((uint64_t)(a.out + s * a.out_stripe_stride + cbase)), threadIdx.x * 16, valid, nullptr);
}

// The arguments every launch of a load-ring pass shares; run_mixed_pass's callback aims them at a
// launch (MixedStep::aim).
inline ApplyArgs mixed_apply_args(const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride, uint8_t *out,
                                  int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nbytes, int n_tiles,
                                  bool accumulate) {
    ApplyArgs a{};
    a.in = in;
    a.out = out;
    a.in_stripe_stride = in_stripe_stride;
    a.in_slot_stride = in_slot_stride;
    a.out_stripe_stride = out_stripe_stride;
    a.out_slot_stride = out_slot_stride;
    a.nbytes = nbytes;
    a.n_tiles = n_tiles;
    a.accumulate = accumulate ? 1 : 0;
    a.tail_chunk = -1;
    return a;
}

// One pass of units (mixed_launch.hpp) through a pattern-set kernel.
struct MixedPass {
    int64_t units = 0, nbytes = 0;
    int64_t divisor = 1, first_unit = 0;
    int tiles = 1;             // workgroups per (unit, chunk): 1, or the plan's T
    bool aligned = false;      // every lane's 16-B accesses are aligned: BatchLayout::aligned16() and the launcher's own
    int max_rows = 0;          // the plan's largest row count
    int preferred_depth = 4;   // the plan's own ring depth
    const char *too_large = "";  // the refusal of a pass whose chunks alone exceed one grid
    const char *what = "";       // names the launch in a HIP error
    int64_t inputs = 1;        // input bytes read per byte of a unit, for the launch registry
};

// One launch of the pass: its grid and where it begins.
struct MixedStep {
    dim3 grid;
    bool safe = false;
    int64_t chunk_begin = 0, n_chunks = 0;
    MixedLaunch l;
    template <class Args>
    void aim(Args &a, const PatternDevicePlan &plan) const {
        a.entries = plan.entries;
        a.chunk_begin = chunk_begin;
        a.n_chunks = n_chunks;
        a.stripe_begin = l.unit_begin;
    }
};

// The instances of a pattern-set kernel: 4 or 8 accumulator rows (the plan's largest record
// decides) at ring depth 4 or 8 for the full chunks of 16-B aligned layouts; one byte-safe
// instance (depth 4 -- every record of either depth's plan is padded to a multiple of 4 -- and 8
// rows) for the partial last chunk and every other layout.  f(SAFE, DEPTH, ROWS) gets them as
// integral constants; a kernel without a ring ignores DEPTH.
// There is no per-layout shape selection here: the work differs from stripe to stripe.
template <class F>
void with_mixed_instance(bool safe, int rows, int depth, F &&f) {
    using std::integral_constant;
    using T = std::true_type;
    using N = std::false_type;
    if (safe) f(T{}, integral_constant<int, 4>{}, integral_constant<int, kTileRows>{});
    else if (rows == 4 && depth == 8) f(N{}, integral_constant<int, 8>{}, integral_constant<int, 4>{});
    else if (rows == 4) f(N{}, integral_constant<int, 4>{}, integral_constant<int, 4>{});
    else if (depth == 8) f(N{}, integral_constant<int, 8>{}, integral_constant<int, kTileRows>{});
    else f(N{}, integral_constant<int, 4>{}, integral_constant<int, kTileRows>{});
}

// The skeleton of a pass.  `prepare(depth, full, rest)` runs once, inside the launch's stream
// scope and before anything is enqueued: the launcher makes resident there whatever its `full`
// full chunks (at ring depth `depth`) and `rest` byte-safe chunks will read, so that a first use
// refused on a capturing stream leaves no node behind.  `launch(SAFE, DEPTH, ROWS, step)` then
// enqueues one instance over one step; mixed_launch.hpp cuts the pass into steps.
template <class Prepare, class Launch>
void run_mixed_pass(const MixedPass &p, hipStream_t stream, Prepare &&prepare, Launch &&launch) {
    // the plan's own ring depth, or the one ecx_tune "depth" forces (4 / 8; others have no instance)
    const Tuning tu = tuning();
    const int depth = tu.depth == 4 || tu.depth == 8 ? tu.depth : p.preferred_depth;
    const int rows = p.max_rows <= 4 ? 4 : kTileRows;
    const int64_t full = p.aligned ? p.nbytes / kChunkBytes : 0;
    const int64_t rest = (p.nbytes - full * kChunkBytes + kChunkBytes - 1) / kChunkBytes;
    if ((full + rest) * p.tiles > kMixedMaxBlocks) throw Error(ECX_E_ILLEGAL_ARGUMENT, p.too_large);

    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    prepare(depth, full, rest);
    auto run = [&](bool safe, int64_t chunk_begin, int64_t n_chunks) {
        if (n_chunks <= 0) return;
        for_mixed_launches(p.units, n_chunks * p.tiles, p.divisor, p.first_unit, kMixedMaxBlocks, [&](const MixedLaunch &l) {
            const MixedStep st{dim3((unsigned)(l.unit_count * n_chunks * p.tiles)), safe, chunk_begin, n_chunks, l};
            with_mixed_instance(safe, rows, depth, [&](auto s, auto d, auto r) { launch(s, d, r, st); });
        });
    };
    run(false, 0, full);
    run(true, full, rest);
    check_hip(hipGetLastError(), p.what);
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, p.units * p.nbytes * p.inputs);
}

}  // namespace ecx
