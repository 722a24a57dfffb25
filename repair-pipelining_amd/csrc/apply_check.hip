// apply_check.hip -- k_gf_check: ReedSolomon.isParityCorrect (ReedSolomon.java:129-178) over
// device-resident stripes, the "Check" half of ReedSolomonBenchmark (:73-87, :126-149).
//
// The check map of a code (ecx_api.cpp rs_check_map) has one row per parity shard p:
// syndrome_p = sum_i parityRows[p][i] * D_i  ^  P_p, which is all zero exactly when P_p is the
// parity of the data.  The kernel runs that map with k_gf_apply's plan, load ring and split-table
// arithmetic (apply.hpp) but never stores a syndrome: each lane OR-folds its rows in registers,
// each wave ballots the result, and a wave that saw a non-zero byte clears its stripe's verdict
// byte (launch_check sets every verdict to 1 first).  Nothing is written to the shards, so the
// read stream is the kernel's whole traffic: (k + m) * byte_count per stripe.
//
// A shard's partial last chunk (200,000-B shards: 48 full 4 KiB chunks and 3,392 B) runs in
// the same launch: its workgroup reads the shard's last 4 KiB window instead, so the bytes
// it shares with the previous chunk are checked twice -- harmless for a read-only check, and
// it keeps every load a full 16-B access (byte counts that are multiples of 16 on aligned
// layouts; otherwise a byte-safe launch covers the remainder).
//
// Over the blocked RS layout (blocked_layout.hpp) the same body runs as
// k_gf_check_blocked: a launch's units are then the block rows of the layout's body pass, `full`
// consecutive ones per caller stripe, and a mismatch clears the verdict of unit / full
// (launch_check_blocked: the verdicts set once, then the body pass and the tail pass).
#include "apply.hpp"
#include "blocked_layout.hpp"
#include "check_blocked.hpp"
#include "layout_probe.hpp"  // note_device_launch

namespace ecx {

#define ECX_CHECK_BOUNDS(ROWS, DEPTH) (ROWS < kTileRows ? (DEPTH >= 16 ? 4 : 5) : (DEPTH >= 16 ? 3 : 5))

template <bool SAFE, int DEPTH, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_CHECK_BOUNDS(ROWS, DEPTH)) k_gf_check(ApplyArgs a) {
#define ECX_CHECK_VERDICT(s) (s)
#include "apply_check_body.inc"
#undef ECX_CHECK_VERDICT
}

// The check over one pass of a blocked batch (blocked_layout.hpp): the launch's units are block
// rows, vd.divisor consecutive ones per caller stripe, and a mismatch clears the verdict of
// unit / divisor instead of the unit's own.  a.out is the verdict of the launch's first unit's
// stripe and vd.rem that unit's place in it.  The unit comes from the block index, so the quotient
// is wave-uniform: two scalar multiplies (verdict_quot), and only in a workgroup that found a
// mismatch.  A kernel of its own, not a field read by k_gf_check: the natural layout's
// instantiations stay what they were.
template <bool SAFE, int DEPTH, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_CHECK_BOUNDS(ROWS, DEPTH)) k_gf_check_blocked(ApplyArgs a, VerdictDiv vd) {
#define ECX_CHECK_VERDICT(s) \
    ((int64_t)verdict_quot(vd, __builtin_amdgcn_readfirstlane((uint32_t)((s) - a.stripe_begin))))
#include "apply_check_body.inc"
#undef ECX_CHECK_VERDICT
}

// verdict[s] = 1 for every stripe, ahead of the check's launches.  A kernel, not hipMemsetAsync:
// on a capturing stream a memset becomes a memset node, and the HIP runtime (ROCm 7.0) replays a
// memset node with the value 0 from its second replay on, in every graph of a process but the
// first one instantiated -- a graph of the memset alone shows it -- so a replayed check reported
// every stripe as corrupt (tests/test_gpu_capture.py).  A kernel node keeps its arguments.
__global__ void __launch_bounds__(256) k_set_verdicts(uint8_t *verdict, int64_t nstripes) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nstripes) verdict[s] = 1;
}

namespace {
template <bool SAFE, int D, int R>
void launch_check_k(dim3 grid, hipStream_t stream, const ApplyArgs &a, const VerdictDiv *vd) {
    if (vd) {
        if (!SAFE) note_kernel("k_gf_check_blocked", SAFE, D, R);
        hipLaunchKernelGGL((k_gf_check_blocked<SAFE, D, R>), grid, dim3(kBlockThreads), 0, stream, a, *vd);
        return;
    }
    if (!SAFE) note_kernel("k_gf_check", SAFE, D, R);
    hipLaunchKernelGGL((k_gf_check<SAFE, D, R>), grid, dim3(kBlockThreads), 0, stream, a);
}
}  // namespace

namespace {
int check_depth(const Tuning &tu) { return tu.depth == 8 || tu.depth == 20 ? tu.depth : 4; }

// Clears verdict[s / divisor] when a syndrome byte of stripe s over bytes [0, nbytes) is non-zero
// (the verdicts were set to 1 by launch_check / launch_check_blocked).  divisor 1: the natural
// layout, k_gf_check; above 1 the stripes are the units of a blocked pass, k_gf_check_blocked.
void launch_check_core(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                       uint8_t *verdict, int64_t nstripes, int64_t nbytes, hipStream_t stream, int64_t divisor = 1) {
    // Ring depth 4 (forced 8 / 20 with ecx_tune "depth"): on RS(17,3) 200,000-B shards depth 4 reads
    // 0.83 of HBM, depth 8 and 20 0.80 -- the short ring leaves registers for more resident waves
    // (profiles/r05_check_sweep.jsonl).  Accumulator rows: 4 when every tile has at most 4 (RS with
    // m <= 4), else 8.
    const Tuning &tu = tuning();
    const int depth = check_depth(tu);
    const int rows = cm.max_tile_rows() <= 4 ? 4 : kTileRows;
    const bool aligned = aligned16(in) && in_stripe_stride % 16 == 0 && in_slot_stride % 16 == 0;
    const int64_t full = aligned ? nbytes / kChunkBytes : 0;
    const int64_t tail = nbytes - full * kChunkBytes;
    // the partial last chunk as a shifted full window (read-only: overlap is re-checked)
    const bool fuse_tail = aligned && full >= 1 && tail > 0 && tail % 16 == 0;
    const DevicePlan &plan = cm.plan_for_current_device(depth);
    const DevicePlan &plan4 = depth == 4 ? plan : cm.plan_for_current_device(4);

    ApplyArgs a{};
    a.in = in;
    a.out = verdict;
    a.zero_page = zero_page_for_current_device();
    a.in_stripe_stride = in_stripe_stride;
    a.in_slot_stride = in_slot_stride;
    a.out_stripe_stride = 1;
    a.out_slot_stride = 0;
    a.nbytes = nbytes;
    a.n_tiles = cm.n_tiles();
    a.stagger = tu.stagger;
    // inputs not 128-B aligned share a boundary line between neighbouring chunks: runs of
    // consecutive units per XCD keep both fetches in one L2 (as launch_rules.cpp choose_launch does)
    const bool misaligned128 = ((uintptr_t)in % 128) != 0 || in_stripe_stride % 128 != 0 || in_slot_stride % 128 != 0;
    a.xcd_group = tu.xcd_group == 3 ? 3 : (tu.xcd_misaligned && misaligned128 ? 3 : 0);
    a.xcd_run = tu.xcd_run;
    a.tail_chunk = fuse_tail ? full : -1;
    auto run = [&](bool safe, const DevicePlan &p, int64_t chunk_begin, int64_t n_chunks) {
        if (n_chunks <= 0) return;
        a.entries = p.entries;
        a.tiles = p.tiles;
        a.chunk_begin = chunk_begin;
        a.n_chunks = n_chunks;
        const int64_t per_stripe = n_chunks * a.n_tiles;
        const int64_t stripes_per_launch = std::max<int64_t>(1, ((int64_t)1 << 30) / per_stripe);
        for (int64_t s0 = 0; s0 < nstripes; s0 += stripes_per_launch) {
            a.stripe_begin = s0;
            const dim3 grid((unsigned)(std::min(stripes_per_launch, nstripes - s0) * per_stripe));
            // blocked: the launch's verdicts start at its first unit's stripe, s0 / divisor, and
            // the kernel divides (s0 % divisor + the unit's index in the launch)
            const VerdictDiv vdiv = divisor > 1 ? verdict_div(divisor, s0) : VerdictDiv{};
            const VerdictDiv *vd = divisor > 1 ? &vdiv : nullptr;
            a.out = divisor > 1 ? verdict + s0 / divisor : verdict;
            if (safe) {
                if (rows == 4) launch_check_k<true, 4, 4>(grid, stream, a, vd);
                else launch_check_k<true, 4, kTileRows>(grid, stream, a, vd);
            } else if (rows == 4) {
                if (depth == 20) launch_check_k<false, 20, 4>(grid, stream, a, vd);
                else if (depth == 8) launch_check_k<false, 8, 4>(grid, stream, a, vd);
                else launch_check_k<false, 4, 4>(grid, stream, a, vd);
            } else {
                if (depth == 20) launch_check_k<false, 20, kTileRows>(grid, stream, a, vd);
                else if (depth == 8) launch_check_k<false, 8, kTileRows>(grid, stream, a, vd);
                else launch_check_k<false, 4, kTileRows>(grid, stream, a, vd);
            }
        }
    };
    const uint64_t notes0 = kernel_notes();
    if (fuse_tail) {
        run(false, plan, 0, full + 1);
    } else {
        run(false, plan, 0, full);
        a.tail_chunk = -1;
        run(true, plan4, full, (tail + kChunkBytes - 1) / kChunkBytes);  // (not noted: byte-safe)
    }
    if (kernel_notes() != notes0)
        set_last_shape_order("stagger=" + std::to_string(a.stagger) + " xcd_group=" + std::to_string(a.xcd_group) +
                             " xcd_run=" + std::to_string(a.xcd_group == 3 ? a.xcd_run : 0));
    check_hip(hipGetLastError(), "k_gf_check launch");
}
}  // namespace

// verdict[s] = 1 when every parity shard of stripe s equals the parity of its
// data over bytes [0, nbytes) of each slot, else 0.  `cm` is a check map (rows = syndromes).
// A start that is not 16-B aligned (isParityCorrect's firstByte may be anything) on 16-B
// strides: the bytes up to the first 16-B boundary go to the byte-safe kernel, the rest to the
// vectorised one, so only the head (< 16 B per slot) pays the byte-safe rate.
void launch_check(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                  uint8_t *verdict, int64_t nstripes, int64_t nbytes, hipStream_t stream) {
    if (nstripes <= 0) return;
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    if (nbytes > 0 && cm.map().n_out != 0) {
        // the device state of the launches below, resident before anything is enqueued: a first
        // use refused on a capturing stream leaves no node behind
        (void)cm.plan_for_current_device(check_depth(tuning()));
        (void)cm.plan_for_current_device(4);
        (void)zero_page_for_current_device();
    }
    hipLaunchKernelGGL(k_set_verdicts, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), 0, stream, verdict, nstripes);
    check_hip(hipGetLastError(), "k_set_verdicts launch");
    if (nbytes <= 0 || cm.map().n_out == 0) return;
    const int64_t head = (int64_t)((16 - (uintptr_t)in % 16) % 16);
    if (head > 0 && head < nbytes && in_stripe_stride % 16 == 0 && in_slot_stride % 16 == 0) {
        launch_check_core(cm, in, in_stripe_stride, in_slot_stride, verdict, nstripes, head, stream);
        launch_check_core(cm, in + head, in_stripe_stride, in_slot_stride, verdict, nstripes, nbytes - head, stream);
    } else {
        launch_check_core(cm, in, in_stripe_stride, in_slot_stride, verdict, nstripes, nbytes, stream);
    }
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, nstripes * nbytes * cm.map().n_in);
}

// launch_check over a blocked batch (blocked_layout.hpp): verdict[s] for the nstripes caller
// stripes, from the two passes of the layout.  One k_set_verdicts, then the body pass -- whose
// units are block rows, `full` of them per stripe, so a mismatch clears verdict[unit / full] --
// and the tail pass, one unit per stripe.  Both only ever clear, so a stripe passes when it
// passes in every block and in its tail.  Each pass takes launch_check_core's alignment rules by
// itself: recommended blocks are whole 4 KiB chunks; a tail slot shorter than a chunk has no
// earlier bytes of its own shard before it (the shifted window would read the neighbouring
// slot), so it runs byte-safe, as does every pass of an odd explicit block.
void launch_check_blocked(CompiledMap &cm, const uint8_t *base, int n, int64_t nstripes, int64_t byte_count,
                          int64_t block, uint8_t *verdict, hipStream_t stream) {
    if (nstripes <= 0) return;
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    BlockedPlan plan;
    const bool work = byte_count > 0 && cm.map().n_out != 0;
    if (work) {
        if (!blocked_plan(n, nstripes, byte_count, block, &plan))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "blocked batch extent overflows");
        // resident before anything is enqueued, as in launch_check
        (void)cm.plan_for_current_device(check_depth(tuning()));
        (void)cm.plan_for_current_device(4);
        (void)zero_page_for_current_device();
    }
    hipLaunchKernelGGL(k_set_verdicts, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), 0, stream, verdict, nstripes);
    check_hip(hipGetLastError(), "k_set_verdicts launch");
    for (int i = 0; i < plan.count; ++i) {
        const BlockedPass &p = plan.pass[i];
        launch_check_core(cm, base + p.offset, p.stripe_stride, p.slot_bytes, verdict, p.units, p.slot_bytes, stream,
                          p.divisor);
    }
    if (plan.count == 0) return;
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, nstripes * byte_count * cm.map().n_in);
}

}  // namespace ecx
