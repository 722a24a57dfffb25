// apply_partial_mixed.hip -- k_gf_partial_mixed: one hop of the pipelined partial-sum chain,
// ReedSolomon.decodeMissingSingle for every missing shard (ReedSolomon.java:288-333), over
// device-resident stripes that each name their erasure pattern and the shard this helper holds
// for them.
//
// A pattern set's partial plan (partial_plan.hpp) holds one entry per (pattern, shard) and 256 row
// counts.  One workgroup covers one (stripe, 4 KiB chunk), stripe-major.  It reads its stripe's
// pattern id and shard byte -- two independent bytes of device arrays the caller wrote, ordinary
// global loads, not the constant path the plan goes through: the caller may rewrite them between
// two replays of a graph -- makes both wave-uniform and leaves when the row count is zero or the
// shard byte is no shard.  Otherwise entry id * n + shard lies inside the plan whatever the two
// arrays hold.  The kernel has ONE input stream, so there is no load ring and no zero-page padding:
// one 16-B load per lane, apply_entry (apply.hpp, the arithmetic of every other kernel), and per
// accumulator row a store, XORed with the old row when the hop accumulates.  The old rows are
// loaded right behind the input, ahead of the multiply, so all of a lane's loads are in flight
// together; the stripe's row count and the hop's mode select a straight-line body for that.
#include "mixed_pass.hpp"

namespace ecx {

struct PartialArgs {
    const uint8_t *in;
    uint8_t *acc;
    const uint32_t *entries;  // the plan: npatterns * n entries
    const uint32_t *rows;     // the plan: kPartialRecords row counts
    const uint8_t *ids;       // per stripe: the pattern
    const uint8_t *shards;    // per stripe: the shard this helper holds
    int64_t in_stripe_stride, in_shard_stride, acc_stripe_stride, acc_row_stride;
    int64_t nbytes, chunk_begin, n_chunks, stripe_begin;
    uint32_t n;      // shards per stripe
    int accumulate;  // 1: acc ^= D * in, 0: acc = D * in
};

// The rows of one lane of a pattern with NR missing shards, straight-line: the input load, the NR
// old rows of an accumulating hop right behind it, the multiply, the stores.  NR and the hop's mode
// are compile-time so that no load sits behind a branch: every load of the lane is in flight
// before the first wait, and the waits count exactly.
template <bool SAFE, int NR, bool ACC>
__device__ __forceinline__ void partial_rows(cu32 *ent, const uint8_t *ip, uint8_t *ap, int64_t row_stride, int valid) {
    const u32x4 x = SAFE ? load_partial(ip, valid) : ld16<true>(ip);
    u32x4 old[NR];
    if (ACC) {
#pragma unroll
        for (int o = 0; o < NR; ++o) old[o] = SAFE ? load_partial(ap + o * row_stride, valid) : load16(ap + o * row_stride);
    }
    u32x4 acc[NR];
#pragma unroll
    for (int o = 0; o < NR; ++o) acc[o] = (u32x4){0u, 0u, 0u, 0u};
    apply_entry<false, NR>(ent, x, acc, nullptr);
#pragma unroll
    for (int o = 0; o < NR; ++o) {
        u32x4 v = acc[o];
        if (ACC) v ^= old[o];
        if (SAFE) store_partial(ap + o * row_stride, v, valid);
        else st16<1>(ap + o * row_stride, v);
    }
}

// The body of the stripe's row count (wave-uniform, 1..ROWS), by scalar branches.  A count above
// ROWS has no body and writes nothing; the launcher picks ROWS from the plan's largest count.
template <bool SAFE, int ROWS, bool ACC, int NR = ROWS>
__device__ __forceinline__ void partial_rows_of(uint32_t nrows, cu32 *ent, const uint8_t *ip, uint8_t *ap,
                                                int64_t row_stride, int valid) {
    if (nrows == (uint32_t)NR) partial_rows<SAFE, NR, ACC>(ent, ip, ap, row_stride, valid);
    else if constexpr (NR > 1) partial_rows_of<SAFE, ROWS, ACC, NR - 1>(nrows, ent, ip, ap, row_stride, valid);
}

template <bool SAFE, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ROWS <= 4 ? 8 : 4) k_gf_partial_mixed(PartialArgs a) {
    // (a launch covers whole stripes: gridDim.x = stripes x n_chunks)
    const uint32_t nc = (uint32_t)a.n_chunks;
    const int64_t s = (int64_t)(blockIdx.x / nc) + a.stripe_begin;
    const int64_t c = (int64_t)(blockIdx.x % nc) + a.chunk_begin;
    const uint32_t idb = ((const gu8 *)a.ids)[s], shb = ((const gu8 *)a.shards)[s];  // both in flight
    const uint32_t id = __builtin_amdgcn_readfirstlane(idb);
    const uint32_t sh = __builtin_amdgcn_readfirstlane(shb);
    const uint32_t nrows = plan_ptr(a.rows)[id];  // id < kPartialRecords: inside the table
    if (nrows == 0 || sh >= a.n) return;          // wave-uniform: the whole workgroup leaves
    // nrows != 0 means id < npatterns, and sh < n: the entry is inside the plan
    cu32 *ent = plan_ptr(a.entries) + (int64_t)(id * a.n + sh) * kEntryDwords;
    // a shard the pattern does not read adds nothing to a running sum
    if (a.accumulate && (ent[1] | ent[2]) == 0) return;
    const int64_t cbase = c * kChunkBytes;
    const uint32_t lane16 = threadIdx.x * 16;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)lane16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    const uint8_t *ip = reinterpret_cast<const uint8_t *>(
                            uniform64((uint64_t)(a.in + s * a.in_stripe_stride + (int64_t)sh * a.in_shard_stride + cbase))) +
                        lane16;
    uint8_t *ap = reinterpret_cast<uint8_t *>(uniform64((uint64_t)(a.acc + s * a.acc_stripe_stride + cbase))) + lane16;
    if (a.accumulate) partial_rows_of<SAFE, ROWS, true>(nrows, ent, ip, ap, a.acc_row_stride, valid);
    else partial_rows_of<SAFE, ROWS, false>(nrows, ent, ip, ap, a.acc_row_stride, valid);
}

// Instances: with_mixed_instance's rows (mixed_pass.hpp) -- 4 or 8 for the full chunks of 16-B
// aligned layouts, one byte-safe instance of 8 -- and no ring depth.  mixed_launch.hpp cuts the
// batch into launches (divisor 1: the units are the stripes).
void launch_partial_mixed(PatternSet &set, int n, const uint8_t *ids, const uint8_t *shards, const uint8_t *in,
                          int64_t in_stripe_stride, int64_t in_shard_stride, uint8_t *acc, int64_t acc_stripe_stride,
                          int64_t acc_row_stride, int64_t nstripes, int64_t nbytes, bool is_first, hipStream_t stream) {
    if (nstripes <= 0 || nbytes <= 0 || set.max_rows() == 0) return;
    const PartialPlan &hp = set.partial_plan(n);
    const BatchLayout b{(uintptr_t)in,     (uintptr_t)acc, in_stripe_stride, in_shard_stride, acc_stripe_stride,
                        acc_row_stride,    nstripes,       nbytes,           !is_first};
    MixedPass pass{nstripes, nbytes, 1, 0, 1, b.aligned16(), hp.max_rows};
    pass.too_large = "byte_count is too large for one launch";
    pass.what = "k_gf_partial_mixed launch";

    PartialArgs a{};
    a.in = in;
    a.acc = acc;
    a.ids = ids;
    a.shards = shards;
    a.in_stripe_stride = in_stripe_stride;
    a.in_shard_stride = in_shard_stride;
    a.acc_stripe_stride = acc_stripe_stride;
    a.acc_row_stride = acc_row_stride;
    a.nbytes = nbytes;
    a.n = (uint32_t)n;
    a.accumulate = is_first ? 0 : 1;
    const PatternDevicePlan *plan = nullptr;
    run_mixed_pass(
        pass, stream,
        [&](int, int64_t, int64_t) {
            plan = &set.partial_plan_for_current_device(n);
            a.rows = plan->records;
        },
        [&](auto safe, auto, auto rows, const MixedStep &st) {
            constexpr bool SAFE = decltype(safe)::value;
            constexpr int R = decltype(rows)::value;
            st.aim(a, *plan);
            if (!SAFE) note_kernel("k_gf_partial_mixed", SAFE, R);
            hipLaunchKernelGGL((k_gf_partial_mixed<SAFE, R>), st.grid, dim3(kBlockThreads), 0, stream, a);
        });
}

}  // namespace ecx
