// blocked_layout.hpp -- the pass plan of a blocked RS batch (include/ecx.h).
//
// A blocked batch stores stripe s, shard i as full = byte_count / block blocks,
// [S][full][n][block] from offset 0, then the tails (byte_count % block bytes) apart as
// [S][n][tail].  Every operation over it runs as at most two passes, each an ordinary batch of
// "units" of n equal slots: the body pass over nstripes * full units of n block-sized slots, then
// the tail pass over nstripes units of n tail-sized slots.  A pass also says how many consecutive
// units of it belong to one caller stripe (its verdict divisor): unit u of a pass belongs to
// caller stripe u / divisor, which is what the blocked check (apply_check.hip
// launch_check_blocked) reports a verdict for.
//
// No HIP header and no other unit of the engine: the plan runs -- and is tested -- on the CPU
// (tests/native/blocked_layout_check.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ECX_BL_HD __host__ __device__ inline
#else
#define ECX_BL_HD inline
#endif

namespace ecx {

// The recommended block: the largest power of two with n blocks (one per shard of a stripe)
// within 1 MiB, 4 KiB..1 MiB -- 32 KiB for RS(17,3) (0.76 of HBM), 64 KiB for RS(12,4) (0.816);
// one block of byte_count bytes for smaller shards.
int64_t recommended_block(int n, int64_t byte_count);
// The block a caller's block_bytes stands for: 0 = the recommended one.  False when negative.
bool resolve_block(int n, int64_t byte_count, int64_t block_bytes, int64_t *block);

struct BlockedPass {
    int64_t offset;         // of the pass's first unit from the batch's base, bytes
    int64_t stripe_stride;  // from one unit to the next: n * slot_bytes
    int64_t slot_bytes;     // bytes of each of a unit's n slots, and their pitch
    int64_t units;
    int64_t divisor;        // consecutive units per caller stripe: full (body), 1 (tail)
};

struct BlockedPlan {
    int count = 0;  // 0 (nothing to do), 1 or 2: the body pass first where there are both
    BlockedPass pass[2];
};

// The passes of nstripes stripes of n shards of byte_count bytes in blocks of `block` bytes.
// False -- and *plan untouched -- when block <= 0 with bytes to cover, or when a stride, a unit
// count or the batch's extent does not fit int64_t.
bool blocked_plan(int n, int64_t nstripes, int64_t byte_count, int64_t block, BlockedPlan *plan);

// unit / divisor without a division on the device.  k_gf_check_blocked computes it once per
// workgroup from wave-uniform values, and gfx950 has no scalar divide: a 32-bit one is expanded
// into a float reciprocal on the vector pipe.  So the host prepares the divisor as a 64-bit
// reciprocal, magic = floor(2^64 / divisor) + 1, and the quotient is the high half of
// t * magic -- two scalar multiplies.  With e = magic * divisor - 2^64 in (0, divisor] the
// result is exact while t * e < 2^64, which t < 2^32 and divisor < 2^31 guarantee.  A launch
// covers fewer than 2^31 units (a grid is at most 2^30 workgroups), so for a divisor of 2^31 or
// more (magic == 0) the quotient of rem + u, rem < divisor, is 0 or 1: one comparison.
struct VerdictDiv {
    uint64_t divisor = 1;
    uint64_t magic = 0;
    uint64_t rem = 0;  // (first unit of the launch) % divisor: the kernel divides rem + local unit
};

// divisor >= 2 (a divisor of 1 is the identity: the caller launches the ordinary check).
// (2^64 - 1) / d is floor(2^64 / d) unless d is a power of two, where it is 2^64 / d - 1: magic
// is then exactly 2^64 / d, e = 0, and the product's high half is t / d with no error term.
inline VerdictDiv verdict_div(int64_t divisor, int64_t first_unit) {
    VerdictDiv d;
    d.divisor = (uint64_t)divisor;
    d.magic = d.divisor < ((uint64_t)1 << 31) ? ~(uint64_t)0 / d.divisor + 1 : 0;
    d.rem = (uint64_t)first_unit % d.divisor;
    return d;
}

// (rem + local) / divisor for local < 2^31
ECX_BL_HD uint64_t verdict_quot(const VerdictDiv &d, uint32_t local) {
    const uint64_t t = d.rem + local;
    if (d.magic == 0) return t >= d.divisor ? 1 : 0;
    const uint32_t t32 = (uint32_t)t;  // < 2^31 + 2^31
    const uint64_t lo = (uint64_t)t32 * (uint32_t)d.magic;
    const uint64_t hi = (uint64_t)t32 * (uint32_t)(d.magic >> 32);
    return (hi + (lo >> 32)) >> 32;
}

}  // namespace ecx
