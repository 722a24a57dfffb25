// blocked_layout.cpp -- the pass plan of a blocked RS batch (blocked_layout.hpp).
#include "blocked_layout.hpp"

namespace ecx {

int64_t recommended_block(int n, int64_t byte_count) {
    int64_t b = 1 << 20;
    while (b > (4 << 10) && b * n > (1 << 20)) b >>= 1;
    return byte_count >= b ? b : byte_count;
}

bool resolve_block(int n, int64_t byte_count, int64_t block_bytes, int64_t *block) {
    if (block_bytes < 0) return false;
    *block = block_bytes == 0 ? recommended_block(n, byte_count) : block_bytes;
    return true;
}

bool blocked_plan(int n, int64_t nstripes, int64_t byte_count, int64_t block, BlockedPlan *plan) {
    BlockedPlan p;
    if (nstripes == 0 || byte_count == 0) {
        *plan = p;
        return true;
    }
    if (n <= 0 || nstripes < 0 || byte_count < 0 || block <= 0) return false;
    const int64_t full = byte_count / block, tail = byte_count % block;
    int64_t stride = 0, units = 0, body = 0, tail_stride = 0, tails = 0, extent = 0;
    if (__builtin_mul_overflow((int64_t)n, block, &stride) || __builtin_mul_overflow(nstripes, full, &units) ||
        __builtin_mul_overflow(units, stride, &body))
        return false;
    // (n * tail < n * block: no overflow)
    tail_stride = (int64_t)n * tail;
    if (__builtin_mul_overflow(nstripes, tail_stride, &tails) || __builtin_add_overflow(body, tails, &extent))
        return false;
    if (full > 0) p.pass[p.count++] = BlockedPass{0, stride, block, units, full};
    if (tail > 0) p.pass[p.count++] = BlockedPass{body, tail_stride, tail, nstripes, 1};
    *plan = p;
    return true;
}

}  // namespace ecx
