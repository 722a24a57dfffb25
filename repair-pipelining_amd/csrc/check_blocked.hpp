// check_blocked.hpp -- the parity check over a blocked RS batch (apply_check.hip).
#pragma once

#include "engine.hpp"

namespace ecx {

// launch_check (engine.hpp) over a blocked batch of n-shard stripes (blocked_layout.hpp:
// [S][full][n][block], then the tails [S][n][tail]): verdict[s] for each of the nstripes caller
// stripes, from the layout's body and tail passes.  Read-only on the batch.
void launch_check_blocked(CompiledMap &cm, const uint8_t *base, int n, int64_t nstripes, int64_t byte_count,
                          int64_t block, uint8_t *verdict, hipStream_t stream);

}  // namespace ecx
