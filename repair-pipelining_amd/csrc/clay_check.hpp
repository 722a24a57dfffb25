// clay_check.hpp -- the Clay codeword check on the device (apply_clay_check.hip): a proved check
// program (clay_check_plan.hpp) with its device records, and its launcher.
#pragma once

#include "clay_check_plan.hpp"
#include "engine.hpp"

namespace ecx {

// The codeword test of a Clay geometry and its device records: the program's node map compiled
// as a one-tile map, so its entries -- one per underlying node, in node order, in engine.hpp's
// entry format -- are uploaded per device by CompiledMap::plan_for_current_device and shared by
// every plane.
class ClayCheck {
public:
    explicit ClayCheck(ClayCheckProgram pg);
    const ClayCheckProgram &program() const { return pg_; }
    CompiledMap &nodes() { return nodes_; }

private:
    ClayCheckProgram pg_;
    CompiledMap nodes_;
};

// Clay isParityCorrect over device-resident stripes (k_clay_check), in
// ecx_clay_perform_coding_batch's input layout: real slot z * n_real + node of stripe s at
// base + s * stripe_stride + slot * sub_stride.  verdict[s] = 1 when every syndrome byte of stripe
// s over [0, buf_size) of every sub-chunk is zero, else 0.  Read-only on the stripes.
void launch_clay_check(ClayCheck &cc, const uint8_t *base, int64_t stripe_stride, int64_t sub_stride, uint8_t *verdict,
                       int64_t nstripes, int64_t buf_size, hipStream_t stream);

}  // namespace ecx
