// clay_check_plan.hpp -- the codeword test of a Clay geometry as a per-plane program, the
// structure the check kernel (apply_clay_check.hip) executes, and its proof.  Plain C++ over the
// planner (codes.hpp); a unit of its own beside it, so that the planner's sources -- which the
// committed PMC profile of the repair kernels is keyed to -- stay byte for byte what they were.
//
// A stripe is a codeword exactly when, in every plane z, the decoupled symbols form a codeword
// of the plane code RS(k + v, m):
//   decouple   U(z, j) = C(z, j) for a dot node j = (x, y), zvec(z)[y] == x; otherwise
//              U(z, j) = pair_a * C(z, j) + pair_b * C(z', j'), z' = z[y := x], j' = (zvec(z)[y], y).
//              A virtual node's own C is zero; its U is not when its partner is real.
//   syndromes  S(z, p) = sum_{j < k+v} prow[p][j] * U(z, j) + U(z, k + v + p),  p < m
// The coefficient columns do not depend on the plane and the partner follows from the digits of
// z, so the program has no per-plane table: node_map() is all the kernel uploads.
#pragma once

#include <vector>

#include "codes.hpp"

namespace ecx {

constexpr int kClayCheckMaxParity = 8;  // one accumulator tile (launch_rules.hpp kTileRows)

struct ClayCheckProgram {
    int q = 0, t = 0, alpha = 0, m = 0, n_under = 0, n_real = 0, virtual_units = 0;
    uint8_t pair_a = 0, pair_b = 0;
    std::vector<uint8_t> prow;  // m x (n_under - m): the parity rows of the plane code
    std::vector<int> real_of;   // underlying node -> real node, -1 = virtual
    // Coefficient of U(z, j) in syndrome p (any z).
    uint8_t coef(int p, int j) const { return j < n_under - m ? prow[(size_t)p * (n_under - m) + j] : (j - (n_under - m) == p); }
    // The m x n_under map of the decoupled symbols of one plane to its syndromes (in_slot = the
    // underlying node): compiled, its one tile's entries are the kernel's per-node records.
    LinearMap node_map() const;
    // The dense syndrome map: m * alpha rows (z * m + p) over the n_real * alpha real input
    // slots z * n_real + real of ecx_clay_perform_coding_batch.
    LinearMap compose() const;
};

// The codeword test of the planner's geometry (its erasure set plays no part), built from the
// planner's primitives as ClayPlanner::repair_program is: pair_a and pair_b from the RS(2,2) pair
// transform's decode map, the parity rows of RS(k + v, m), q, t, the real slot numbering.  The
// program is proved before it is returned: with E = perform_coding_map of the parity nodes from
// the data nodes, compose() applied to [I; E] is zero entry for entry (every codeword passes), and
// compose()'s square block over the parity nodes' m * alpha columns is invertible (nothing else
// does).  Throws ECX_E_ILLEGAL_ARGUMENT when pair_a ^ pair_b != 1, when parity_units exceeds
// kClayCheckMaxParity, when the nodes do not fill the q x t grid, or when a proof fails.
// swap_pair (tests only): build the program with pair_a and pair_b exchanged.
ClayCheckProgram clay_check_program(const ClayPlanner &pl, bool swap_pair = false);

}  // namespace ecx
