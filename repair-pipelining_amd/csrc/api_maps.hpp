// api_maps.hpp -- what the C ABI (ecx_api.cpp) decides before it launches anything: the
// coefficient maps of the per-call and partial-sum entry points, the key their plans are cached
// under, and the small pure rules of the layout and check exports.
//
// The planner's types (codes.hpp, gf.hpp) and nothing else: no HIP header, so every map here is
// compared with its definition on the CPU (tests/native/api_core_check.cpp).
#pragma once

#include <cstdint>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "codes.hpp"

namespace ecx {

std::vector<bool> present_vec(const uint8_t *p, int n);

// The n_out x n_in matrix `m` over slots 0..n_in-1 -> 0..n_out-1, zero columns kept.
LinearMap dense_map(const uint8_t *m, int n_out, int n_in);

// checkSomeShards' map: row o = rows[o] over the n_in inputs plus 1 x to_check[o] (slot n_in + o),
// i.e. the syndrome, all zero exactly when to_check[o] is right.  Pruned.
LinearMap check_map(const uint8_t *rows, int n_out, int n_in);
// isParityCorrect's (ReedSolomon.java:129-178): the check map of the parity rows over a stripe.
LinearMap rs_check_map(const RsCode &c);

// One-input map: row o = the coefficient of input slot `column_slot` in row o of `m` (0 where `m`
// does not read it), out slots 0..n_out-1.
LinearMap single_input_map(const LinearMap &m, int column_slot);
// One-input map of encodeParity: row p = parityRows[p][input_index], out slots 0..m-1.
LinearMap encode_partial_map(const RsCode &c, int input_index);

// decodeMissingSingle's map over the inputs [shard, outputs 0..output_count-1]: row j =
// D^-1[missing_j][index] x shard, plus 1 x output j unless `is_first` (= or ^=); pruned.  Throws,
// in this order: fewer than k present -> ECX_E_SINGULAR; more outputs or missing data shards than
// parity rows -> ECX_E_INDEX; more outputs than missing data shards -> ECX_E_NULL; `index` outside
// 0..k-1 -> ECX_E_INDEX.
LinearMap decode_single_map(const RsCode &c, const std::vector<bool> &present, int index, int output_count,
                            bool is_first);

// out (=|^=) c x in over the inputs [in, out]: the row [c, accumulate], both columns kept.
LinearMap scale_map(uint8_t c, bool accumulate);

// A map's content -- shape, slots, coefficients -- as a cache key: equal exactly for equal maps.
std::string map_key(const LinearMap &m);

// The plain layout's pitch: the smallest ODD multiple of 4 KiB at or
// above the shard.  4 KiB-aligned shards run full-chunk kernels only, and an odd count keeps the
// streams off the power-of-two boundaries whose address bits the HBM interleave does not spread.
int64_t recommended_pitch(int64_t byte_count);

// base + (count - 1) * stride per (count, stride) pair + bytes, as the furthest byte a batch reaches
// from its base pointer; false when a stride is negative or the sum leaves int64_t.
bool extent_fits(std::initializer_list<std::pair<int64_t, int64_t>> dims, int64_t bytes);

// The distinct rows of present[nstripes][shards] (as 0 / 1) into `patterns` in first-seen order,
// each stripe's row number into `ids`; returns their count, throws ECX_E_ILLEGAL_ARGUMENT past `cap`.
int index_patterns(int shards, const uint8_t *present, int64_t nstripes, uint8_t *patterns, int cap, uint8_t *ids);

// A blocked check's pass into the per-stripe verdicts: verdict[s] = (first_pass ? 1 : verdict[s])
// && every one of the stripe's `divisor` unit verdicts.
void fold_unit_verdicts(const uint8_t *unit, int64_t divisor, bool first_pass, uint8_t *verdict, int64_t nstripes);

}  // namespace ecx
