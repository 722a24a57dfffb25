// locate2_plan.hpp -- the pair plan of an RS code (include/ecx.h ecx_rs_locate_corrupt2_batch,
// DESIGN.md section 4.8.1): which PAIR of shards, replaced together, can make a stripe that fails
// isParityCorrect (ReedSolomon.java:129-178) pass again.
//
// With H = [P | I] the m x n check matrix and S(b) = H * x(b) the syndromes at byte b (locate_plan.hpp),
// the pair {i, j}, i < j, explains the stripe exactly when S(b) lies in span(H_i, H_j) at every b.
// That is m - 2 TEST ROWS per pair, linear in the syndromes and all zero exactly then: a basis of
// the left null space of the m x 2 matrix [H_i H_j], from one Gaussian elimination of [H_i H_j | I]
// whatever kind of shard i and j are (a row reads at most three syndromes: its own and the two
// pivots').  Any basis will do, only zero or non-zero matters.
// The C(n,2) * (m - 2) rows, pair after pair in lexicographic pair order, are cut into tiles of at
// most kLocateTileRows rows in locate_plan.hpp's format: every tile holds exactly m entry records
// in syndrome order (an unused syndrome has empty masks), and tile dword 4 + r names the SUSPECT
// INDEX of row r, n + p with p = i(2n - i - 1)/2 + (j - i - 1): a stripe's suspect row is its n
// single suspects, then its C(n,2) pair suspects.  `members` is the pair -> (i, j) table, two bytes
// per pair, that the wave shortcut reads.
//
// The wave shortcut (apply_locate2.hip): any three columns of H being independent -- the builder
// checks every triple and refuses a matrix that has a dependent one -- a wave (64 lanes x 16 B)
// whose syndromes are non-zero somewhere and that keeps the single candidate i keeps exactly the
// pairs that contain i.  It evaluates no pair tile and clears the other C(n-1,2) pair suspects
// from `members`.
//
// No HIP header, like locate_plan.hpp (tests/native/locate2_plan_check.cpp).
#pragma once

#include "locate_plan.hpp"

namespace ecx {

constexpr int kLocate2MinParity = 4;   // two errors need 2 * 2 <= m
constexpr int kLocate2MaxShards = 64;  // a wave holds one 64-bit mask of cleared single candidates
constexpr int kLocate2SpanBytes = 1024;  // one wave: 64 lanes x 16 B

struct Locate2Plan {
    std::vector<uint32_t> entries;  // n_tiles * m entries of kLocateEntryDwords
    std::vector<uint32_t> tiles;    // n_tiles records of kLocateTileDwords
    std::vector<int> suspect;       // n_pairs * (m - 2): the suspect index n + p of each test row
    std::vector<uint8_t> members;   // n_pairs * 2: (i, j) of pair p
    int k = 0, m = 0;
    int n_pairs = 0;
    int n_tiles = 0;
};

constexpr int pair_index(int n, int i, int j) { return i * (2 * n - i - 1) / 2 + (j - i - 1); }

// `parity` as build_locate_plan takes it.  False -- and *out untouched -- when k < 1, m is outside
// kLocate2MinParity..kLocateMaxParity, k + m > kLocate2MaxShards, a pointer is null, or some three
// columns of H are dependent.
bool build_locate2_plan(const uint8_t *parity, int k, int m, Locate2Plan *out);

// Both plans applied to one stripe as k_gf_locate2 reads them, span of kLocate2SpanBytes after span
// (a wave): `syn` as emulate_locate takes it; suspect[0..n) are the single suspects and
// suspect[n + p] the pair suspects, 1 when every test row of the candidate is zero at every byte.
// A span whose syndromes are all zero clears nothing.  With `shortcut`, a span that keeps exactly
// one single candidate clears the pairs that do not contain it from `members`; every other span,
// and every span without `shortcut`, evaluates the pair tiles.  False when a plan breaks its
// invariants or `single` is of another code.
bool emulate_locate2(const Locate2Plan &p, const LocatePlan &single, const uint8_t *syn, int64_t syn_stride,
                     int64_t len, uint8_t *suspect, bool shortcut);

}  // namespace ecx
