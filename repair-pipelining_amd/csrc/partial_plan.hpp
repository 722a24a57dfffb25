// partial_plan.hpp -- the partial-sum plan of a pattern set (include/ecx.h
// ecx_rs_decode_partial_batch_mixed): one hop of the pipelined repair
// chain -- ReedSolomon.decodeMissingSingle (ReedSolomon.java:288-333) for every missing shard --
// over stripes that name their erasure pattern AND the shard this helper holds with one byte each.
//
// For every pattern p < npatterns and shard i < n the plan holds ONE entry in the engine's entry
// format (engine.hpp: kEntryDwords; [0] input slot, [1] rows with a general coefficient, [2] rows
// with coefficient 1, [4 + 5r ..) the split tables of row r): the entry of the one-input map whose
// row o is D_p[o][i], the coefficient of shard i in the o-th missing shard of pattern p (ascending;
// data and parity rows; zero when pattern p does not read shard i -- it is missing, or present but
// not among the first k).  Entry (p, i) is entry p * n + i.  The input slot is always 0: the kernel
// has one input stream.  A table of kPartialRecords (256) row counts, zero past npatterns, says how
// many accumulator rows pattern p has; a stripe names its pattern with one byte, so every value of
// that byte selects a count inside the table, and a count of zero ends the workgroup before it
// forms an entry index -- k_gf_partial_mixed (apply_partial_mixed.hip) needs no bounds branch on
// the id, and one compare of the shard byte against n.
//
// No HIP header and no other unit of the engine but the field (gf.hpp): the plan and its
// interpreter run -- and are tested -- on the CPU (tests/native/partial_plan_check.cpp).  The
// constants repeat engine.hpp's; pattern_set.hpp asserts that they agree.
#pragma once

#include <cstdint>
#include <vector>

namespace ecx {

constexpr int kPartialRecords = 256;
constexpr int kPartialEntryDwords = 48;
constexpr int kPartialRows = 8;

// One pattern's decode map as LinearMap holds it: `matrix` is [rows][n_in], row o the o-th missing
// shard, column j the coefficient of shard in_slot[j].  rows == 0: nothing missing.
struct PartialPatternIn {
    int rows = 0;
    int n_in = 0;
    const uint8_t *matrix = nullptr;
    const int *in_slot = nullptr;
};

struct PartialPlan {
    std::vector<uint32_t> entries;  // npatterns * n entries of kPartialEntryDwords
    std::vector<uint32_t> rows;     // kPartialRecords row counts, zero past npatterns
    int npatterns = 0;
    int n = 0;         // shards per stripe
    int max_rows = 0;  // the largest row count of the set: which ROWS instance can run it
};

// False -- and *out untouched -- when npatterns is outside 1..kPartialRecords, n is not positive,
// a pattern has more than kPartialRows rows or a negative count, or a pointer it needs is null.
bool build_partial_plan(const PartialPatternIn *patterns, int npatterns, int n, PartialPlan *out);

// The plan applied to one stripe as k_gf_partial_mixed reads it for id byte `id` and shard byte
// `shard` (any bytes): `in` is the helper's len input bytes, acc row o lies at acc + o * row_stride.
// Rows [0, rows of the pattern) are assigned (is_first) or XOR-accumulated; nothing else is
// written, and nothing at all for a row count of zero or shard >= n.  False when the plan breaks
// its invariants (table or entry array of the wrong size, a row count above kPartialRows, an entry
// with a non-zero slot or with mask bits at or above its row count).
bool emulate_partial(const PartialPlan &p, uint8_t id, uint8_t shard, const uint8_t *in, uint8_t *acc,
                     int64_t row_stride, int64_t len, bool is_first);

}  // namespace ecx
