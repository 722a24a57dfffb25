// tuning.hpp -- the launch-shape knobs (include/ecx_tune.h).  No HIP: read by the launch rules
// (launch_rules.hpp) as well as by the engine.
#pragma once

#include <cstdint>

namespace ecx {

// Launch-shape knobs (diagnostics / tuning, include/ecx_tune.h).
struct Tuning {
    // Defaults are the fastest shape measured on MI355X (profiles/r01_kbench.txt).
    int depth = 0;            // k_gf_apply load ring depth: 0 = per map (preferred_depth), or forced
    int nontemporal = 1;      // 0 never, 1 auto (NT stores; NT loads for single-tile maps), 2 always
    int xcd_group = 0;        // multi-tile maps: tiles of a chunk on one XCD (measured slower: off)
    int xcd_run = 8;          // xcd_group 3 (any map): runs of this many consecutive units per XCD
    int xcd_misaligned = 1;   // xcd_group 0: single-tile maps with inputs not 128-B aligned use the runs of 3
    // Multi-tile maps: 1 = k_gf_apply_lds (tile groups share inputs via LDS), 2 =
    // k_gf_apply_grp (tile groups in one workgroup, direct loads).  Off by
    // default: Clay(10,4)'s 64-row groups still need 1.23x the unique inputs and the
    // per-stage barriers cost more than the saved traffic (profiles/r01_multitile.jsonl).
    int wave_groups = 0;
    // k_gf_apply: 0 = every table dword from the plan in SGPRs (a v_mov per 8-entry table
    // and row); 1 = the low table dwords staged once per workgroup in LDS and read as
    // VGPRs, for multi-tile maps; 2 = for every map.
    int lds_tables = 1;
    // Non-temporal output stores: 0 = `nt`; 1 = `nt sc0 sc1` (written through, dropped
    // from L2; scripts/copy_probe.hip).
    int store_scope = 0;
    // k_gf_apply: extra dynamic LDS bytes per workgroup, which caps the workgroups resident
    // per CU (160 KiB of LDS each) without touching the kernel.  0 = no cap (default); -1 =
    // single-tile maps over >= 8 inputs on rings of <= 8 loads held to 4 waves per SIMD; > 0 =
    // that many bytes.  Measured mixed on the RS maps (+2 % in fresh-process A/B runs, -2 to
    // -5 % in one-process interleaved sweeps; profiles/r03_occupancy.jsonl, r03_occ_bench.jsonl).
    int occ_lds = 0;
    // k_gf_apply block order: 0 = stripe-major (a stripe's chunks back to back), 1 = chunk-major.
    int chunk_major = 0;
    // k_gf_apply / k_gf_apply_skew unit order: 0 / 1 = none; G >= 2 = G stripes interleaved,
    // each starting at a different chunk offset (apply.hpp unit_of).
    int stagger = 0;
    // k_gf_apply workgroup: 256 threads over 4 KiB chunks (default) or 64 threads (one
    // wave) over 1 KiB chunks.
    int block_threads = 0;  // 0 = auto (launch_apply), 256 or 64 forced
    // Single-tile maps of at most 2 / 4 rows: 1 = k_gf_apply variants with that many
    // accumulator rows (fewer VGPRs, depth-12 rings possible); 0 = the 8-row kernel.
    int small_tiles = 2;  // 2 = auto (launch_apply), 1 = forced, 0 = the 8-row kernel
    // Per-call host APIs on the gather path: 1 = the kernel reads / writes the pinned
    // staging area directly over PCIe instead of one H2D and one D2H copy (20-40 % lower
    // latency per call, profiles/r01_percall_native.jsonl).
    int host_zero_copy = 1;
    // Multi-tile maps: 1 = wide tiles (pairs of 8-row tiles sharing inputs, one
    // workgroup each: 16 accumulator rows, each shared input loaded once per pair).
    int wide_tiles = 1;
    // Single-tile maps: 2 / 4 = k_gf_apply_skew with that many 4 KiB chunks per
    // workgroup, each entry's chunk rotated; 1 = 4 when the input slot pitch is a
    // multiple of 4 MiB; 0 = off.
    int skew_chunks = 1;
    // Many-stream single-tile maps (>= 8 inputs, <= 4 rows) with the shape knobs on auto: 1 =
    // the launch shape chosen per batch layout by timing the caller's own first launches
    // (kernels.hip launch_apply; default), 0 = the static rules only.
    int layout_select = 1;
    // Per-call CodingLoop entry points: compiled plans kept, by map content (0 = none).
    int plan_cache = 256;
    // Bit-sliced kernel (k_gf_bits): 2 = for every map it can run (aligned layout, 32-bit
    // slot offsets, 4 KiB chunks), 1 = for multi-tile maps that do not pair into wide
    // tiles, 0 = never (default: it measured 4-10 % slower on every BASELINE map, bound
    // by its scalar branches -- profiles/r02_bits_ab.jsonl, r02_bits_sq_ab.json).
    int bitslice = 0;
    // LDS lookup-table kernel (k_gf_lut, apply_lut.hip) for the full 4 KiB chunks of
    // aligned layouts, forced-only: 1 = log/antilog tables, 2 = one 256-B product row per
    // coefficient (single-tile maps of <= kLutMaxPairs general coefficients); 0 = never
    // (default: measured against the split tables in DESIGN.md 4.4).
    int lds_lut = 0;
    // Clay single-node repair batches: the per-helper-plane kernel generated for the
    // repair and compiled with hiprtc (clay_rtc.hpp) for whole 4 KiB chunks -- 1 = when
    // the composed map spans several tiles (auto), 2 = always, 0 = never.
    int clay_rtc = 1;
    int rtc_lookahead = 1;  // the generated kernel's load lookahead (items), 0..3
    int rtc_waves = 3;      // its __launch_bounds__ minimum waves per SIMD, 2..4
    int rtc_group = 1;      // 1: the plane-group kernel (k_clay_repair_grp) where the program allows it
                            // (+4-8 % over one plane per workgroup on Clay(10,4), profiles/r02_grp_sweep.jsonl)
    int rtc_persist = 0;    // its persistent grid: workgroups per CU (0 = one workgroup per unit)
    int rtc_diag = 0;       // its DIAGNOSTIC builds (clay_rtc.hpp RtcShape::diag; ECX_DIAGNOSTIC=1 only)
    int rtc_units = 1;      // plane-group kernel: 512-B slices per workgroup, 1 or 2 (software-pipelined)
    int rtc_sched = 2;      // plane-group kernel load schedule: 0 = rtc_lookahead's, 1 = lean, 2 = all loads
                            // up front with pinned accumulators (+0.8-2.4 % over 0 on two boxes,
                            // profiles/r03_clay104_final.jsonl, r03_clay104_lean_run2.jsonl)
    int rtc_wide = 0;       // plane-group kernel: 1 = 64-bit load addresses on every layout (auto, 0: only
                            // where slot offsets exceed 31 bits, RtcShape::wide)
    int rtc_nt = 5;         // non-temporal loads in the generated Clay kernels (RtcShape::nt bits):
                            // 5 = the plane-group kernel's read-once rows and row-yc partner loads,
                            // +3-6 % on Clay(10,4) over cached loads (profiles/r03_clay104_nt.jsonl)
    int rtc_xcd = 2;        // its block order: 1 = the helper planes of a (stripe, chunk) on one XCD;
                            // 2 (plane-group kernel): whole (stripe, chunk) units per XCD, +4.5 %
                            // (+1.1 % on Clay(10,4), profiles/r02_rtc_sweep.jsonl)
    // Generated bit-plane kernel for one composed map (k_map_planes, map_rtc.hpp): 1 = auto
    // for multi-tile maps of <= 16 rows whose coefficients outnumber their inputs by 4x or
    // more (vector-bound under the split tables: the Clay(4,2) two-node repairs), on
    // batches of >= 64 MiB of input; 2 = wherever it fits; 0 = never.
    int map_planes = 1;
    int planes_lookahead = 12;  // its load lookahead (inputs in flight), 0..15 (profiles/r02_planes_ab.jsonl)
    int planes_waves = 2;      // its __launch_bounds__ minimum waves per SIMD, 1..4
    int64_t host_chunk = 64 << 20;  // host-batch pipeline: input bytes per H2D chunk
    int host_buffers = 3;           // host-batch pipeline: device buffer sets in flight
    // per-call host APIs: byte counts up to this gather the used slots into pinned staging (one
    // H2D / one D2H); above it the runtime copies each slot (512 KiB: the crossover of the two,
    // profiles/r02_percall_sizes.jsonl)
    int64_t host_gather_max = 512 << 10;
    int host_contexts = 1;  // per-call host APIs: 1 = a pool of contexts (streams) leased per call, 0 = one per device
    // per-call host APIs: byte counts up to this run on the calling thread (host_exec.cpp) instead of
    // the device -- the measured per-call crossover (profiles/r06_percall_threshold.jsonl): with one
    // caller thread the device first wins at 2 MiB (Clay(4,2) performCoding; the RS(2,2) pair never,
    // to 4 MiB), with 16 at no size to 4 MiB; 0 = never
    int64_t host_exec_max = 1 << 20;
    // single-tile maps: (stripe, chunk) units per workgroup with one load ring across them
    // (k_gf_apply_multi, apply_multi.hip): 1 = one unit per workgroup (k_gf_apply), 2 or 4
    int units = 1;
};

}  // namespace ecx
