// launch_rules.hpp -- which kernels a composed-map batch launches, and in what shape.
//
// choose_launch() is a pure function of the map's traits, the tuning knobs and the batch
// layout: it touches no device and includes no HIP header, so every rule below runs -- and is
// tested -- on the CPU (tests/native/launch_rules_check.cpp, GfMap.launch_plan).  Its result,
// a LaunchPlan, lists the launches in issue order; kernels.hip launch_apply_core only walks it.
// describe() is the string ecx_last_launch_shape reports after that walk.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

#include "tuning.hpp"

namespace ecx {

constexpr int kTileRows = 8;
constexpr int kChunkBytes = 4096;  // one 256-thread workgroup x 16 bytes per lane
constexpr int kBlockThreads = 256;
constexpr size_t kLdsPerCu = 160 * 1024;  // MI355X (gfx950) LDS per CU
constexpr int kSimdsPerCu = 4;
constexpr int kOccWavesPerSimd = 4;       // the residency cap of the many-stream single-tile maps
constexpr int kWaveChunkBytes = 1024;  // k_gf_apply_lds: 64 lanes x 16 bytes per wave
constexpr int kAtabDwords = 2 * kTileRows;
constexpr int kMaxLdsTileEntries = 512;  // 32 KiB of LDS per workgroup at most
constexpr int kLutMaxPairs = 256;  // k_gf_lut mode 1: 64 KiB of product rows per workgroup at most

// Everything the rules read from a CompiledMap (CompiledMap::traits()).
struct MapTraits {
    int n_tiles = 0, n_groups = 0, group_size = 0, n_wide_tiles = 0;
    double wide_sharing = 1.0;
    int wide_depth = 4, preferred_depth = 4, max_tile_rows = 0;
    int max_in_slot = -1, max_out_slot = -1;
    int n_in = 0, n_out = 0, nnz = 0;
    int used_inputs = 0;           // input columns with a non-zero coefficient
    int general_coeffs = 0;        // coefficients other than 0 and 1 (k_gf_lut's product rows)
    bool planes_supported = false; // a bit-plane generator exists for the map (map_rtc.hpp)
    int max_tile_count = 0;        // entries of the longest tile, unpadded
    bool slots_intersect = false;  // some output slot is also an input slot
    // HostPlan::max_tile_entries of the plan padded for load-ring depth `depth`
    int max_tile_entries(int depth) const { return (max_tile_count + depth - 1) / depth * depth; }
};

struct BatchLayout {
    uintptr_t in = 0, out = 0;
    int64_t in_stripe_stride = 0, in_slot_stride = 0, out_stripe_stride = 0, out_slot_stride = 0;
    int64_t nstripes = 0, nbytes = 0;
    bool accumulate = false;
    bool aligned16() const {
        return ((in | out) & 15) == 0 && in_stripe_stride % 16 == 0 && in_slot_stride % 16 == 0 &&
               out_stripe_stride % 16 == 0 && out_slot_stride % 16 == 0;
    }
};

// "The generated bit-plane kernel is available for this accumulate mode": the one input of
// the rules that may compile something, asked only where the auto rule has chosen the kernel.
struct PlanesAvailable {
    bool (*fn)(void *ctx) = nullptr;
    void *ctx = nullptr;
    bool operator()() const { return fn && fn(ctx); }
};

enum class Family { Apply, ApplyTail, Wide, Skew, Planes, Lds, Grp, Bits, Lut, Multi };

// One kernel launch (per batch of stripes: launch_apply_core splits grids over 2^30 blocks).
struct Launch {
    Family family = Family::Apply;
    // the template instance: what each family reads of these is what its name shows
    bool safe = false;   // the byte-safe instance (partial chunks, unaligned layouts)
    bool ntl = false;    // non-temporal loads
    int nts = 0;         // store policy (apply.hpp st16)
    int depth = 4;       // load ring
    bool tlds = false;   // k_gf_apply: low table dwords in LDS
    int threads = kBlockThreads;
    int rows = kTileRows;
    int skew = 0;        // k_gf_apply_skew: 4 KiB chunks per workgroup
    int units = 1;       // k_gf_apply_multi: (stripe, chunk) units per workgroup
    int lut_mode = 0, lut_pairs = 0;  // k_gf_lut
    // the bytes it covers: chunks [chunk_begin, chunk_begin + n_chunks) of chunk_bytes each
    int64_t chunk_begin = 0, n_chunks = 0;
    int chunk_bytes = kChunkBytes;
    int64_t units_per_stripe = 0;  // grid blocks (k_gf_apply_multi: units) per stripe
    size_t lds = 0;                // dynamic LDS: the TLDS tables plus ecx_tune "occ_lds"
    // k_gf_apply_tail / _multi: the launch's last chunk is the shard's partial last chunk
    bool fused_tail = false;
    int64_t tail_chunk = -1;
    int tail_bytes = 0;
    bool of_record = false;  // names the call in ecx_last_kernel (never a byte-safe launch, nor
                             // a launch of the partial chunk alone)
};

struct LaunchPlan {
    std::array<Launch, 4> launches;  // in issue order
    int n_launches = 0;
    int depth = 4;       // the padded plan the launches read (CompiledMap::plan_for_current_device)
    // the unit order of the whole call (ApplyArgs)
    int stagger = 0, xcd_group = 0, xcd_run = 0, chunk_major = 0;
    int skew = 0;
    int record = -1;     // the launch of record, -1: the call leaves ecx_last_kernel as it was
    bool planes = false; // k_map_planes is among the launches: no unit order is reported
};

// pick: -1 = the static rules (skew on 4 MiB-multiple input slot pitches, one-wave
// workgroups for narrow maps otherwise); else shape + 8 * stagger with shape 0 = 256-thread
// workgroups over 4 KiB chunks, 1 = skewed chunks, 2 = one-wave workgroups over 1 KiB
// chunks, 3 = skewed chunks on one-wave workgroups (1 KiB columns, diagnostic build), and
// stagger the unit order (apply.hpp unit_of) -- the per-layout candidates.
// `diag`: the diagnostic build (make DIAG=1), the only one that holds the lab kernels.
LaunchPlan choose_launch(const MapTraits &m, const Tuning &tu, const BatchLayout &b, int pick, bool diag,
                         PlanesAvailable planes_available);

// The kernel instance of one launch as rocprofv3 names it.
std::string kernel_name(const Launch &l);
// "stagger=G xcd_group=X xcd_run=R[ skew=K]": the unit order the kernel name does not encode;
// empty when the call has no kernel of record or runs k_map_planes.
std::string unit_order(const LaunchPlan &p);
// What ecx_last_launch_shape reports after the call ("" = what it reported before).
std::string describe(const LaunchPlan &p);

// May a partial last chunk run in the main launch (apply.hpp: that workgroup re-reads the end of
// the previous chunk)?  Only if no output byte of the launch is an input byte of it: disjoint
// buffers, or one buffer laid out as [stripe][slot][bytes] whose output slots are not inputs.
bool outputs_never_read(const MapTraits &m, const BatchLayout &b);

// Per-layout launch-shape selection (kernels.hip launch_apply): candidate 0 = the static rules,
// then shape + 8 * stagger (choose_launch's pick); -2 for an index out of range.
constexpr int kLayoutCand[] = {-1, 0, 1, 2, 2 + 8 * 2, 2 + 8 * 8, 0 + 8 * 4};
constexpr int kLayoutNCand = (int)(sizeof(kLayoutCand) / sizeof(kLayoutCand[0]));
int layout_candidate_code(int cand);
// Batches under kLayoutMinBytes of input and forced shapes use the static rules: whether this
// map, layout and tuning take part in the selection (a stream being captured never does).
constexpr int64_t kLayoutMinBytes = (int64_t)256 << 20;
bool layout_select_eligible(const MapTraits &m, const Tuning &tu, const BatchLayout &b);

}  // namespace ecx
