// engine.hpp -- compiled GF(256) maps, device contexts and kernel launches.
//
// Kernel plan format (one "entry" per (output tile, input slot) pair with a
// non-zero coefficient; tiles of up to kTileRows output rows):
//
//   entry (kEntryDwords u32):
//     [0] input slot   [1] rows with a general coefficient (bitmask)
//     [2] rows whose coefficient is 1 (bitmask: plain XOR)   [3] 0
//     [4+5r .. 8+5r]  split multiply tables for tile row r:
//        T0a,T0b = c*v for v in 0..7        (low 3 bits of the byte)
//        T1a,T1b = c*(v<<3) for v in 0..7   (middle 3 bits)
//        T2      = c*(v<<6) for v in 0..3   (top 2 bits)
//     so that c*b = T0[b&7] ^ T1[(b>>3)&7] ^ T2[b>>6]; each lookup is one
//     v_perm_b32 over four bytes at once (GF(2)-linearity of c*b).
//   tile (kTileDwords u32): [0] first entry [1] entry count [2] rows
//     [4..4+kTileRows) output slot of each row.
#pragma once

#include <hip/hip_runtime.h>

#ifndef ECX_DIAG
#define ECX_DIAG 0  // 1: the diagnostic build (Makefile DIAG=1) with the measured-and-rejected kernels
#endif

#include <array>
#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "codes.hpp"
#include "host_exec.hpp"
#include "launch_rules.hpp"  // the shape constants (kTileRows, kChunkBytes, ...), Tuning, MapTraits
#include "layout_probe.hpp"  // LayoutSelection

namespace ecx {

constexpr int kEntryDwords = 48;
constexpr int kTileDwords = 16;
constexpr int kWaveGroup = 8;       // k_gf_apply_lds: up to 8 tiles (one wave each) per workgroup
constexpr int kGroupDwords = 16;    // group: [0..7] tiles (kNoTile = none), [8] union begin, [9] union count
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

void check_hip(hipError_t e, const char *what);

// Stream capture.  A launcher names the caller's stream for the length of
// its call (LaunchStreamScope: launch_apply, launch_check, the generated Clay kernels' branch of
// ecx_clay_perform_coding_batch); the first-use sites -- a map's device plan, the zero page, a
// generated kernel's module and table -- call refuse_if_capturing before their first HIP call.
// When the named stream is being captured (or its status cannot be read) that throws
// ECX_E_DEVICE: an allocation, a blocking copy or a module load does not belong in a capture,
// and the caller is told to run the same call once outside it.  The stream is only asked on a
// first use, so a launch whose state is resident pays nothing.  Outside a scope (the host-batch
// pipelines, which own their streams) nothing is refused.
// (stream_is_capturing: layout_probe.hpp)
class LaunchStreamScope {
public:
    explicit LaunchStreamScope(hipStream_t s);
    ~LaunchStreamScope();
    LaunchStreamScope(const LaunchStreamScope &) = delete;
    LaunchStreamScope &operator=(const LaunchStreamScope &) = delete;

private:
    hipStream_t prev_;
    bool prev_set_;
};
void refuse_if_capturing(const char *what);

class MapPlanes;  // map_rtc.hpp

constexpr uint32_t kDummySlot = 0xFFFFFFFFu;  // entry padding: loads the device's zero page

struct DevicePlan {
    uint32_t *entries = nullptr;
    uint32_t *tiles = nullptr;
    uint32_t *groups = nullptr;  // n_groups x kGroupDwords
    uint32_t *unions = nullptr;  // per group: input slots in staging order, padded (kDummySlot)
    // Per padded entry, kTileRows x {T0a, T1a}: the low table dwords of every row,
    // staged per workgroup into LDS by k_gf_apply<..., TLDS=true> (kernels.hip).
    uint32_t *atab = nullptr;
    uint32_t *wentries = nullptr;  // wide tiles (k_gf_apply_wide)
    uint32_t *wtiles = nullptr;
    uint32_t *bentries = nullptr;  // bit-sliced kernel (k_gf_bits): kBitsEntryDwords per padded entry
    int max_tile_entries = 0;  // padded
};
// Wide tiles (k_gf_apply_wide): two 8-row tiles A, B applied by one workgroup over the
// union of their inputs.  A wide entry is A's entry for the input followed by B's
// (kEntryDwords each; zero masks where a half does not read the input).  A wide tile
// record: [0] first wide entry [1] entry count [2] rows of A [3] rows of B
// [4..12) output slots of A's rows [12..20) output slots of B's rows.
constexpr int kWideEntryDwords = 2 * kEntryDwords;
constexpr int kWideTileDwords = 32;
// Bit-sliced kernel (k_gf_bits, apply_bits.hip): per padded entry [0] input slot
// [1] rows with a non-zero coefficient (bitmask) [2] coefficients of rows 0-3 (one
// byte each) [3] coefficients of rows 4-7.  Parallel to the padded `entries` array,
// so the padded `tiles` index both.
constexpr int kBitsEntryDwords = 4;
constexpr int kBitsThreads = 128;  // 128 lanes x 32 bytes = one 4 KiB chunk (kChunkBytes)

// The padded plan exactly as uploaded to a device for one load-ring depth
// (CompiledMap::padded_plan): entries/tiles padded to multiples of `depth`,
// group unions padded to whole LDS stages, and the TLDS low-table array.
struct HostPlan {
    std::vector<uint32_t> entries, tiles, groups, unions, atab, wentries, wtiles, bentries;
    int max_tile_entries = 0;
};

// 4 KiB of zeros per device, never written: the load target of padding entries
// (always L2-resident, so padding costs no HBM traffic).
const uint8_t *zero_page_for_current_device();

// A LinearMap compiled to the kernel's table format, uploaded lazily per device.
class CompiledMap {
public:
    explicit CompiledMap(LinearMap m);
    ~CompiledMap();
    const LinearMap &map() const { return map_; }
    int n_tiles() const { return n_tiles_; }
    // Multi-tile maps: tiles grouped by shared inputs, one workgroup per group
    // (engine.cpp group_tiles / align_group).
    int n_groups() const { return n_groups_; }
    int group_size() const { return group_size_; }
    int n_entries() const { return (int)(entries_.size() / kEntryDwords); }  // unpadded (1 if empty)
    // Wide tiles: the 8-row tiles paired by shared inputs (multi-tile maps only).
    int n_wide_tiles() const { return n_wide_; }
    int wide_entries() const { return (int)(wentries_.size() / kWideEntryDwords); }  // unpadded
    int wide_depth() const { return wide_depth_; }
    // Input reads saved by pairing: (sum of the paired tiles' input counts) / (sum of
    // the pairs' union sizes); 1.0 = the pairs share nothing.
    double wide_sharing() const { return wide_union_ ? (double)wide_reads_ / (double)wide_union_ : 1.0; }
    int union_total() const { return (int)unions_.size(); }                   // unpadded
    int max_in_slot() const { return max_in_slot_; }
    int max_out_slot() const { return max_out_slot_; }
    // Load-ring depth for this map: 8 when every non-empty tile has >= 12 entries
    // (padding to a multiple of 8 then costs little), else 4 (profiles/r01_configs_depth.jsonl, r01_configs_sweep2.jsonl).
    int preferred_depth() const { return preferred_depth_; }
    int max_tile_rows() const { return max_tile_rows_; }
    // What the launch rules read of this map (launch_rules.hpp), computed once at compile time.
    const MapTraits &traits() const { return traits_; }
    // The plan uploaded for the current device, each tile's entry list padded to a
    // multiple of `depth` with zero-coefficient kDummySlot entries.
    const DevicePlan &plan_for_current_device(int depth);
    // The same map over densely renumbered slots: input column j reads compact slot
    // rank(in_slot[j]) among used_in_slots() (sorted), likewise for outputs.  This is
    // the device-side layout of the host-batch pipeline (host_pipe.cpp).
    // Host interpretation of the compiled plan (diagnostics, ecx_map_selftest):
    // applies the entry tables exactly as the kernels read them -- by input slot
    // (k_gf_apply) or through the group unions (k_gf_apply_lds) -- to `in`
    // ([max_in_slot+1][len]) and writes `out` ([max_out_slot+1][len]).  Throws
    // if the union bookkeeping is inconsistent.
    void emulate(const uint8_t *in, uint8_t *out, int64_t len, bool via_unions) const;
    // The host arrays plan_for_current_device(depth) uploads.
    HostPlan padded_plan(int depth) const;
    // Host interpretation of a padded plan as k_gf_apply reads it: padding entries
    // read zeros, and with `tlds` the low dword of each 8-entry table comes from
    // HostPlan::atab (the LDS copy) instead of the entry.
    void emulate_padded(const HostPlan &p, const uint8_t *in, uint8_t *out, int64_t len, bool tlds, int depth) const;
    // The same for the padded wide-tile arrays (k_gf_apply_wide).
    void emulate_wide(const HostPlan &p, const uint8_t *in, uint8_t *out, int64_t len) const;
    // k_gf_bits on the host: the bit-sliced arithmetic of apply_bits.hip (the same
    // __host__ __device__ transpose / xtime / nibble code) over the padded
    // `bentries`, for `len` a multiple of kChunkBytes (the kernel's chunk).
    void emulate_bits(const HostPlan &p, const uint8_t *in, uint8_t *out, int64_t len) const;
    CompiledMap &compact();
    // The generated bit-plane kernel for this map (map_rtc.hpp), created on first use;
    // nullptr when the map does not fit it (more than 16 rows, too many coefficients).
    MapPlanes *planes();
    const std::vector<int> &used_in_slots();
    const std::vector<int> &used_out_slots();
    // The per-layout launch-shape selection of this map (kernels.hip launch_apply, ecx_tune
    // "layout_select"; layout_select.hpp has the rules).
    LayoutSelection &layout_selection() { return layout_; }
    // The candidate kept for the most recently selected layout with input slot pitch
    // `pitch`, -1 if none yet; with `ms`, the per-candidate median launch times (ms, -1 =
    // unsampled) of that layout; with `state` its state (LayoutState) and with `dropped` the
    // timings it dropped as contaminated.
    int layout_choice(int64_t pitch, std::vector<float> *ms = nullptr, int *state = nullptr, int *dropped = nullptr) {
        return layout_.choice(pitch, ms, state, dropped);
    }

private:
    LayoutSelection layout_;
    LinearMap map_;
    std::unique_ptr<CompiledMap> compact_;
    std::unique_ptr<MapPlanes> planes_;
    bool planes_checked_ = false;
    std::vector<int> used_in_, used_out_;
    std::vector<uint32_t> entries_, tiles_;  // unpadded
    std::vector<uint32_t> groups_, unions_;  // unpadded unions
    std::vector<uint32_t> wentries_, wtiles_;  // unpadded wide tiles
    int n_groups_ = 0, group_size_ = 0, n_wide_ = 0, wide_depth_ = 4;
    int64_t wide_reads_ = 0, wide_union_ = 0;
    int n_tiles_ = 0, max_in_slot_ = -1, max_out_slot_ = -1, preferred_depth_ = 4, max_tile_rows_ = 0;
    MapTraits traits_;
    std::mutex mu_;
    std::map<std::pair<int, int>, DevicePlan> dev_;  // (device, depth)
};

struct ApplyArgs {
    const uint8_t *in;
    uint8_t *out;
    const uint32_t *entries;
    const uint32_t *tiles;
    const uint32_t *groups;
    const uint32_t *unions;
    const uint32_t *atab;
    const uint32_t *wentries;
    const uint32_t *wtiles;
    const uint32_t *bentries;
    const uint8_t *zero_page;
    int64_t in_stripe_stride, in_slot_stride, out_stripe_stride, out_slot_stride;
    int64_t nbytes, chunk_begin, n_chunks, stripe_begin;
    int n_tiles;
    int n_wide;           // k_gf_apply_wide: wide tiles (workgroups per chunk)
    int n_groups;         // k_gf_apply_lds: tile groups (workgroups per chunk)
    int xcd_group;        // k_gf_apply: keep the tiles of one chunk on one XCD
    int xcd_run;          // k_gf_apply, xcd_group 3: units (stripe, chunk) per XCD run
    int accumulate;       // 1: out ^= M * in (partial sums along a repair chain), 0: out = M * in
    int lane_zero;        // always 0 (keeps k_gf_apply's LDS table base in a VGPR)
    int chunk_major;      // k_gf_apply block order: 0 = stripe by stripe, 1 = chunk c of every stripe, then c + 1
    int stagger;          // k_gf_apply / _skew unit order: > 1 = groups of that many stripes interleaved (unit_of)
    // k_gf_apply (not byte-safe): the chunk index holding a shard's partial last chunk when it
    // runs in the same launch as the full chunks (-1: none), and its byte count (a multiple of 16)
    int64_t tail_chunk;
    int tail_bytes;
    int64_t multi_total;  // k_gf_apply_multi: (stripe, chunk) units in the launch
};

void launch_probe(int kind, const uint8_t *src, uint8_t *dst, int64_t nbytes, bool nt, hipStream_t stream);
// The process-wide tuning (include/ecx_tune.h).  tuning() returns a snapshot taken under
// the lock update_tuning() holds while ecx_tune changes a field, so a launch reads one
// consistent set of knobs even while another thread tunes.
Tuning tuning();
void update_tuning(const std::function<void(Tuning &)> &f);

// The kernel instance of the last full-chunk (non-byte-safe) launch enqueued on this
// thread, as rocprofv3 names it ("k_gf_apply<false, true, 1, 20, false, 256, 8>").
// Diagnostics: bench.py's roofline.kernel and its PMC-profile match (ecx_last_kernel).
void set_last_kernel(std::string name);
const std::string &last_kernel();
// The full launch shape of that launch: the kernel instance plus the unit order the kernel name
// does not encode ("stagger=G xcd_group=X xcd_run=R"), set by the launcher after the kernel is
// noted (ecx_last_launch_shape; bench.py's roofline.launch_shape and its PMC-profile key).
uint64_t kernel_notes();  // set_last_kernel calls on this thread so far
void set_last_shape_order(std::string order);
std::string last_launch_shape();
inline std::string kernel_param(bool v) { return v ? "true" : "false"; }
inline std::string kernel_param(int v) { return std::to_string(v); }
template <typename... P>
void note_kernel(const char *name, P... params) {
    std::string s = name;
    s += '<';
    const char *sep = "";
    ((s += sep, s += kernel_param(params), sep = ", "), ...);
    s += '>';
    set_last_kernel(std::move(s));
}

// Enqueue out = M * in over nstripes stripes (kernels.hip); which kernels run, and in what
// shape, is decided by launch_rules.hpp choose_launch.
void launch_apply(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride, uint8_t *out,
                  int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes, int64_t nbytes,
                  hipStream_t stream, bool accumulate = false);
// isParityCorrect over device-resident stripes (apply_check.hip k_gf_check): `cm` is a check
// map (one syndrome row per parity shard); verdict[s] = 1 when every syndrome byte of stripe s
// over [0, nbytes) is zero, else 0.  Read-only on the stripes.
void launch_check(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                  uint8_t *verdict, int64_t nstripes, int64_t nbytes, hipStream_t stream);
void launch_fill_random(uint8_t *dst, int64_t nbytes, uint64_t seed, hipStream_t stream);
void launch_count_mismatch(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t nrows,
                           int64_t row_bytes, uint64_t *d_count, hipStream_t stream);

// Per-device contexts for the host (byte[][]) entry points: a stream and growable
// device / pinned staging areas each.  A call leases a free context of the current
// device for its duration (acquire), so calls from different threads run on different
// streams and overlap; a new context is created only when every existing one is busy,
// so their number follows the peak concurrency, not the thread count (a JVM thread pool
// that replaces its threads creates none).  Tuning::host_contexts 0 = one shared,
// serialised context per device.
class DeviceContext {
public:
    struct Lease {
        DeviceContext *ctx;
        std::unique_lock<std::mutex> lk;
    };
    static Lease acquire();
    std::mutex mu;
    hipStream_t stream = nullptr;
    int device = 0;
    uint8_t *ensure(size_t bytes);
    uint8_t *ensure_pinned(size_t bytes);  // page-locked host staging
    uint64_t *counter();

private:
    uint8_t *staging_ = nullptr;
    size_t staging_size_ = 0;
    uint8_t *pinned_ = nullptr;
    size_t pinned_size_ = 0;
    uint64_t *counter_ = nullptr;
};

// Host-pointer execution of a compiled map: moves each used input slot
// (`inputs[slot] + offset`, byte_count bytes) into HBM, applies the map and
// copies each output row back to `outputs[slot] + offset`.  Synchronous.  Up to
// Tuning::host_gather_max bytes the used slots are gathered into pinned staging
// (one H2D, the compact map, one D2H, scatter): per-call latency is then a few
// copies, not one pageable transfer per slot.
void run_host(CompiledMap &cm, const uint8_t *const *inputs, uint8_t *const *outputs, int64_t offset,
              int64_t byte_count);
// As run_host, but instead of copying outputs back, returns whether every
// output byte is zero (used for checkSomeShards / isParityCorrect).
bool run_host_all_zero(CompiledMap &cm, const uint8_t *const *inputs, int64_t offset, int64_t byte_count);

// The per-call executor below the CPU/GPU crossover (host_exec.hpp): whether a per-call entry point
// of `byte_count` bytes runs on the calling thread (Tuning::host_exec_max); throws ECX_E_DEVICE
// when the process has no HIP device, as the device path would.
bool host_exec_wanted(int64_t byte_count);

// Host-memory batch over many stripes (host_pipe.cpp): the batch layout of
// launch_apply, but `in`/`out` are host pointers.  Chunks of stripes are
// pipelined H2D (copy stream) -> kernel (compute stream) -> D2H (copy stream)
// through `host_buffers` device buffer sets; only the map's used slots cross
// PCIe.  Synchronous.  Pinned host memory runs at the PCIe rate.
void run_host_batch(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                    uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                    int64_t nbytes);

// Part j of `parts` contiguous stripe ranges of nstripes, the remainder on the first parts (the
// rule of shard_stripes, __init__.py; run_host_batch_devices' split).
void stripe_range(int64_t nstripes, int parts, int j, int64_t *begin, int64_t *end);
// run_host_batch over several devices (host_pipe.cpp): device j of `devices` takes the
// contiguous stripe range j of ndev (remainder on the first), on a worker thread of its own
// with that device's pipe.  Refuses bad device ids before any copy; joins every worker, then
// throws the first failing device's error.
void run_host_batch_devices(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                            uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                            int64_t nbytes, const int *devices, int ndev);

}  // namespace ecx
