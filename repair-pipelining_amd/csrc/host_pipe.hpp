// host_pipe.hpp -- the host-memory batches of host_pipe.cpp: the read-only check and the in-place
// mixed decode, each over one device or a device list, and the plan report of the map batches.
// host_plan.hpp has what they decide; this is what they enqueue.  The map batches themselves
// (run_host_batch, run_host_batch_devices) are declared in engine.hpp, which this includes:
// engine.hpp is hashed with the kernel sources of the committed PMC profile
// (profiles/pmc_traffic.json), so its text moves only together with a new profile.
#pragma once

#include <functional>

#include "engine.hpp"
#include "host_plan.hpp"

namespace ecx {

class PatternSet;

// How run_host_batch would move a batch (host_batch_plan over the map's used slots and the knobs).
HostBatchPlan plan_host_batch(CompiledMap &cm, int64_t in_stripe_stride, int64_t in_slot_stride,
                              int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes, int64_t nbytes);

// launch_check over host-memory stripes: the check map's used slots of each chunk of stripes
// go H2D, k_gf_check writes the chunk's verdict bytes on the device and only those come back
// into the host array `verdict` (one byte per stripe).  Synchronous, on the current device.
void run_host_check_batch(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                          int64_t nstripes, int64_t nbytes, uint8_t *verdict);
// run_host_check_batch split over a device list, as run_host_batch_devices.
void run_host_check_batch_devices(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride,
                                  int64_t in_slot_stride, int64_t nstripes, int64_t nbytes, uint8_t *verdict,
                                  const int *devices, int ndev);

// The mixed decode over HOST memory, synchronous, in place, on the current device: one pass of
// `units` units of n slots of nbytes bytes (stripe_stride / slot_stride apart in host memory),
// `divisor` units per caller stripe; `dev_ids` is the device copy of the caller's ids.  Chunks of
// units go H2D (up_slots), through launch_apply_mixed_units, and D2H (down_slots).
void run_host_mixed_batch(PatternSet &set, const uint8_t *dev_ids, uint8_t *base, int64_t stripe_stride,
                          int64_t slot_stride, int n, int64_t units, int64_t nbytes, int64_t divisor);
// What the out-of-place ring needs of a set: the input slots that go up, the output slots
// 0 .. n-1 that come back, and the launch over one chunk of stripes -- unit u of the chunk runs
// the list ids[first_unit + u].  A composed set (PatternSet, launch_map_mixed) and a generated
// one (ClaySetRtc, k_clay_repair_set) both fill it in.
struct MapMixedRun {
    const std::vector<int> &in_slots;
    const std::vector<int> &out_slots;
    std::function<void(const uint8_t *ids, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                       uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t units, int64_t nbytes,
                       int64_t first_unit, hipStream_t stream)>
        launch;
};
// The out-of-place twin for a set of maps of several tiles (the Clay repair with a list per
// stripe), synchronous, on the current device: `nstripes` stripes of n_in input slots at `in` and
// out_slots.size() output slots at `out`, both in host memory.  Chunks of stripes go H2D
// (in_slots), through run.launch into an output area cleared on the compute stream, and
// D2H (out_slots): what a stripe's own pattern does not write comes back as zeros.
void run_host_map_mixed_batch(const MapMixedRun &run, const uint8_t *dev_ids, const uint8_t *in,
                              int64_t in_stripe_stride, int64_t in_slot_stride, int n_in, uint8_t *out,
                              int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes, int64_t nbytes);
// The caller's host ids on the current device for the length of one host call (freed by the
// destructor): they cross once per call, not once per chunk.
class HostMixedIds {
public:
    HostMixedIds(const uint8_t *host_ids, int64_t nstripes);
    ~HostMixedIds();
    HostMixedIds(const HostMixedIds &) = delete;
    HostMixedIds &operator=(const HostMixedIds &) = delete;
    const uint8_t *get() const { return dev_; }

private:
    uint8_t *dev_ = nullptr;
};

// The refusals of a device list, before anything is copied: a null list, an empty one, an id that
// is not among the visible devices.
void check_device_list(const int *devices, int ndev);

}  // namespace ecx
