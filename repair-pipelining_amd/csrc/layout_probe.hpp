// layout_probe.hpp -- the HIP side of the per-layout launch-shape selection: the events that time a
// call, the launch registry that tells whether another stream may have shared the GPU with it, and
// the guard kernels.hip launch_apply brackets its launch with.  What the timings decide is
// layout_select.hpp's LayoutTable; nothing here chooses a shape.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "layout_select.hpp"

namespace ecx {

// Per-device launch registry, read by the layout selection's contamination check:
// every batch launch of the library (launch_apply, launch_check, the generated Clay kernels)
// records its stream and input bytes here.  note_device_launch returns the launch's serial and,
// for a launch of >= 64 MiB, records an event behind it (smaller launches run for microseconds
// and never count as overlapping a probe); stream_last_launch is the serial of a stream's latest
// launch (0 = none); other_stream_may_run whether a stream other than `s` on device `dev` has a
// large launch that may still run (its event is not done; or no event could be recorded and it
// came after `since`).  Streams unseen for 4,096 launches age out of the registry.
// A launch on a stream that is being captured (or whose capture status cannot be read) makes no
// event call at all: a record would become a node of the caller's graph, replayed long after the
// registry has destroyed the event, and a query of another stream's probe may invalidate the
// capture.  Such a launch does not run now, so it marks nothing either; the graph's replays never
// pass through here and are invisible to the contamination check.
bool stream_is_capturing(hipStream_t s);  // true also when the status is unknown
uint64_t note_device_launch(int dev, hipStream_t s, int64_t bytes);
uint64_t stream_last_launch(int dev, hipStream_t s);
bool other_stream_may_run(int dev, hipStream_t s, uint64_t since);
// A layout probe whose end event `e1` is recorded on `s`: registered (unless already `dirty`)
// so that note_device_launch on another stream of `dev` flags it while it runs; close_probe
// unregisters it before its events are destroyed.
std::shared_ptr<std::atomic<bool>> open_probe(int dev, hipStream_t s, hipEvent_t e1, bool dirty);
void close_probe(int dev, hipEvent_t e1);

// A map's selection: the decision table plus the events of its timed calls still running.  A probe
// is CONTAMINATED, not counted, when another stream of the same device had a large libecx launch
// that may still run when the probe was enqueued, or enqueued one while the probe was still running
// (the first such launch that finds the probe's end event done closes its window;
// note_device_launch): that kernel may have shared the GPU with the probe.
// Lock order: this object's lock, then the registry's; never the reverse.
class LayoutSelection {
public:
    ~LayoutSelection();
    int choice(int64_t pitch, std::vector<float> *ms, int *state, int *dropped);  // LayoutTable::choice

private:
    friend class ProbeGuard;
    struct Probe {
        uint64_t ticket;
        hipEvent_t e0, e1;
        int dev;
        std::shared_ptr<std::atomic<bool>> dirty;  // set when another stream's launch may overlap it
    };
    // Reads the finished probes of `key` (non-blocking) and reports each to the table.
    void poll(const LayoutKey &key);
    std::mutex mu_;
    LayoutTable table_;
    std::map<LayoutKey, std::vector<Probe>> running_;  // per layout, in launch order
};

// One call of layout `key` on `stream` of device `dev`: polls the layout's finished probes, then
// picks the candidate to run.  When the call is to be timed, start() is the event to record in front
// of the kernels (null otherwise) and finish() -- after the launch and its note_device_launch --
// records the end event and hands both to the selection.  A guard that was not finished (the launch
// threw, an event could not be created or recorded) destroys its events and gives its ticket back.
class ProbeGuard {
public:
    ProbeGuard(LayoutSelection &sel, const LayoutKey &key, int dev, hipStream_t stream);
    ~ProbeGuard();
    ProbeGuard(const ProbeGuard &) = delete;
    ProbeGuard &operator=(const ProbeGuard &) = delete;
    int cand() const { return cand_; }
    hipEvent_t start() const { return e0_; }
    void finish();

private:
    void drop();  // destroys the events and cancels the ticket, if it still holds one
    LayoutSelection &sel_;
    const LayoutKey key_;
    const int dev_;
    const hipStream_t stream_;
    int cand_ = 0;
    uint64_t ticket_ = 0;  // 0: untimed, or finished
    uint64_t since_ = 0;   // the stream's last launch serial before this probe (note_device_launch)
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

}  // namespace ecx
