// layout_probe.cpp -- launch registry, probe events and the probe guard (layout_probe.hpp).
#include "layout_probe.hpp"

#include "launch_rules.hpp"  // kLayoutNCand

namespace ecx {

namespace {
// A filled layout probe still open to contamination: until a launch on another stream of its
// device finds its end event done, such a launch may share the GPU with it (`dirty`).
struct OpenProbe {
    hipStream_t stream;
    hipEvent_t e1;
    std::shared_ptr<std::atomic<bool>> dirty;
};
// A stream's launches: the latest one's serial, and an event recorded behind its latest LARGE
// launch (>= kMarkBytes of input), so a probe can tell whether one may still run.  A smaller
// launch runs for microseconds, negligible against a multi-millisecond probe, and is not marked.
struct StreamMark {
    uint64_t serial = 0;
    hipEvent_t done = nullptr;
    bool marked = false;  // `done` was recorded behind a large launch of this stream
};
constexpr int64_t kMarkBytes = 64 << 20;
constexpr uint64_t kUnmarkedLarge = 1ull << 63;  // serial flag: a large launch whose event failed
struct DevLaunches {
    uint64_t serial = 0;
    std::map<hipStream_t, StreamMark> last;  // aged out, below
    std::vector<OpenProbe> open;
};
constexpr uint64_t kStreamAge = 4096;  // a stream silent for this many launches leaves `last`
std::mutex g_launch_mu;
std::map<int, DevLaunches> g_launches;
}  // namespace

bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return true;  // unknown: treated as capturing
    }
    return cap != hipStreamCaptureStatusNone;
}

uint64_t note_device_launch(int dev, hipStream_t s, int64_t bytes) {
    // Only a large launch and the ageing pass make event calls, so only they ask the stream; a
    // capturing stream then makes none (layout_probe.hpp): its launch is counted, nothing else.
    const bool large = bytes >= kMarkBytes && !stream_is_capturing(s);
    std::lock_guard<std::mutex> lk(g_launch_mu);
    DevLaunches &d = g_launches[dev];
    StreamMark &mk = d.last[s];
    mk.serial = ++d.serial;
    if (large) {
        if (!mk.done && hipEventCreateWithFlags(&mk.done, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            mk.done = nullptr;
        }
        // unmarked when the record fails: this large launch then counts as possibly running
        mk.marked = mk.done && hipEventRecord(mk.done, s) == hipSuccess;
        if (!mk.marked) {
            (void)hipGetLastError();
            mk.serial |= kUnmarkedLarge;
        }
    }
    // An open probe on another stream, at a large launch: still running -> this launch may
    // overlap it (dirty); finished -> no later launch can, so its window closes here.  Either way
    // it leaves the list.
    for (auto it = d.open.begin(); large && it != d.open.end();) {
        if (it->stream == s) {  // same stream: queued behind the probe
            ++it;
            continue;
        }
        const hipError_t q = hipEventQuery(it->e1);
        if (q == hipErrorNotReady) it->dirty->store(true);
        else if (q != hipSuccess) (void)hipGetLastError();
        it = d.open.erase(it);
    }
    // bounded: streams not seen for kStreamAge launches are forgotten (their events are destroyed:
    // not from a capturing stream, which leaves the pass to a later launch)
    if (d.serial % 256 == 0 && (large || (bytes < kMarkBytes && !stream_is_capturing(s))))
        for (auto it = d.last.begin(); it != d.last.end();) {
            if ((it->second.serial & ~kUnmarkedLarge) + kStreamAge >= d.serial) {
                ++it;
                continue;
            }
            if (it->second.done) (void)hipEventDestroy(it->second.done);
            it = d.last.erase(it);
        }
    return d.serial;
}

uint64_t stream_last_launch(int dev, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_launch_mu);
    auto it = g_launches.find(dev);
    if (it == g_launches.end()) return 0;
    auto jt = it->second.last.find(s);
    return jt == it->second.last.end() ? 0 : jt->second.serial & ~kUnmarkedLarge;
}

bool other_stream_may_run(int dev, hipStream_t s, uint64_t since) {
    std::lock_guard<std::mutex> lk(g_launch_mu);
    auto it = g_launches.find(dev);
    if (it == g_launches.end()) return false;
    for (const auto &kv : it->second.last) {
        if (kv.first == s) continue;
        const StreamMark &mk = kv.second;
        if (mk.serial & kUnmarkedLarge) {  // a large launch without an event: assume it may run
            if ((mk.serial & ~kUnmarkedLarge) > since) return true;
        } else if (mk.marked) {  // its latest large launch: running iff the event is not done
            const hipError_t q = hipEventQuery(mk.done);
            if (q == hipErrorNotReady) return true;
            if (q != hipSuccess) (void)hipGetLastError();
        }
    }
    return false;
}

std::shared_ptr<std::atomic<bool>> open_probe(int dev, hipStream_t s, hipEvent_t e1, bool dirty) {
    auto flag = std::make_shared<std::atomic<bool>>(dirty);
    std::lock_guard<std::mutex> lk(g_launch_mu);
    if (!dirty) g_launches[dev].open.push_back({s, e1, flag});
    return flag;
}

void close_probe(int dev, hipEvent_t e1) {
    std::lock_guard<std::mutex> lk(g_launch_mu);
    auto it = g_launches.find(dev);
    if (it == g_launches.end()) return;
    auto &v = it->second.open;
    for (auto jt = v.begin(); jt != v.end(); ++jt)
        if (jt->e1 == e1) {
            v.erase(jt);
            return;
        }
}

LayoutSelection::~LayoutSelection() {
    for (auto &kv : running_)
        for (auto &p : kv.second) {
            close_probe(p.dev, p.e1);
            (void)hipEventDestroy(p.e0);
            (void)hipEventDestroy(p.e1);
        }
}

int LayoutSelection::choice(int64_t pitch, std::vector<float> *ms, int *state, int *dropped) {
    std::lock_guard<std::mutex> lk(mu_);
    return table_.choice(pitch, ms, state, dropped);
}

void LayoutSelection::poll(const LayoutKey &key) {
    auto kt = running_.find(key);
    if (kt == running_.end()) return;
    auto &v = kt->second;
    for (auto it = v.begin(); it != v.end();) {
        const hipError_t q = hipEventQuery(it->e1);
        if (q == hipErrorNotReady) {
            ++it;
            continue;
        }
        float ms = 0.f;
        const bool timed = q == hipSuccess && hipEventElapsedTime(&ms, it->e0, it->e1) == hipSuccess && ms > 0.f;
        close_probe(it->dev, it->e1);  // before its events go
        if (!timed) (void)hipGetLastError();  // a failed probe is dropped; its candidate is timed again
        const ProbeOutcome::Kind kind = !timed              ? ProbeOutcome::kFailed
                                        : it->dirty->load() ? ProbeOutcome::kContaminated
                                                            : ProbeOutcome::kClean;
        table_.report(key, it->ticket, {kind, ms});
        (void)hipEventDestroy(it->e0);
        (void)hipEventDestroy(it->e1);
        it = v.erase(it);
    }
}

ProbeGuard::ProbeGuard(LayoutSelection &sel, const LayoutKey &key, int dev, hipStream_t stream)
    : sel_(sel), key_(key), dev_(dev), stream_(stream) {
    {
        std::lock_guard<std::mutex> lk(sel_.mu_);
        sel_.poll(key_);  // also after the choice, so late probes free their events
        const LayoutTable::Pick p = sel_.table_.pick(key_, kLayoutNCand, kLayoutSamples);
        cand_ = p.cand;
        ticket_ = p.ticket;
        if (ticket_) since_ = stream_last_launch(dev_, stream_);
    }
    if (ticket_ && (hipEventCreate(&e0_) != hipSuccess || hipEventCreate(&e1_) != hipSuccess)) {
        (void)hipGetLastError();
        drop();
    }
}

ProbeGuard::~ProbeGuard() { drop(); }

void ProbeGuard::drop() {
    if (!ticket_) return;
    if (e0_) (void)hipEventDestroy(e0_);
    if (e1_) (void)hipEventDestroy(e1_);
    e0_ = e1_ = nullptr;
    std::lock_guard<std::mutex> lk(sel_.mu_);
    sel_.table_.cancel(key_, ticket_);
    ticket_ = 0;
}

void ProbeGuard::finish() {
    if (!ticket_) return;
    if (hipEventRecord(e1_, stream_) != hipSuccess) {
        (void)hipGetLastError();
        return;  // the destructor drops the probe
    }
    std::lock_guard<std::mutex> lk(sel_.mu_);
    // contaminated already if another stream's latest launch may still run as the probe
    // is enqueued; later launches are judged by note_device_launch while it is open
    sel_.running_[key_].push_back(
        {ticket_, e0_, e1_, dev_, open_probe(dev_, stream_, e1_, other_stream_may_run(dev_, stream_, since_))});
    ticket_ = 0;
    e0_ = e1_ = nullptr;
}

}  // namespace ecx
