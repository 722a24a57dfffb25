// host_pipe.cpp -- pipelined host-memory batches.
//
// The reference's repair path starts and ends in host memory.  Helper
// sub-chunks arrive on sockets into ByteBuffers (ClayCoordinator.kt:372-395),
// and repaired sub-chunks leave the same way (ClayCodeNode.kt:330-347).
// run_host_batch takes the device batch layout with host pointers.  It streams
// chunks of stripes through a ring of device buffer sets on three streams, so
// the PCIe transfers of chunk i+1 and i-1 overlap the kernel of chunk i
// (run_ring has the waits).
//
// Only the map's used input slots cross PCIe; the Clay(4,2) e=1 repair, for
// example, moves 20 of the 48 sub-chunks of a stripe.  Consecutive used slots
// that are also consecutive in host memory form a run; a chunk's copies are
// planned from the runs (host_plan.cpp make_plan): periodic runs folded into one 2D copy,
// other progressions of equal runs in one 3D copy each, a one-chunk batch of
// huge stripes cut into column slices, and over a device list, few stripes
// split by byte ranges (ecx_map_host_plan reports the plan).
//
// run_host_check_batch is the same ring with one verdict byte per stripe coming back, and
// run_host_mixed_batch the same ring for a pattern set decoded in place:
// the union of the patterns' slots goes up, the union of their output slots comes back.
// run_host_map_mixed_batch is the ring for a pattern set run out of place.
//
// Everything here touches HIP; what a batch decides is host_plan.cpp.
#include <algorithm>
#include <cstring>
#include <thread>

#include "host_pipe.hpp"
#include "pattern_set.hpp"

namespace ecx {
namespace {

// Copy `rows` rows of `width` bytes between two pitched layouts.
void copy_rows(uint8_t *dst, int64_t dpitch, const uint8_t *src, int64_t spitch, int64_t width, int64_t rows,
               hipMemcpyKind kind, hipStream_t s) {
    if (rows == 1 || (dpitch == width && spitch == width)) {
        check_hip(hipMemcpyAsync(dst, src, (size_t)(width * rows), kind, s), "hipMemcpyAsync (host batch)");
        return;
    }
    if (dpitch >= width && spitch >= width) {
        check_hip(hipMemcpy2DAsync(dst, (size_t)dpitch, src, (size_t)spitch, (size_t)width, (size_t)rows, kind, s),
                  "hipMemcpy2DAsync (host batch)");
        return;
    }
    for (int64_t r = 0; r < rows; ++r)
        check_hip(hipMemcpyAsync(dst + r * dpitch, src + r * spitch, (size_t)width, kind, s),
                  "hipMemcpyAsync (host batch row)");
}

// One planned copy for the `n` stripes of a chunk: host side at `host` (stripe stride
// `host_stripe`), device side at `dev` (stripe stride `dev_stripe`), in direction `kind`.
void issue_copy(const Copy &c, const uint8_t *host_base, uint8_t *dev_base, int64_t host_stripe, int64_t dev_stripe,
                int64_t n, hipMemcpyKind kind, hipStream_t s) {
    uint8_t *host = const_cast<uint8_t *>(host_base) + c.host_off;
    uint8_t *dev = dev_base + c.dev_off;
    const bool h2d = kind == hipMemcpyHostToDevice;
    if (c.three_d) {
        hipMemcpy3DParms p;
        std::memset(&p, 0, sizeof(p));
        const hipPitchedPtr hptr = make_hipPitchedPtr(host, (size_t)c.host_pitch, (size_t)c.width,
                                                      (size_t)(host_stripe / c.host_pitch));
        const hipPitchedPtr dptr = make_hipPitchedPtr(dev, (size_t)c.dev_pitch, (size_t)c.width,
                                                      (size_t)(dev_stripe / c.dev_pitch));
        p.srcPtr = h2d ? hptr : dptr;
        p.dstPtr = h2d ? dptr : hptr;
        p.extent = make_hipExtent((size_t)c.width, (size_t)c.rows, (size_t)n);
        p.kind = kind;
        if (hipMemcpy3DAsync(&p, s) == hipSuccess) return;
        (void)hipGetLastError();  // refused shape (nothing enqueued): the same rows as per-stripe 2D copies
        for (int64_t t = 0; t < n; ++t)
            copy_rows(h2d ? dev + t * dev_stripe : host + t * host_stripe, h2d ? c.dev_pitch : c.host_pitch,
                      h2d ? host + t * host_stripe : dev + t * dev_stripe, h2d ? c.host_pitch : c.dev_pitch, c.width,
                      c.rows, kind, s);
        return;
    }
    if (h2d) copy_rows(dev, c.dev_pitch, host, c.host_pitch, c.width, n * c.rows, kind, s);
    else copy_rows(host, c.host_pitch, dev, c.dev_pitch, c.width, n * c.rows, kind, s);
}

// Bytes [c0, c0 + w) of every used slot of `n` stripes between the host layout (stripe stride
// host_stripe, slot stride slot_stride) and a compact device slice ([stripe][used slot][w]): per
// stripe, each progression of runs is one 3D copy -- w bytes of each of a run's slots (slot_stride
// apart), runs ds slots apart -- or a 2D copy for a lone run.
void issue_sliced(const std::vector<Run> &runs, const std::vector<Segment> &segs, const uint8_t *host_base,
                  uint8_t *dev_base, int64_t host_stripe, int64_t slot_stride, int64_t used, int64_t n, int64_t w,
                  hipMemcpyKind kind, hipStream_t s) {
    const bool h2d = kind == hipMemcpyHostToDevice;
    for (int64_t t = 0; t < n; ++t)
        for (const Segment &g : segs) {
            const Run &r = runs[g.i];
            uint8_t *host = const_cast<uint8_t *>(host_base) + t * host_stripe + r.slot0 * slot_stride;
            uint8_t *dev = dev_base + (t * used + r.compact0) * w;
            if (g.j > g.i) {
                hipMemcpy3DParms p;
                std::memset(&p, 0, sizeof(p));
                const hipPitchedPtr hptr = make_hipPitchedPtr(host, (size_t)slot_stride, (size_t)w, (size_t)g.ds);
                const hipPitchedPtr dptr = make_hipPitchedPtr(dev, (size_t)w, (size_t)w, (size_t)g.dc);
                p.srcPtr = h2d ? hptr : dptr;
                p.dstPtr = h2d ? dptr : hptr;
                p.extent = make_hipExtent((size_t)w, (size_t)r.len, g.j - g.i + 1);
                p.kind = kind;
                if (hipMemcpy3DAsync(&p, s) == hipSuccess) continue;
                (void)hipGetLastError();  // refused shape (nothing enqueued): run by run
            }
            for (size_t k = g.i; k <= g.j; ++k) {
                uint8_t *hk = host + (runs[k].slot0 - r.slot0) * slot_stride;
                uint8_t *dk = dev + (runs[k].compact0 - r.compact0) * w;
                if (h2d) copy_rows(dk, w, hk, slot_stride, w, runs[k].len, kind, s);
                else copy_rows(hk, slot_stride, dk, w, w, runs[k].len, kind, s);
            }
        }
}

// Per-device streams, buffer sets and events of the host-batch pipeline.
class HostPipe {
public:
    struct Set {
        uint8_t *in = nullptr, *out = nullptr;
        size_t in_cap = 0, out_cap = 0;
        hipEvent_t loaded = nullptr, computed = nullptr, drained = nullptr;
    };

    static HostPipe &current() {
        static std::mutex reg_mu;
        static std::map<int, std::unique_ptr<HostPipe>> reg;
        int dev = 0;
        check_hip(hipGetDevice(&dev), "hipGetDevice");
        std::lock_guard<std::mutex> lk(reg_mu);
        auto &slot = reg[dev];
        if (!slot) {
            auto p = std::make_unique<HostPipe>();
            for (hipStream_t *s : {&p->h2d, &p->cmp, &p->d2h})
                check_hip(hipStreamCreateWithFlags(s, hipStreamNonBlocking), "hipStreamCreate (host batch)");
            slot = std::move(p);
        }
        return *slot;
    }

    // Called with every stream idle (the previous call synchronised).
    void ensure(int nb, size_t in_bytes, size_t out_bytes) {
        while ((int)sets.size() < nb) {
            Set s;
            for (hipEvent_t *e : {&s.loaded, &s.computed, &s.drained})
                check_hip(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate (host batch)");
            sets.push_back(s);
        }
        for (int k = 0; k < nb; ++k) {
            Set &s = sets[k];
            if (s.in_cap < in_bytes) {
                if (s.in) check_hip(hipFree(s.in), "hipFree (host batch)");
                s.in = nullptr;
                s.in_cap = 0;
                check_hip(hipMalloc(&s.in, in_bytes), "hipMalloc (host batch)");
                s.in_cap = in_bytes;
            }
            if (s.out_cap < out_bytes) {
                if (s.out) check_hip(hipFree(s.out), "hipFree (host batch)");
                s.out = nullptr;
                s.out_cap = 0;
                check_hip(hipMalloc(&s.out, out_bytes), "hipMalloc (host batch)");
                s.out_cap = out_bytes;
            }
        }
    }

    void drain() {
        for (hipStream_t s : {h2d, cmp, d2h}) (void)hipStreamSynchronize(s);
    }

    std::mutex mu;
    hipStream_t h2d = nullptr, cmp = nullptr, d2h = nullptr;
    std::vector<Set> sets;
};

// The ring every host batch runs through: `units` units over the current device's pipe, unit i in
// buffer set i % nb (each of in_bytes / out_bytes at least).  Per unit, up(i, set) enqueues its
// H2D copies on `h2d`, launch(i, set) its kernels on `cmp`, down(i, set) its D2H copies on `d2h`:
//
//   h2d stream:  [in i] [in i+1] ...
//   cmp stream:         [run i]  ...
//   d2h stream:                [out i] ...
//
// A set is reused by unit i once i >= nb, while unit i - nb may still be in flight; what each
// stream then waits for depends on where the launch writes:
//
//   output                          | H2D waits on | compute waits on             | D2H waits on
//   separate (map batches, check)   | computed     | loaded, and drained once the | computed
//                                   |              | ring has wrapped             |
//   in place (mixed)                | drained      | loaded only                  | computed
//
// Separate: the set's input may be overwritten as soon as the kernel that read it is done, and
// the kernel must not write the output area before the earlier unit's D2H has left it.  In place:
// the input buffer IS the output, so the H2D itself must wait for the earlier unit's D2H -- and
// the kernel, ordered after that H2D by `loaded`, needs no wait of its own on `drained`.
//
// Returns with every copy landed (d2h synchronised; `sync_what` names the path in that error); on
// any error all three streams are drained before it is rethrown, so no copy still targets the
// caller's memory.
template <typename Up, typename Launch, typename Down>
void run_ring(int nb, int64_t units, size_t in_bytes, size_t out_bytes, bool in_place, const char *sync_what,
              Up &&up, Launch &&launch, Down &&down) {
    HostPipe &p = HostPipe::current();
    std::lock_guard<std::mutex> lk(p.mu);
    try {
        p.ensure(nb, in_bytes, out_bytes);
        for (int64_t i = 0; i < units; ++i) {
            HostPipe::Set &b = p.sets[(size_t)(i % nb)];
            if (i >= nb)
                check_hip(hipStreamWaitEvent(p.h2d, in_place ? b.drained : b.computed, 0), "hipStreamWaitEvent");
            up(i, b, p.h2d);
            check_hip(hipEventRecord(b.loaded, p.h2d), "hipEventRecord");
            check_hip(hipStreamWaitEvent(p.cmp, b.loaded, 0), "hipStreamWaitEvent");
            if (i >= nb && !in_place) check_hip(hipStreamWaitEvent(p.cmp, b.drained, 0), "hipStreamWaitEvent");
            launch(i, b, p.cmp);
            check_hip(hipEventRecord(b.computed, p.cmp), "hipEventRecord");
            check_hip(hipStreamWaitEvent(p.d2h, b.computed, 0), "hipStreamWaitEvent");
            down(i, b, p.d2h);
            check_hip(hipEventRecord(b.drained, p.d2h), "hipEventRecord");
        }
        check_hip(hipStreamSynchronize(p.d2h), sync_what);
    } catch (...) {
        p.drain();
        throw;
    }
}

}  // namespace

void run_host_batch(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                    uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                    int64_t nbytes) {
    if (nstripes <= 0 || nbytes <= 0 || cm.map().n_out == 0) return;
    CompiledMap &cc = cm.compact();
    const Tuning &t = tuning();
    const Plan pl = make_plan(cm.used_in_slots(), cm.used_out_slots(), in_stripe_stride, in_slot_stride,
                              out_stripe_stride, out_slot_stride, nstripes, nbytes, true, t.host_chunk, t.host_buffers);
    const int64_t in_per = pl.in_per, out_per = pl.out_per, chunk = pl.chunk;
    const bool sliced = pl.nslices > 1;
    const int64_t used_in = (int64_t)cm.used_in_slots().size(), used_out = (int64_t)cm.used_out_slots().size();
    // a unit: n whole-slot stripes from stripe lo, or (sliced) bytes [c0, c0 + w) of every stripe
    struct Unit {
        int64_t lo, n, c0, w;
    };
    auto unit = [&](int64_t i) -> Unit {
        if (sliced) return {0, nstripes, i * pl.slice, std::min(pl.slice, nbytes - i * pl.slice)};
        return {i * chunk, std::min(chunk, nstripes - i * chunk), 0, nbytes};
    };
    run_ring(
        pl.nb, sliced ? pl.nslices : pl.nchunks,
        (size_t)(sliced ? nstripes * used_in * pl.slice : chunk * in_per),
        (size_t)(sliced ? nstripes * used_out * pl.slice : chunk * out_per), false,
        "hipStreamSynchronize (host batch)",
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            const Unit u = unit(i);
            if (sliced)
                issue_sliced(pl.rin, pl.sin, in + u.c0, b.in, in_stripe_stride, in_slot_stride, used_in, u.n, u.w,
                             hipMemcpyHostToDevice, s);
            else
                for (const Copy &c : pl.cin)
                    issue_copy(c, in + u.lo * in_stripe_stride, b.in, in_stripe_stride, in_per, u.n,
                               hipMemcpyHostToDevice, s);
        },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            const Unit u = unit(i);
            launch_apply(cc, b.in, used_in * u.w, u.w, b.out, used_out * u.w, u.w, u.n, u.w, s);
        },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            const Unit u = unit(i);
            if (sliced)
                issue_sliced(pl.rout, pl.sout, out + u.c0, b.out, out_stripe_stride, out_slot_stride, used_out, u.n,
                             u.w, hipMemcpyDeviceToHost, s);
            else
                for (const Copy &c : pl.cout)
                    issue_copy(c, out + u.lo * out_stripe_stride, b.out, out_stripe_stride, out_per, u.n,
                               hipMemcpyDeviceToHost, s);
        });
}

HostBatchPlan plan_host_batch(CompiledMap &cm, int64_t in_stripe_stride, int64_t in_slot_stride,
                              int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes, int64_t nbytes) {
    if (cm.map().n_out == 0) return HostBatchPlan();  // run_host_batch moves nothing
    const Tuning &t = tuning();
    return host_batch_plan(cm.used_in_slots(), cm.used_out_slots(), in_stripe_stride, in_slot_stride,
                           out_stripe_stride, out_slot_stride, nstripes, nbytes, t.host_chunk, t.host_buffers);
}

void run_host_check_batch(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                          int64_t nstripes, int64_t nbytes, uint8_t *verdict) {
    if (nstripes <= 0) return;
    if (!verdict) throw Error(ECX_E_NULL, "verdict buffer is null");
    if (nbytes <= 0 || cm.map().n_out == 0) {  // nothing to compare: every stripe passes (as launch_check)
        std::memset(verdict, 1, (size_t)nstripes);
        return;
    }
    // The read-only twin of run_host_batch: the check map's used slots cross PCIe into a set's
    // compact buffer, k_gf_check writes one verdict byte per stripe of the chunk into the set's
    // output area, and only those bytes come back.
    CompiledMap &cc = cm.compact();
    const Tuning &t = tuning();
    const Plan pl = make_plan(cm.used_in_slots(), cm.used_out_slots(), in_stripe_stride, in_slot_stride, 0, 0, nstripes,
                              nbytes, false, t.host_chunk, t.host_buffers);
    const int64_t in_per = pl.in_per, chunk = pl.chunk;
    auto count = [&](int64_t i) { return std::min(chunk, nstripes - i * chunk); };
    run_ring(
        pl.nb, pl.nchunks, (size_t)(chunk * in_per), (size_t)chunk, false, "hipStreamSynchronize (host check batch)",
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            for (const Copy &c : pl.cin)
                issue_copy(c, in + i * chunk * in_stripe_stride, b.in, in_stripe_stride, in_per, count(i),
                           hipMemcpyHostToDevice, s);
        },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            launch_check(cc, b.in, in_per, nbytes, b.out, count(i), nbytes, s);
        },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            check_hip(hipMemcpyAsync(verdict + i * chunk, b.out, (size_t)count(i), hipMemcpyDeviceToHost, s),
                      "hipMemcpyAsync (verdicts)");
        });
}

HostMixedIds::HostMixedIds(const uint8_t *host_ids, int64_t nstripes) {
    if (nstripes <= 0) return;
    check_hip(hipMalloc(&dev_, (size_t)nstripes), "hipMalloc (pattern ids)");
    if (hipMemcpy(dev_, host_ids, (size_t)nstripes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev_);
        dev_ = nullptr;
        throw Error(ECX_E_DEVICE, "hipMemcpy (pattern ids)");
    }
}

HostMixedIds::~HostMixedIds() {
    if (dev_) (void)hipFree(dev_);
}

// The in-place twin of run_host_batch for a pattern set.  The plan of a set addresses slots by
// their shard index (each pattern its own), so a set's buffer keeps all n slots of a unit at the
// pass's own pitch and only the copies are sparse (make_mixed_plan): up_slots go H2D, the mixed
// launch runs over the buffer in place with the chunk's first unit (a chunk may begin mid-stripe:
// the launcher finds each unit's id through the divisor), and down_slots come back.  up_slots
// contains down_slots (pattern_set.hpp): a down slot comes back for every stripe, also for one
// whose pattern leaves it alone, and must then carry that stripe's own bytes.
void run_host_mixed_batch(PatternSet &set, const uint8_t *dev_ids, uint8_t *base, int64_t stripe_stride,
                          int64_t slot_stride, int n, int64_t units, int64_t nbytes, int64_t divisor) {
    if (units <= 0 || nbytes <= 0 || set.down_slots().empty()) return;
    const Tuning &t = tuning();
    const HostMixedPlan mp = make_mixed_plan(set.up_slots(), set.down_slots(), stripe_stride, slot_stride, n, units,
                                             nbytes, t.host_chunk, t.host_buffers);
    const int64_t per = mp.per, chunk = mp.chunk;
    auto count = [&](int64_t i) { return std::min(chunk, units - i * chunk); };
    auto copies = [&](const std::vector<Copy> &cs, int64_t i, HostPipe::Set &b, hipMemcpyKind kind, hipStream_t s) {
        for (const Copy &c : cs)
            issue_copy(c, base + i * chunk * stripe_stride, b.in, stripe_stride, per, count(i), kind, s);
    };
    run_ring(
        mp.nb, mp.nchunks, (size_t)(chunk * per), 0, true, "hipStreamSynchronize (host mixed batch)",
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) { copies(mp.cin, i, b, hipMemcpyHostToDevice, s); },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            launch_apply_mixed_units(set, dev_ids, b.in, per, nbytes, count(i), nbytes, divisor, i * chunk, s);
        },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) { copies(mp.cout, i, b, hipMemcpyDeviceToHost, s); });
}

// The out-of-place twin for a tiled set: the ring in its separate-output mode.  A set's input
// buffer keeps every input slot of a stripe at its own index and its output buffer every output
// slot (make_map_mixed_plan).  The launch writes only what a stripe's own pattern writes, and every
// output slot of every stripe goes back, so the chunk's output area is cleared on the compute
// stream first -- after the ring's wait for the earlier unit's D2H, before the launch.
void run_host_map_mixed_batch(const MapMixedRun &run, const uint8_t *dev_ids, const uint8_t *in,
                              int64_t in_stripe_stride, int64_t in_slot_stride, int n_in, uint8_t *out,
                              int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes, int64_t nbytes) {
    if (nstripes <= 0 || nbytes <= 0 || run.out_slots.empty()) return;
    const Tuning &t = tuning();
    const int n_out = (int)run.out_slots.size();
    const HostMapMixedPlan mp = make_map_mixed_plan(run.in_slots, run.out_slots, in_stripe_stride, in_slot_stride,
                                                    n_in, out_stripe_stride, out_slot_stride, n_out, nstripes, nbytes,
                                                    t.host_chunk, t.host_buffers);
    const int64_t chunk = mp.chunk;
    auto count = [&](int64_t i) { return std::min(chunk, nstripes - i * chunk); };
    run_ring(
        mp.nb, mp.nchunks, (size_t)(chunk * mp.in_per), (size_t)(chunk * mp.out_per), false,
        "hipStreamSynchronize (host map mixed batch)",
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            for (const Copy &c : mp.cin)
                issue_copy(c, in + i * chunk * in_stripe_stride, b.in, in_stripe_stride, mp.in_per, count(i),
                           hipMemcpyHostToDevice, s);
        },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            check_hip(hipMemsetAsync(b.out, 0, (size_t)(count(i) * mp.out_per), s), "hipMemsetAsync (host map mixed batch)");
            run.launch(dev_ids, b.in, mp.in_per, nbytes, b.out, mp.out_per, nbytes, count(i), nbytes, i * chunk, s);
        },
        [&](int64_t i, HostPipe::Set &b, hipStream_t s) {
            for (const Copy &c : mp.cout)
                issue_copy(c, out + i * chunk * out_stripe_stride, b.out, out_stripe_stride, mp.out_per, count(i),
                           hipMemcpyDeviceToHost, s);
        });
}

void check_device_list(const int *devices, int ndev) {
    if (!devices) throw Error(ECX_E_NULL, "null device list");
    if (ndev <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "empty device list");
    int count = 0;
    check_hip(hipGetDeviceCount(&count), "hipGetDeviceCount");
    for (int j = 0; j < ndev; ++j)
        if (devices[j] < 0 || devices[j] >= count)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "device " + std::to_string(devices[j]) + " of " +
                                                    std::to_string(count) + " visible");
}

namespace {

// One worker thread per device entry over contiguous stripe ranges; `range(j, lo, n)` runs on
// entry j's worker with its device current.  Bad ids are refused before any worker starts; the
// first failing device's status is thrown after every worker has joined (each drains its own pipe).
template <typename F>
void on_devices(const int *devices, int ndev, int64_t nstripes, F &&range) {
    check_device_list(devices, ndev);
    if (nstripes <= 0) return;
    struct Result {
        int code = ECX_OK;
        std::string what;
    };
    std::vector<Result> res((size_t)ndev);
    auto work = [&](int j) {
        int64_t lo = 0, hi = 0;
        stripe_range(nstripes, ndev, j, &lo, &hi);
        if (hi <= lo) return;
        try {
            check_hip(hipSetDevice(devices[j]), "hipSetDevice (host batch worker)");
            range(j, lo, hi - lo);
        } catch (const Error &e) {
            res[(size_t)j] = {e.code, e.what()};
        } catch (const std::bad_alloc &) {
            res[(size_t)j] = {ECX_E_NOMEM, "out of memory"};
        } catch (const std::exception &e) {
            res[(size_t)j] = {ECX_E_ILLEGAL_ARGUMENT, e.what()};
        }
    };
    // the caller's thread (and its current device) only waits
    std::vector<std::thread> th;
    th.reserve((size_t)ndev);
    try {
        for (int j = 0; j < ndev; ++j) th.emplace_back(work, j);
    } catch (...) {
        for (std::thread &t : th) t.join();
        throw Error(ECX_E_NOMEM, "cannot start a host-batch worker thread");
    }
    for (std::thread &t : th) t.join();
    for (int j = 0; j < ndev; ++j)
        if (res[(size_t)j].code != ECX_OK)
            throw Error(res[(size_t)j].code, "device " + std::to_string(devices[j]) + ": " + res[(size_t)j].what);
}

}  // namespace

void run_host_batch_devices(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                            uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                            int64_t nbytes, const int *devices, int ndev) {
    if (nbytes <= 0 || cm.map().n_out == 0) nstripes = 0;  // validate the list, touch nothing
    if (const int64_t units = column_units(nstripes, ndev, nbytes)) {  // byte ranges of every slot
        on_devices(devices, ndev, units, [&](int, int64_t u0, int64_t nu) {
            const int64_t c0 = u0 * kColUnit, w = std::min(nu * kColUnit, nbytes - c0);
            run_host_batch(cm, in + c0, in_stripe_stride, in_slot_stride, out + c0, out_stripe_stride, out_slot_stride,
                           nstripes, w);
        });
        return;
    }
    on_devices(devices, ndev, nstripes, [&](int, int64_t lo, int64_t n) {
        run_host_batch(cm, in + lo * in_stripe_stride, in_stripe_stride, in_slot_stride, out + lo * out_stripe_stride,
                       out_stripe_stride, out_slot_stride, n, nbytes);
    });
}

void run_host_check_batch_devices(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride,
                                  int64_t in_slot_stride, int64_t nstripes, int64_t nbytes, uint8_t *verdict,
                                  const int *devices, int ndev) {
    if (nstripes > 0 && !verdict) throw Error(ECX_E_NULL, "verdict buffer is null");
    // Byte ranges: each entry checks its range of every slot into its own verdicts, and a stripe
    // passes when it passes in every range.
    const int64_t units = cm.map().n_out > 0 ? column_units(nstripes, ndev, nbytes) : 0;
    if (units) {
        std::vector<std::vector<uint8_t>> part((size_t)ndev);
        on_devices(devices, ndev, units, [&](int j, int64_t u0, int64_t nu) {
            std::vector<uint8_t> &v = part[(size_t)j];
            v.assign((size_t)nstripes, 0);
            const int64_t c0 = u0 * kColUnit, w = std::min(nu * kColUnit, nbytes - c0);
            run_host_check_batch(cm, in + c0, in_stripe_stride, in_slot_stride, nstripes, w, v.data());
        });
        std::memset(verdict, 1, (size_t)nstripes);
        for (const std::vector<uint8_t> &v : part)
            for (size_t s2 = 0; s2 < v.size(); ++s2) verdict[s2] = (uint8_t)(verdict[s2] && v[s2]);
        return;
    }
    on_devices(devices, ndev, nstripes, [&](int, int64_t lo, int64_t n) {
        run_host_check_batch(cm, in + lo * in_stripe_stride, in_stripe_stride, in_slot_stride, n, nbytes,
                             verdict + lo);
    });
}

}  // namespace ecx
