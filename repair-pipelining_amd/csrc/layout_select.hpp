// layout_select.hpp -- the decisions of the per-layout launch-shape selection (ecx_tune
// "layout_select"): which candidate shape a call of a batch layout runs, and whether it is timed.
//
// LayoutTable holds no event and no stream and includes no HIP header: what a timed call measured
// is REPORTED to it (layout_probe.hpp does the timing), so every rule below runs -- and is tested
// -- on the CPU (tests/native/layout_select_check.cpp, tests/golden/layout_trace.txt.gz).
//
// A layout (its key: strides, size classes, mode, device -- kernels.hip launch_apply) starts
// EXPLORING: pick() hands the candidates out in turn, each with a non-zero ticket, until every one
// of the n_cand candidates has `samples` clean times; a ticket stays pending, and counts towards
// its candidate, until it is reported or cancelled, so concurrent callers are never handed the
// same probe twice and no candidate is timed more than `samples` times at once (when every probe
// is in flight the call runs candidate 0, untimed).  Then the fastest median is CHOSEN: candidate 0
// -- the static rules -- unless another is faster by kLayoutMargin.  report() takes what became of
// a ticket: a clean time is counted, a contaminated one (another stream's launch may have shared
// the GPU with it) is DROPPED and only bumps `dropped`, a failed one vanishes, and its candidate is
// timed again.  After kLayoutMaxDropped dropped probes the layout is CONTENDED and keeps
// candidate 0 untimed.  A chosen shape is re-validated once, after kLayoutRevalidate further
// picks, against its alternative -- the static rules for a non-static choice, the runner-up for a
// static one: `samples` clean times of each (REVALIDATING), and the alternative takes over if it
// wins by the margin (a non-static choice must keep beating the static rules by it); the layout is
// then REVALIDATED and never timed again.  At most kMaxLayouts layouts are selected per table
// (later ones get candidate 0, untimed, and no entry).
//
// Not synchronised: the owner (layout_probe.hpp LayoutSelection) calls it under its own lock.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace ecx {

using LayoutKey = std::array<int64_t, 8>;

enum LayoutState { kLayoutExploring = 0, kLayoutChosen = 1, kLayoutRevalidating = 2, kLayoutRevalidated = 3,
                   kLayoutContended = 4 };

constexpr int kLayoutSamples = 5;  // median of 5: 3 left a 2-5 % spread between fresh maps (scripts/select_check.py)
constexpr float kLayoutMargin = 0.98f;   // another shape replaces the static rules' only if 2 % faster
constexpr size_t kMaxLayouts = 64;       // layouts selected per map; past that, new ones use the static rules
constexpr int kLayoutMaxDropped = 64;    // contaminated probes before a layout is declared contended
constexpr int64_t kLayoutRevalidate = 512;  // launches after a choice before its one re-validation

// What became of a timed call.
struct ProbeOutcome {
    enum Kind { kClean, kContaminated, kFailed } kind;
    float ms;  // kClean: the launch time
};

class LayoutTable {
public:
    struct Pick {
        int cand;         // the candidate this call runs
        uint64_t ticket;  // non-zero: the call is to be timed, then reported or cancelled
    };
    // One layout's selection (read-only outside the table: the CPU check reads the counts).
    struct Layout {
        struct Pending {
            int cand;
            uint64_t ticket;
        };
        std::vector<std::vector<float>> ms;  // per candidate: clean launch times of its probes
        std::vector<Pending> pending;        // tickets handed out, not yet reported or cancelled
        int chosen = -1;
        int state = kLayoutExploring;
        int dropped = 0;                     // probes discarded as contaminated
        int64_t steady = 0;                  // picks since the choice (re-validation trigger)
        int reval_alt = 0;                   // the shape the kept one is re-validated against
        std::vector<float> reval_ms[2];      // re-validation timings: [0] the alternative, [1] the kept shape
        uint64_t serial = 0;                 // order of the choices (choice() reports the latest)
    };

    // The candidate to run for this call of layout `key`.  The caller reports the probes of `key`
    // that have finished BEFORE it picks (also after the choice, so late probes are retired).
    Pick pick(const LayoutKey &key, int n_cand, int samples);
    // A clean time goes to the exploration's list of the ticket's candidate, or to the
    // re-validation's pair; in any other state, or for a candidate the layout does not have, it is
    // discarded.  An unknown key or ticket is ignored.
    void report(const LayoutKey &key, uint64_t ticket, ProbeOutcome outcome);
    // Gives a ticket back untimed (its launch failed).  An unknown key or ticket is ignored.
    void cancel(const LayoutKey &key, uint64_t ticket);
    // The candidate kept for the most recently chosen layout with input slot pitch `pitch`
    // (key[0]), -1 if none yet; with `ms`, the per-candidate median launch times (ms, -1 =
    // unsampled) of that layout; with `state` its LayoutState and with `dropped` the probes it
    // dropped as contaminated.
    int choice(int64_t pitch, std::vector<float> *ms = nullptr, int *state = nullptr, int *dropped = nullptr) const;
    const Layout *layout(const LayoutKey &key) const;  // nullptr: never picked, or past kMaxLayouts

private:
    std::map<LayoutKey, Layout> layouts_;
    uint64_t choice_serial_ = 0;
    uint64_t ticket_serial_ = 0;
};

}  // namespace ecx
