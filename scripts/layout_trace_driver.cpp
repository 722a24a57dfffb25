// layout_trace_driver.cpp -- drives the layout selection AS IT WAS before it became
// csrc/layout_select.cpp, and prints what it decided (scripts/record_layout_trace.py builds and
// runs this; it is not part of the library).
//
// The recorder lifts the text of CompiledMap::harvest, next_layout_pick, fill_layout_probe,
// cancel_layout_probe and layout_choice, their constants and the LayoutSel struct out of the
// recorded commit, unaltered, into the three parent_*.inc files included below.  That code
// read its timings from HIP events; here an event is a plain struct the script below completes
// when it likes, and the launch registry is a stub (a probe is made contaminated by setting its
// flag directly).
//
// Output, one line per operation, `<operation> | <read-out>`:
//   S <name>                      a fresh map
//   K <k> <8 integers>            layout key k of this map
//   P <k> <cand> <ticket>         a pick on key k and what it returned
//   F <k> <ticket>                the timed call was launched: its events are filled in
//   X <k> <ticket>                the ticket is cancelled
//   D <k> <ticket> <c|d|f> <ms>   the probe's events complete: clean, contaminated (dirty), failed;
//                                 the selection sees it at the next pick of key k
// and the read-out is layout_choice at the key's pitch: `-1`, or `<choice> <state> <dropped>
// <median ms per candidate>`, floats as %a.
#include <algorithm>
#include <array>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

// ---- the fake events
struct FakeEvent {
    bool ready = false, ok = true;
    float ms = 0.f;
};
using hipEvent_t = FakeEvent *;
using hipStream_t = void *;
enum hipError_t { hipSuccess = 0, hipErrorNotReady, hipErrorUnknown };
static hipError_t hipEventQuery(hipEvent_t e) { return !e->ready ? hipErrorNotReady : e->ok ? hipSuccess : hipErrorUnknown; }
static hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t e1) {
    *ms = e1->ms;
    return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
    delete e;
    return hipSuccess;
}
static hipError_t hipGetLastError() { return hipSuccess; }

namespace ecx {
static void close_probe(int, hipEvent_t) {}
static std::shared_ptr<std::atomic<bool>> open_probe(int, hipStream_t, hipEvent_t, bool dirty) {
    return std::make_shared<std::atomic<bool>>(dirty);
}
static uint64_t stream_last_launch(int, hipStream_t) { return 0; }
static bool other_stream_may_run(int, hipStream_t, uint64_t) { return false; }

#include "parent_rules.inc"  // kLayoutCand, kLayoutNCand (launch_rules.hpp); kLayoutSamples (kernels.hip)

class CompiledMap {
public:
#include "parent_class.inc"  // enum LayoutState, struct LayoutSel (engine.hpp)
    int next_layout_pick(const std::array<int64_t, 8> &key, int n_cand, int samples, int dev, hipStream_t stream,
                         uint64_t *ticket);
    void fill_layout_probe(const std::array<int64_t, 8> &key, uint64_t ticket, hipEvent_t e0, hipEvent_t e1);
    void cancel_layout_probe(const std::array<int64_t, 8> &key, uint64_t ticket);
    int layout_choice(int64_t pitch, std::vector<float> *ms = nullptr, int *state = nullptr, int *dropped = nullptr);
    void harvest(LayoutSel &s, int n_cand);
    std::map<std::array<int64_t, 8>, LayoutSel> layout_sel_;
    uint64_t layout_serial_ = 0;
    uint64_t ticket_serial_ = 0;
    std::mutex mu_;
};

#include "parent_funcs.inc"  // the constants, median_of and the five functions (engine.cpp)
}  // namespace ecx

// ---- the scripts
namespace {
using Key = std::array<int64_t, 8>;

struct Rng {
    uint64_t x;
    uint64_t next() {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    float unit() { return (float)(next() >> 40) / (float)(1 << 24); }  // [0, 1)
    bool chance(float p) { return unit() < p; }
};

struct Scenario {
    const char *name;
    uint64_t seed;
    int keys;          // layout keys, picked uniformly
    int picks;         // picks in all
    int max_delay;     // a probe completes up to this many picks after its launch
    float spread;      // candidates' times: 1 +- spread around the static rules' (margin is 2 %)
    float static_bias; // added to every non-static candidate's time (> 0: the static rules tend to win) ...
    float late_bias;   // ... while exploring, and after the choice
    float p_dirty, p_fail, p_cancel, p_late_fill;
    bool share_pitch;  // keys 2j and 2j + 1 share their slot pitch (the read-out reports the later choice)
};

// Times are redrawn once a layout has chosen, so its re-validation sees other medians than its
// exploration did and all of kept / replaced x static / non-static occur.
const Scenario kScenarios[] = {
    {"plain", 1, 2, 1400, 3, 0.05f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false},
    {"tight", 2, 3, 2100, 2, 0.025f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false},
    {"static-wins", 3, 3, 2100, 3, 0.03f, 0.04f, -0.015f, 0.f, 0.02f, 0.02f, 0.2f, false},
    {"static-wins-tight", 4, 4, 2800, 1, 0.015f, 0.025f, 0.025f, 0.f, 0.f, 0.f, 0.f, true},
    {"noisy", 5, 3, 2400, 8, 0.06f, 0.f, 0.f, 0.05f, 0.05f, 0.05f, 0.3f, false},
    {"in-flight", 6, 1, 900, 60, 0.05f, 0.f, 0.f, 0.02f, 0.02f, 0.02f, 0.3f, false},
    {"in-flight-static", 7, 2, 1800, 40, 0.03f, 0.035f, -0.015f, 0.f, 0.02f, 0.02f, 0.3f, true},
    {"contended", 8, 2, 700, 6, 0.05f, 0.f, 0.f, 0.7f, 0.02f, 0.02f, 0.2f, false},
    {"contended-late", 9, 1, 600, 30, 0.05f, 0.f, 0.f, 0.6f, 0.02f, 0.f, 0.2f, false},
    {"many-keys", 10, 70, 900, 2, 0.05f, 0.f, 0.f, 0.f, 0.f, 0.05f, 0.2f, false},
    {"shared-pitch", 11, 4, 2800, 3, 0.04f, 0.01f, 0.01f, 0.01f, 0.01f, 0.01f, 0.2f, true},
    {"mixed", 12, 5, 3500, 5, 0.035f, 0.015f, 0.015f, 0.02f, 0.03f, 0.03f, 0.3f, false},
};

void print_readout(ecx::CompiledMap &cm, int64_t pitch) {
    std::vector<float> ms;
    int state = 0, dropped = 0;
    const int c = cm.layout_choice(pitch, &ms, &state, &dropped);
    if (c < 0) {
        std::printf(" | -1\n");
        return;
    }
    std::printf(" | %d %d %d", c, state, dropped);
    for (float m : ms) std::printf(" %a", (double)m);
    std::printf("\n");
}

struct Flight {
    int key;
    uint64_t ticket;
    int cand;
    hipEvent_t e0 = nullptr, e1 = nullptr;  // null: reserved, not yet filled
    int due = 0;                            // the pick before which it is filled / completes
};

void run(const Scenario &sc) {
    Rng rng{sc.seed * 0x1234567ull};
    ecx::CompiledMap cm;
    std::printf("S %s\n", sc.name);
    std::vector<Key> keys(sc.keys);
    for (int k = 0; k < sc.keys; ++k) {
        const int64_t pitch = 1000 + (sc.share_pitch ? k / 2 : k);
        keys[k] = {pitch, 48 * pitch, 4096, 8 * 4096, 12, 28 + k % 3, k % 2, 0};
        if (sc.share_pitch) keys[k][5] = 28 + k % 2;
        std::printf("K %d", k);
        for (int64_t v : keys[k]) std::printf(" %lld", (long long)v);
        std::printf("\n");
    }
    // per key and phase (0 exploring, 1 after the choice): each candidate's time
    std::vector<std::array<std::vector<float>, 2>> base(sc.keys);
    for (auto &b : base)
        for (int phase = 0; phase < 2; ++phase) {
            b[phase].assign(ecx::kLayoutNCand, 1.f);
            for (int c = 1; c < ecx::kLayoutNCand; ++c)
                b[phase][c] = 1.f + (phase ? sc.late_bias : sc.static_bias) + sc.spread * (2.f * rng.unit() - 1.f);
        }
    std::vector<Flight> reserved, flying;
    std::vector<int> picked;  // the distinct keys picked so far, in order
    auto fill = [&](Flight f, int now) {
        f.e0 = new FakeEvent;
        f.e1 = new FakeEvent;
        cm.fill_layout_probe(keys[f.key], f.ticket, f.e0, f.e1);
        std::printf("F %d %llu", f.key, (unsigned long long)f.ticket);
        print_readout(cm, keys[f.key][0]);
        f.due = now + rng.below(sc.max_delay + 1);
        flying.push_back(f);
    };
    auto cancel = [&](int key, uint64_t ticket) {
        cm.cancel_layout_probe(keys[key], ticket);
        std::printf("X %d %llu", key, (unsigned long long)ticket);
        print_readout(cm, keys[key][0]);
    };
    auto complete = [&](const Flight &f) {
        const bool phase = cm.layout_choice(keys[f.key][0]) >= 0;
        const float ms = base[f.key][phase][f.cand] * (1.f + 0.01f * (2.f * rng.unit() - 1.f));
        const char kind = rng.chance(sc.p_fail) ? 'f' : rng.chance(sc.p_dirty) ? 'd' : 'c';
        f.e1->ready = true;
        f.e1->ok = kind != 'f';
        f.e1->ms = ms;
        if (kind == 'd')
            for (auto &p : cm.layout_sel_[keys[f.key]].pending)
                if (p.ticket == f.ticket) p.dirty->store(true);
        std::printf("D %d %llu %c %a", f.key, (unsigned long long)f.ticket, kind, (double)ms);
        print_readout(cm, keys[f.key][0]);
    };
    for (int now = 0; now < sc.picks; ++now) {
        for (size_t i = 0; i < reserved.size();)  // late fills and cancels: other picks ran in between
            if (reserved[i].due <= now) {
                const Flight f = reserved[i];
                reserved.erase(reserved.begin() + i);
                if (rng.chance(0.5f)) cancel(f.key, f.ticket);
                else fill(f, now);
            } else {
                ++i;
            }
        for (size_t i = 0; i < flying.size();)
            if (flying[i].due <= now) {
                complete(flying[i]);
                flying.erase(flying.begin() + i);
            } else {
                ++i;
            }
        const int k = rng.below(sc.keys);
        // a ticket nobody holds, on a layout that has an entry (the recorded cancel would create one)
        if (now % 97 == 96) cancel(picked[rng.below((int)std::min<size_t>(picked.size(), 64))], 1000000000ull + now);
        if (std::find(picked.begin(), picked.end(), k) == picked.end()) picked.push_back(k);
        uint64_t ticket = 0;
        const int cand = cm.next_layout_pick(keys[k], ecx::kLayoutNCand, ecx::kLayoutSamples, 0, nullptr, &ticket);
        std::printf("P %d %d %llu", k, cand, (unsigned long long)ticket);
        print_readout(cm, keys[k][0]);
        if (!ticket) continue;
        Flight f{k, ticket, cand};
        if (rng.chance(sc.p_late_fill)) {
            f.due = now + 1 + rng.below(4);
            reserved.push_back(f);
        } else if (rng.chance(sc.p_cancel)) {
            cancel(k, ticket);
        } else {
            fill(f, now);
        }
    }
    // the class above has no destructor: complete what still flies and pick once more per key, so
    // that every event is read and freed
    for (const Flight &f : reserved) cancel(f.key, f.ticket);
    for (const Flight &f : flying) complete(f);
    for (int k = 0; k < sc.keys; ++k) {
        uint64_t ticket = 0;
        const int cand = cm.next_layout_pick(keys[k], ecx::kLayoutNCand, ecx::kLayoutSamples, 0, nullptr, &ticket);
        std::printf("P %d %d %llu", k, cand, (unsigned long long)ticket);
        print_readout(cm, keys[k][0]);
        if (ticket) cancel(k, ticket);
    }
}
}  // namespace

int main() {
    for (const Scenario &sc : kScenarios) run(sc);
    return 0;
}
