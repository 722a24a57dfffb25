// layout_select_check.cpp -- the per-layout launch-shape decisions (csrc/layout_select.cpp) on the
// CPU.  Host-only: built from layout_select.cpp alone under ASan + UBSan by tests/test_native.py.
//
// 1. Invariants.  Seeded random scripts of pick, report (clean, contaminated, failed) and cancel over
//    several keys, n_cand = kLayoutNCand, samples = kLayoutSamples.  After every operation:
//      * a ticket is never handed out twice, and never with a candidate index >= n_cand;
//      * the tickets a layout holds pending are exactly those handed out and not yet reported or
//        cancelled, and the in-flight probes plus recorded times of a candidate never exceed
//        `samples` while exploring, nor, while re-validating, for the two shapes compared;
//      * an untimed pick returns candidate 0 while exploring and the kept choice afterwards; a timed
//        one while re-validating runs the kept shape or its alternative;
//      * `dropped` never decreases, and a pick that finds kLayoutMaxDropped of them while exploring or
//        re-validating yields state 4 with choice 0;
//      * a non-static choice is made only when its median is below kLayoutMargin x the static
//        median, and is then the fastest median; the static rules are chosen only when no other
//        median is;
//      * a re-validation replaces the kept shape only by the stated rule: a non-static kept shape
//        must still beat the static rules by the margin, a static one yields only to a runner-up
//        that beats it by the margin;
//      * states 3 and 4 never issue a ticket again and never change state or choice;
//      * the 65th distinct key gets candidate 0 untimed and never appears in the read-out;
//      * cancel and report of an unknown ticket change nothing.
// 2. Replay (argv[1]: tests/golden/layout_trace.txt, unpacked).  The rules above do not say that the
//    tie-breaks and the order of the tests in a pick are those of the code the table was split out
//    of.  scripts/record_layout_trace.py recorded that code's decisions over a fixed set of scripts,
//    one line per operation (format: scripts/layout_trace_driver.cpp); the same operations are run
//    here -- finished probes of a key are reported in launch order just before its next pick, as
//    layout_probe.cpp does -- and every line must come out identical.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../repair-pipelining_amd/csrc/launch_rules.hpp"  // kLayoutNCand
#include "../../repair-pipelining_amd/csrc/layout_select.hpp"

using namespace ecx;

namespace {
uint64_t g_rng = 0;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33) % n;
}
float unit() { return (float)rnd(1 << 24) / (float)(1 << 24); }

long g_ops = 0;
int g_seed = 0;
#define REQUIRE(cond, ...)                                                                   \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::printf("layout_select_check: FAILED (seed %d, op %ld): %s\n  ", g_seed, g_ops, #cond); \
            std::printf(__VA_ARGS__);                                                        \
            std::printf("\n");                                                               \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

float median_of(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? -1.f : v[v.size() / 2];
}

bool same(const LayoutTable::Layout &a, const LayoutTable::Layout &b) {
    if (a.pending.size() != b.pending.size()) return false;
    for (size_t i = 0; i < a.pending.size(); ++i)
        if (a.pending[i].cand != b.pending[i].cand || a.pending[i].ticket != b.pending[i].ticket) return false;
    return a.ms == b.ms && a.chosen == b.chosen && a.state == b.state && a.dropped == b.dropped &&
           a.steady == b.steady && a.reval_alt == b.reval_alt && a.reval_ms[0] == b.reval_ms[0] &&
           a.reval_ms[1] == b.reval_ms[1] && a.serial == b.serial;
}

LayoutKey key_of(int k) { return {1000 + k, 48000 + k, 4096, 32768, 12, 28, k % 2, 0}; }

// What must hold of layout k after any operation, given the tickets the script still holds.
void check_layout(const LayoutTable &t, int k, const std::map<uint64_t, std::pair<int, int>> &held) {
    const LayoutTable::Layout *s = t.layout(key_of(k));
    REQUIRE(s, "key %d has no layout", k);
    std::vector<int> flying(kLayoutNCand, 0);
    size_t mine = 0;
    for (const auto &h : held)
        if (h.second.first == k) {
            ++mine;
            ++flying[h.second.second];
            const bool pending = std::any_of(s->pending.begin(), s->pending.end(), [&](const LayoutTable::Layout::Pending &p) {
                return p.ticket == h.first && p.cand == h.second.second;
            });
            REQUIRE(pending, "key %d: held ticket %" PRIu64 " is not pending", k, h.first);
        }
    REQUIRE(mine == s->pending.size(), "key %d: %zu pending, %zu held", k, s->pending.size(), mine);
    REQUIRE((int)s->ms.size() == kLayoutNCand, "key %d: %zu candidates", k, s->ms.size());
    if (s->state == kLayoutExploring) {
        REQUIRE(s->chosen == -1, "key %d explores with choice %d", k, s->chosen);
        for (int c = 0; c < kLayoutNCand; ++c)
            REQUIRE(flying[c] + (int)s->ms[c].size() <= kLayoutSamples, "key %d cand %d: %d in flight + %zu timed", k, c,
                    flying[c], s->ms[c].size());
    } else {
        REQUIRE(s->chosen >= 0 && s->chosen < kLayoutNCand, "key %d state %d choice %d", k, s->state, s->chosen);
    }
    if (s->state == kLayoutRevalidating) {
        REQUIRE(s->reval_alt != s->chosen, "key %d re-validates %d against itself", k, s->chosen);
        REQUIRE(flying[s->reval_alt] + (int)s->reval_ms[0].size() <= kLayoutSamples, "key %d alternative %d: %d + %zu", k,
                s->reval_alt, flying[s->reval_alt], s->reval_ms[0].size());
        REQUIRE(flying[s->chosen] + (int)s->reval_ms[1].size() <= kLayoutSamples, "key %d kept %d: %d + %zu", k, s->chosen,
                flying[s->chosen], s->reval_ms[1].size());
    }
    // the read-out agrees (pitches are unique here)
    std::vector<float> ms;
    int state = -1, dropped = -1;
    const int c = t.choice(key_of(k)[0], &ms, &state, &dropped);
    REQUIRE(c == s->chosen, "key %d: read-out choice %d, layout %d", k, c, s->chosen);
    if (c >= 0) {
        REQUIRE(state == s->state && dropped == s->dropped && (int)ms.size() == kLayoutNCand, "key %d read-out", k);
        for (int i = 0; i < kLayoutNCand; ++i) REQUIRE(ms[i] == median_of(s->ms[i]), "key %d median %d", k, i);
    }
}

void run_script(int seed) {
    g_seed = seed;
    g_rng = 0x9E3779B97F4A7C15ull * (uint64_t)(seed + 1);
    g_ops = 0;
    LayoutTable t;
    const bool many = seed % 8 == 7;  // more keys than the table takes
    const int n_keys = many ? (int)kMaxLayouts + 6 : 1 + seed % 4;
    const int steps = many ? 12000 : 900 * n_keys;
    const float p_dirty = seed % 4 == 1 ? 0.5f : seed % 4 == 2 ? 0.04f : 0.f;
    const float spread = 0.01f + 0.01f * (float)(seed % 5);
    // per key, phase (before / after the choice) and candidate: the time, around the static rules' 1.0
    std::vector<std::vector<float>> base(n_keys * 2, std::vector<float>(kLayoutNCand, 1.f));
    for (auto &b : base)
        for (int c = 1; c < kLayoutNCand; ++c) b[c] = 1.f + (seed % 3 == 0 ? 0.02f : 0.f) + spread * (2.f * unit() - 1.f);
    std::map<uint64_t, std::pair<int, int>> held;  // ticket -> (key, cand)
    std::set<uint64_t> issued;
    std::vector<int> admitted;  // the distinct keys picked, in order: the first kMaxLayouts get a layout
    for (; g_ops < steps; ++g_ops) {
        const int k = (int)rnd(n_keys);
        const LayoutKey key = key_of(k);
        const uint32_t what = rnd(100);
        if (what < 55 || held.empty()) {  // pick
            if (std::find(admitted.begin(), admitted.end(), k) == admitted.end()) admitted.push_back(k);
            const bool past = (size_t)(std::find(admitted.begin(), admitted.end(), k) - admitted.begin()) >= kMaxLayouts;
            LayoutTable::Layout before;
            if (t.layout(key)) before = *t.layout(key);
            const LayoutTable::Pick p = t.pick(key, kLayoutNCand, kLayoutSamples);
            if (past) {
                REQUIRE(p.cand == 0 && p.ticket == 0, "key %d past the limit got %d / %" PRIu64, k, p.cand, p.ticket);
                REQUIRE(!t.layout(key) && t.choice(key[0]) == -1, "key %d past the limit has a layout", k);
                continue;
            }
            const LayoutTable::Layout &s = *t.layout(key);
            if (p.ticket) {
                REQUIRE(issued.insert(p.ticket).second, "ticket %" PRIu64 " handed out twice", p.ticket);
                REQUIRE(p.cand >= 0 && p.cand < kLayoutNCand, "ticket with candidate %d", p.cand);
                REQUIRE(s.state == kLayoutExploring || s.state == kLayoutRevalidating, "ticket in state %d", s.state);
                REQUIRE(s.state == kLayoutExploring || p.cand == s.chosen || p.cand == s.reval_alt,
                        "re-validation times %d (kept %d, alternative %d)", p.cand, s.chosen, s.reval_alt);
                held[p.ticket] = {k, p.cand};
            } else {
                REQUIRE(p.cand == (s.state == kLayoutExploring ? 0 : s.chosen), "untimed pick ran %d in state %d (choice %d)",
                        p.cand, s.state, s.chosen);
            }
            if (before.state == kLayoutRevalidated || before.state == kLayoutContended)
                REQUIRE(!p.ticket && s.state == before.state && s.chosen == before.chosen && s.serial == before.serial,
                        "kept state %d moved: state %d choice %d -> %d", before.state, s.state, before.chosen, s.chosen);
            if (before.dropped >= kLayoutMaxDropped && (before.state == kLayoutExploring || before.state == kLayoutRevalidating))
                REQUIRE(s.state == kLayoutContended && s.chosen == 0 && !p.ticket, "%d dropped in state %d -> state %d choice %d",
                        before.dropped, before.state, s.state, s.chosen);
            if (s.state == kLayoutContended) REQUIRE(s.dropped >= kLayoutMaxDropped && s.chosen == 0, "contended at %d", s.dropped);
            if (before.state == kLayoutChosen && s.state != kLayoutChosen)
                REQUIRE(before.steady + 1 == kLayoutRevalidate && before.chosen != before.reval_alt, "re-validation after %" PRId64,
                        before.steady + 1);
            if (before.state == kLayoutExploring && s.state == kLayoutChosen) {
                std::vector<float> m;
                for (const auto &v : s.ms) {
                    REQUIRE((int)v.size() >= kLayoutSamples, "chosen on %zu timings", v.size());
                    m.push_back(median_of(v));
                }
                for (int c = 1; c < kLayoutNCand; ++c) {
                    if (s.chosen == 0) REQUIRE(!(m[c] < kLayoutMargin * m[0]), "static kept though %d is faster by the margin", c);
                    else REQUIRE(!(m[c] < m[s.chosen]), "chose %d though %d is faster", s.chosen, c);
                }
                if (s.chosen != 0) {
                    REQUIRE(m[s.chosen] < kLayoutMargin * m[0], "chose %d inside the margin", s.chosen);
                    REQUIRE(s.reval_alt == 0, "non-static choice re-validated against %d", s.reval_alt);
                } else {
                    for (int c = 1; c < kLayoutNCand; ++c)
                        REQUIRE(!(m[c] < m[s.reval_alt]), "runner-up %d though %d is faster", s.reval_alt, c);
                }
            }
            if (before.state == kLayoutRevalidating && s.state == kLayoutRevalidated) {
                REQUIRE((int)s.reval_ms[0].size() >= kLayoutSamples && (int)s.reval_ms[1].size() >= kLayoutSamples, "re-validated early");
                const float alt = median_of(s.reval_ms[0]), kept = median_of(s.reval_ms[1]);
                const bool replace = before.chosen != 0 ? !(kept < kLayoutMargin * alt) : alt < kLayoutMargin * kept;
                REQUIRE(s.chosen == (replace ? before.reval_alt : before.chosen), "re-validation of %d against %d (%a, %a) kept %d",
                        before.chosen, before.reval_alt, (double)kept, (double)alt, s.chosen);
            }
            REQUIRE(s.dropped == before.dropped, "a pick changed dropped");
        } else if (what < 97) {  // report or cancel a held ticket
            auto it = held.begin();
            std::advance(it, rnd((uint32_t)held.size()));
            const uint64_t ticket = it->first;
            const int hk = it->second.first, cand = it->second.second;
            held.erase(it);
            const LayoutTable::Layout before = *t.layout(key_of(hk));
            const uint32_t r = rnd(100);
            const float ms = base[2 * hk + (before.chosen >= 0)][cand] * (1.f + 0.01f * (2.f * unit() - 1.f));
            const bool dirty = unit() < p_dirty;
            if (r < 4) t.cancel(key_of(hk), ticket);
            else t.report(key_of(hk), ticket, {r < 8 ? ProbeOutcome::kFailed : dirty ? ProbeOutcome::kContaminated : ProbeOutcome::kClean, ms});
            const LayoutTable::Layout &s = *t.layout(key_of(hk));
            REQUIRE(s.state == before.state && s.chosen == before.chosen, "a report changed state or choice");
            REQUIRE(s.dropped == before.dropped + (r >= 8 && dirty), "dropped %d -> %d", before.dropped, s.dropped);
            check_layout(t, hk, held);
            continue;
        } else {  // a ticket nobody holds, or a key nobody picked
            const uint64_t ticket = 1000000000ull + rnd(1000);
            const bool known = t.layout(key);
            LayoutTable::Layout before;
            if (known) before = *t.layout(key);
            if (rnd(2)) t.cancel(key, ticket);
            else t.report(key, ticket, {rnd(2) ? ProbeOutcome::kClean : ProbeOutcome::kContaminated, 1.f});
            REQUIRE(known == (t.layout(key) != nullptr), "an unknown ticket made a layout");
            if (known) REQUIRE(same(before, *t.layout(key)), "an unknown ticket changed key %d", k);
            if (!known) continue;
        }
        check_layout(t, k, held);
    }
}

// ---- replay of the recorded trace
std::string readout(const LayoutTable &t, int64_t pitch) {
    std::vector<float> ms;
    int state = 0, dropped = 0;
    const int c = t.choice(pitch, &ms, &state, &dropped);
    if (c < 0) return " | -1";
    char buf[64];
    std::snprintf(buf, sizeof buf, " | %d %d %d", c, state, dropped);
    std::string s = buf;
    for (float m : ms) {
        std::snprintf(buf, sizeof buf, " %a", (double)m);
        s += buf;
    }
    return s;
}

struct Flying {
    uint64_t ticket;
    bool ready;
    ProbeOutcome outcome;
};

long replay(const char *path) {
    std::ifstream f(path);
    if (!f) {
        std::printf("layout_select_check: cannot read %s\n", path);
        std::exit(1);
    }
    LayoutTable t;
    std::map<int, LayoutKey> keys;
    std::map<int, std::vector<Flying>> flying;  // per key, in launch order
    std::string line, name;
    long n = 0, picks = 0;
    while (std::getline(f, line)) {
        ++n;
        char kind = 0, outcome = 0;
        int k = 0;
        unsigned long long ticket = 0;
        std::string got;
        char buf[96];
        if (line[0] == 'S') {
            t = LayoutTable();
            keys.clear();
            flying.clear();
            name = line.substr(2);
            continue;
        }
        if (line[0] == 'K') {
            long long v[8];
            if (std::sscanf(line.c_str(), "K %d %lld %lld %lld %lld %lld %lld %lld %lld", &k, v, v + 1, v + 2, v + 3, v + 4, v + 5,
                            v + 6, v + 7) != 9)
                break;
            for (int i = 0; i < 8; ++i) keys[k][i] = v[i];
            continue;
        }
        if (line[0] == 'P' && std::sscanf(line.c_str(), "P %d", &k) == 1 && keys.count(k)) {
            auto &v = flying[k];
            for (auto it = v.begin(); it != v.end();)
                if (it->ready) {
                    t.report(keys[k], it->ticket, it->outcome);
                    it = v.erase(it);
                } else {
                    ++it;
                }
            const LayoutTable::Pick p = t.pick(keys[k], kLayoutNCand, kLayoutSamples);
            std::snprintf(buf, sizeof buf, "P %d %d %llu", k, p.cand, (unsigned long long)p.ticket);
            ++picks;
        } else if (line[0] == 'F' && std::sscanf(line.c_str(), "F %d %llu", &k, &ticket) == 2 && keys.count(k)) {
            flying[k].push_back({ticket, false, {ProbeOutcome::kFailed, 0.f}});
            std::snprintf(buf, sizeof buf, "F %d %llu", k, ticket);
        } else if (line[0] == 'X' && std::sscanf(line.c_str(), "X %d %llu", &k, &ticket) == 2 && keys.count(k)) {
            t.cancel(keys[k], ticket);
            std::snprintf(buf, sizeof buf, "X %d %llu", k, ticket);
        } else if (line[0] == 'D' && std::sscanf(line.c_str(), "%c %d %llu %c", &kind, &k, &ticket, &outcome) == 4 && keys.count(k)) {
            const size_t bar = line.find(" | "), sp = line.rfind(' ', bar - 1);
            const float ms = std::strtof(line.c_str() + sp + 1, nullptr);
            for (auto &p : flying[k])
                if (p.ticket == ticket) {
                    p.ready = true;
                    p.outcome = {outcome == 'f' ? ProbeOutcome::kFailed : outcome == 'd' ? ProbeOutcome::kContaminated : ProbeOutcome::kClean, ms};
                }
            std::snprintf(buf, sizeof buf, "D %d %llu %c %a", k, ticket, outcome, (double)ms);
        } else {
            break;  // not a line of the format
        }
        got = buf + readout(t, keys[k][0]);
        if (got != line) {
            std::printf("layout_select_check: FAILED: replay of %s differs at line %ld (script %s)\n  recorded: %s\n  now:      %s\n",
                        path, n, name.c_str(), line.c_str(), got.c_str());
            std::exit(1);
        }
    }
    if (!f.eof() || picks == 0) {
        std::printf("layout_select_check: FAILED: %s line %ld is not a trace line: %s\n", path, n, line.c_str());
        std::exit(1);
    }
    return n;
}
}  // namespace

int main(int argc, char **argv) {
    long ops = 0;
    for (int seed = 0; seed < 96; ++seed) {
        run_script(seed);
        ops += g_ops;
    }
    long lines = 0;
    if (argc > 1) lines = replay(argv[1]);
    std::printf("layout_select_check: ok (%ld operations, %ld trace lines replayed)\n", ops, lines);
    return 0;
}
