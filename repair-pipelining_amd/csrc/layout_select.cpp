// layout_select.cpp -- the per-layout launch-shape decisions (layout_select.hpp).
#include "layout_select.hpp"

#include <algorithm>

namespace ecx {

namespace {
float median_of(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? -1.f : v[v.size() / 2];
}
}  // namespace

LayoutTable::Pick LayoutTable::pick(const LayoutKey &key, int n_cand, int samples) {
    const bool fresh = !layouts_.count(key);
    if (fresh && layouts_.size() >= kMaxLayouts) return {0, 0};  // bounded: the static rules
    Layout &s = layouts_[key];
    if ((int)s.ms.size() != n_cand) s.ms.assign(n_cand, {});
    auto reserve = [&](int cand) {
        s.pending.push_back({cand, ++ticket_serial_});
        return Pick{cand, ticket_serial_};
    };
    auto in_flight = [&](int cand) {
        int n = 0;
        for (const auto &p : s.pending) n += p.cand == cand;
        return n;
    };
    if (s.state == kLayoutContended || s.state == kLayoutRevalidated) return {s.chosen, 0};
    if (s.state == kLayoutChosen) {
        if (s.chosen == s.reval_alt || ++s.steady < kLayoutRevalidate) return {s.chosen, 0};
        s.state = kLayoutRevalidating;  // once: the kept shape against its alternative, clean timings
    }
    if (s.dropped >= kLayoutMaxDropped) {
        // another stream keeps the device busy while probes run: no timing here is trustworthy
        s.chosen = 0;
        s.state = kLayoutContended;
        s.serial = ++choice_serial_;
        return {0, 0};
    }
    if (s.state == kLayoutRevalidating) {
        const int have[2] = {(int)s.reval_ms[0].size() + in_flight(s.reval_alt),
                             (int)s.reval_ms[1].size() + in_flight(s.chosen)};
        if ((int)s.reval_ms[0].size() >= samples && (int)s.reval_ms[1].size() >= samples) {
            const float alt = median_of(s.reval_ms[0]), kept = median_of(s.reval_ms[1]);
            // a shape other than the static rules (candidate 0) must keep beating them by the margin;
            // a kept static choice is replaced only by a runner-up that beats it by the margin
            const bool keep = s.reval_alt == 0 ? kept < kLayoutMargin * alt : !(alt < kLayoutMargin * kept);
            if (!keep) s.chosen = s.reval_alt;
            s.state = kLayoutRevalidated;
            s.serial = ++choice_serial_;
            return {s.chosen, 0};
        }
        if (have[0] >= samples && have[1] >= samples) return {s.chosen, 0};  // all in flight: untimed
        return reserve(have[0] <= have[1] ? s.reval_alt : s.chosen);
    }
    // exploring
    std::vector<int> queued(n_cand, 0);
    bool done = true;
    for (int c = 0; c < n_cand; ++c) {
        queued[c] = (int)s.ms[c].size();
        done = done && queued[c] >= samples;
    }
    if (done) {
        const float base = median_of(s.ms[0]);
        int best = 0, second = -1;
        float best_ms = base;
        for (int c = 1; c < n_cand; ++c) {
            const float m = median_of(s.ms[c]);
            if (m < best_ms && m < kLayoutMargin * base) {
                best = c;
                best_ms = m;
            }
        }
        for (int c = 0; c < n_cand; ++c)  // the runner-up: what a kept static choice is re-checked against
            if (c != best && (second < 0 || median_of(s.ms[c]) < median_of(s.ms[second]))) second = c;
        s.chosen = best;
        s.reval_alt = best != 0 ? 0 : (second >= 0 ? second : 0);
        s.state = kLayoutChosen;
        s.steady = 0;
        s.serial = ++choice_serial_;
        return {best, 0};
    }
    for (const auto &p : s.pending) ++queued[p.cand];
    int c = 0;
    for (int k = 1; k < n_cand; ++k)
        if (queued[k] < queued[c]) c = k;
    if (queued[c] >= samples) return {0, 0};  // every probe is in flight: the static rules, untimed
    return reserve(c);
}

void LayoutTable::report(const LayoutKey &key, uint64_t ticket, ProbeOutcome outcome) {
    auto kt = layouts_.find(key);
    if (kt == layouts_.end()) return;
    Layout &s = kt->second;
    auto it = std::find_if(s.pending.begin(), s.pending.end(), [&](const Layout::Pending &p) { return p.ticket == ticket; });
    if (it == s.pending.end()) return;
    const int cand = it->cand;
    s.pending.erase(it);
    if (outcome.kind == ProbeOutcome::kFailed) return;  // its candidate is timed again
    if (outcome.kind == ProbeOutcome::kContaminated) ++s.dropped;
    else if (s.state == kLayoutRevalidating) {
        if (cand == s.reval_alt) s.reval_ms[0].push_back(outcome.ms);
        else if (cand == s.chosen) s.reval_ms[1].push_back(outcome.ms);
    } else if (s.state == kLayoutExploring && cand < (int)s.ms.size()) {
        s.ms[cand].push_back(outcome.ms);
    }
}

void LayoutTable::cancel(const LayoutKey &key, uint64_t ticket) { report(key, ticket, {ProbeOutcome::kFailed, 0.f}); }

int LayoutTable::choice(int64_t pitch, std::vector<float> *ms, int *state, int *dropped) const {
    const Layout *latest = nullptr;
    for (const auto &kv : layouts_)
        if (kv.first[0] == pitch && kv.second.chosen >= 0 && (!latest || kv.second.serial > latest->serial))
            latest = &kv.second;
    if (!latest) return -1;
    if (ms) {
        ms->clear();
        for (const auto &v : latest->ms) ms->push_back(median_of(v));
    }
    if (state) *state = latest->state;
    if (dropped) *dropped = latest->dropped;
    return latest->chosen;
}

const LayoutTable::Layout *LayoutTable::layout(const LayoutKey &key) const {
    auto it = layouts_.find(key);
    return it == layouts_.end() ? nullptr : &it->second;
}

}  // namespace ecx
