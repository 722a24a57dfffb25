// pattern_set.cpp -- a pattern set's host plans and their per-device upload (pattern_set.hpp).
#include "pattern_set.hpp"

#include <algorithm>
#include <set>

namespace ecx {

PatternSet::PatternSet(const std::vector<const CompiledMap *> &maps) : maps_(maps) {
    // each map's unpadded entries and tile records: its plan padded to a multiple of 1
    std::vector<HostPlan> plans;
    plans.reserve(maps.size());
    std::vector<TiledPatternIn> in;
    for (const CompiledMap *m : maps) {
        if (m->n_tiles() > kMixedMaxTiles)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern of a pattern set has more than " +
                                                    std::to_string(kMixedMaxTiles * kTileRows) + " rows");
        plans.push_back(m->padded_plan(1));
        // (a map without rows still has one record, of zeros)
        in.push_back(TiledPatternIn{plans.back().entries.data(), plans.back().tiles.data(), std::max(1, m->n_tiles())});
    }
    if (!build_tiled_plan(in.data(), (int)in.size(), 4, &plan4_) || !build_tiled_plan(in.data(), (int)in.size(), 8, &plan8_))
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern set holds 1.." + std::to_string(kMixedRecords) + " patterns");
    depth_ = tiled_depth(in.data(), (int)in.size());
    // the slots a host batch moves.  In place (pattern_set.hpp up_slots): every record's output
    // slots down; those and every slot an entry loads up.  Out of place: the loaded slots up,
    // every output slot up to the largest down.
    std::set<int> ins, down;
    const int T = plan4_.tiles_per_pattern;
    for (int p = 0; p < plan4_.npatterns * T; ++p) {
        const uint32_t *tile = plan4_.tiles.data() + (size_t)p * kTileDwords;
        for (uint32_t r = 0; r < tile[2]; ++r) down.insert((int)tile[4 + r]);
        for (uint32_t e = 0; e < tile[1]; ++e) {
            const uint32_t slot = plan4_.entries[((size_t)tile[0] + e) * kEntryDwords];
            if (tile[2] != 0 && slot != kDummySlot) ins.insert((int)slot);
        }
    }
    in_slots_.assign(ins.begin(), ins.end());
    for (int s = 0; s <= plan4_.max_out_slot; ++s) out_slots_.push_back(s);
    std::set<int> up = ins;
    up.insert(down.begin(), down.end());
    up_slots_.assign(up.begin(), up.end());
    down_slots_.assign(down.begin(), down.end());
}

PatternSet::~PatternSet() {
    for (auto &kv : dev_) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) continue;
        (void)hipSetDevice(std::get<1>(kv.first));
        (void)hipFree(kv.second.entries);
        (void)hipFree(kv.second.records);
        (void)hipSetDevice(cur);
    }
}

const PatternDevicePlan &PatternSet::resident(PlanKind kind, int depth, const std::vector<uint32_t> &entries,
                                              const std::vector<uint32_t> &records, const char *what) {
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(mu_);
    const auto key = std::make_tuple((int)kind, dev, depth);
    auto it = dev_.find(key);
    if (it != dev_.end()) return it->second;
    refuse_if_capturing(what);
    PatternDevicePlan p;
    auto upload = [what](uint32_t **dst, const std::vector<uint32_t> &src) {
        check_hip(hipMalloc(dst, src.size() * 4), what);
        check_hip(hipMemcpy(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice), what);
    };
    try {
        upload(&p.entries, entries);
        upload(&p.records, records);
    } catch (...) {  // a half-uploaded plan is never published
        (void)hipFree(p.entries);
        (void)hipFree(p.records);
        throw;
    }
    return dev_.emplace(key, p).first->second;
}

const PatternDevicePlan &PatternSet::plan_for_current_device(int depth, const char *what) {
    const TiledPlan &hp = plan(depth);
    return resident(kPlan, hp.depth, hp.entries, hp.tiles, what);
}

const PartialPlan &PatternSet::partial_plan(int n) {
    std::lock_guard<std::mutex> lk(mu_);
    if (partial_.npatterns != 0) {
        if (partial_.n != n) throw Error(ECX_E_ILLEGAL_ARGUMENT, "the pattern set's partial plan is of another code");
        return partial_;
    }
    std::vector<PartialPatternIn> in;
    for (const CompiledMap *m : maps_) {
        const LinearMap &lm = m->map();
        in.push_back(PartialPatternIn{lm.n_out, lm.n_in, lm.a.data(), lm.in_slot.data()});
    }
    if (!build_partial_plan(in.data(), (int)in.size(), n, &partial_))
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern set's partial plan takes patterns of at most " +
                                                std::to_string(kPartialRows) + " missing shards");
    return partial_;
}

const PatternDevicePlan &PatternSet::partial_plan_for_current_device(int n) {
    const PartialPlan &hp = partial_plan(n);
    return resident(kPartial, 0, hp.entries, hp.rows, "the pattern set's partial-sum plan");
}

const ClayPartialPlan &PatternSet::clay_partial_plan(int n, int depth) {
    std::lock_guard<std::mutex> lk(mu_);
    if (clay_partial4_.npatterns == 0) {
        ClayPartialPlan p4, p8;  // both or neither
        if (!build_clay_partial_plan(plan4_, n, 4, &p4) || !build_clay_partial_plan(plan4_, n, 8, &p8))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern set's Clay partial plan takes a code of 1..255 nodes");
        clay_partial4_ = std::move(p4);
        clay_partial8_ = std::move(p8);
    }
    if (clay_partial4_.n != n) throw Error(ECX_E_ILLEGAL_ARGUMENT, "the pattern set's partial plan is of another code");
    return depth == 8 ? clay_partial8_ : clay_partial4_;
}

const PatternDevicePlan &PatternSet::clay_partial_plan_for_current_device(int n, int depth) {
    const ClayPartialPlan &hp = clay_partial_plan(n, depth);
    return resident(kClayPartial, hp.depth, hp.entries, hp.tiles, "the pattern set's Clay partial-sum plan");
}

}  // namespace ecx
