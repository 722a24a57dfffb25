// pattern_set.cpp -- a pattern set's host plans and their per-device upload (pattern_set.hpp).
#include "pattern_set.hpp"

#include <algorithm>
#include <set>

namespace ecx {

PatternSet::PatternSet(const std::vector<const CompiledMap *> &maps) : maps_(maps) {
    // each map's unpadded entries and tile records: its plan padded to a multiple of 1
    std::vector<HostPlan> plans;
    plans.reserve(maps.size());
    std::vector<MixedPatternIn> in;
    std::vector<TiledPatternIn> tin;
    bool single = true;
    for (const CompiledMap *m : maps) {
        if (m->n_tiles() > kMixedMaxTiles)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern of a pattern set has more than " +
                                                    std::to_string(kMixedMaxTiles * kTileRows) + " rows");
        single &= m->n_tiles() <= 1;
        plans.push_back(m->padded_plan(1));
        in.push_back(MixedPatternIn{plans.back().entries.data(), plans.back().tiles.data()});
        // (a map without rows still has one record, of zeros)
        tin.push_back(TiledPatternIn{plans.back().entries.data(), plans.back().tiles.data(), std::max(1, m->n_tiles())});
    }
    const bool built = build_tiled_plan(tin.data(), (int)tin.size(), 4, &tiled4_) &&
                       build_tiled_plan(tin.data(), (int)tin.size(), 8, &tiled8_) &&
                       (!single || (build_mixed_plan(in.data(), (int)in.size(), 4, &plan4_) &&
                                    build_mixed_plan(in.data(), (int)in.size(), 8, &plan8_)));
    if (!built)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern set holds 1.." + std::to_string(kMixedRecords) + " patterns");
    if (single) preferred_depth_ = mixed_depth(in.data(), (int)in.size());
    tiled_depth_ = tiled_depth(tin.data(), (int)tin.size());
    // the slots a host batch moves.  In place (pattern_set.hpp up_slots): every record's output
    // slots down; those and every slot an entry loads up.  Out of place: the loaded slots up,
    // every output slot up to the largest down.
    std::set<int> ins, down;
    const int T = tiled4_.tiles_per_pattern;
    for (int p = 0; p < tiled4_.npatterns * T; ++p) {
        const uint32_t *tile = tiled4_.tiles.data() + (size_t)p * kTileDwords;
        for (uint32_t r = 0; r < tile[2]; ++r) down.insert((int)tile[4 + r]);
        for (uint32_t e = 0; e < tile[1]; ++e) {
            const uint32_t slot = tiled4_.entries[((size_t)tile[0] + e) * kEntryDwords];
            if (tile[2] != 0 && slot != kDummySlot) ins.insert((int)slot);
        }
    }
    in_slots_.assign(ins.begin(), ins.end());
    for (int s = 0; s <= tiled4_.max_out_slot; ++s) out_slots_.push_back(s);
    std::set<int> up = ins;
    up.insert(down.begin(), down.end());
    up_slots_.assign(up.begin(), up.end());
    down_slots_.assign(down.begin(), down.end());
}

PatternSet::~PatternSet() {
    for (auto &kv : dev_) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) continue;
        (void)hipSetDevice(kv.first.first);
        (void)hipFree(kv.second.entries);
        (void)hipFree(kv.second.tiles);
        (void)hipSetDevice(cur);
    }
    for (auto &kv : tiled_dev_) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) continue;
        (void)hipSetDevice(kv.first.first);
        (void)hipFree(kv.second.entries);
        (void)hipFree(kv.second.tiles);
        (void)hipSetDevice(cur);
    }
    for (auto &kv : clay_partial_dev_) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) continue;
        (void)hipSetDevice(kv.first.first);
        (void)hipFree(kv.second.entries);
        (void)hipFree(kv.second.tiles);
        (void)hipSetDevice(cur);
    }
    for (auto &kv : partial_dev_) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) continue;
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second.entries);
        (void)hipFree(kv.second.rows);
        (void)hipSetDevice(cur);
    }
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

const PartialDevicePlan &PatternSet::partial_plan_for_current_device(int n) {
    const PartialPlan &hp = partial_plan(n);
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(mu_);
    auto it = partial_dev_.find(dev);
    if (it != partial_dev_.end()) return it->second;
    refuse_if_capturing("the pattern set's partial-sum plan");
    PartialDevicePlan p;
    auto upload = [](uint32_t **dst, const std::vector<uint32_t> &src, const char *what) {
        check_hip(hipMalloc(dst, src.size() * 4), what);
        check_hip(hipMemcpy(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice), "partial plan upload");
    };
    try {
        upload(&p.entries, hp.entries, "hipMalloc(partial plan entries)");
        upload(&p.rows, hp.rows, "hipMalloc(partial plan rows)");
    } catch (...) {  // a half-uploaded plan is never published
        (void)hipFree(p.entries);
        (void)hipFree(p.rows);
        throw;
    }
    return partial_dev_.emplace(dev, p).first->second;
}

const ClayPartialPlan &PatternSet::clay_partial_plan(int n, int depth) {
    std::lock_guard<std::mutex> lk(mu_);
    if (clay_partial4_.npatterns == 0) {
        ClayPartialPlan p4, p8;  // both or neither
        if (!build_clay_partial_plan(tiled4_, n, 4, &p4) || !build_clay_partial_plan(tiled4_, n, 8, &p8))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern set's Clay partial plan takes a code of 1..255 nodes");
        clay_partial4_ = std::move(p4);
        clay_partial8_ = std::move(p8);
    }
    if (clay_partial4_.n != n) throw Error(ECX_E_ILLEGAL_ARGUMENT, "the pattern set's partial plan is of another code");
    return depth == 8 ? clay_partial8_ : clay_partial4_;
}

const MixedDevicePlan &PatternSet::clay_partial_plan_for_current_device(int n, int depth) {
    const ClayPartialPlan &hp = clay_partial_plan(n, depth);
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(mu_);
    auto it = clay_partial_dev_.find({dev, hp.depth});
    if (it != clay_partial_dev_.end()) return it->second;
    refuse_if_capturing("the pattern set's Clay partial-sum plan");
    MixedDevicePlan p;
    auto upload = [](uint32_t **dst, const std::vector<uint32_t> &src, const char *what) {
        check_hip(hipMalloc(dst, src.size() * 4), what);
        check_hip(hipMemcpy(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice), "Clay partial plan upload");
    };
    try {
        upload(&p.entries, hp.entries, "hipMalloc(Clay partial plan entries)");
        upload(&p.tiles, hp.tiles, "hipMalloc(Clay partial plan tiles)");
    } catch (...) {  // a half-uploaded plan is never published
        (void)hipFree(p.entries);
        (void)hipFree(p.tiles);
        throw;
    }
    return clay_partial_dev_.emplace(std::make_pair(dev, hp.depth), p).first->second;
}

const MixedDevicePlan &PatternSet::plan_for_current_device(int depth) {
    depth = depth == 8 ? 8 : 4;
    const MixedPlan &hp = plan(depth);
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(mu_);
    auto it = dev_.find({dev, depth});
    if (it != dev_.end()) return it->second;
    refuse_if_capturing("the pattern set's device plan");
    MixedDevicePlan p;
    auto upload = [](uint32_t **dst, const std::vector<uint32_t> &src, const char *what) {
        check_hip(hipMalloc(dst, src.size() * 4), what);
        check_hip(hipMemcpy(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice), "pattern set upload");
    };
    try {
        upload(&p.entries, hp.entries, "hipMalloc(pattern set entries)");
        upload(&p.tiles, hp.tiles, "hipMalloc(pattern set tiles)");
    } catch (...) {  // a half-uploaded plan is never published
        (void)hipFree(p.entries);
        (void)hipFree(p.tiles);
        throw;
    }
    return dev_.emplace(std::make_pair(dev, depth), p).first->second;
}

const MixedDevicePlan &PatternSet::tiled_plan_for_current_device(int depth) {
    const TiledPlan &hp = tiled_plan(depth);
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(mu_);
    auto it = tiled_dev_.find({dev, hp.depth});
    if (it != tiled_dev_.end()) return it->second;
    refuse_if_capturing("the pattern set's tiled device plan");
    MixedDevicePlan p;
    auto upload = [](uint32_t **dst, const std::vector<uint32_t> &src, const char *what) {
        check_hip(hipMalloc(dst, src.size() * 4), what);
        check_hip(hipMemcpy(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice), "pattern set upload");
    };
    try {
        upload(&p.entries, hp.entries, "hipMalloc(pattern set entries)");
        upload(&p.tiles, hp.tiles, "hipMalloc(pattern set tiles)");
    } catch (...) {  // a half-uploaded plan is never published
        (void)hipFree(p.entries);
        (void)hipFree(p.tiles);
        throw;
    }
    return tiled_dev_.emplace(std::make_pair(dev, hp.depth), p).first->second;
}

}  // namespace ecx
