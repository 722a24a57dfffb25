// host_plan.cpp -- the plans of the host-memory batches (host_plan.hpp); host_pipe.cpp enqueues them.
#include "host_plan.hpp"

#include <algorithm>

namespace ecx {

std::vector<Run> runs_of(const std::vector<int> &slots, int64_t slot_stride, int64_t nbytes) {
    std::vector<Run> runs;
    for (size_t i = 0; i < slots.size(); ++i) {
        if (!runs.empty() && slot_stride == nbytes && slots[i] == runs.back().slot0 + runs.back().len) {
            ++runs.back().len;
            continue;
        }
        runs.push_back({slots[i], (int)i, 1});
    }
    return runs;
}

std::vector<Segment> progressions_of(const std::vector<Run> &runs) {
    std::vector<Segment> sg;
    for (size_t i = 0; i < runs.size();) {
        size_t j = i;
        int64_t ds = 0, dc = 0;
        if (i + 1 < runs.size() && runs[i + 1].len == runs[i].len) {
            ds = runs[i + 1].slot0 - runs[i].slot0;
            dc = runs[i + 1].compact0 - runs[i].compact0;
            while (j + 1 < runs.size() && runs[j + 1].len == runs[i].len && runs[j + 1].slot0 - runs[j].slot0 == ds &&
                   runs[j + 1].compact0 - runs[j].compact0 == dc)
                ++j;
        }
        sg.push_back({i, j, ds, dc});
        i = j + 1;
    }
    return sg;
}

// The runs of a stripe often repeat with a fixed step: a Clay repair reads the same helper nodes
// of every plane of a plane group (Clay(4,2) {0,3}: nodes 1-2 and 4-5 of all 8 planes, 16 runs;
// shortened Clay(10,4), node 0: nodes 1-13 of planes 0-63, 64 runs), a check on a padded pitch
// reads every shard.  One copy then moves many runs of every stripe of a chunk:
//  * folded 2D: when runs[i + period] is runs[i] moved by fixed host and compact steps for every i
//    and `count` steps span exactly one stripe on both sides, the k-th run of every period of
//    every stripe lies at a fixed pitch -- one strided copy of count x stripes rows per run of
//    the first period (Clay(4,2) {0,3}: 1 copy per chunk instead of 16, e2e 71.6 -> 75.9 GiB/s,
//    profiles/r06_fold_ab.jsonl);
//  * 3D: otherwise each maximal progression of equal runs at fixed steps (that divide the stripe
//    on both sides) is one hipMemcpy3DAsync -- its rows, then the next stripe (Clay(10,4) node 3:
//    3 copies per chunk instead of 65; H2D of node 0's 64 runs 53.2 -> 57.2 GB/s,
//    profiles/r06_copy3d_probe.jsonl; its e2e 56.7 -> 62.5 GiB/s, the headline's 68.0 -> 69.4,
//    profiles/r06_copy3d_ab.jsonl);
//  * any other run: one strided copy of its rows of the chunk's stripes.
std::vector<Copy> plan_copies(const std::vector<Run> &runs, int64_t stripe_stride, int64_t slot_stride, int64_t per,
                              int64_t nbytes) {
    std::vector<Copy> cs;
    const size_t n = runs.size();
    for (size_t p = 1; p < n; ++p) {  // folded 2D
        if (n % p) continue;
        const int64_t ds = runs[p].slot0 - runs[0].slot0, dc = runs[p].compact0 - runs[0].compact0;
        const int64_t count = (int64_t)(n / p);
        if (ds <= 0 || dc <= 0 || count * ds * slot_stride != stripe_stride || count * dc * nbytes != per) continue;
        bool ok = true;
        for (size_t i = 0; ok && i + p < n; ++i)
            ok = runs[i + p].len == runs[i].len && runs[i + p].slot0 - runs[i].slot0 == ds &&
                 runs[i + p].compact0 - runs[i].compact0 == dc;
        if (!ok) continue;
        for (size_t k = 0; k < p; ++k)
            cs.push_back({runs[k].slot0 * slot_stride, runs[k].compact0 * nbytes, runs[k].len * nbytes, count,
                          ds * slot_stride, dc * nbytes, false});
        return cs;
    }
    for (const Segment &g : progressions_of(runs)) {
        const int64_t hp = g.ds * slot_stride, dp = g.dc * nbytes;
        if (g.j > g.i && hp > 0 && dp > 0 && stripe_stride > 0 && stripe_stride % hp == 0 && per % dp == 0) {
            cs.push_back({runs[g.i].slot0 * slot_stride, runs[g.i].compact0 * nbytes, runs[g.i].len * nbytes,
                          (int64_t)(g.j - g.i + 1), hp, dp, true});
        } else {
            for (size_t k = g.i; k <= g.j; ++k)
                cs.push_back({runs[k].slot0 * slot_stride, runs[k].compact0 * nbytes, runs[k].len * nbytes, 1,
                              stripe_stride, per, false});
        }
    }
    return cs;
}

namespace {

// Buffer sets in flight for a ring of `units`: host_buffers within 1..8, no more than the units.
int ring_depth(int host_buffers, int64_t units) {
    return (int)std::min<int64_t>(std::max(1, std::min(host_buffers, 8)), std::max<int64_t>(1, units));
}

}  // namespace

Chunking chunking_of(int64_t up_per, size_t ncopies, int64_t units, int64_t host_chunk, int host_buffers) {
    // Stripes per chunk: host_chunk bytes of input, but at least kMinRows stripes when a chunk still
    // takes more than 8 copies after folding and 3D (Clay(10,4) node 4: 17), so each copy moves rows
    // of many stripes instead of a few KiB -- within 8x host_chunk.  The DMA queue idles ~16 us
    // between copies (the copy trace); with one copy per run, 160 rows beat 64, 96, 256
    // and 512 and equal-size chunks (profiles/r06_minrows_ab*.jsonl); once 3D copies took Clay(10,4)
    // node 3 to 3 copies, dropping the floor for it gained another 4 % (profiles/r06_floor_ab.jsonl).
    constexpr int64_t kMinRows = 160;
    const int64_t up = std::max<int64_t>(1, up_per);
    int64_t chunk = host_chunk / up;
    if (ncopies > 8) chunk = std::max(chunk, std::min(kMinRows, 8 * host_chunk / up));
    chunk = std::max<int64_t>(1, std::min<int64_t>(units, chunk));
    const int64_t nchunks = (units + chunk - 1) / chunk;
    return {chunk, nchunks, ring_depth(host_buffers, nchunks)};
}

Plan make_plan(const std::vector<int> &ins, const std::vector<int> &outs, int64_t in_stripe_stride,
               int64_t in_slot_stride, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
               int64_t nbytes, bool outputs, int64_t host_chunk, int host_buffers) {
    Plan pl;
    pl.in_per = (int64_t)ins.size() * nbytes;
    pl.rin = runs_of(ins, in_slot_stride, nbytes);
    pl.cin = plan_copies(pl.rin, in_stripe_stride, in_slot_stride, pl.in_per, nbytes);
    if (outputs) {
        pl.out_per = (int64_t)outs.size() * nbytes;
        pl.rout = runs_of(outs, out_slot_stride, nbytes);
        pl.cout = plan_copies(pl.rout, out_stripe_stride, out_slot_stride, pl.out_per, nbytes);
    }
    const Chunking ch = chunking_of(pl.in_per, pl.cin.size(), nstripes, host_chunk, host_buffers);
    pl.chunk = ch.chunk;
    pl.nchunks = ch.nchunks;
    pl.nb = ch.nb;
    constexpr int64_t kSliceAlign = 4096;
    if (outputs && pl.nchunks == 1 && nbytes >= 2 * kSliceAlign && nstripes * pl.in_per >= 4 * host_chunk) {
        const int64_t want = (nstripes * pl.in_per + host_chunk - 1) / host_chunk;  // slices of ~host_chunk
        int64_t w = (nbytes + want - 1) / want;
        w = (w + kSliceAlign - 1) / kSliceAlign * kSliceAlign;
        pl.slice = std::min(w, nbytes);
        pl.nslices = (nbytes + pl.slice - 1) / pl.slice;
        pl.sin = progressions_of(pl.rin);
        pl.sout = progressions_of(pl.rout);
        pl.nb = ring_depth(host_buffers, pl.nslices);
    }
    return pl;
}

HostMixedPlan make_mixed_plan(const std::vector<int> &up, const std::vector<int> &down, int64_t stripe_stride,
                              int64_t slot_stride, int n, int64_t units, int64_t nbytes, int64_t host_chunk,
                              int host_buffers) {
    HostMixedPlan mp;
    mp.per = (int64_t)n * nbytes;
    auto copies = [&](const std::vector<int> &slots) {
        std::vector<Run> runs = runs_of(slots, slot_stride, nbytes);
        for (Run &r : runs) r.compact0 = r.slot0;  // not compacted
        return plan_copies(runs, stripe_stride, slot_stride, mp.per, nbytes);
    };
    mp.cin = copies(up);
    mp.cout = copies(down);
    const Chunking ch = chunking_of((int64_t)up.size() * nbytes, mp.cin.size(), units, host_chunk, host_buffers);
    mp.chunk = ch.chunk;
    mp.nchunks = ch.nchunks;
    mp.nb = ch.nb;
    return mp;
}

HostMapMixedPlan make_map_mixed_plan(const std::vector<int> &ins, const std::vector<int> &outs, int64_t in_stripe_stride,
                                     int64_t in_slot_stride, int n_in, int64_t out_stripe_stride,
                                     int64_t out_slot_stride, int n_out, int64_t nstripes, int64_t nbytes,
                                     int64_t host_chunk, int host_buffers) {
    HostMapMixedPlan mp;
    mp.in_per = (int64_t)n_in * nbytes;
    mp.out_per = (int64_t)n_out * nbytes;
    auto copies = [&](const std::vector<int> &slots, int64_t stripe_stride, int64_t slot_stride, int64_t per) {
        std::vector<Run> runs = runs_of(slots, slot_stride, nbytes);
        for (Run &r : runs) r.compact0 = r.slot0;  // not compacted
        return plan_copies(runs, stripe_stride, slot_stride, per, nbytes);
    };
    mp.cin = copies(ins, in_stripe_stride, in_slot_stride, mp.in_per);
    mp.cout = copies(outs, out_stripe_stride, out_slot_stride, mp.out_per);
    const Chunking ch = chunking_of((int64_t)ins.size() * nbytes, mp.cin.size(), nstripes, host_chunk, host_buffers);
    mp.chunk = ch.chunk;
    mp.nchunks = ch.nchunks;
    mp.nb = ch.nb;
    return mp;
}

HostBatchPlan host_batch_plan(const std::vector<int> &ins, const std::vector<int> &outs, int64_t in_stripe_stride,
                              int64_t in_slot_stride, int64_t out_stripe_stride, int64_t out_slot_stride,
                              int64_t nstripes, int64_t nbytes, int64_t host_chunk, int host_buffers) {
    HostBatchPlan hp;
    if (nstripes <= 0 || nbytes <= 0) return hp;
    const Plan pl = make_plan(ins, outs, in_stripe_stride, in_slot_stride, out_stripe_stride, out_slot_stride, nstripes,
                              nbytes, true, host_chunk, host_buffers);
    hp.chunk = pl.chunk;
    hp.nchunks = pl.nchunks;
    hp.buffers = pl.nb;
    hp.h2d_copies = (int64_t)pl.cin.size();
    hp.d2h_copies = (int64_t)pl.cout.size();
    for (const Copy &c : pl.cin) hp.h2d_rows = std::max(hp.h2d_rows, c.rows), hp.h2d_3d += c.three_d;
    for (const Copy &c : pl.cout) hp.d2h_rows = std::max(hp.d2h_rows, c.rows), hp.d2h_3d += c.three_d;
    hp.slices = pl.nslices;
    if (pl.nslices > 1) {  // per slice: a copy per progression per stripe
        hp.h2d_copies = (int64_t)pl.sin.size() * nstripes;
        hp.d2h_copies = (int64_t)pl.sout.size() * nstripes;
    }
    return hp;
}

void stripe_range(int64_t nstripes, int parts, int j, int64_t *begin, int64_t *end) {
    // contiguous ranges, the remainder on the first ones (shard_stripes, __init__.py)
    const int64_t base = nstripes / parts, extra = nstripes % parts;
    *begin = j * base + std::min<int64_t>(j, extra);
    *end = *begin + base + (j < extra ? 1 : 0);
}

int64_t column_units(int64_t nstripes, int ndev, int64_t nbytes) {
    if (nstripes <= 0 || nstripes >= ndev || nbytes < 2 * kColUnit) return 0;
    return (nbytes + kColUnit - 1) / kColUnit;
}

}  // namespace ecx
