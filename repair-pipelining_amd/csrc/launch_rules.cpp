// launch_rules.cpp -- the launch-shape rules of the composed-map kernels (launch_rules.hpp).
// Plain C++: built by the host compiler alone, like host_exec.cpp.
#include "launch_rules.hpp"

#include <algorithm>

namespace ecx {

bool outputs_never_read(const MapTraits &m, const BatchLayout &b) {
    const int64_t iss = b.in_stripe_stride, isl = b.in_slot_stride, oss = b.out_stripe_stride, osl = b.out_slot_stride;
    if (iss < 0 || isl < 0 || oss < 0 || osl < 0) return false;
    const int max_in = std::max(0, m.max_in_slot), max_out = std::max(0, m.max_out_slot);
    const uintptr_t in_hi = b.in + (uintptr_t)((b.nstripes - 1) * iss + (int64_t)max_in * isl + b.nbytes);
    const uintptr_t out_hi = b.out + (uintptr_t)((b.nstripes - 1) * oss + (int64_t)max_out * osl + b.nbytes);
    if (in_hi <= b.out || out_hi <= b.in) return true;
    const int max_slot = std::max(max_in, max_out);
    if (b.in != b.out || iss != oss || isl != osl || isl < b.nbytes || iss < (int64_t)(max_slot + 1) * isl) return false;
    return !m.slots_intersect;
}

int layout_candidate_code(int cand) { return cand >= 0 && cand < kLayoutNCand ? kLayoutCand[cand] : -2; }

bool layout_select_eligible(const MapTraits &m, const Tuning &tu, const BatchLayout &b) {
    return tu.layout_select && tu.skew_chunks == 1 && tu.block_threads == 0 && tu.stagger == 0 && !tu.lds_lut &&
           tu.bitslice != 2 && tu.nontemporal == 1 && tu.store_scope == 0 && m.n_tiles == 1 && m.n_in >= 8 &&
           m.max_tile_rows <= 4 && b.aligned16() && b.in_slot_stride > 0 && b.nbytes >= 4 * kChunkBytes &&
           b.nstripes * ((int64_t)m.n_in * b.nbytes) >= kLayoutMinBytes;
}

LaunchPlan choose_launch(const MapTraits &m, const Tuning &tu, const BatchLayout &b, int pick, bool diag,
                         PlanesAvailable planes_available) {
    LaunchPlan p;
    if (b.nstripes <= 0 || b.nbytes <= 0 || m.n_out == 0) return p;
    const int64_t nbytes = b.nbytes;
    // (the lab kernels -- tile groups, bit-sliced, LDS lookup tables, residency caps -- exist
    // only in the diagnostic build, `make DIAG=1`; their knobs are refused otherwise)
    const bool waves = diag && m.n_tiles > 1 && m.n_groups > 0 && tu.wave_groups;
    // Non-temporal policy: 0 never; 1 auto (NT stores, NT loads for single-tile maps); 2 always.
    const int ntmode = tu.nontemporal == 2 ? 2 : (tu.nontemporal == 1 ? (m.n_tiles == 1 ? 2 : 1) : 0);
    const int nts = ntmode == 0 ? 0 : (tu.store_scope ? 2 : 1);
    // Launch shapes that exist (apply_launch.inc); anything else is clamped here.
    // Workgroup size: 256 threads over 4 KiB chunks; one wave over 1 KiB chunks when forced
    // (64) or, in auto (0), for single-tile maps of <= 2 rows over >= 8 inputs whose slot
    // pitch is not a 4 MiB multiple (RS(12,4) decode on its padded pitch: +2.4-2.8 %; every
    // other BASELINE map -- LRC encode's 4 rows included -- is 3-8 % slower on one wave,
    // profiles/r02_block_threads.jsonl).  3-row maps (RS(17,3) encode) run on 4 KiB
    // workgroups: 0-4 % faster than one wave once the byte-safe tail took 16-B accesses
    // (profiles/r03_rs_km.jsonl, r03_rs173_pitch.jsonl, r03_rs173_ab.jsonl).
    const int shape = pick < 0 ? -1 : pick & 7;
    // Skewed chunk order (k_gf_apply_skew) for single-tile maps: forced (2 / 4 chunks),
    // or auto (1) when the input slot pitch is a multiple of 4 MiB -- the layouts whose
    // same-offset streams collide in HBM, where rotation recovers +10-17 %; on other
    // pitches it helps or costs by layout (profiles/r01_pitch_sweep.jsonl).  Auto needs
    // at least 4 input streams: one helper's partial sum (1 input) only loses.
    const bool skew_auto =
        pick < 0 ? b.in_slot_stride % ((int64_t)4 << 20) == 0 && m.n_in >= 4 : (shape == 1 || shape == 3);
    const bool one_wave = tu.block_threads == 64 ||
                          (tu.block_threads == 0 && m.n_tiles == 1 && tu.bitslice != 2 && !tu.lds_lut &&
                           (pick < 0 ? m.max_tile_rows <= 2 && m.n_in >= 8 && !skew_auto : (shape == 2 || shape == 3)));
    const int threads = one_wave && nts == 1 ? 64 : kBlockThreads;
    // Small-row kernel variants: forced (1), or auto (2) for maps of <= 2 rows over <= 4
    // inputs (LRC block repair: +2.5-3 %; wider narrow maps gain nothing or lose,
    // profiles/r02_small_tiles_ab.jsonl).
    const int map_rows = m.max_tile_rows <= 2 ? 2 : (m.max_tile_rows <= 4 ? 4 : kTileRows);
    const bool small = tu.small_tiles == 1 ||
                       (tu.small_tiles == 2 && m.max_tile_rows <= 2 && m.n_in <= 4 && m.n_tiles == 1);
    const int rows = small && !waves && threads == kBlockThreads && ntmode == 2 && nts == 1 ? map_rows : kTileRows;
    const bool default_nt = ntmode == 2 && nts == 1;  // NT loads, plain-nt stores: the shape most variants need

    // The load ring of the one-workgroup-per-tile kernel, clamped to the instances that exist
    // (apply_launch.inc): small tiles 4 / 8 / 12; depth 2 on 256 threads with plain-nt stores;
    // deep rings (10-24) for single-tile maps with NT loads and stores and SGPR tables.
    int depth = tu.depth ? tu.depth : m.preferred_depth;
    if (rows < kTileRows) {
        if (depth != 4 && depth != 8 && depth != 12) depth = 4;
    } else {
        if (depth == 2 && (waves || threads != kBlockThreads || nts != 1)) depth = 4;
        if (depth > 8 && (m.n_tiles != 1 || threads != kBlockThreads || ntmode != 2 ||
                          (nts != 1 && !(nts == 2 && depth == 20)) || tu.lds_tables == 2))
            depth = 8;
    }
    // Wide tiles (pairs of 8-row tiles) for multi-tile maps: auto (1) when pairing
    // saves at least 1/6 of the input reads (Clay(4,2) encode / repair {0,3}: 40 reads
    // over a 32-column union, +7-10 %; Clay(10,4) shortened: 80 over 76, where the
    // 16-row workgroup is 2x slower -- profiles/r01_wide.jsonl), forced (2), off (0).
    const bool offsets32 =
        b.in_slot_stride >= 0 && (int64_t)m.max_in_slot * b.in_slot_stride + kChunkBytes <= 0x7FFFFFFF;
    const bool aligned = b.aligned16();
    const bool full4k = aligned && nbytes >= kChunkBytes;  // the layout has whole, aligned 4 KiB chunks
    bool wide = (tu.wide_tiles == 2 || (tu.wide_tiles == 1 && m.wide_sharing >= 1.2)) && !waves &&
                m.n_wide_tiles > 0 && threads == kBlockThreads && rows == kTileRows && offsets32;
    if (wide) depth = tu.depth == 8 || tu.depth == 4 ? tu.depth : m.wide_depth;
    int skew = tu.skew_chunks == 1 ? (skew_auto ? 4 : 0) : tu.skew_chunks;
    if (skew == 4 && map_rows == kTileRows) skew = 2;  // 8 rows x 4 chunks would not fit the VGPRs
    // (one-wave workgroups take the skewed order over 1 KiB columns of <= 4-row maps in the
    // diagnostic build only: measured slower than the selected shapes)
    if (!(skew && m.n_tiles == 1 && !waves &&
          (threads == kBlockThreads || (diag && threads == 64 && map_rows <= 4)) && default_nt && aligned &&
          nbytes >= skew * kChunkBytes))
        skew = 0;
    if (skew) depth = depth == 4 || map_rows == kTileRows ? 4 : 8;
    // Bit-sliced kernel (k_gf_bits, apply_bits.hip) for the full 4 KiB chunks: forced (2)
    // wherever it can run, or auto (1) for multi-tile maps that do not pair into wide
    // tiles -- the maps with many coefficients per input, where the split-table
    // kernel is bound by vector issue (Clay(10,4)).  Its ring is 4
    // deep (2 on request); the byte-safe tail then runs on the same padded plan.
    const bool bits = diag && full4k && offsets32 && !waves && threads == kBlockThreads && ntmode != 0 && !skew &&
                      (tu.bitslice == 2 || (tu.bitslice == 1 && m.n_tiles > 1 && !wide));
    if (bits) {
        depth = tu.depth == 2 ? 2 : 4;
        wide = false;  // the byte-safe tail runs k_gf_apply over the same padded tiles
    }
    // Generated bit-plane kernel (k_map_planes, map_rtc.hpp) for the full 4 KiB chunks:
    // forced (2) wherever it fits, or auto (1) for multi-tile maps of <= 16 rows whose
    // coefficients outnumber their used inputs 4x or more -- where the split tables are
    // bound by vector issue (the Clay(4,2) two-node repairs: 184 coefficients over 32
    // inputs) -- on batches big enough (>= 64 MiB of input) to amortise the one-time
    // hiprtc compile.  The byte-safe tail runs on the composed plan below.  Auto falls back
    // to the composed kernels when the generated one cannot be built here.
    bool planes = false;
    if (tu.map_planes && full4k && offsets32 && !waves && m.planes_supported) {
        if (tu.map_planes == 2)
            planes = true;
        else if (m.n_tiles > 1 && m.nnz >= 4 * m.used_inputs &&
                 b.nstripes * (nbytes / kChunkBytes) * m.used_inputs >= 16384)
            planes = planes_available();
    }
    if (planes) skew = 0;  // (and no bit-sliced launch: bits_run below)
    // LDS lookup-table kernel (k_gf_lut, apply_lut.hip), forced only: 1 = log/antilog, 2 =
    // product rows for single-tile maps of <= kLutMaxPairs general coefficients.  Full
    // 4 KiB chunks of aligned layouts on the depth-4 padded plan; the byte-safe tail
    // runs k_gf_apply on the same plan.
    const bool lut = diag && tu.lds_lut && full4k && !waves && threads == kBlockThreads &&
                     (tu.lds_lut == 1 || (m.n_tiles == 1 && m.general_coeffs <= kLutMaxPairs));
    if (lut) {
        planes = wide = false;
        skew = 0;
        depth = 4;
    }
    const bool bits_run = bits && !planes && !lut;
    // Several units per workgroup with one ring across them (k_gf_apply_multi, ecx_tune "units"):
    // single-tile maps on the default NT shape, rings of 4 / 8 (and 20 on 256 threads)
    const bool multi = diag && tu.units > 1 && m.n_tiles == 1 && !waves && !wide && !bits_run && !lut && !planes &&
                       !skew && rows == kTileRows && default_nt && tu.lds_tables != 2 &&
                       (depth == 4 || depth == 8 || (depth == 20 && threads == kBlockThreads));

    // Multi-tile maps can run as tile groups (one wave per tile, 1 KiB chunks); otherwise
    // one workgroup per (stripe, chunk, tile) with 4 KiB (256 threads) or 1 KiB (64) chunks.
    const int chunk = waves ? kWaveChunkBytes : threads * 16;
    const int64_t full = aligned ? nbytes / chunk : 0;  // in units of `chunk`
    const int64_t tail_chunks = (nbytes - full * chunk + chunk - 1) / chunk;

    p.depth = depth;
    p.chunk_major = tu.chunk_major;
    p.stagger = pick < 0 ? tu.stagger : pick >> 3;
    // Single-tile maps whose input slots are not 128-B aligned: consecutive chunks of a slot
    // share a boundary cache line, fetched twice from HBM unless both chunks run on one XCD
    // (one L2) -- runs of consecutive units per XCD (RS(17,3) on 200,000-B shards: reads
    // 1.035x the algorithmic bytes, +5 % with the runs, profiles/r03_rs173_xcd_align.jsonl).
    const bool misaligned128 = b.in % 128 != 0 || b.in_stripe_stride % 128 != 0 || b.in_slot_stride % 128 != 0;
    p.xcd_group = (m.n_tiles > 1 || tu.xcd_group == 3)
                      ? tu.xcd_group
                      : (tu.xcd_group == 0 && tu.xcd_misaligned && misaligned128 ? 3 : 0);
    p.xcd_run = tu.xcd_run;
    p.skew = skew;
    p.planes = planes;

    auto add = [&](Launch l) {
        if (l.n_chunks <= 0) return;
        if (l.of_record) p.record = p.n_launches;
        p.launches[p.n_launches++] = l;
    };
    // One launch of the per-chunk kernels over chunks [begin, begin + n): the tile groups, the
    // bit-sliced kernel, the wide tiles, the multi-unit kernel or k_gf_apply, in that order.
    auto run = [&](bool safe, int64_t begin, int64_t n, bool tail) {
        Launch l;
        l.safe = safe;
        l.chunk_begin = begin;
        l.n_chunks = n;
        l.chunk_bytes = chunk;
        l.threads = threads;
        l.units_per_stripe = n * (waves ? m.n_groups : (wide ? m.n_wide_tiles : m.n_tiles));
        l.of_record = !safe && !(tail && n == 1);
        if (tail) {
            l.fused_tail = true;
            l.tail_chunk = full;
            l.tail_bytes = (int)(nbytes - full * chunk);
        }
        if (waves) {
            l.family = tu.wave_groups == 2 ? Family::Grp : Family::Lds;
            l.threads = 64 * m.group_size;
            l.depth = !safe && depth == 8 ? 8 : 4;
        } else if (bits_run && !safe) {
            l.family = Family::Bits;
            l.ntl = ntmode == 2;
            l.depth = depth;
        } else if (wide) {
            l.family = Family::Wide;
            l.ntl = !safe && (ntmode == 2 || (ntmode == 1 && m.n_wide_tiles == 1));  // one pair: no re-reads
            l.nts = safe ? 0 : 1;
            l.depth = safe ? 4 : depth;
        } else if (multi && !safe) {  // measured slower on every single-tile map: DESIGN.md section 4.5
            l.family = Family::Multi;
            l.units = tu.units;
            l.depth = depth;
        } else if (safe) {  // the byte-safe kernel's ring must match the plan's padding
            l.depth = depth % 4 ? 2 : 4;
        } else {
            l.family = tail ? Family::ApplyTail : Family::Apply;
            l.ntl = ntmode == 2;
            l.nts = nts;
            l.depth = depth;
            l.rows = rows;
            // TLDS kernels address inputs through a buffer descriptor with 32-bit slot
            // offsets (apply.hpp): every slot's chunk must lie within 2 GiB of the stripe chunk.
            const int mte = m.max_tile_entries(depth);
            l.tlds = rows == kTileRows && mte > 0 && offsets32 && mte <= kMaxLdsTileEntries &&
                     (tu.lds_tables == 2 || (tu.lds_tables == 1 && m.n_tiles > 1));
            // Residency cap (ecx_tune "occ_lds"): dummy LDS per workgroup.  Auto: the many-stream
            // single-tile maps (>= 8 inputs, rings of <= 8 loads) at 4 waves per SIMD -- 4
            // 256-thread or 16 one-wave workgroups per CU -- instead of the 5 their registers allow.
            size_t occ = diag && tu.occ_lds > 0 ? (size_t)tu.occ_lds : 0;
            if (diag && tu.occ_lds < 0 && m.n_tiles == 1 && m.n_in >= 8 && depth <= 8)
                occ = kLdsPerCu / (kOccWavesPerSimd * kSimdsPerCu / (threads / 64));
            if (!tail) l.lds = (l.tlds ? (size_t)mte * kAtabDwords * 4 : 0) + occ;
        }
        add(l);
    };

    int64_t first = 0;  // first full chunk left to the one-chunk kernels
    if (lut) {
        Launch l;
        l.family = Family::Lut;
        l.lut_mode = tu.lds_lut - 1;
        l.lut_pairs = l.lut_mode == 1 ? m.general_coeffs : 0;
        l.ntl = ntmode == 2;
        l.n_chunks = full;
        l.units_per_stripe = full * m.n_tiles;
        l.lds = (size_t)l.lut_pairs * 256;
        l.of_record = true;
        add(l);
        first = full;
    }
    if (planes) {
        Launch l;
        l.family = Family::Planes;
        l.n_chunks = nbytes / kChunkBytes * (kChunkBytes / chunk);
        l.chunk_bytes = chunk;
        l.threads = 128;
        l.units_per_stripe = nbytes / kChunkBytes;
        l.of_record = true;
        add(l);
        first = l.n_chunks;
    }
    if (skew) {
        const int64_t cols = kChunkBytes / chunk;  // workgroups per 4 KiB chunk (4 for one wave)
        const int64_t groups = full / (skew * cols);
        Launch l;
        l.family = Family::Skew;
        l.ntl = true;
        l.nts = 1;
        l.depth = depth;
        l.rows = map_rows;
        l.skew = skew;
        l.threads = threads;
        l.n_chunks = groups * skew * cols;
        l.chunk_bytes = chunk;
        l.units_per_stripe = groups * cols;
        l.of_record = true;
        add(l);
        first = l.n_chunks;
    }
    // A partial last chunk whose byte count is a multiple of 16 (RS(17,3) on the published
    // 200,000-B shards: 48 full 4 KiB chunks and 3,392 B) runs in the same k_gf_apply launch
    // as the full chunks, as a workgroup over the shard's last chunk-sized window whose lanes
    // store only the partial chunk (apply.hpp); otherwise the byte-safe kernel takes it in a
    // launch of its own.
    const int64_t tail_len = nbytes - full * chunk;
    const bool fuse_tail = aligned && full >= 1 && tail_len > 0 && tail_len % 16 == 0 && (depth == 4 || depth == 8) &&
                           m.n_tiles == 1 && rows == kTileRows && default_nt && tu.lds_tables != 2 && !waves && !wide &&
                           !bits_run && !lut && outputs_never_read(m, b);
    if (fuse_tail) {
        run(false, first, full + 1 - first, true);
    } else {
        run(false, first, full - first, false);
        run(true, full, tail_chunks, false);
    }
    return p;
}

namespace {
const char *tf(bool v) { return v ? "true" : "false"; }
std::string params(std::initializer_list<std::string> v) {
    std::string s = "<";
    const char *sep = "";
    for (const std::string &x : v) {
        s += sep;
        s += x;
        sep = ", ";
    }
    return s + ">";
}
std::string n(int v) { return std::to_string(v); }
}  // namespace

std::string kernel_name(const Launch &l) {
    switch (l.family) {
    case Family::Apply:
        return "k_gf_apply" + params({tf(l.safe), tf(l.ntl), n(l.nts), n(l.depth), tf(l.tlds), n(l.threads), n(l.rows)});
    case Family::ApplyTail:
        return "k_gf_apply_tail" + params({tf(l.ntl), n(l.nts), n(l.depth), tf(l.tlds), n(l.threads), n(l.rows)});
    case Family::Wide: return "k_gf_apply_wide" + params({tf(l.safe), tf(l.ntl), n(l.nts), n(l.depth)});
    case Family::Skew: return "k_gf_apply_skew" + params({tf(l.ntl), n(l.depth), n(l.rows), n(l.skew), n(l.threads)});
    case Family::Planes: return "k_map_planes";
    case Family::Lds: return "k_gf_apply_lds" + params({tf(l.safe), n(l.depth)});
    case Family::Grp: return "k_gf_apply_grp" + params({tf(l.safe), n(l.depth)});
    case Family::Bits: return "k_gf_bits" + params({tf(l.ntl), n(l.depth)});
    case Family::Lut: return "k_gf_lut" + params({n(l.lut_mode), tf(l.ntl)});
    case Family::Multi:
        return "k_gf_apply_multi" + params({n(l.depth), n(kTileRows), n(l.units), n(l.threads), tf(l.fused_tail)});
    }
    return std::string();
}

std::string unit_order(const LaunchPlan &p) {
    if (p.record < 0 || p.planes) return std::string();
    return "stagger=" + n(p.stagger) + " xcd_group=" + n(p.xcd_group) + " xcd_run=" + n(p.xcd_group == 3 ? p.xcd_run : 0) +
           (p.skew ? " skew=" + n(p.skew) : std::string());
}

std::string describe(const LaunchPlan &p) {
    if (p.record < 0) return std::string();
    const std::string order = unit_order(p);
    return order.empty() ? kernel_name(p.launches[p.record]) : kernel_name(p.launches[p.record]) + " " + order;
}

}  // namespace ecx
