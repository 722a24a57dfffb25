// launch_rules_check.cpp -- structural invariants of every plan the launch rules make
// (csrc/launch_rules.cpp), over a dense grid of synthetic map traits x batch layouts x knobs,
// each knob one at a time from the defaults and then in random combinations.  Host-only:
// built from launch_rules.cpp alone under ASan + UBSan by tests/test_native.py.
//
// For every plan:
//   * the launches' chunk ranges tile [0, ceil(nbytes / chunk)) exactly once, in order;
//   * a launch that is not byte-safe covers full chunks of a 16-B-aligned layout only -- but for
//     the fused tail, the partial last chunk, a multiple of 16 B, and only when no output byte
//     of the batch is an input byte of it (outputs_never_read);
//   * kernels that address inputs through 32-bit slot offsets (LDS-table k_gf_apply, wide
//     tiles, bit-sliced, bit-plane) are chosen only when every offset fits;
//   * the one-workgroup-per-tile, tail, wide, skew, bit-sliced and tile-group launches name an
//     instance that exists (apply_launch.inc, apply_skew.hip, apply_bits.hip, kernels.hip), and
//     their rings divide the padded plan's;
//   * the kernel of record is the last launch that is neither byte-safe nor the partial chunk
//     alone, and describe() is empty exactly when there is none;
//   * the product build never plans a lab kernel.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../repair-pipelining_amd/csrc/launch_rules.hpp"

using namespace ecx;

namespace {
long g_plans = 0;
bool g_planes_available = true;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33) % n;
}

[[noreturn]] void fail(const char *what, const MapTraits &m, const Tuning &tu, const BatchLayout &b, int pick, bool diag,
                       const LaunchPlan &p) {
    std::printf("launch_rules_check: FAILED: %s\n  map: tiles %d rows %d n_in %d n_out %d max_in_slot %d wide %d pref %d\n"
                "  layout: in %llx out %llx iss %lld isl %lld oss %lld osl %lld S %lld n %lld acc %d  pick %d diag %d\n"
                "  knobs: depth %d nt %d scope %d small %d wide %d ldst %d thr %d skew %d planes %d waves %d bits %d lut %d units %d\n"
                "  plan: %s (%d launches)\n",
                what, m.n_tiles, m.max_tile_rows, m.n_in, m.n_out, m.max_in_slot, m.n_wide_tiles, m.preferred_depth,
                (unsigned long long)b.in, (unsigned long long)b.out, (long long)b.in_stripe_stride,
                (long long)b.in_slot_stride, (long long)b.out_stripe_stride, (long long)b.out_slot_stride,
                (long long)b.nstripes, (long long)b.nbytes, (int)b.accumulate, pick, (int)diag, tu.depth, tu.nontemporal,
                tu.store_scope, tu.small_tiles, tu.wide_tiles, tu.lds_tables, tu.block_threads, tu.skew_chunks,
                tu.map_planes, tu.wave_groups, tu.bitslice, tu.lds_lut, tu.units, describe(p).c_str(), p.n_launches);
    for (int i = 0; i < p.n_launches; ++i)
        std::printf("    %s chunks [%lld, +%lld) of %d\n", kernel_name(p.launches[i]).c_str(),
                    (long long)p.launches[i].chunk_begin, (long long)p.launches[i].n_chunks, p.launches[i].chunk_bytes);
    std::exit(1);
}

bool in(int v, std::initializer_list<int> set) {
    for (int x : set)
        if (x == v) return true;
    return false;
}

// apply_launch.inc launch_shape_t, as a predicate
bool apply_instance(const Launch &l) {
    const int T = l.threads;
    if (T != 64 && T != 256) return false;
    if (l.family == Family::ApplyTail)
        return !l.safe && l.ntl && l.nts == 1 && !l.tlds && l.rows == kTileRows && in(l.depth, {4, 8});
    if (l.safe) return in(l.depth, {2, 4});
    if (l.ntl ? l.nts == 0 : l.nts < 0 || l.nts > 2) return false;
    if (T == 64 && l.nts != 1) return false;
    if (l.rows < kTileRows) return T == 256 && in(l.rows, {2, 4}) && l.ntl && l.nts == 1 && !l.tlds && in(l.depth, {4, 8, 12});
    if (l.rows != kTileRows) return false;
    if (in(l.depth, {4, 8})) return true;
    if (T == 256 && l.ntl && !l.tlds && l.nts == 2) return l.depth == 20;
    if (T == 256 && l.ntl && !l.tlds && l.nts == 1 && in(l.depth, {10, 12, 16, 20, 24})) return true;
    return T == 256 && l.nts == 1 && l.depth == 2;
}

void check(const MapTraits &m, const Tuning &tu, const BatchLayout &b, int pick, bool diag) {
    const LaunchPlan p = choose_launch(m, tu, b, pick, diag, {[](void *) { return g_planes_available; }, nullptr});
    ++g_plans;
    auto bad = [&](const char *what) { fail(what, m, tu, b, pick, diag, p); };
    if (b.nstripes <= 0 || b.nbytes <= 0 || m.n_out == 0) {
        if (p.n_launches != 0 || !describe(p).empty()) bad("an empty batch launches something");
        return;
    }
    if (p.n_launches < 1 || p.n_launches > (int)p.launches.size()) bad("launch count");
    const int chunk = p.launches[0].chunk_bytes;
    const bool offsets32 = b.in_slot_stride >= 0 && (int64_t)m.max_in_slot * b.in_slot_stride + kChunkBytes <= 0x7FFFFFFF;
    int64_t next = 0;
    int record = -1;
    bool planes = false;
    for (int i = 0; i < p.n_launches; ++i) {
        const Launch &l = p.launches[i];
        if (l.chunk_bytes != chunk || !in(chunk, {1024, 4096})) bad("launches disagree on the chunk size");
        if (l.n_chunks <= 0 || l.chunk_begin != next) bad("chunk ranges leave a gap or overlap");
        next += l.n_chunks;
        if (l.units_per_stripe <= 0 || l.units_per_stripe > ((int64_t)1 << 30)) bad("grid units per stripe");
        const bool lab = in((int)l.family, {(int)Family::Lds, (int)Family::Grp, (int)Family::Bits, (int)Family::Lut, (int)Family::Multi});
        if (lab && !diag) bad("a lab kernel in the product build");
        if (!diag && l.family == Family::Skew && l.threads != 256) bad("one-wave skew in the product build");
        if (!l.safe) {
            if (!b.aligned16()) bad("a 16-B kernel on an unaligned layout");
            const int64_t end = l.chunk_begin + l.n_chunks;
            const int64_t full_end = l.fused_tail ? end - 1 : end;
            if (full_end * chunk > b.nbytes) bad("a kernel that is not byte-safe covers a partial chunk");
            if (l.fused_tail) {
                if (!in((int)l.family, {(int)Family::ApplyTail, (int)Family::Multi})) bad("fused tail on a family without one");
                if (l.tail_chunk != end - 1 || l.tail_bytes != b.nbytes - l.tail_chunk * chunk || l.tail_bytes <= 0 ||
                    l.tail_bytes % 16 || l.tail_bytes >= chunk || l.tail_chunk < 1)
                    bad("fused tail geometry");
                if (!outputs_never_read(m, b)) bad("fused tail although outputs may be read");
            } else if (l.tail_chunk != -1 || l.tail_bytes != 0) {
                bad("tail fields on a launch without a fused tail");
            }
            if (l.of_record) record = i;
            if (l.of_record == (l.fused_tail && l.n_chunks == 1)) bad("kernel-of-record flag");
        } else if (l.of_record || l.fused_tail || !in((int)l.family, {(int)Family::Apply, (int)Family::Wide, (int)Family::Lds, (int)Family::Grp})) {
            bad("byte-safe launch flags");
        }
        const bool needs32 = (l.family == Family::Apply && l.tlds) || l.family == Family::Wide || l.family == Family::Bits ||
                             l.family == Family::Planes;
        if (needs32 && !offsets32) bad("32-bit slot offsets do not fit");
        if (l.family == Family::Planes) planes = true;
        if ((l.family == Family::Bits || l.family == Family::Lut) && chunk != kChunkBytes) bad("a 4 KiB-chunk kernel on 1 KiB chunks");
        switch (l.family) {
        case Family::Apply:
        case Family::ApplyTail:
            if (!apply_instance(l)) bad("no k_gf_apply instance");
            if (l.threads * 16 != chunk || l.units_per_stripe != l.n_chunks * m.n_tiles) bad("k_gf_apply grid");
            if (l.tlds && (l.lds < (size_t)m.max_tile_entries(p.depth) * kAtabDwords * 4 || l.lds > 64 * 1024 + 65536))
                bad("LDS table bytes");
            break;
        case Family::Wide:
            if (!in(l.depth, {4, 8}) || (l.safe && (l.depth != 4 || l.ntl || l.nts)) || (!l.safe && l.nts != 1)) bad("no k_gf_apply_wide instance");
            if (m.n_wide_tiles <= 0 || l.units_per_stripe != l.n_chunks * m.n_wide_tiles || chunk != kChunkBytes) bad("wide grid");
            break;
        case Family::Skew: {
            const int cols = kChunkBytes / chunk;
            if (!l.ntl || !in(l.depth, {4, 8}) || !in(l.rows, {2, 4, 8}) || !in(l.skew, {2, 4}) || (l.rows == 8 && (l.skew != 2 || l.depth != 4)) ||
                (l.threads == 64 && l.rows == 8) || l.threads * 16 != chunk)
                bad("no k_gf_apply_skew instance");
            if (l.n_chunks % (l.skew * cols) || l.units_per_stripe != l.n_chunks / l.skew || m.n_tiles != 1 || l.skew != p.skew)
                bad("skew grid");
            break;
        }
        case Family::Planes:
            if (!m.planes_supported || l.units_per_stripe * kChunkBytes != l.n_chunks * chunk) bad("bit-plane launch");
            break;
        case Family::Bits:
            if (!in(l.depth, {2, 4})) bad("no k_gf_bits instance");
            break;
        case Family::Lds:
        case Family::Grp:
            if (!in(l.depth, {4, 8}) || (l.safe && l.depth != 4) || chunk != kWaveChunkBytes || l.threads != 64 * m.group_size)
                bad("no tile-group instance");
            break;
        case Family::Lut:
            if (!in(l.lut_mode, {0, 1}) || l.lds != (size_t)l.lut_pairs * 256 || l.lds > 64 * 1024) bad("k_gf_lut shape");
            break;
        case Family::Multi:
            if (!in(l.units, {2, 4}) || m.n_tiles != 1) bad("k_gf_apply_multi shape");
            break;
        }
        if (!in((int)l.family, {(int)Family::Planes, (int)Family::Lut, (int)Family::Bits}) && p.depth % l.depth)
            bad("a launch's ring does not divide the padded plan's");
    }
    if (next != (b.nbytes + chunk - 1) / chunk) bad("the launches do not cover the shard");
    if (record != p.record || planes != p.planes) bad("kernel of record");
    if (describe(p).empty() != (record < 0)) bad("describe() and the kernel of record disagree");
    if (record >= 0 && describe(p).compare(0, kernel_name(p.launches[record]).size(), kernel_name(p.launches[record])) != 0)
        bad("describe() does not start with the kernel of record");
    if (unit_order(p).empty() != (record < 0 || planes)) bad("unit order");
}

struct Knob {
    int Tuning::*field;
    std::vector<int> values;
};
const std::vector<Knob> kKnobs = {
    {&Tuning::depth, {0, 2, 4, 8, 10, 12, 16, 20, 24}}, {&Tuning::nontemporal, {0, 1, 2}}, {&Tuning::store_scope, {0, 1}},
    {&Tuning::small_tiles, {0, 1, 2}}, {&Tuning::wide_tiles, {0, 1, 2}}, {&Tuning::lds_tables, {0, 1, 2}},
    {&Tuning::block_threads, {0, 64, 256}}, {&Tuning::skew_chunks, {0, 1, 2, 4}}, {&Tuning::xcd_group, {0, 1, 2, 3}},
    {&Tuning::xcd_misaligned, {0, 1}}, {&Tuning::stagger, {0, 1, 2, 8, 64}}, {&Tuning::chunk_major, {0, 1}},
    {&Tuning::map_planes, {0, 1, 2}}, {&Tuning::wave_groups, {0, 1, 2}}, {&Tuning::bitslice, {0, 1, 2}},
    {&Tuning::lds_lut, {0, 1, 2}}, {&Tuning::units, {1, 2, 4}}, {&Tuning::occ_lds, {-1, 0, 4096}},
};

std::vector<MapTraits> make_traits() {
    std::vector<MapTraits> out;
    for (int rows : {1, 2, 4, 8, 16, 64})
        for (int n_in : {1, 4, 8, 17, 600})
            for (int count : {1, 12}) {
                if (count > n_in && count != 1) continue;
                MapTraits m;
                m.n_out = rows;
                m.n_in = n_in;
                m.n_tiles = (rows + kTileRows - 1) / kTileRows;
                m.max_tile_rows = rows < kTileRows ? rows : kTileRows;
                m.max_tile_count = count == 1 ? n_in : count;
                m.used_inputs = n_in;
                m.nnz = rows * (n_in < 8 ? n_in : 8);
                m.general_coeffs = m.nnz - (rows < n_in ? rows : n_in);
                m.max_in_slot = n_in + rows - 1;
                m.max_out_slot = rows - 1;
                m.planes_supported = rows <= 16;
                m.preferred_depth = m.max_tile_count >= 12 ? 8 : 4;
                if (m.n_tiles == 1 && rows == kTileRows && m.max_tile_count > 16 && m.max_tile_count <= 20) m.preferred_depth = 20;
                if (m.n_tiles > 1) {
                    m.n_groups = (m.n_tiles + 7) / 8;
                    m.group_size = m.n_tiles < 8 ? m.n_tiles : 8;
                    m.n_wide_tiles = (m.n_tiles + 1) / 2;
                    m.wide_depth = m.max_tile_count >= 12 ? 8 : 4;
                }
                for (double sharing : {1.0, 1.25}) {
                    if (sharing > 1.0 && m.n_tiles == 1) continue;
                    m.wide_sharing = sharing;
                    for (bool meet : {false, true}) {
                        m.slots_intersect = meet;
                        out.push_back(m);
                    }
                }
            }
    return out;
}

std::vector<BatchLayout> make_layouts(const MapTraits &m) {
    std::vector<BatchLayout> out;
    const int64_t slots = (m.max_in_slot > m.max_out_slot ? m.max_in_slot : m.max_out_slot) + 1;
    for (int64_t n : {64, 4096, 8176, 8208, 200000})
        for (int64_t pitch : {(n + 15) / 16 * 16, (int64_t)4 << 20, n + 1, (int64_t)1 << 31})
            for (int off : {0, 16, 1})
                for (int place = 0; place < 3; ++place)  // in place, disjoint, overlapping out of step
                    for (int64_t S : {3}) {
                        BatchLayout b;
                        b.in = ((uintptr_t)1 << 40) + off;
                        b.in_slot_stride = b.out_slot_stride = pitch;
                        b.in_stripe_stride = b.out_stripe_stride = slots * pitch;
                        b.out = place == 0 ? b.in : (place == 1 ? ((uintptr_t)1 << 50) + off : b.in + 2 * pitch);
                        b.nstripes = S;
                        b.nbytes = n;
                        b.accumulate = (n + off + place + S) & 1;
                        out.push_back(b);
                    }
    BatchLayout e;  // nothing to do
    out.push_back(e);
    return out;
}
}  // namespace

int main() {
    const std::vector<MapTraits> traits = make_traits();
    const int picks[] = {-1, 0, 1, 2, 3, 2 + 8 * 2, 2 + 8 * 8, 0 + 8 * 4};
    // every knob, one at a time from the defaults, on the static rules; the defaults on every candidate
    std::vector<std::vector<BatchLayout>> layouts;
    for (const MapTraits &m : traits) layouts.push_back(make_layouts(m));
    for (size_t t = 0; t < traits.size(); ++t)
        for (const BatchLayout &b : layouts[t])
            for (bool diag : {false, true}) {
                const MapTraits &m = traits[t];
                for (int pick : picks) check(m, Tuning{}, b, pick, diag);
                for (const Knob &k : kKnobs)
                    for (int v : k.values) {
                        Tuning tu;
                        if (tu.*(k.field) == v) continue;  // the defaults ran above
                        tu.*(k.field) = v;
                        check(m, tu, b, -1, diag);
                    }
            }
    // random combinations of knobs, candidates and an unavailable bit-plane kernel
    for (int i = 0; i < 200000; ++i) {
        const size_t t = rnd((uint32_t)traits.size());
        const MapTraits &m = traits[t];
        Tuning tu;
        for (const Knob &k : kKnobs)
            if (rnd(3) == 0) tu.*(k.field) = k.values[rnd((uint32_t)k.values.size())];
        g_planes_available = rnd(4) != 0;
        check(m, tu, layouts[t][rnd((uint32_t)layouts[t].size())], picks[rnd(8)], rnd(2) != 0);
    }
    std::printf("launch_rules_check: ok (%ld plans)\n", g_plans);
    return 0;
}
