// kernels.hip -- CDNA4 (gfx950) kernels of the GF(256) erasure engine.
//
// k_gf_apply applies one compiled GF(256) map (engine.hpp) to a batch of
// stripes.  It replaces the reference's per-(input,output) byte loop
// (InputOutputByteTableCodingLoop.java:27-29,39-41) and, through the planner,
// the whole stage sequence of ClayCodeErasureDecodingStep.doDecodeSingle /
// doDecodeMulti and ReedSolomon.decodeMissing in ONE pass over HBM:
//
//   * a 256-thread workgroup owns one (stripe, 4 KiB chunk, output tile);
//     each lane owns 16 consecutive byte positions of every sub-chunk;
//   * per input entry the lane issues one coalesced 16-B load (a wave moves
//     1 KiB contiguous per instruction) -- the next entry's load is issued
//     before the current one is consumed;
//   * the byte is split into 3+3+2 bits once per input, and every GF multiply
//     is three v_perm_b32 table lookups over four bytes (tables are wave-
//     uniform scalar loads from the plan) plus XOR into register accumulators;
//     coefficient 1 is a bare XOR (LRC local parity);
//   * no LDS, no MFMA: this is HBM-bound byte work.
#include "apply.hpp"
#include "layout_probe.hpp"
#include "map_rtc.hpp"

namespace ecx {

#if ECX_DIAG  // measured and rejected: `make DIAG=1` only
// Multi-tile maps: one workgroup = one (stripe, 1 KiB chunk, tile GROUP), one
// wave per tile.  The tiles of a group share inputs (Clay(10,4): 8 tiles read
// 208 distinct inputs 320 times), so instead of each wave loading its own
// inputs, the group's union of inputs streams through LDS exactly once:
//
//   stage k: wave w stores union[k*G + w] (held in its load ring) to LDS buffer
//            k&1 and refills the ring DEPTH stages ahead; barrier; every wave
//            applies the entries of its tile whose union position falls in
//            stage k, reading the 1 KiB rows from LDS.
//
// Two LDS buffers make one barrier per stage enough: buffer k&1 is rewritten at
// stage k+2, after every wave has passed the barrier of stage k+1.  HBM reads
// are the algorithmic bytes (1.0x instead of the re-read factor); the union is
// padded with zero-page entries to whole ring groups so refills are branch-free.
template <bool SAFE, int DEPTH>
__global__ void __launch_bounds__(64 * kWaveGroup, DEPTH == 4 ? 6 : 5) k_gf_apply_lds(ApplyArgs a) {
    __shared__ u32x4 stage[2][kWaveGroup][64];  // 16 KiB
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t G = blockDim.x >> 6;
    const uint32_t b = blockIdx.x;
    const uint32_t g = b % (uint32_t)a.n_groups;
    const uint32_t rest = b / (uint32_t)a.n_groups;
    cu32 *grp = plan_ptr(a.groups) + g * kGroupDwords;
    const uint32_t tl = __builtin_amdgcn_readfirstlane(grp[wave]);
    const int nst = (int)(grp[9] / G);  // stages; a multiple of DEPTH
    cu32 *uni = plan_ptr(a.unions) + grp[8];
    const int64_t c = a.chunk_begin + (int64_t)(rest % (uint32_t)a.n_chunks);
    const int64_t s = a.stripe_begin + (int64_t)(rest / (uint32_t)a.n_chunks);
    const int64_t cbase = c * kWaveChunkBytes;
    const uint32_t lane16 = lane * 16;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)lane16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    const uint8_t *ib = reinterpret_cast<const uint8_t *>(uniform64((uint64_t)(a.in + s * a.in_stripe_stride + cbase))) + lane16;
    auto load = [&](uint32_t slot) -> u32x4 {
        const uint8_t *p = slot == kDummySlot ? a.zero_page + lane16 : ib + (int64_t)slot * a.in_slot_stride;
        return SAFE ? load_partial(p, valid) : ld16<true>(p);  // each union input is read once: stream it
    };

    const bool active = tl != kNoTile;
    cu32 *tile = plan_ptr(a.tiles) + (active ? tl : 0u) * kTileDwords;
    const int ecnt = active ? (int)tile[3] : 0;
    cu32 *ent = plan_ptr(a.entries) + (int64_t)tile[0] * kEntryDwords;
    int e = 0;
    uint32_t next_pos = ecnt > 0 ? ent[3] : 0xFFFFFFFFu;

    u32x4 acc[kTileRows];
#pragma unroll
    for (int r = 0; r < kTileRows; ++r) acc[r] = (u32x4){0u, 0u, 0u, 0u};

    auto consume = [&](int k, int buf) {  // entries of this tile staged at stage k
        const uint32_t hi = (uint32_t)(k + 1) * G;
        while (next_pos < hi) {
            cu32 *r = ent + (int64_t)e * kEntryDwords;
            apply_entry<false>(r, stage[buf][next_pos - (uint32_t)k * G][lane], acc, nullptr);
            ++e;
            next_pos = e < ecnt ? r[kEntryDwords + 3] : 0xFFFFFFFFu;
        }
    };

    u32x4 ring[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) ring[u] = load(uni[u * G + wave]);
    const int last = nst - DEPTH;
    for (int k0 = 0; k0 < last; k0 += DEPTH) {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int k = k0 + u;
            stage[u & 1][wave][lane] = ring[u];  // DEPTH is even: k & 1 == u & 1
            ring[u] = load(uni[(k + DEPTH) * G + wave]);
            __syncthreads();
            consume(k, u & 1);
        }
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
        stage[u & 1][wave][lane] = ring[u];
        __syncthreads();
        consume(last + u, u & 1);
    }
    if (!active) return;
    uint8_t *ob = reinterpret_cast<uint8_t *>(uniform64((uint64_t)(a.out + s * a.out_stripe_stride + cbase))) + lane16;
    const int nrows = (int)tile[2];
#pragma unroll
    for (int o = 0; o < kTileRows; ++o) {
        if (o < nrows) {
            uint8_t *p = ob + (int64_t)tile[4 + o] * a.out_slot_stride;
            u32x4 v = acc[o];
            if (a.accumulate) v ^= SAFE ? load_partial(p, valid) : load16(p);
            if (SAFE) store_partial(p, v, valid);
            else st16<true>(p, v);
        }
    }
}
#endif  // ECX_DIAG

// Wide tiles: one 256-thread workgroup = one (stripe, 4 KiB chunk, pair of 8-row
// tiles A and B).  Each input of the pair's union is loaded once and applied to
// both halves (A's and B's entry tables), so a pair that shares inputs reads each of
// them once instead of twice.  16 accumulator rows; otherwise the loop of apply_tile
// (zero-page-padded ring of DEPTH loads, SGPR tables).
template <bool SAFE, bool NTL, int NTS, int DEPTH>
__global__ void __launch_bounds__(kBlockThreads, 4) k_gf_apply_wide(ApplyArgs a) {
    const uint32_t w = blockIdx.x % (uint32_t)a.n_wide;
    const uint32_t rest = blockIdx.x / (uint32_t)a.n_wide;
    const int64_t c = a.chunk_begin + (int64_t)(rest % (uint32_t)a.n_chunks);
    const int64_t s = a.stripe_begin + (int64_t)(rest / (uint32_t)a.n_chunks);
    const int64_t cbase = c * kChunkBytes;
    const uint32_t lane16 = threadIdx.x * 16;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)lane16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    cu32 *rec = plan_ptr(a.wtiles) + __builtin_amdgcn_readfirstlane(w) * kWideTileDwords;
    const uint64_t in_base = uniform64((uint64_t)(a.in + s * a.in_stripe_stride + cbase));
    const uint8_t *ib = reinterpret_cast<const uint8_t *>(in_base) + lane16;
    // Buffer-descriptor addressing as in apply_tile's TLDS kernels (apply.hpp): the
    // slot offset is a scalar soffset, padding re-reads the pair's first input.
    cu32 *went = plan_ptr(a.wentries) + (int64_t)rec[0] * kWideEntryDwords;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t first_soff = 0;
    if constexpr (!SAFE) {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(in_base), 0, 0x7FFFFFFF, 0x00020000);
        if (rec[1] > 0) first_soff = went[0] * (uint32_t)a.in_slot_stride;  // a pair with no inputs loads nothing
    }
    auto load = [&](uint32_t slot) -> u32x4 {
        if constexpr (!SAFE) {
            const uint32_t soff = slot == kDummySlot ? first_soff : slot * (uint32_t)a.in_slot_stride;
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)lane16, (int)soff, NTL ? 2 : 0);
            return (u32x4){(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]};
        } else {
            const uint8_t *p = slot == kDummySlot ? a.zero_page + lane16 : ib + (int64_t)slot * a.in_slot_stride;
            return load_partial(p, valid);
        }
    };
    u32x4 acc_a[kTileRows], acc_b[kTileRows];
#pragma unroll
    for (int r = 0; r < kTileRows; ++r) acc_a[r] = acc_b[r] = (u32x4){0u, 0u, 0u, 0u};
    const int ecnt = (int)rec[1];
    cu32 *ent = plan_ptr(a.wentries) + (int64_t)rec[0] * kWideEntryDwords;
    if (ecnt > 0) {
        u32x4 ring[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) ring[u] = load(ent[u * kWideEntryDwords]);
        const int last = ecnt - DEPTH;
        for (int e0 = 0; e0 < last; e0 += DEPTH) {
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                cu32 *r = ent + (int64_t)(e0 + u) * kWideEntryDwords;
                apply_entry<false>(r, ring[u], acc_a, nullptr);
                apply_entry<false>(r + kEntryDwords, ring[u], acc_b, nullptr);
                ring[u] = load(r[DEPTH * kWideEntryDwords]);
            }
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            cu32 *r = ent + (int64_t)(last + u) * kWideEntryDwords;
            apply_entry<false>(r, ring[u], acc_a, nullptr);
            apply_entry<false>(r + kEntryDwords, ring[u], acc_b, nullptr);
        }
    }
    uint8_t *ob = reinterpret_cast<uint8_t *>(uniform64((uint64_t)(a.out + s * a.out_stripe_stride + cbase))) + lane16;
    const int rows_a = (int)rec[2], rows_b = (int)rec[3];
#pragma unroll
    for (int o = 0; o < kTileRows; ++o) {
        if (o < rows_a) {
            uint8_t *p = ob + (int64_t)rec[4 + o] * a.out_slot_stride;
            u32x4 v = acc_a[o];
            if (a.accumulate) v ^= SAFE ? load_partial(p, valid) : load16(p);
            if (SAFE) store_partial(p, v, valid);
            else st16<NTS>(p, v);
        }
        if (o < rows_b) {
            uint8_t *p = ob + (int64_t)rec[12 + o] * a.out_slot_stride;
            u32x4 v = acc_b[o];
            if (a.accumulate) v ^= SAFE ? load_partial(p, valid) : load16(p);
            if (SAFE) store_partial(p, v, valid);
            else st16<NTS>(p, v);
        }
    }
}

#if ECX_DIAG  // measured and rejected: `make DIAG=1` only
// Multi-tile maps, tile groups without staging: one workgroup = one (stripe, 1 KiB
// chunk, tile GROUP), one wave per tile, each wave loading its own entries directly.
// The group's tiles share inputs, and each tile's entry list is ordered by the
// group's staging schedule (engine.cpp align_group), so the waves of a workgroup --
// on one CU -- request a shared input at about the same time and the repeats are
// served by that CU's L1 / the XCD's L2 rather than by another CU's fetch.  No LDS,
// no barriers: a wave whose slot in the group is empty exits at once.
template <bool SAFE, int DEPTH>
__global__ void __launch_bounds__(64 * kWaveGroup, DEPTH == 4 ? 6 : 5) k_gf_apply_grp(ApplyArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x;
    const uint32_t g = b % (uint32_t)a.n_groups;
    const uint32_t rest = b / (uint32_t)a.n_groups;
    const uint32_t tl = __builtin_amdgcn_readfirstlane(plan_ptr(a.groups)[g * kGroupDwords + wave]);
    if (tl == kNoTile) return;
    const int64_t c = a.chunk_begin + (int64_t)(rest % (uint32_t)a.n_chunks);
    const int64_t s = a.stripe_begin + (int64_t)(rest / (uint32_t)a.n_chunks);
    const int64_t cbase = c * kWaveChunkBytes;
    const uint32_t lane16 = lane * 16;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)lane16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    apply_tile<SAFE, false, SAFE ? 0 : 1, DEPTH, false, 64, kTileRows>(
        a, plan_ptr(a.tiles) + tl * kTileDwords, uniform64((uint64_t)(a.in + s * a.in_stripe_stride + cbase)),
        uniform64((uint64_t)(a.out + s * a.out_stripe_stride + cbase)), lane16, valid, nullptr);
}
#endif  // ECX_DIAG

namespace {
struct PlanesQuery {
    CompiledMap *cm;
    bool accumulate;
};

// One launch of the plan over `blocks` grid units: the family's instance table.
void issue_blocks(const Launch &l, int64_t blocks, hipStream_t stream, ApplyArgs &a) {
    const dim3 grid((unsigned)blocks);
    switch (l.family) {
    case Family::Apply:
    case Family::ApplyTail: {
        Shape s;
        s.safe = l.safe;
        s.ntl = l.ntl;
        s.nts = l.nts;
        s.depth = l.depth;
        s.tlds = l.tlds;
        s.threads = l.threads;
        s.rows = l.rows;
        s.tail = l.family == Family::ApplyTail;
        s.note = l.of_record;
        if (l.threads == 64) launch_shape_t<64>(s, grid, l.lds, stream, a);
        else launch_shape_t<kBlockThreads>(s, grid, l.lds, stream, a);
        return;
    }
    case Family::Wide: {
        const dim3 blk(kBlockThreads);
        if (l.of_record) note_kernel("k_gf_apply_wide", false, l.ntl, 1, l.depth);
        if (l.safe) hipLaunchKernelGGL((k_gf_apply_wide<true, false, 0, 4>), grid, blk, 0, stream, a);
        else if (l.depth == 8 && l.ntl) hipLaunchKernelGGL((k_gf_apply_wide<false, true, 1, 8>), grid, blk, 0, stream, a);
        else if (l.depth == 8) hipLaunchKernelGGL((k_gf_apply_wide<false, false, 1, 8>), grid, blk, 0, stream, a);
        else if (l.depth == 4 && l.ntl) hipLaunchKernelGGL((k_gf_apply_wide<false, true, 1, 4>), grid, blk, 0, stream, a);
        else if (l.depth == 4) hipLaunchKernelGGL((k_gf_apply_wide<false, false, 1, 4>), grid, blk, 0, stream, a);
        else throw Error(ECX_E_ILLEGAL_ARGUMENT, "no k_gf_apply_wide instance for this launch shape");
        return;
    }
    case Family::Skew: launch_skew(l.skew, l.rows, l.depth, l.ntl, l.threads, grid, stream, a); return;
#if ECX_DIAG
    case Family::Lds:
    case Family::Grp: {
        const dim3 blk(l.threads);
        const bool grp = l.family == Family::Grp;  // direct loads, no LDS staging
        if (l.of_record) note_kernel(grp ? "k_gf_apply_grp" : "k_gf_apply_lds", false, l.depth);
        if (grp) {
            if (l.safe) hipLaunchKernelGGL((k_gf_apply_grp<true, 4>), grid, blk, 0, stream, a);
            else if (l.depth == 8) hipLaunchKernelGGL((k_gf_apply_grp<false, 8>), grid, blk, 0, stream, a);
            else hipLaunchKernelGGL((k_gf_apply_grp<false, 4>), grid, blk, 0, stream, a);
        } else {
            if (l.safe) hipLaunchKernelGGL((k_gf_apply_lds<true, 4>), grid, blk, 0, stream, a);
            else if (l.depth == 8) hipLaunchKernelGGL((k_gf_apply_lds<false, 8>), grid, blk, 0, stream, a);
            else hipLaunchKernelGGL((k_gf_apply_lds<false, 4>), grid, blk, 0, stream, a);
        }
        return;
    }
    case Family::Bits: launch_bits(l.ntl, l.depth, grid, stream, a); return;
    case Family::Multi:
        a.multi_total = blocks;
        launch_multi(l.units, l.depth, l.threads, l.fused_tail, dim3((unsigned)((blocks + l.units - 1) / l.units)), stream, a);
        return;
#endif
    default: throw Error(ECX_E_ILLEGAL_ARGUMENT, "launch plan names a kernel this build does not hold");
    }
}

// One launch of the plan over every stripe, in batches of stripes that keep a grid under 2^30 blocks.
void issue(const Launch &l, CompiledMap &cm, const BatchLayout &b, hipStream_t stream, ApplyArgs &a) {
    a.chunk_begin = l.chunk_begin;
    a.n_chunks = l.n_chunks;
    a.stripe_begin = 0;
    a.tail_chunk = l.tail_chunk;
    a.tail_bytes = l.tail_bytes;
    if (l.family == Family::Planes) {
        cm.planes()->launch(a.in, b.in_stripe_stride, b.in_slot_stride, a.out, b.out_stripe_stride, b.out_slot_stride,
                            b.nstripes, l.units_per_stripe, b.accumulate, stream);
        return;
    }
#if ECX_DIAG
    if (l.family == Family::Lut) {  // persistent workgroups: one launch walks every unit
        launch_lut(l.lut_mode, l.ntl, l.lut_pairs, b.nstripes * l.units_per_stripe, stream, a);
        return;
    }
#endif
    // k_gf_apply_skew counts chunk groups: one per 4 KiB / chunk_bytes columns of workgroups
    if (l.family == Family::Skew) a.n_chunks = l.units_per_stripe / (kChunkBytes / l.chunk_bytes);
    const int64_t max_blocks = (int64_t)1 << 30;
    const int64_t stripes_per_launch = std::max<int64_t>(1, max_blocks / l.units_per_stripe);
    for (int64_t s0 = 0; s0 < b.nstripes; s0 += stripes_per_launch) {
        a.stripe_begin = s0;
        issue_blocks(l, std::min(stripes_per_launch, b.nstripes - s0) * l.units_per_stripe, stream, a);
    }
}

// Issues the launches launch_rules.cpp choose_launch decides on (`pick`: its candidate code).
void launch_apply_core(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                       uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                       int64_t nbytes, hipStream_t stream, bool accumulate, int pick,
                       hipEvent_t probe_start = nullptr) {
    const MapTraits &m = cm.traits();
    const BatchLayout b{(uintptr_t)in,     (uintptr_t)out,  in_stripe_stride, in_slot_stride, out_stripe_stride,
                        out_slot_stride, nstripes,        nbytes,           accumulate};
    PlanesQuery q{&cm, accumulate};
    const LaunchPlan p = choose_launch(
        m, tuning(), b, pick, ECX_DIAG != 0,
        {[](void *c) { return ((PlanesQuery *)c)->cm->planes()->available(((PlanesQuery *)c)->accumulate); }, &q});
    if (p.n_launches == 0) return;
    const DevicePlan &plan = cm.plan_for_current_device(p.depth);

    ApplyArgs a;
    a.in = in;
    a.out = out;
    a.entries = plan.entries;
    a.tiles = plan.tiles;
    a.groups = plan.groups;
    a.unions = plan.unions;
    a.atab = plan.atab;
    a.wentries = plan.wentries;
    a.wtiles = plan.wtiles;
    a.bentries = plan.bentries;
    a.n_wide = m.n_wide_tiles;
    a.lane_zero = 0;
    a.chunk_major = p.chunk_major;
    a.stagger = p.stagger;
    a.n_groups = m.n_groups;
    a.zero_page = zero_page_for_current_device();
    a.in_stripe_stride = in_stripe_stride;
    a.in_slot_stride = in_slot_stride;
    a.out_stripe_stride = out_stripe_stride;
    a.out_slot_stride = out_slot_stride;
    a.nbytes = nbytes;
    a.n_tiles = m.n_tiles;
    a.xcd_group = p.xcd_group;
    a.xcd_run = p.xcd_run;
    a.accumulate = accumulate ? 1 : 0;
    a.multi_total = 0;

    // a layout probe's start: after the host-side work (plan upload on first use), so the
    // probe times the kernels alone; a failed record only drops that probe
    if (probe_start && hipEventRecord(probe_start, stream) != hipSuccess) (void)hipGetLastError();
    for (int i = 0; i < p.n_launches; ++i) issue(p.launches[i], cm, b, stream, a);
    if (p.record >= 0 && !p.planes) set_last_shape_order(unit_order(p));  // a composed-map kernel of record
    check_hip(hipGetLastError(), "k_gf_apply launch");
}
}  // namespace

// Launch shape per batch layout, measured on the caller's own launches.  The many-stream
// single-tile maps (RS decode / encode: >= 8 input streams, <= 4 rows) move 0.63-0.79 of
// HBM depending only on where their streams sit: same-offset streams whose addresses differ
// in the bits the HBM interleave does not spread (a 4 MiB shard pitch, or 1 MiB + 4 KiB,
// whose stripes collide) queue on one bank (scripts/addr_probe.hip), and
// no static rule predicts which shape -- 4 KiB or one-wave workgroups, skewed chunks,
// staggered stripes -- is fastest at a given pitch (scripts/layout_sweep.py).  So for a
// new layout (map, strides, size classes of the shard and the batch, device) the first calls run the
// candidates in turn, each launch bracketed by two events on the caller's stream; the
// events are read without blocking on later calls, and once every candidate has
// kLayoutSamples timings the fastest median is kept for that layout (layout_select.hpp).  Every candidate
// computes the same bytes, and nothing is launched that the caller did not ask for: the
// exploration costs only the slower candidates' launches.  Batches under kLayoutMinBytes of
// input, streams being captured and forced shapes use the static rules
// (launch_rules.hpp layout_select_eligible; the candidates are its kLayoutCand).
void launch_apply(CompiledMap &cm, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride, uint8_t *out,
                  int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes, int64_t nbytes,
                  hipStream_t stream, bool accumulate) {
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    const int64_t in_bytes = (int64_t)cm.map().n_in * nbytes;  // per stripe
    bool select = layout_select_eligible(cm.traits(), tuning(),
                                         BatchLayout{(uintptr_t)in, (uintptr_t)out, in_stripe_stride, in_slot_stride,
                                                     out_stripe_stride, out_slot_stride, nstripes, nbytes, accumulate});
    if (select) select = !stream_is_capturing(stream);  // capturing or unknown: no events
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    if (!select) {
        launch_apply_core(cm, in, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nstripes,
                          nbytes, stream, accumulate, -1);
        note_device_launch(dev, stream, nstripes * in_bytes);
        return;
    }
    // A layout is its strides, the size class of the shard (log2 of the byte count) and of the
    // batch (log2 of its input bytes), the mode and the device: callers whose batch sizes vary
    // from call to call share one selection instead of exploring anew at every size.
    auto log2i = [](int64_t v) { return (int64_t)(63 - __builtin_clzll((unsigned long long)std::max<int64_t>(v, 1))); };
    const LayoutKey key{in_slot_stride, in_stripe_stride, out_slot_stride, out_stripe_stride,
                        log2i(nbytes), log2i(nstripes * in_bytes), (int64_t)accumulate, (int64_t)dev};
    ProbeGuard probe(cm.layout_selection(), key, dev, stream);
    launch_apply_core(cm, in, in_stripe_stride, in_slot_stride, out, out_stripe_stride, out_slot_stride, nstripes,
                      nbytes, stream, accumulate, kLayoutCand[probe.cand()], probe.start());
    note_device_launch(dev, stream, nstripes * in_bytes);
    probe.finish();
}

// ---------------------------------------------------------------- synthetic data
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Byte i of the region is byte (i % 8) of splitmix64(seed + (i / 8) * golden).
__global__ void __launch_bounds__(256) k_fill_random(uint8_t *dst, int64_t nbytes, uint64_t seed) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 16;
    for (int64_t off = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; off < nbytes; off += stride) {
        const uint64_t w0 = splitmix64(seed + (uint64_t)(off / 8) * 0x9E3779B97F4A7C15ull);
        const uint64_t w1 = splitmix64(seed + (uint64_t)(off / 8 + 1) * 0x9E3779B97F4A7C15ull);
        if (off + 16 <= nbytes && aligned16(dst + off)) {
            u32x4 v;
            v.x = (uint32_t)w0;
            v.y = (uint32_t)(w0 >> 32);
            v.z = (uint32_t)w1;
            v.w = (uint32_t)(w1 >> 32);
            store16(dst + off, v);
        } else {
            for (int b = 0; b < 16 && off + b < nbytes; ++b) dst[off + b] = (uint8_t)((b < 8 ? w0 : w1) >> (8 * (b & 7)));
        }
    }
}

void launch_fill_random(uint8_t *dst, int64_t nbytes, uint64_t seed, hipStream_t stream) {
    if (nbytes <= 0) return;
    const int64_t granules = (nbytes + 15) / 16;
    const unsigned blocks = (unsigned)std::min<int64_t>((granules + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(k_fill_random, dim3(blocks), dim3(256), 0, stream, dst, nbytes, seed);
    check_hip(hipGetLastError(), "k_fill_random launch");
}

// ---------------------------------------------------------------- bandwidth probes (diagnostics)
// Each workgroup streams a 16 KiB contiguous region: 4 x (256 lanes x 16 B).
template <bool NT>
__global__ void __launch_bounds__(256) k_probe_read(const uint8_t *src, int64_t nbytes, uint32_t *sink) {
    const int64_t base = (int64_t)blockIdx.x * 16384 + threadIdx.x * 16;
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ld16<NT>(src + base + k * 4096);
    u32x4 x = v[0] ^ v[1] ^ v[2] ^ v[3];
    uint32_t r = x.x ^ x.y ^ x.z ^ x.w;
    if (r == 0x9E3779B9u) atomicXor(sink, r);  // practically never taken; keeps the loads live
}

template <bool NT>
__global__ void __launch_bounds__(256) k_probe_copy(const uint8_t *src, uint8_t *dst, int64_t nbytes) {
    const int64_t base = (int64_t)blockIdx.x * 16384 + threadIdx.x * 16;
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ld16<NT>(src + base + k * 4096);
#pragma unroll
    for (int k = 0; k < 4; ++k) st16<NT>(dst + base + k * 4096, v[k]);
}

void launch_probe(int kind, const uint8_t *src, uint8_t *dst, int64_t nbytes, bool nt, hipStream_t stream) {
    const unsigned blocks = (unsigned)(nbytes / 16384);
    if (!blocks) return;
    if (kind == 0) {
        if (nt) hipLaunchKernelGGL(k_probe_read<true>, dim3(blocks), dim3(256), 0, stream, src, nbytes, (uint32_t *)dst);
        else hipLaunchKernelGGL(k_probe_read<false>, dim3(blocks), dim3(256), 0, stream, src, nbytes, (uint32_t *)dst);
    } else {
        if (nt) hipLaunchKernelGGL(k_probe_copy<true>, dim3(blocks), dim3(256), 0, stream, src, dst, nbytes);
        else hipLaunchKernelGGL(k_probe_copy<false>, dim3(blocks), dim3(256), 0, stream, src, dst, nbytes);
    }
    check_hip(hipGetLastError(), "probe launch");
}

// ---------------------------------------------------------------- verification
__global__ void __launch_bounds__(256) k_count_mismatch(const uint8_t *a, int64_t a_stride, const uint8_t *b,
                                                        int64_t b_stride, int64_t nrows, int64_t row_bytes,
                                                        uint64_t *count) {
    uint64_t n = 0;
    const int64_t total = nrows * row_bytes;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / row_bytes, c = i - r * row_bytes;
        n += a[r * a_stride + c] != (b ? b[r * b_stride + c] : 0);
    }
    for (int sh = 32; sh > 0; sh >>= 1) n += __shfl_xor(n, sh);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long *)count, (unsigned long long)n);
}

void launch_count_mismatch(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t nrows,
                           int64_t row_bytes, uint64_t *d_count, hipStream_t stream) {
    const int64_t total = nrows * row_bytes;
    if (total <= 0) return;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_count_mismatch, dim3(blocks), dim3(256), 0, stream, a, a_stride, b, b_stride, nrows, row_bytes,
                       d_count);
    check_hip(hipGetLastError(), "k_count_mismatch launch");
}

}  // namespace ecx
