// apply_check_body.inc -- the body of k_gf_check and k_gf_check_blocked (apply_check.hip), over
// the kernel's ApplyArgs `a`, and stage one of k_gf_locate and k_gf_locate_blocked (apply_locate.hip).
// ECX_CHECK_VERDICT(s) is the verdict index of stripe (unit) s.
// Included text, not a shared __device__ function: routed through one, the natural layout's
// instantiations came out with other register counts than before (two more VGPRs and one wave
// less per SIMD on <true, 4, 8>); as text they are instruction for instruction what they were.
    const uint32_t w = logical_block(a.xcd_group, (uint32_t)a.n_tiles, (uint32_t)a.xcd_run);
    const uint32_t tl = w % (uint32_t)a.n_tiles;
    const uint32_t rest = w / (uint32_t)a.n_tiles;
    const uint32_t nst = gridDim.x / ((uint32_t)a.n_tiles * (uint32_t)a.n_chunks);
    int64_t s, c;
    unit_of(rest, (uint32_t)a.n_chunks, nst, 0, (uint32_t)a.stagger, s, c);
    s += a.stripe_begin;
    c += a.chunk_begin;
    int64_t cbase = c * kChunkBytes;
    if (!SAFE && c == a.tail_chunk) cbase = a.nbytes - kChunkBytes;  // the shard's last full window
    const uint32_t lane16 = threadIdx.x * 16;
    int valid = 16;
    if (SAFE) {
        const int64_t v = a.nbytes - cbase - (int64_t)lane16;
        valid = v <= 0 ? 0 : (v >= 16 ? 16 : (int)v);
    }
    cu32 *tile = plan_ptr(a.tiles) + __builtin_amdgcn_readfirstlane(tl) * kTileDwords;
    const uint8_t *ib =
        reinterpret_cast<const uint8_t *>(uniform64((uint64_t)(a.in + s * a.in_stripe_stride + cbase))) + lane16;
    auto load = [&](uint32_t slot) -> u32x4 {  // padding entries read the zero page
        const uint8_t *p = slot == kDummySlot ? a.zero_page + lane16 : ib + (int64_t)slot * a.in_slot_stride;
        return SAFE ? load_partial(p, valid) : ld16<true>(p);
    };
    const int ecnt = (int)tile[1];  // padded to a multiple of DEPTH
    const int nrows = (int)tile[2];
    u32x4 acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = (u32x4){0u, 0u, 0u, 0u};
    cu32 *ent = plan_ptr(a.entries) + (int64_t)tile[0] * kEntryDwords;
    if (ecnt > 0) {
        u32x4 ring[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) ring[u] = load(ent[u * kEntryDwords]);
        const int last = ecnt - DEPTH;
        for (int e0 = 0; e0 < last; e0 += DEPTH) {
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                cu32 *r = ent + (int64_t)(e0 + u) * kEntryDwords;
                apply_entry<false, ROWS>(r, ring[u], acc, nullptr);
                ring[u] = load(r[DEPTH * kEntryDwords]);
            }
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
            apply_entry<false, ROWS>(ent + (int64_t)(last + u) * kEntryDwords, ring[u], acc, nullptr);
    }
    uint32_t nz = 0;
#pragma unroll
    for (int o = 0; o < ROWS; ++o)
        if (o < nrows) nz |= acc[o].x | acc[o].y | acc[o].z | acc[o].w;
#ifndef ECX_CHECK_KEEP_SYNDROMES  // (k_gf_locate, apply_locate.hip, goes on from acc[] and nz itself)
    // one vector byte store per wave that saw a mismatch (every writer stores the same 0)
    if (__builtin_amdgcn_ballot_w64(nz != 0) && (threadIdx.x & 63) == 0) {
        gu8 *v = (gu8 *)(a.out + ECX_CHECK_VERDICT(s) * a.out_stripe_stride);
        *v = 0;
    }
#endif
