// apply_clay_check.hip -- k_clay_check: isParityCorrect for Clay stripes in one read-only launch.
//
// A stripe is a codeword exactly when, in every plane z, the decoupled symbols U(z, .) form a
// codeword of the plane code RS(k + v, m) (clay_check_plan.hpp ClayCheckProgram, proved against
// perform_coding_map before it may run).  One workgroup takes one (stripe, 4 KiB
// chunk, plane z), a lane 16 bytes, as in apply_check_body.inc.  It walks the underlying nodes
// j = (x, y) in node order with loads running DEPTH nodes ahead of use:
//   own      C(z, j): real slot z * n_real + real(j), or the zero page for a virtual node;
//   partner  C(z', j'), z' = z[y := x], j' = (zvec(z)[y], y), which may be virtual too; a dot
//            node (zvec(z)[y] == x) loads its own address again, an L1 hit;
//   decouple U = C' ^ 3 * (C ^ C')  (= 3 C ^ 2 C'; a dot gives U = C), 3 x = x ^ xtime(x) as SWAR
//            operations on a dword, no table;
//   fold     U into the m syndrome rows with apply_entry and the node's entry record.
// The coefficient columns do not depend on the plane, so the records are the n_under entries of
// the program's node map (ClayCheck::nodes), uploaded once per geometry and device; z, its
// digits and the partner's slot are scalar arithmetic on the workgroup's index, one division per
// grid row, all before the first load.  After the walk the first m rows are OR-folded, each wave
// ballots, and a wave that saw a non-zero byte stores 0 to verdict[s] (launch_clay_check sets
// every verdict to 1 first, with a kernel).
//
// Block order: the alpha planes of one (stripe, chunk) are consecutive logical blocks on one
// XCD (logical_block with n_tiles = alpha), so a plane's partner loads are its neighbours' own
// loads and meet them in that XCD's L2; every load is a plain cached load for that reason.
#include "apply.hpp"
#include "clay_check.hpp"
#include "layout_probe.hpp"  // note_device_launch

namespace ecx {

static_assert(kClayCheckMaxParity == kTileRows, "the check folds its syndromes into one accumulator tile");

struct ClayCheckArgs {
    const uint8_t *in;
    uint8_t *verdict;
    const uint32_t *entries;  // the node map's padded tile: n_under records, then zero-mask padding
    const uint32_t *tiles;
    const uint8_t *zero_page;
    int64_t stripe_stride, sub_stride, nbytes, chunk_begin, n_chunks, stripe_begin;
    int q, t, alpha, n_under, n_real, k_real, v;  // real data nodes [0, k_real), virtual [k_real, k_real + v)
    int wgt[16];                                  // q^(t-1-y): the weight of digit y of a plane index
    int xcd_group, xcd_run;
};

// 3 * x for four packed bytes (generating polynomial 29: xtime reduces by 0x1d).
__device__ __forceinline__ uint32_t gf_mul3_4(uint32_t x) {
    const uint32_t xt = ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1du);
    return x ^ xt;
}

#define ECX_CLAY_CHECK_BOUNDS(ROWS, DEPTH) (ROWS < kTileRows ? (DEPTH >= 8 ? 4 : 5) : (DEPTH >= 8 ? 3 : 4))

template <bool SAFE, int DEPTH, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_CLAY_CHECK_BOUNDS(ROWS, DEPTH)) k_clay_check(ClayCheckArgs a) {
    const uint32_t alpha = (uint32_t)a.alpha;
    const uint32_t w = logical_block(a.xcd_group, alpha, (uint32_t)a.xcd_run);
    const uint32_t z = __builtin_amdgcn_readfirstlane(w % alpha);
    const uint32_t rest = __builtin_amdgcn_readfirstlane(w / alpha);
    const int64_t s = (int64_t)(rest / (uint32_t)a.n_chunks) + a.stripe_begin;
    const int64_t c = (int64_t)(rest % (uint32_t)a.n_chunks) + a.chunk_begin;
    const int64_t cbase = c * kChunkBytes;
    const uint32_t lane16 = threadIdx.x * 16;
    int valid = 16;
    if (SAFE) {
        const int64_t vb = a.nbytes - cbase - (int64_t)lane16;
        valid = vb <= 0 ? 0 : (vb >= 16 ? 16 : (int)vb);
    }
    const uint8_t *sb =
        reinterpret_cast<const uint8_t *>(uniform64((uint64_t)(a.in + s * a.stripe_stride + cbase))) + lane16;
    const uint8_t *zp = a.zero_page + lane16;
    auto ld = [&](const uint8_t *p) -> u32x4 { return SAFE ? load_partial(p, valid) : ld16<false>(p); };
    // sub-chunk of underlying node u in plane zz; a virtual node reads zeros
    auto sub = [&](uint32_t zz, uint32_t u) -> const uint8_t * {
        const bool virt = u >= (uint32_t)a.k_real && u < (uint32_t)(a.k_real + a.v);
        const uint32_t real = u < (uint32_t)a.k_real ? u : u - (uint32_t)a.v;
        return virt ? zp : sb + (int64_t)(zz * (uint32_t)a.n_real + real) * a.sub_stride;
    };
    // The walk: node j = x + q * y is the next to be loaded.  The digits of z are split once, up
    // front (one division per grid row), and packed four bits each; the weight q^(t-1-y) of digit
    // y comes from the kernel arguments.  Everything here is wave-uniform, and issue() is
    // straight-line code -- selects, no branch -- so that the loads keep compile-time vmcnt counts.
    const uint32_t q = (uint32_t)a.q;
    uint64_t digits = 0;
    {
        uint32_t zr = z;
        for (int y = a.t - 1; y >= 0; --y) {
            const uint32_t nx = zr / q;
            digits |= (uint64_t)(zr - nx * q) << (4 * y);
            zr = nx;
        }
        digits = uniform64(digits);
    }
    uint32_t j = 0, x = 0, y = 0;
    auto issue = [&](u32x4 &own, u32x4 &par) {
        const bool pad = j >= (uint32_t)a.n_under;  // padding records: zero masks, zeros
        const uint32_t d = (uint32_t)(digits >> (4 * (y & 15))) & 15u;  // (y == t only while padding is issued)
        const uint32_t wgt = (uint32_t)a.wgt[y & 15];
        const bool dot = x == d;  // a dot node is its own partner
        // the partner (d, y) in plane z + (x - d) * wgt
        const uint8_t *po = sub(z, j);
        const uint8_t *pp = sub(dot ? z : z + (x - d) * wgt, dot ? j : j - x + d);
        own = ld(pad ? zp : po);
        par = ld(pad ? zp : pp);
        ++j;
        const bool wrap = !pad && x + 1 == q;
        x = wrap ? 0u : x + 1;
        y += wrap ? 1u : 0u;
    };
    auto decouple = [&](const u32x4 &own, const u32x4 &par) -> u32x4 {
        const u32x4 e = own ^ par;
        return (u32x4){par.x ^ gf_mul3_4(e.x), par.y ^ gf_mul3_4(e.y), par.z ^ gf_mul3_4(e.z), par.w ^ gf_mul3_4(e.w)};
    };
    cu32 *tile = plan_ptr(a.tiles);
    const int ecnt = (int)tile[1];  // padded to a multiple of DEPTH
    const int nrows = (int)tile[2];
    u32x4 acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = (u32x4){0u, 0u, 0u, 0u};
    cu32 *ent = plan_ptr(a.entries) + (int64_t)tile[0] * kEntryDwords;
    if (ecnt > 0) {
        u32x4 own[DEPTH], par[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) issue(own[u], par[u]);
        const int last = ecnt - DEPTH;
        for (int e0 = 0; e0 < last; e0 += DEPTH) {
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                apply_entry<false, ROWS>(ent + (int64_t)(e0 + u) * kEntryDwords, decouple(own[u], par[u]), acc, nullptr);
                issue(own[u], par[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
            apply_entry<false, ROWS>(ent + (int64_t)(last + u) * kEntryDwords, decouple(own[u], par[u]), acc, nullptr);
    }
    uint32_t nz = 0;
#pragma unroll
    for (int o = 0; o < ROWS; ++o)
        if (o < nrows) nz |= acc[o].x | acc[o].y | acc[o].z | acc[o].w;
    // one vector byte store per wave that saw a mismatch (every writer stores the same 0)
    if (__builtin_amdgcn_ballot_w64(nz != 0) && (threadIdx.x & 63) == 0) {
        gu8 *vp = (gu8 *)(a.verdict + s);
        *vp = 0;
    }
}

ClayCheck::ClayCheck(ClayCheckProgram pg) : pg_(std::move(pg)), nodes_(pg_.node_map()) {
    // the kernel hard-codes what it reads off the program: U = C' ^ 3 (C ^ C'), one tile, node order
    if (pg_.pair_a != 3 || pg_.pair_b != 2)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "Clay check: the kernel decouples with (pair_a, pair_b) = (3, 2) only");
    if (pg_.m > kTileRows || nodes_.n_tiles() != 1)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "Clay check: the syndromes do not fit one accumulator tile");
    // digits of a plane index are packed four bits each into 64, and read at positions 0 .. t
    if (pg_.t > 15 || pg_.q > 15) throw Error(ECX_E_ILLEGAL_ARGUMENT, "Clay check: grid beyond the kernel's packed digits");
    const HostPlan hp = nodes_.padded_plan(4);
    if ((int)hp.tiles[1] < pg_.n_under) throw Error(ECX_E_ILLEGAL_ARGUMENT, "Clay check: node records missing");
    for (int j = 0; j < pg_.n_under; ++j)
        if (hp.entries[(size_t)(hp.tiles[0] + j) * kEntryDwords] != (uint32_t)j)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "Clay check: node records out of node order");
}

// verdict[s] = 1 for every stripe, ahead of the check's launches: apply_check.hip's k_set_verdicts,
// restated here because that kernel is local to its unit.  A kernel, not hipMemsetAsync: a captured
// memset node replays with the value 0 from its second replay on.
__global__ void __launch_bounds__(256) k_clay_set_verdicts(uint8_t *verdict, int64_t nstripes) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nstripes) verdict[s] = 1;
}

namespace {
template <bool SAFE, int D, int R>
void launch_clay_check_k(dim3 grid, hipStream_t stream, const ClayCheckArgs &a) {
    if (!SAFE) note_kernel("k_clay_check", SAFE, D, R);
    hipLaunchKernelGGL((k_clay_check<SAFE, D, R>), grid, dim3(kBlockThreads), 0, stream, a);
}

// Ring depth 2 (forced 4 / 8 with ecx_tune "depth"): two (own, partner) pairs in flight and 49
// VGPRs, 8 waves per SIMD, measured faster than depth 4 on Clay(4,2) and level with it on
// Clay(10,4) (DESIGN.md section 4.9 has the sweep).  The byte-safe instance stays at 4.
int clay_check_depth(const Tuning &tu) { return tu.depth == 4 || tu.depth == 8 ? tu.depth : 2; }
}  // namespace

void launch_clay_check(ClayCheck &cc, const uint8_t *base, int64_t stripe_stride, int64_t sub_stride, uint8_t *verdict,
                       int64_t nstripes, int64_t buf_size, hipStream_t stream) {
    if (nstripes <= 0) return;
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    const ClayCheckProgram &pg = cc.program();
    const Tuning &tu = tuning();
    const int depth = clay_check_depth(tu);
    if (buf_size > 0) {
        // resident before anything is enqueued: a first use refused on a capturing stream leaves no node behind
        (void)cc.nodes().plan_for_current_device(depth);
        (void)cc.nodes().plan_for_current_device(4);
        (void)zero_page_for_current_device();
    }
    // one launch covers whole stripes: a stripe's workgroups must fit a grid (checked before anything is enqueued)
    if ((buf_size + kChunkBytes - 1) / kChunkBytes > (((int64_t)1 << 30) / pg.alpha))
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "Clay check: buf_size needs more than 2^30 workgroups per stripe");
    hipLaunchKernelGGL(k_clay_set_verdicts, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), 0, stream, verdict, nstripes);
    check_hip(hipGetLastError(), "k_clay_set_verdicts launch");
    if (buf_size <= 0) return;
    const DevicePlan &plan = cc.nodes().plan_for_current_device(depth);
    const DevicePlan &plan4 = depth == 4 ? plan : cc.nodes().plan_for_current_device(4);
    const int rows = pg.m <= 4 ? 4 : kTileRows;
    const bool aligned = aligned16(base) && stripe_stride % 16 == 0 && sub_stride % 16 == 0;
    const int64_t full = aligned ? buf_size / kChunkBytes : 0;
    const int64_t tail = buf_size - full * kChunkBytes;

    ClayCheckArgs a{};
    a.in = base;
    a.verdict = verdict;
    a.zero_page = zero_page_for_current_device();
    a.stripe_stride = stripe_stride;
    a.sub_stride = sub_stride;
    a.nbytes = buf_size;
    a.q = pg.q;
    a.t = pg.t;
    for (int y = pg.t - 1, w = 1; y >= 0; --y, w *= pg.q) a.wgt[y] = w;
    a.alpha = pg.alpha;
    a.n_under = pg.n_under;
    a.n_real = pg.n_real;
    a.k_real = pg.n_real - pg.m;
    a.v = pg.virtual_units;
    // the planes of a (stripe, chunk) on one XCD (ecx_tune "rtc_xcd" 0: dispatch order; "xcd_group"
    // 3: runs of "xcd_run" such units per XCD)
    a.xcd_group = tu.xcd_group == 3 ? 3 : (tu.rtc_xcd ? 2 : 0);
    a.xcd_run = tu.xcd_run;
    auto run = [&](bool safe, const DevicePlan &p, int64_t chunk_begin, int64_t n_chunks) {
        if (n_chunks <= 0) return;
        a.entries = p.entries;
        a.tiles = p.tiles;
        a.chunk_begin = chunk_begin;
        a.n_chunks = n_chunks;
        const int64_t per_stripe = n_chunks * pg.alpha;
        const int64_t stripes_per_launch = std::max<int64_t>(1, ((int64_t)1 << 30) / per_stripe);
        for (int64_t s0 = 0; s0 < nstripes; s0 += stripes_per_launch) {
            a.stripe_begin = s0;
            const dim3 grid((unsigned)(std::min(stripes_per_launch, nstripes - s0) * per_stripe));
            if (safe) {
                if (rows == 4) launch_clay_check_k<true, 4, 4>(grid, stream, a);
                else launch_clay_check_k<true, 4, kTileRows>(grid, stream, a);
            } else if (rows == 4) {
                if (depth == 8) launch_clay_check_k<false, 8, 4>(grid, stream, a);
                else if (depth == 2) launch_clay_check_k<false, 2, 4>(grid, stream, a);
                else launch_clay_check_k<false, 4, 4>(grid, stream, a);
            } else {
                if (depth == 8) launch_clay_check_k<false, 8, kTileRows>(grid, stream, a);
                else if (depth == 2) launch_clay_check_k<false, 2, kTileRows>(grid, stream, a);
                else launch_clay_check_k<false, 4, kTileRows>(grid, stream, a);
            }
        }
    };
    const uint64_t notes0 = kernel_notes();
    run(false, plan, 0, full);
    run(true, plan4, full, (tail + kChunkBytes - 1) / kChunkBytes);  // (not noted: byte-safe)
    if (kernel_notes() != notes0)
        set_last_shape_order("xcd_group=" + std::to_string(a.xcd_group) + " xcd_run=" + std::to_string(a.xcd_group == 3 ? a.xcd_run : 0));
    check_hip(hipGetLastError(), "k_clay_check launch");
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, nstripes * buf_size * (int64_t)pg.n_real * pg.alpha);
}

}  // namespace ecx
