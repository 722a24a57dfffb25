// apply_locate2.hip -- k_gf_locate2: which one or two shards, replaced together, make a stripe that
// fails ReedSolomon.isParityCorrect (ReedSolomon.java:129-178) pass again (include/ecx.h
// ecx_rs_locate_corrupt2_batch).  Codes with 4 <= m <= 8 and n <= 64.
//
// Stage one is k_gf_locate's (apply_locate.hip): the check's body (apply_check_body.inc) leaves the
// m syndromes of this lane's 16 bytes in registers, and a wave whose ballot of non-zero syndromes is
// empty leaves, having written nothing.  Stage two is one loop over the tiles of the code's locate
// plan followed by those of its pair plan (locate2_plan.hpp; one copy of the unrolled tile body):
//   two-a  the single-candidate tiles clear single suspects as k_gf_locate does and OR the candidate
//          of every row that is non-zero anywhere in the wave into a wave-uniform 64-bit mask;
//   two-b  where exactly one single candidate i survives, the wave evaluates no pair tile: any three
//          columns of the check matrix being independent (the plan's builder checked), the pairs
//          that explain the wave's bytes are exactly those that contain i, and the lanes stride
//          over the pair-member table and store 0 to every other pair suspect;
//   two-c  where none survives (or more than one, which non-zero syndromes never leave) the pair
//          tiles run exactly as the single ones did.
// launch_locate2 sets every suspect of the n + C(n,2)-byte rows to 1 first (k_set_suspects), so
// every writer stores the same 0 and the waves, chunks and blocks of a stripe combine without
// atomics.  k_fold_suspects2 then turns each row into two culprits and a heal id.  Every store is a
// plain vector store.
#include "apply.hpp"
#include "locate2.hpp"
#include "locate_launch.hpp"
#include "layout_probe.hpp"  // note_device_launch

namespace ecx {

Locate2Set::~Locate2Set() {
    for (auto &kv : dev_) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) continue;
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second.entries);
        (void)hipFree(kv.second.tiles);
        (void)hipFree(kv.second.members);
        (void)hipSetDevice(cur);
    }
}

const Locate2DevicePlan &Locate2Set::plan_for_current_device() {
    const char *what = "pair plan upload";
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(mu_);
    auto it = dev_.find(dev);
    if (it != dev_.end()) return it->second;
    refuse_if_capturing(what);
    Locate2DevicePlan p;
    auto upload = [what](auto **dst, const void *src, size_t bytes) {
        check_hip(hipMalloc(dst, bytes), what);
        check_hip(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice), what);
    };
    try {
        upload(&p.entries, plan_.entries.data(), plan_.entries.size() * 4);
        upload(&p.tiles, plan_.tiles.data(), plan_.tiles.size() * 4);
        upload(&p.members, plan_.members.data(), plan_.members.size());
    } catch (...) {  // a half-uploaded plan is never published
        (void)hipFree(p.entries);
        (void)hipFree(p.tiles);
        (void)hipFree(p.members);
        throw;
    }
    return dev_.emplace(dev, p).first->second;
}

// What stage two reads besides ApplyArgs: the locate plan (tiles [0, n_tiles1) of the loop), the
// pair plan (the n_tiles2 after them) and the pair-member table, on this device.
struct Locate2Args {
    const uint32_t *entries1;
    const uint32_t *tiles1;
    const uint32_t *entries2;
    const uint32_t *tiles2;
    const uint16_t *members;
    int n_tiles1, n_tiles2;
    int n, n_pairs;
};

#define ECX_LOCATE_BOUNDS(ROWS) (ROWS < kTileRows ? 5 : 4)

// Stage two, over stage one's acc[] (syndrome p in acc[p], p < nrows) and nz; `row` is the stripe's
// suspect row.  Included text like stage one, for the same reason.  `cleared` is the same in every
// lane: ballots and the plan's scalar loads.
#define ECX_LOCATE2_STAGE_TWO(row)                                                                       \
    if (!__builtin_amdgcn_ballot_w64(nz != 0)) return;                                                   \
    uint64_t cleared = 0;                                                                                \
    for (int t = 0; t < l2.n_tiles1 + l2.n_tiles2; ++t) {                                                \
        const bool pairs = t >= l2.n_tiles1;                                                             \
        if (t == l2.n_tiles1) {                                                                          \
            const uint64_t alive = ~cleared & (~(uint64_t)0 >> (64 - l2.n));                             \
            if (__builtin_popcountll(alive) == 1) { /* two-b */                                          \
                const uint32_t i = (uint32_t)__builtin_ctzll(alive);                                     \
                for (int p = (int)(threadIdx.x & 63); p < l2.n_pairs; p += 64) {                         \
                    const uint32_t ij = l2.members[p];                                                   \
                    if ((ij & 255u) != i && (ij >> 8) != i) (row)[l2.n + p] = 0;                          \
                }                                                                                        \
                return;                                                                                  \
            }                                                                                            \
        }                                                                                                \
        cu32 *lt = plan_ptr(pairs ? l2.tiles2 : l2.tiles1) + (pairs ? t - l2.n_tiles1 : t) * kTileDwords; \
        cu32 *le = plan_ptr(pairs ? l2.entries2 : l2.entries1) + (int64_t)lt[0] * kEntryDwords;          \
        u32x4 test[kTileRows];                                                                           \
        _Pragma("unroll") for (int r = 0; r < kTileRows; ++r) test[r] = (u32x4){0u, 0u, 0u, 0u};         \
        _Pragma("unroll") for (int p = 0; p < ROWS; ++p) if (p < nrows)                                  \
            apply_entry<false, kTileRows>(le + p * kEntryDwords, acc[p], test, nullptr);                 \
        const int nr = (int)lt[2];                                                                       \
        _Pragma("unroll") for (int r = 0; r < kTileRows; ++r) {                                          \
            if (r < nr) {                                                                                \
                const uint32_t z = test[r].x | test[r].y | test[r].z | test[r].w;                        \
                if (__builtin_amdgcn_ballot_w64(z != 0)) {                                               \
                    if (!pairs) cleared |= (uint64_t)1 << (lt[4 + r] & 63u);                             \
                    if ((threadIdx.x & 63) == 0) (row)[lt[4 + r]] = 0;                                   \
                }                                                                                        \
            }                                                                                            \
        }                                                                                                \
    }

#define ECX_CHECK_KEEP_SYNDROMES  // stage one ends with acc[] and nz in registers, no verdict store

template <bool SAFE, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_LOCATE_BOUNDS(ROWS)) k_gf_locate2(ApplyArgs a, Locate2Args l2) {
    constexpr int DEPTH = 4;
#include "apply_check_body.inc"
    gu8 *row = (gu8 *)(a.out + s * a.out_stripe_stride);
    ECX_LOCATE2_STAGE_TWO(row)
}

// Over one pass of a blocked batch, as k_gf_locate_blocked: the suspect row is that of stripe
// unit / divisor, formed only in a wave that found a mismatch.
template <bool SAFE, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_LOCATE_BOUNDS(ROWS)) k_gf_locate2_blocked(ApplyArgs a, Locate2Args l2,
                                                                                              VerdictDiv vd) {
    constexpr int DEPTH = 4;
#include "apply_check_body.inc"
    if (!__builtin_amdgcn_ballot_w64(nz != 0)) return;
    gu8 *row = (gu8 *)(a.out + (int64_t)verdict_quot(vd, __builtin_amdgcn_readfirstlane((uint32_t)(s - a.stripe_begin))) *
                                   a.out_stripe_stride);
    ECX_LOCATE2_STAGE_TWO(row)
}

#undef ECX_CHECK_KEEP_SYNDROMES

// culprit[s][0..1] and heal_id[s] (may be null) from suspect row s (locate2.hpp has the table).
__global__ void __launch_bounds__(256) k_fold_suspects2(const uint8_t *suspect, int n, int n_pairs, const uint16_t *members,
                                                        int32_t *culprit, uint8_t *heal_id, int64_t nstripes) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstripes) return;
    const uint8_t *row = suspect + s * (n + n_pairs);
    int singles = 0, first = -1, pairs = 0, first_pair = -1;
    for (int j = 0; j < n; ++j) {
        if (row[j]) {
            if (first < 0) first = j;
            ++singles;
        }
    }
    for (int p = 0; p < n_pairs; ++p) {
        if (row[n + p]) {
            if (first_pair < 0) first_pair = p;
            ++pairs;
        }
    }
    int32_t c0 = -2, c1 = -2;
    int heal = 255;
    if (singles == n) {
        c0 = c1 = -1;
    } else if (singles == 1) {
        c0 = first;
        c1 = -1;
        heal = first;
    } else if (singles == 0 && pairs == 1) {
        const uint32_t ij = members[first_pair];
        c0 = (int32_t)(ij & 255u);
        c1 = (int32_t)(ij >> 8);
        heal = n + first_pair;
    }
    culprit[2 * s] = c0;
    culprit[2 * s + 1] = c1;
    if (heal_id) heal_id[s] = (uint8_t)heal;
}

namespace {
template <bool SAFE, int R>
void launch_locate2_k(dim3 grid, hipStream_t stream, const ApplyArgs &a, const Locate2Args &l2, const VerdictDiv *vd) {
    if (vd) {
        if (!SAFE) note_kernel("k_gf_locate2_blocked", SAFE, R);
        hipLaunchKernelGGL((k_gf_locate2_blocked<SAFE, R>), grid, dim3(kBlockThreads), 0, stream, a, l2, *vd);
        return;
    }
    if (!SAFE) note_kernel("k_gf_locate2", SAFE, R);
    hipLaunchKernelGGL((k_gf_locate2<SAFE, R>), grid, dim3(kBlockThreads), 0, stream, a, l2);
}

// The passes of locate_launch.hpp with k_gf_locate2, over suspect rows of n + C(n,2) bytes.
void launch_locate2_core(CompiledMap &cm, const Locate2Args &l2, const uint8_t *in, int64_t in_stripe_stride,
                         int64_t in_slot_stride, uint8_t *suspect, int64_t nstripes, int64_t nbytes, hipStream_t stream,
                         int64_t divisor = 1) {
    launch_locate_passes(cm, l2.n + l2.n_pairs, in, in_stripe_stride, in_slot_stride, suspect, nstripes, nbytes, divisor,
                         "k_gf_locate2 launch",
                         [&](bool safe, int rows, dim3 grid, const ApplyArgs &a, const VerdictDiv *vd) {
                             if (safe) {
                                 if (rows == 4) launch_locate2_k<true, 4>(grid, stream, a, l2, vd);
                                 else launch_locate2_k<true, kTileRows>(grid, stream, a, l2, vd);
                             } else {
                                 if (rows == 4) launch_locate2_k<false, 4>(grid, stream, a, l2, vd);
                                 else launch_locate2_k<false, kTileRows>(grid, stream, a, l2, vd);
                             }
                         });
}

// The shape of the code, from the plans alone (what byte_count == 0 leaves of Locate2Args).
Locate2Args shape_of(LocateSet &ls, Locate2Set &l2) {
    const LocatePlan &lp = ls.plan();
    const Locate2Plan &pp = l2.plan();
    if (pp.k != lp.k || pp.m != lp.m) throw Error(ECX_E_ILLEGAL_ARGUMENT, "the pair plan is of another code than the locate plan");
    Locate2Args a{};
    a.n_tiles1 = lp.n_tiles;
    a.n_tiles2 = pp.n_tiles;
    a.n = pp.k + pp.m;
    a.n_pairs = pp.n_pairs;
    return a;
}

// The device state of a locate, resident before anything is enqueued: a first use refused on a
// capturing stream leaves no node behind.
void make_resident(CompiledMap &cm, LocateSet &ls, Locate2Set &l2, Locate2Args *a) {
    if (cm.n_tiles() != 1 || cm.map().n_out != a->n - l2.plan().k || cm.map().n_in != a->n)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "the pair plan is of another code than the check map");
    (void)cm.plan_for_current_device(4);
    (void)zero_page_for_current_device();
    const LocateDevicePlan &d1 = ls.plan_for_current_device();
    const Locate2DevicePlan &d2 = l2.plan_for_current_device();
    a->entries1 = d1.entries;
    a->tiles1 = d1.tiles;
    a->entries2 = d2.entries;
    a->tiles2 = d2.tiles;
    a->members = d2.members;
}

// The pair-member table is read by the fold whatever byte_count is: resident with the rest.
void fold_suspects2(const uint8_t *suspect, const Locate2Args &l2, const uint16_t *members, int32_t *culprit,
                    uint8_t *heal_id, int64_t nstripes, hipStream_t stream) {
    hipLaunchKernelGGL(k_fold_suspects2, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), 0, stream, suspect, l2.n,
                       l2.n_pairs, members, culprit, heal_id, nstripes);
    check_hip(hipGetLastError(), "k_fold_suspects2 launch");
}
}  // namespace

// A start that is not 16-B aligned on 16-B strides is split as launch_locate splits it.
void launch_locate2(CompiledMap &cm, LocateSet &ls, Locate2Set &l2s, const uint8_t *in, int64_t in_stripe_stride,
                    int64_t in_slot_stride, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id, int64_t nstripes,
                    int64_t nbytes, hipStream_t stream) {
    if (nstripes <= 0) return;
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    Locate2Args l2 = shape_of(ls, l2s);
    if (nbytes > 0) make_resident(cm, ls, l2s, &l2);
    const uint16_t *members = l2s.plan_for_current_device().members;
    set_suspects(suspect, nstripes, l2.n + l2.n_pairs, stream);
    if (nbytes > 0) {
        const int64_t head = (int64_t)((16 - (uintptr_t)in % 16) % 16);
        if (head > 0 && head < nbytes && in_stripe_stride % 16 == 0 && in_slot_stride % 16 == 0) {
            launch_locate2_core(cm, l2, in, in_stripe_stride, in_slot_stride, suspect, nstripes, head, stream);
            launch_locate2_core(cm, l2, in + head, in_stripe_stride, in_slot_stride, suspect, nstripes, nbytes - head,
                                stream);
        } else {
            launch_locate2_core(cm, l2, in, in_stripe_stride, in_slot_stride, suspect, nstripes, nbytes, stream);
        }
    }
    fold_suspects2(suspect, l2, members, culprit, heal_id, nstripes, stream);
    if (nbytes <= 0) return;
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, nstripes * nbytes * cm.map().n_in);
}

void launch_locate2_blocked(CompiledMap &cm, LocateSet &ls, Locate2Set &l2s, const uint8_t *base, int n,
                            int64_t nstripes, int64_t byte_count, int64_t block, uint8_t *suspect, int32_t *culprit,
                            uint8_t *heal_id, hipStream_t stream) {
    if (nstripes <= 0) return;
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    Locate2Args l2 = shape_of(ls, l2s);
    if (n != l2.n) throw Error(ECX_E_ILLEGAL_ARGUMENT, "the pair plan is of another code");
    BlockedPlan plan;
    if (byte_count > 0) {
        if (!blocked_plan(n, nstripes, byte_count, block, &plan))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "blocked batch extent overflows");
        make_resident(cm, ls, l2s, &l2);
    }
    const uint16_t *members = l2s.plan_for_current_device().members;
    set_suspects(suspect, nstripes, l2.n + l2.n_pairs, stream);
    for (int i = 0; i < plan.count; ++i) {
        const BlockedPass &p = plan.pass[i];
        launch_locate2_core(cm, l2, base + p.offset, p.stripe_stride, p.slot_bytes, suspect, p.units, p.slot_bytes,
                            stream, p.divisor);
    }
    fold_suspects2(suspect, l2, members, culprit, heal_id, nstripes, stream);
    if (plan.count == 0) return;
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, nstripes * byte_count * cm.map().n_in);
}

}  // namespace ecx
