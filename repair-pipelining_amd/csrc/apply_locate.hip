// apply_locate.hip -- k_gf_locate: which single shard, replaced alone, makes a stripe that fails
// ReedSolomon.isParityCorrect (ReedSolomon.java:129-178) pass again (include/ecx.h
// ecx_rs_locate_corrupt_batch).
//
// Stage one is the check's (apply_check_body.inc): the check map's plan, the depth-4 load ring,
// apply_entry's arithmetic and the shifted last window, leaving the m syndromes of this lane's 16
// bytes in registers.  A wave whose ballot of non-zero syndromes is empty leaves: a clean stripe
// costs what the check costs and writes nothing.  Otherwise stage two runs over the registers, no
// memory traffic but the plan's scalar loads: for each tile of the locate plan (locate_plan.hpp:
// exactly m entry records, record p the coefficients of syndrome p in the tile's test rows) a
// second accumulator set takes the m records -- a loop over p unrolled across the syndrome
// registers -- each test row is OR-folded and balloted, and lane 0 clears suspect[stripe][candidate
// of the row] for every row that is non-zero anywhere in the wave.  launch_locate sets every
// suspect to 1 first (k_set_suspects), so every writer stores the same 0, workgroups of different
// chunks of one stripe combine without atomics, and a shard stays a suspect exactly when its
// m - 1 rows are zero at every byte.  k_fold_suspects then turns each stripe's n suspects into its
// culprit and heal id.  Every store is a plain vector store.
#include "apply.hpp"
#include "locate.hpp"
#include "locate_launch.hpp"
#include "layout_probe.hpp"  // note_device_launch

#include <climits>

namespace ecx {

LocateSet::~LocateSet() {
    for (auto &kv : dev_) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) continue;
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second.entries);
        (void)hipFree(kv.second.tiles);
        (void)hipSetDevice(cur);
    }
}

const LocateDevicePlan &LocateSet::plan_for_current_device() {
    const char *what = "locate plan upload";
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(mu_);
    auto it = dev_.find(dev);
    if (it != dev_.end()) return it->second;
    refuse_if_capturing(what);
    LocateDevicePlan p;
    auto upload = [what](uint32_t **dst, const std::vector<uint32_t> &src) {
        check_hip(hipMalloc(dst, src.size() * 4), what);
        check_hip(hipMemcpy(*dst, src.data(), src.size() * 4, hipMemcpyHostToDevice), what);
    };
    try {
        upload(&p.entries, plan_.entries);
        upload(&p.tiles, plan_.tiles);
    } catch (...) {  // a half-uploaded plan is never published
        (void)hipFree(p.entries);
        (void)hipFree(p.tiles);
        throw;
    }
    return dev_.emplace(dev, p).first->second;
}

// What stage two reads besides ApplyArgs: the locate plan on this device.
struct LocateArgs {
    const uint32_t *entries;
    const uint32_t *tiles;
    int n_tiles;
};

#define ECX_LOCATE_BOUNDS(ROWS) (ROWS < kTileRows ? 5 : 4)

// Stage two, over stage one's acc[] (syndrome p in acc[p], p < nrows) and nz; `row` is the stripe's
// suspect row.  Included text like stage one, for the same reason.
#define ECX_LOCATE_STAGE_TWO(row)                                                                        \
    if (!__builtin_amdgcn_ballot_w64(nz != 0)) return;                                                   \
    for (int t = 0; t < la.n_tiles; ++t) {                                                               \
        cu32 *lt = plan_ptr(la.tiles) + t * kTileDwords;                                                 \
        cu32 *le = plan_ptr(la.entries) + (int64_t)lt[0] * kEntryDwords;                                 \
        u32x4 test[kTileRows];                                                                           \
        _Pragma("unroll") for (int r = 0; r < kTileRows; ++r) test[r] = (u32x4){0u, 0u, 0u, 0u};         \
        _Pragma("unroll") for (int p = 0; p < ROWS; ++p) if (p < nrows)                                  \
            apply_entry<false, kTileRows>(le + p * kEntryDwords, acc[p], test, nullptr);                 \
        const int nr = (int)lt[2];                                                                       \
        _Pragma("unroll") for (int r = 0; r < kTileRows; ++r) {                                          \
            if (r < nr) {                                                                                \
                const uint32_t z = test[r].x | test[r].y | test[r].z | test[r].w;                        \
                if (__builtin_amdgcn_ballot_w64(z != 0) && (threadIdx.x & 63) == 0) (row)[lt[4 + r]] = 0; \
            }                                                                                            \
        }                                                                                                \
    }

#define ECX_CHECK_KEEP_SYNDROMES  // stage one ends with acc[] and nz in registers, no verdict store

template <bool SAFE, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_LOCATE_BOUNDS(ROWS)) k_gf_locate(ApplyArgs a, LocateArgs la) {
    constexpr int DEPTH = 4;
#include "apply_check_body.inc"
    gu8 *row = (gu8 *)(a.out + s * a.out_stripe_stride);
    ECX_LOCATE_STAGE_TWO(row)
}

// Over one pass of a blocked batch: the launch's units are block rows, vd.divisor consecutive ones
// per caller stripe, and a failing test row clears a suspect of stripe unit / divisor, as
// k_gf_check_blocked clears that stripe's verdict (a.out is the suspect row of the launch's first
// unit's stripe).  The quotient is only formed in a wave that found a mismatch.
template <bool SAFE, int ROWS>
__global__ void __launch_bounds__(kBlockThreads, ECX_LOCATE_BOUNDS(ROWS)) k_gf_locate_blocked(ApplyArgs a, LocateArgs la,
                                                                                             VerdictDiv vd) {
    constexpr int DEPTH = 4;
#include "apply_check_body.inc"
    if (!__builtin_amdgcn_ballot_w64(nz != 0)) return;
    gu8 *row = (gu8 *)(a.out + (int64_t)verdict_quot(vd, __builtin_amdgcn_readfirstlane((uint32_t)(s - a.stripe_begin))) *
                                   a.out_stripe_stride);
    ECX_LOCATE_STAGE_TWO(row)
}

#undef ECX_CHECK_KEEP_SYNDROMES

// suspect[i] = 1 for all nstripes * n bytes, ahead of the passes.  A kernel, not hipMemsetAsync:
// a replayed memset node loses its value (apply_check.hip k_set_verdicts has the story).
__global__ void __launch_bounds__(256) k_set_suspects(uint8_t *suspect, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) suspect[i] = 1;
}

// culprit[s] and heal_id[s] (may be null) from the count and the first set index of suspect row s:
// n suspects -> -1 (clean), one -> its index, anything else -> -2; heal_id is the index or 255.
__global__ void __launch_bounds__(256) k_fold_suspects(const uint8_t *suspect, int n, int32_t *culprit, uint8_t *heal_id,
                                                       int64_t nstripes) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstripes) return;
    const uint8_t *row = suspect + s * n;
    int count = 0, first = -1;
    for (int j = 0; j < n; ++j) {
        if (row[j]) {
            if (first < 0) first = j;
            ++count;
        }
    }
    const int32_t c = count == n ? -1 : (count == 1 ? first : -2);
    culprit[s] = c;
    if (heal_id) heal_id[s] = c >= 0 ? (uint8_t)c : (uint8_t)255;
}

namespace {
template <bool SAFE, int R>
void launch_locate_k(dim3 grid, hipStream_t stream, const ApplyArgs &a, const LocateArgs &la, const VerdictDiv *vd) {
    if (vd) {
        if (!SAFE) note_kernel("k_gf_locate_blocked", SAFE, R);
        hipLaunchKernelGGL((k_gf_locate_blocked<SAFE, R>), grid, dim3(kBlockThreads), 0, stream, a, la, *vd);
        return;
    }
    if (!SAFE) note_kernel("k_gf_locate", SAFE, R);
    hipLaunchKernelGGL((k_gf_locate<SAFE, R>), grid, dim3(kBlockThreads), 0, stream, a, la);
}

// The passes of locate_launch.hpp with k_gf_locate: clears suspect[s / divisor][j] when a test row
// of candidate j over bytes [0, nbytes) of stripe (unit) s is non-zero.
void launch_locate_core(CompiledMap &cm, const LocateArgs &la, int n, const uint8_t *in, int64_t in_stripe_stride,
                        int64_t in_slot_stride, uint8_t *suspect, int64_t nstripes, int64_t nbytes, hipStream_t stream,
                        int64_t divisor = 1) {
    launch_locate_passes(cm, n, in, in_stripe_stride, in_slot_stride, suspect, nstripes, nbytes, divisor,
                         "k_gf_locate launch",
                         [&](bool safe, int rows, dim3 grid, const ApplyArgs &a, const VerdictDiv *vd) {
                             if (safe) {
                                 if (rows == 4) launch_locate_k<true, 4>(grid, stream, a, la, vd);
                                 else launch_locate_k<true, kTileRows>(grid, stream, a, la, vd);
                             } else {
                                 if (rows == 4) launch_locate_k<false, 4>(grid, stream, a, la, vd);
                                 else launch_locate_k<false, kTileRows>(grid, stream, a, la, vd);
                             }
                         });
}

// The device state of a locate, resident before anything is enqueued: a first use refused on a
// capturing stream leaves no node behind.
LocateArgs resident(CompiledMap &cm, LocateSet &ls) {
    const LocatePlan &lp = ls.plan();
    if (cm.n_tiles() != 1 || cm.map().n_out != lp.m || cm.map().n_in != lp.k + lp.m)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "the locate plan is of another code than the check map");
    (void)cm.plan_for_current_device(4);
    (void)zero_page_for_current_device();
    const LocateDevicePlan &dp = ls.plan_for_current_device();
    return LocateArgs{dp.entries, dp.tiles, lp.n_tiles};
}

void fold_suspects(const uint8_t *suspect, int n, int32_t *culprit, uint8_t *heal_id, int64_t nstripes,
                   hipStream_t stream) {
    hipLaunchKernelGGL(k_fold_suspects, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), 0, stream, suspect, n,
                       culprit, heal_id, nstripes);
    check_hip(hipGetLastError(), "k_fold_suspects launch");
}
}  // namespace

void set_suspects(uint8_t *suspect, int64_t nstripes, int n, hipStream_t stream) {
    const int64_t count = nstripes * n, blocks = (count + 255) / 256;
    if (blocks > INT_MAX) throw Error(ECX_E_ILLEGAL_ARGUMENT, "too many stripes for one locate");
    hipLaunchKernelGGL(k_set_suspects, dim3((unsigned)blocks), dim3(256), 0, stream, suspect, count);
    check_hip(hipGetLastError(), "k_set_suspects launch");
}

// A start that is not 16-B aligned on 16-B strides is split as launch_check splits it: the bytes up
// to the first 16-B boundary go to the byte-safe kernel, the rest to the vectorised one.
void launch_locate(CompiledMap &cm, LocateSet &ls, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                   uint8_t *suspect, int32_t *culprit, uint8_t *heal_id, int64_t nstripes, int64_t nbytes,
                   hipStream_t stream) {
    if (nstripes <= 0) return;
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    const int n = ls.plan().k + ls.plan().m;
    LocateArgs la{};
    if (nbytes > 0) la = resident(cm, ls);
    set_suspects(suspect, nstripes, n, stream);
    if (nbytes > 0) {
        const int64_t head = (int64_t)((16 - (uintptr_t)in % 16) % 16);
        if (head > 0 && head < nbytes && in_stripe_stride % 16 == 0 && in_slot_stride % 16 == 0) {
            launch_locate_core(cm, la, n, in, in_stripe_stride, in_slot_stride, suspect, nstripes, head, stream);
            launch_locate_core(cm, la, n, in + head, in_stripe_stride, in_slot_stride, suspect, nstripes, nbytes - head,
                               stream);
        } else {
            launch_locate_core(cm, la, n, in, in_stripe_stride, in_slot_stride, suspect, nstripes, nbytes, stream);
        }
    }
    fold_suspects(suspect, n, culprit, heal_id, nstripes, stream);
    if (nbytes <= 0) return;
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, nstripes * nbytes * cm.map().n_in);
}

void launch_locate_blocked(CompiledMap &cm, LocateSet &ls, const uint8_t *base, int n, int64_t nstripes,
                           int64_t byte_count, int64_t block, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id,
                           hipStream_t stream) {
    if (nstripes <= 0) return;
    const LaunchStreamScope scope(stream);  // first use of device state is refused under capture (engine.hpp)
    if (n != ls.plan().k + ls.plan().m) throw Error(ECX_E_ILLEGAL_ARGUMENT, "the locate plan is of another code");
    BlockedPlan plan;
    LocateArgs la{};
    if (byte_count > 0) {
        if (!blocked_plan(n, nstripes, byte_count, block, &plan))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "blocked batch extent overflows");
        la = resident(cm, ls);
    }
    set_suspects(suspect, nstripes, n, stream);
    for (int i = 0; i < plan.count; ++i) {
        const BlockedPass &p = plan.pass[i];
        launch_locate_core(cm, la, n, base + p.offset, p.stripe_stride, p.slot_bytes, suspect, p.units, p.slot_bytes,
                           stream, p.divisor);
    }
    fold_suspects(suspect, n, culprit, heal_id, nstripes, stream);
    if (plan.count == 0) return;
    int dev = 0;
    check_hip(hipGetDevice(&dev), "hipGetDevice");
    note_device_launch(dev, stream, nstripes * byte_count * cm.map().n_in);
}

}  // namespace ecx
