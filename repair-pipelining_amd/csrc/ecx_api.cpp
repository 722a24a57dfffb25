// ecx_api.cpp -- the C ABI (include/ecx.h).  Translates planner/HIP errors into
// ecx_status codes; every arithmetic entry point executes on the HIP device.
// The exports get their C linkage from their declarations in ecx.h and ecx_tune.h: an entry point
// defined here without one there is not exported under its name.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>

#include "api_maps.hpp"
#include "blocked_layout.hpp"
#include "check_blocked.hpp"
#include "clay_check.hpp"
#include "clay_rtc.hpp"
#include "codec_cache.hpp"
#include "map_rtc.hpp"
#include "engine.hpp"
#include "host_pipe.hpp"
#include "layout_probe.hpp"  // note_device_launch
#include "locate.hpp"
#include "locate2.hpp"
#include "pattern_set.hpp"
#include "tune_table.hpp"
#include "../../include/ecx_tune.h"

using namespace ecx;

struct ecx_map {
    explicit ecx_map(LinearMap m) : cm(std::move(m)) {}
    CompiledMap cm;
};

// What one of a codec's maps was built for.
struct MapKey {
    enum What { encode, check, decode, decode_partial, encode_partial, coding, helper_plane, locate, locate2 };
    MapKey(What w, const std::vector<bool> &p = {}, int i = -1, int h = -1)
        : what(w), present(p.begin(), p.end()), index(i), helper(h) {}
    What what;
    std::vector<uint8_t> present;  // the pattern of a decode / coding map (bytes: compared at once)
    int index;                     // *_partial: the one input shard; helper_plane: the erased node
    int helper;                    // helper_plane: which
    bool operator<(const MapKey &o) const {
        return std::tie(what, present, index, helper) < std::tie(o.what, o.present, o.index, o.helper);
    }
};
using MapMemo = Memo<MapKey, ecx_map>;  // plans live as long as the codec
using LocateMemo = Memo<MapKey, LocateSet>;  // the locate plan (locate_plan.hpp), beside the check map
using Locate2Memo = Memo<MapKey, Locate2Set>;  // the pair plan (locate2_plan.hpp), beside the locate plan

struct ecx_rs {
    explicit ecx_rs(int k, int m) : code(k, m) {}
    RsCode code;
    MapMemo maps;
    LocateMemo locates;
    Locate2Memo locates2;
};

// A pattern set (ecx.h): the decode maps of its patterns as one device plan.  `rs` is a reference
// of the set's own on the codec whose maps it was built from.
struct ecx_rs_pattern_set {
    ecx_rs *rs = nullptr;
    std::unique_ptr<PatternSet> set;
    int npatterns = 0, max_missing = 0;
};

struct ecx_clay {
    ecx_clay(int k, int m, std::vector<int> e, int v = 0, bool is_test = false) : pl(k, m, std::move(e), v, is_test) {}
    ClayPlanner pl;
    MapMemo maps;
    std::mutex mu;  // of the rtc state
    // Single-node repair as the per-helper-plane kernel (clay_rtc.hpp), built on first use.
    std::unique_ptr<ClayRtc> rtc;
    int rtc_state = 0;  // 0 = not tried, 1 = available, -1 = not representable
    std::string rtc_why;
    // The geometry's codeword test (ecx_clay_is_parity_correct_batch) and its device records, proved on first use.
    std::unique_ptr<ClayCheck> check;
    int check_state = 0;  // 0 = not tried, 1 = proved, -1 = refused
    std::string check_why;
};

namespace {

thread_local std::string g_last_error;

// roctx ranges around the entry points (ecx_tune "roctx", or ECX_ROCTX=1 in the
// environment): `rocprofv3 --marker-trace` then shows which call issued which kernels.
// The marker library is opened on first use; without it the ranges are no-ops.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
};
const Roctx &roctx_lib() {
    static const Roctx r = [] {
        Roctx x;
        void *h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_LOCAL);
        if (h) {
            x.push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
            x.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (!x.push || !x.pop) x = Roctx{};
        }
        return x;
    }();
    return r;
}
std::atomic<int> g_roctx{[] {
    const char *e = std::getenv("ECX_ROCTX");
    return e && e[0] == '1' ? 1 : 0;
}()};

struct Range {
    const Roctx *lib = nullptr;
    explicit Range(const char *name) {
        if (g_roctx.load(std::memory_order_relaxed) && roctx_lib().push) {
            lib = &roctx_lib();
            lib->push(name);
        }
    }
    ~Range() {
        if (lib) lib->pop();
    }
};

template <class F>
int guarded(const char *name, F &&f) {
    Range range(name);
    try {
        return f();
    } catch (const Error &e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc &) {
        g_last_error = "out of memory";
        return ECX_E_NOMEM;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return ECX_E_ILLEGAL_ARGUMENT;
    }
}

// ReedSolomon.checkBuffersAndSizes, ReedSolomon.java:338-363.
void check_buffers(const RsCode &c, uint8_t *const *shards, int shard_count, int shard_length, int offset,
                   int byte_count) {
    if (shard_count != c.n()) throw Error(ECX_E_ILLEGAL_ARGUMENT, "wrong number of shards: " + std::to_string(shard_count));
    if (!shards) throw Error(ECX_E_NULL, "shards is null");
    for (int i = 0; i < shard_count; ++i)
        if (!shards[i]) throw Error(ECX_E_NULL, "shard " + std::to_string(i) + " is null");
    if (offset < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "offset is negative: " + std::to_string(offset));
    if (byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "byteCount is negative: " + std::to_string(byte_count));
    if ((long long)shard_length < (long long)offset + byte_count)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "buffers to small: " + std::to_string(byte_count) + std::to_string(offset));
}

// The CodingLoop entry points receive their matrix with every call: the reference
// passes the codec's parity rows or decode rows each time (ReedSolomon.java:105-107,
// :262-264).  Compiling a plan costs the planner, a device upload and, when the plan
// is dropped, a hipFree that synchronises the device, so plans are cached by the
// map's content (least recently used first out; ecx_tune "plan_cache" sets the size,
// 0 compiles every call).
std::shared_ptr<CompiledMap> cached_plan(LinearMap lm) {
    static LruCache<std::string, CompiledMap> plans;
    const size_t cap = (size_t)tuning().plan_cache;
    auto compile = [&] { return std::make_shared<CompiledMap>(std::move(lm)); };
    return cap == 0 ? compile() : plans.get(map_key(lm), cap, compile);  // (no cache, no key to build)
}

ecx_map *rs_decode_map(ecx_rs *rs, const std::vector<bool> &present) {
    return rs->maps.get({MapKey::decode, present}, [&] { return rs->code.decode_map(present); });
}

ecx_map *rs_check_plan(ecx_rs *rs) {
    return rs->maps.get({MapKey::check}, [&] { return rs_check_map(rs->code); });
}

// The locate plan of a codec (2 <= m <= 8), built once beside its check map.
LocateSet *rs_locate_plan(ecx_rs *rs) {
    return rs->locates.get({MapKey::locate}, [&] {
        const RsCode &c = rs->code;
        std::vector<uint8_t> parity;
        for (int p = 0; p < c.m(); ++p) parity.insert(parity.end(), c.parity_row(p), c.parity_row(p) + c.k());
        LocatePlan plan;
        if (!build_locate_plan(parity.data(), c.k(), c.m(), &plan))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "no locate plan for this code");
        return plan;
    });
}

// The pair plan of a codec (4 <= m <= 8, n <= 64), built once beside its locate plan.
Locate2Set *rs_locate2_plan(ecx_rs *rs) {
    return rs->locates2.get({MapKey::locate2}, [&] {
        const RsCode &c = rs->code;
        std::vector<uint8_t> parity;
        for (int p = 0; p < c.m(); ++p) parity.insert(parity.end(), c.parity_row(p), c.parity_row(p) + c.k());
        Locate2Plan plan;
        if (!build_locate2_plan(parity.data(), c.k(), c.m(), &plan))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "no pair plan for this code");
        return plan;
    });
}

// What both locate2 entry points refuse about the codec and the outputs it was asked for.
void check_locatable2(const ecx_rs *rs, const uint8_t *heal_id) {
    const int m = rs->code.m(), n = rs->code.n();
    if (m < kLocate2MinParity) throw Error(ECX_E_ILLEGAL_ARGUMENT, "locate2 needs m >= 4: two errors need 2 * 2 <= m");
    if (m > kLocateMaxParity)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "locate2 takes m <= " + std::to_string(kLocateMaxParity) + " (one check tile)");
    if (n > kLocate2MaxShards)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "locate2 takes n <= " + std::to_string(kLocate2MaxShards) + " (one 64-bit mask per wave)");
    if (heal_id && n + n * (n - 1) / 2 > 255)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "heal ids are bytes: n + C(n,2) must be <= 255 (n <= 22)");
}

// What both locate entry points refuse about the codec and the outputs it was asked for.
void check_locatable(const ecx_rs *rs, const uint8_t *heal_id) {
    const int m = rs->code.m();
    if (m < 2) throw Error(ECX_E_ILLEGAL_ARGUMENT, "locate needs m >= 2: with one syndrome every shard explains it");
    if (m > kLocateMaxParity)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "locate takes m <= " + std::to_string(kLocateMaxParity) + " (one check tile)");
    if (heal_id && rs->code.n() > 255) throw Error(ECX_E_ILLEGAL_ARGUMENT, "heal ids are bytes: n must be <= 255");
}

ecx_map *clay_coding_map(ecx_clay *c, const std::vector<bool> &present) {
    return c->maps.get({MapKey::coding, present}, [&] { return c->pl.perform_coding_map(present); });
}

ecx_map *clay_standard_map(ecx_clay *c) {
    const int n = c->pl.n_real(), a = c->pl.alpha();
    std::vector<bool> present((size_t)n * a, true);
    for (int z = 0; z < a; ++z)
        for (int e : c->pl.erased())
            if (e >= 0 && e < n) present[(size_t)z * n + e] = false;
    return clay_coding_map(c, present);
}

// Process-wide codec registries (codec_cache.hpp RefRegistry): equal codecs are one
// reference-counted object.  ecx_*_create takes a reference, ecx_*_destroy drops it.  A codec
// nobody references stays registered, idle, so that the next create of the same codec (the
// reference builds one per file or repair) finds its compiled plans and generated kernels; at most
// kCodecIdleMax idle codecs are kept, and an evicted codec frees its device state.  Past
// kCodecRegistryMax registered codecs, creates return private objects that destroy frees at once.
constexpr size_t kCodecRegistryMax = 4096;
constexpr size_t kCodecIdleMax = 64;

using RsRegistry = RefRegistry<ecx_rs, std::pair<int, int>>;
RsRegistry &rs_registry() {
    static RsRegistry r(kCodecRegistryMax, kCodecIdleMax);
    return r;
}
using ClayRegistry = RefRegistry<ecx_clay, std::tuple<int, int, int, std::vector<int>, int>>;
ClayRegistry &clay_registry() {
    static ClayRegistry r(kCodecRegistryMax, kCodecIdleMax);
    return r;
}
using ClayKey = std::tuple<int, int, int, std::vector<int>, int>;
}  // namespace

const char *ecx_status_string(int s) {
    switch (s) {
    case ECX_OK: return "ok";
    case ECX_E_ILLEGAL_ARGUMENT: return "IllegalArgumentException";
    case ECX_E_NOT_ENOUGH_SHARDS: return "Not enough shards present";
    case ECX_E_SINGULAR: return "Matrix is singular";
    case ECX_E_TOO_MANY_SHARDS: return "too many shards - max is 256";
    case ECX_E_INDEX: return "ArrayIndexOutOfBoundsException";
    case ECX_E_NULL: return "NullPointerException";
    case ECX_E_NOMEM: return "out of memory";
    case ECX_E_DEVICE: return "HIP device error";
    default: return "unknown status";
    }
}

const char *ecx_last_error(void) { return g_last_error.c_str(); }
int ecx_version(void) { return 110; }  // 1.10: 1.09 (1.08 + the two-shard locate) + the Clay codeword check

// ---------------------------------------------------------------- device
int ecx_device_count(int *count) {
    return guarded(__func__, [&]() -> int {
        int n = 0;
        check_hip(hipGetDeviceCount(&n), "hipGetDeviceCount");
        *count = n;
        return ECX_OK;
    });
}

int ecx_set_device(int device) {
    return guarded(__func__, [&]() -> int {
        check_hip(hipSetDevice(device), "hipSetDevice");
        return ECX_OK;
    });
}

int ecx_synchronize(void *stream) {
    return guarded(__func__, [&]() -> int {
        check_hip(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- Galois / Matrix
int ecx_gf_multiply(int a, int b) { return Field::get().mul((uint8_t)a, (uint8_t)b); }

int ecx_gf_divide(int a, int b) {
    return guarded(__func__, [&]() -> int { return (int)Field::get().div((uint8_t)a, (uint8_t)b); });
}

int ecx_gf_exp(int a, int n) {
    return guarded(__func__, [&]() -> int {
        if (n < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative exponent");
        return (int)Field::get().pow((uint8_t)a, n);
    });
}

int ecx_gf_tables(int16_t *log_table, uint8_t *exp_table, uint8_t *mul_table) {
    const Field &f = Field::get();
    if (log_table)
        for (int i = 0; i < 256; ++i) log_table[i] = f.log((uint8_t)i);
    if (exp_table)
        for (int i = 0; i < 510; ++i) exp_table[i] = f.exp(i);
    if (mul_table)
        for (int a = 0; a < 256; ++a) std::memcpy(mul_table + 256 * a, f.row((uint8_t)a), 256);
    return ECX_OK;
}

int ecx_matrix_times(const uint8_t *a, int ar, int ac, const uint8_t *b, int br, int bc, uint8_t *out) {
    return guarded(__func__, [&]() -> int {
        Matrix A(ar, ac), B(br, bc);
        std::memcpy(A.row(0), a, (size_t)ar * ac);
        std::memcpy(B.row(0), b, (size_t)br * bc);
        Matrix C = A * B;
        std::memcpy(out, C.row(0), (size_t)ar * bc);
        return ECX_OK;
    });
}

int ecx_matrix_invert(const uint8_t *m, int n, uint8_t *out) {
    return guarded(__func__, [&]() -> int {
        Matrix A(n, n);
        std::memcpy(A.row(0), m, (size_t)n * n);
        Matrix I = A.inverse();
        std::memcpy(out, I.row(0), (size_t)n * n);
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- CodingLoop
int ecx_code_some_shards(const uint8_t *matrix_rows, const uint8_t *const *inputs, int input_count,
                         uint8_t *const *outputs, int output_count, int offset, int byte_count) {
    return guarded(__func__, [&]() -> int {
        if (input_count <= 0 || output_count < 0 || offset < 0 || byte_count < 0)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "invalid counts");
        const std::shared_ptr<CompiledMap> cm = cached_plan(dense_map(matrix_rows, output_count, input_count).pruned());
        run_host(*cm, inputs, outputs, offset, byte_count);
        // Rows with every coefficient zero have no entries but are still written (as zeros) by the kernel.
        return ECX_OK;
    });
}

int ecx_check_some_shards(const uint8_t *matrix_rows, const uint8_t *const *inputs, int input_count,
                          const uint8_t *const *to_check, int check_count, int offset, int byte_count,
                          uint8_t *temp_buffer) {
    (void)temp_buffer;
    return guarded(__func__, [&]() -> int {
        if (input_count <= 0 || check_count < 0 || offset < 0 || byte_count < 0)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "invalid counts");
        // row o: sum_i M[o][i]*in[i] + 1*to_check[o] == 0  <=>  to_check[o] is correct
        std::vector<const uint8_t *> ptrs(inputs, inputs + input_count);
        ptrs.insert(ptrs.end(), to_check, to_check + check_count);
        const std::shared_ptr<CompiledMap> cm = cached_plan(check_map(matrix_rows, check_count, input_count));
        return run_host_all_zero(*cm, ptrs.data(), offset, byte_count) ? 1 : 0;
    });
}

int ecx_code_single(const uint8_t *matrix_rows, int row_length, const uint8_t *input, int index, uint8_t *output,
                    int output_index, int offset, int byte_count, int is_first_time) {
    return guarded(__func__, [&]() -> int {
        if (index < 0 || index >= row_length || output_index < 0) throw Error(ECX_E_INDEX, "matrix index");
        if (offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "invalid counts");
        const uint8_t c = matrix_rows[(size_t)output_index * row_length + index];
        if (host_exec_wanted(byte_count)) {  // below the per-call crossover: no plan, no device round trip
            if (!input || !output) throw Error(ECX_E_NULL, "null buffer");
            host_exec_scale(c, input + offset, output + offset, byte_count, !is_first_time);
            return ECX_OK;
        }
        const std::shared_ptr<CompiledMap> cm = cached_plan(scale_map(c, !is_first_time));
        const uint8_t *ins[2] = {input, output};
        uint8_t *outs[1] = {output};
        run_host(*cm, ins, outs, offset, byte_count);
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- ReedSolomon
// Codec objects are immutable after creation apart from their lock-protected plan caches,
// so equal codecs are one object: the reference builds a ReedSolomon (or a Clay decoding
// step) per file or repair (SampleEncoder.java:83, ClayCode.java:43-51), and sharing keeps
// the compiled, device-resident plans -- and the hiprtc-compiled Clay kernels -- of every
// earlier call instead of rebuilding them per object.  Shared codecs are reference-
// counted; up to kCodecIdleMax unreferenced ones stay cached (rs_registry above).
int ecx_rs_create(int data_shards, int parity_shards, ecx_rs **out) {
    return guarded(__func__, [&]() -> int {
        *out = nullptr;
        *out = rs_registry().get(std::make_pair(data_shards, parity_shards),
                                 [&] { return new ecx_rs(data_shards, parity_shards); });
        return ECX_OK;
    });
}

void ecx_rs_destroy(ecx_rs *rs) { rs_registry().release(rs); }

int ecx_rs_matrix(const ecx_rs *rs, uint8_t *out) {
    const Matrix &m = rs->code.matrix();
    std::memcpy(out, m.row(0), (size_t)m.rows() * m.cols());
    return ECX_OK;
}

int ecx_rs_shape(const ecx_rs *rs, int *data_shards, int *parity_shards) {
    if (!rs) return ECX_E_NULL;
    if (data_shards) *data_shards = rs->code.k();
    if (parity_shards) *parity_shards = rs->code.m();
    return ECX_OK;
}

int ecx_rs_encode_map(ecx_rs *rs, const ecx_map **out) {
    return guarded(__func__, [&]() -> int {
        *out = rs->maps.get({MapKey::encode}, [&] { return rs->code.encode_map(); });
        return ECX_OK;
    });
}

int ecx_rs_decode_map(ecx_rs *rs, const uint8_t *shard_present, const ecx_map **out) {
    return guarded(__func__, [&]() -> int {
        std::vector<bool> present = present_vec(shard_present, rs->code.n());
        const int np = (int)std::count(present.begin(), present.end(), true);
        if (np < rs->code.k()) throw Error(ECX_E_NOT_ENOUGH_SHARDS, "Not enough shards present");
        *out = rs_decode_map(rs, present);
        return ECX_OK;
    });
}

int ecx_rs_encode_parity_batch(ecx_rs *rs, uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                               int64_t nstripes, int64_t offset, int64_t byte_count, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!base) throw Error(ECX_E_NULL, "null device pointer");
        const ecx_map *m = nullptr;
        const int st = ecx_rs_encode_map(rs, &m);
        if (st) return st;
        launch_apply(const_cast<ecx_map *>(m)->cm, base + offset, stripe_stride, shard_stride, base + offset,
                     stripe_stride, shard_stride, nstripes, byte_count, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_decode_missing_batch(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base, int64_t stripe_stride,
                                int64_t shard_stride, int64_t nstripes, int64_t offset, int64_t byte_count,
                                void *stream) {
    return guarded(__func__, [&]() -> int {
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!base) throw Error(ECX_E_NULL, "null device pointer");
        const ecx_map *m = nullptr;
        const int st = ecx_rs_decode_map(rs, shard_present, &m);  // Not enough shards -> -2
        if (st) return st;
        if (m->cm.map().n_out == 0) return ECX_OK;  // all present (ReedSolomon.java:216-218)
        launch_apply(const_cast<ecx_map *>(m)->cm, base + offset, stripe_stride, shard_stride, base + offset,
                     stripe_stride, shard_stride, nstripes, byte_count, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_pattern_set_create(ecx_rs *rs, const uint8_t *patterns, int npatterns, ecx_rs_pattern_set **out) {
    return guarded(__func__, [&]() -> int {
        if (out) *out = nullptr;
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (!patterns || !out) throw Error(ECX_E_NULL, "null pattern list or out pointer");
        if (npatterns < 1 || npatterns > kMixedRecords)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern set holds 1..256 patterns: " + std::to_string(npatterns));
        const int n = rs->code.n(), k = rs->code.k(), m = rs->code.m();
        int max_missing = 0;
        for (int p = 0; p < npatterns; ++p) {
            int np = 0;
            for (int i = 0; i < n; ++i) np += patterns[(size_t)p * n + i] != 0;
            if (np < k) throw Error(ECX_E_NOT_ENOUGH_SHARDS, "Not enough shards present (pattern " + std::to_string(p) + ")");
            if (n - np > kTileRows)
                throw Error(ECX_E_ILLEGAL_ARGUMENT,
                            "pattern " + std::to_string(p) + " misses " + std::to_string(n - np) + " shards, a pattern set "
                            "takes at most " + std::to_string(kTileRows) + ": decode such stripes with "
                            "ecx_rs_decode_missing_batch, one pattern per call");
            max_missing = std::max(max_missing, n - np);
        }
        // the set's own reference: equal codecs are one object, so its maps are the codec's
        // (rs_decode_map: the first-k rule and parity-from-all-data stay the reference's)
        ecx_rs *own = rs_registry().get(std::make_pair(k, m), [&] { return new ecx_rs(k, m); });
        try {
            std::vector<const CompiledMap *> maps;
            for (int p = 0; p < npatterns; ++p)
                maps.push_back(&rs_decode_map(own, present_vec(patterns + (size_t)p * n, n))->cm);
            auto set = std::make_unique<ecx_rs_pattern_set>();
            set->set = std::make_unique<PatternSet>(maps);
            set->rs = own;
            set->npatterns = npatterns;
            set->max_missing = max_missing;
            *out = set.release();
        } catch (...) {
            rs_registry().release(own);
            throw;
        }
        return ECX_OK;
    });
}

void ecx_rs_pattern_set_destroy(ecx_rs_pattern_set *set) {
    if (!set) return;
    ecx_rs *rs = set->rs;
    delete set;  // the device plans first (hipFree), then the codec reference
    rs_registry().release(rs);
}

int ecx_rs_pattern_set_info(const ecx_rs_pattern_set *set, int *npatterns, int *shards, int *max_missing) {
    if (!set) return ECX_E_NULL;
    if (npatterns) *npatterns = set->npatterns;
    if (shards) *shards = set->rs->code.n();
    if (max_missing) *max_missing = set->max_missing;
    return ECX_OK;
}

int ecx_rs_decode_missing_batch_mixed(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                      uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                      int64_t nstripes, int64_t offset, int64_t byte_count, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!set) throw Error(ECX_E_NULL, "null pattern set");
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!base || !pattern_of_stripe) throw Error(ECX_E_NULL, "null device pointer");
        launch_apply_mixed(*set->set, pattern_of_stripe, base + offset, stripe_stride, shard_stride, nstripes,
                           byte_count, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_index_patterns(int shards, const uint8_t *present, int64_t nstripes, uint8_t *patterns, int cap,
                          int *npatterns, uint8_t *ids) {
    return guarded(__func__, [&]() -> int {
        if (!present || !patterns || !npatterns || !ids) throw Error(ECX_E_NULL, "null array");
        if (shards <= 0 || nstripes < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (cap < 1 || cap > kMixedRecords)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "cap is outside 1..256: " + std::to_string(cap));
        *npatterns = index_patterns(shards, present, nstripes, patterns, cap, ids);
        return ECX_OK;
    });
}

namespace {
// The blocked layout's block and its passes are blocked_layout.hpp's (no HIP header there: the
// plan is tested on the CPU); here its refusals become status codes.
int64_t resolve_block(int n, int64_t byte_count, int64_t block_bytes) {
    int64_t block = 0;
    if (!ecx::resolve_block(n, byte_count, block_bytes, &block))
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative block size");
    return block;
}

void blocked_plan_or_throw(int n, int64_t nstripes, int64_t byte_count, int64_t block, BlockedPlan *plan) {
    if (!blocked_plan(n, nstripes, byte_count, block, plan))
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "blocked batch extent overflows");
}

// Where a blocked encode / decode batch runs: on a stream over device memory, or from host memory
// as pipelined host batches (host_pipe.cpp), split over a device list where there is one.
struct BlockedTarget {
    bool host, multi;
    void *stream;
    const int *devices;
    int ndev;
};

// The one body of the six blocked encode / decode exports (ecx.h); tests/test_blocked_apply_cpu.py
// pins the order of its checks.  The two passes of the layout run in place: the full blocks as
// nstripes * full "stripes" of n block-sized slots, then the tails as nstripes stripes of n
// tail-sized slots.  From host memory each pass is a host batch of its own, the second after the
// first has drained (each is synchronous); with a device list each is split over the entries like
// any host batch: the full blocks as nstripes * full small stripes, the tails by stripes (by byte
// ranges where there are fewer stripes than entries).
int rs_apply_blocked(const char *fn, ecx_rs *rs, bool decode, const uint8_t *shard_present, uint8_t *base,
                     int64_t nstripes, int64_t byte_count, int64_t block_bytes, const BlockedTarget &to) {
    return guarded(fn, [&]() -> int {
        if (to.host && !rs) throw Error(ECX_E_NULL, "null codec");  // (the device forms do not look)
        if (to.multi && !to.devices) throw Error(ECX_E_NULL, "null device list");
        if (to.multi && to.ndev <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "empty device list");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        // a host batch of no stripes needs no buffer
        if (!base && !to.host) throw Error(ECX_E_NULL, "null device pointer");
        if (!base && nstripes > 0) throw Error(ECX_E_NULL, "null host pointer");
        const ecx_map *m = nullptr;
        const int st = decode ? ecx_rs_decode_map(rs, shard_present, &m)  // Not enough shards -> -2
                              : ecx_rs_encode_map(rs, &m);
        if (st) return st;
        CompiledMap &cm = const_cast<ecx_map *>(m)->cm;
        const int n = rs->code.n();
        const int64_t block = resolve_block(n, byte_count, block_bytes);
        if (decode && cm.map().n_out == 0) {  // all present (ReedSolomon.java:216-218): nothing to touch,
            if (!to.multi) return ECX_OK;
            nstripes = 0;  // but the device list is still checked
        }
        if (to.multi) check_device_list(to.devices, to.ndev);  // even for an empty batch
        BlockedPlan plan;
        blocked_plan_or_throw(n, nstripes, byte_count, block, &plan);
        for (int i = 0; i < plan.count; ++i) {
            const BlockedPass &p = plan.pass[i];
            uint8_t *at = base + p.offset;
            const int64_t ss = p.stripe_stride, len = p.slot_bytes;
            if (to.multi) run_host_batch_devices(cm, at, ss, len, at, ss, len, p.units, len, to.devices, to.ndev);
            else if (to.host) run_host_batch(cm, at, ss, len, at, ss, len, p.units, len);
            else launch_apply(cm, at, ss, len, at, ss, len, p.units, len, (hipStream_t)to.stream);
        }
        return ECX_OK;
    });
}
}  // namespace

int ecx_rs_blocked_layout(int data_shards, int parity_shards, int64_t byte_count, int64_t *layout) {
    return guarded(__func__, [&]() -> int {
        if (!layout) throw Error(ECX_E_NULL, "null layout");
        if (byte_count < 0 || data_shards <= 0 || parity_shards <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "bad shape");
        if (data_shards + parity_shards > 256) throw Error(ECX_E_TOO_MANY_SHARDS, "too many shards - max is 256");
        const int64_t b = recommended_block(data_shards + parity_shards, byte_count);
        layout[0] = b;
        layout[1] = b ? byte_count / b : 0;
        layout[2] = b ? byte_count % b : 0;
        return ECX_OK;
    });
}

int ecx_rs_recommended_pitch(int data_shards, int parity_shards, int64_t byte_count, int64_t *pitch) {
    return guarded(__func__, [&]() -> int {
        if (!pitch) throw Error(ECX_E_NULL, "null pitch");
        if (byte_count < 0 || data_shards <= 0 || parity_shards <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "bad shape");
        if (data_shards + parity_shards > 256) throw Error(ECX_E_TOO_MANY_SHARDS, "too many shards - max is 256");
        *pitch = recommended_pitch(byte_count);
        return ECX_OK;
    });
}

int ecx_rs_encode_parity_blocked_batch(ecx_rs *rs, uint8_t *base, int64_t nstripes, int64_t byte_count,
                                       int64_t block_bytes, void *stream) {
    return rs_apply_blocked(__func__, rs, false, nullptr, base, nstripes, byte_count, block_bytes,
                            {false, false, stream, nullptr, 0});
}

int ecx_rs_decode_missing_blocked_batch(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base, int64_t nstripes,
                                        int64_t byte_count, int64_t block_bytes, void *stream) {
    return rs_apply_blocked(__func__, rs, true, shard_present, base, nstripes, byte_count, block_bytes,
                            {false, false, stream, nullptr, 0});
}

int ecx_rs_encode_parity_blocked_batch_host(ecx_rs *rs, uint8_t *base, int64_t nstripes, int64_t byte_count,
                                            int64_t block_bytes) {
    return rs_apply_blocked(__func__, rs, false, nullptr, base, nstripes, byte_count, block_bytes,
                            {true, false, nullptr, nullptr, 0});
}

int ecx_rs_decode_missing_blocked_batch_host(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base,
                                             int64_t nstripes, int64_t byte_count, int64_t block_bytes) {
    return rs_apply_blocked(__func__, rs, true, shard_present, base, nstripes, byte_count, block_bytes,
                            {true, false, nullptr, nullptr, 0});
}

int ecx_rs_encode_parity_blocked_batch_host_devices(ecx_rs *rs, uint8_t *base, int64_t nstripes, int64_t byte_count,
                                                    int64_t block_bytes, const int *devices, int ndev) {
    return rs_apply_blocked(__func__, rs, false, nullptr, base, nstripes, byte_count, block_bytes,
                            {true, true, nullptr, devices, ndev});
}

int ecx_rs_decode_missing_blocked_batch_host_devices(ecx_rs *rs, const uint8_t *shard_present, uint8_t *base,
                                                     int64_t nstripes, int64_t byte_count, int64_t block_bytes,
                                                     const int *devices, int ndev) {
    return rs_apply_blocked(__func__, rs, true, shard_present, base, nstripes, byte_count, block_bytes,
                            {true, true, nullptr, devices, ndev});
}

namespace {
// The one body of the two blocked mixed decodes (ecx.h); tests/test_mixed_blocked_cpu.py pins the
// order of its checks.  Each pass of the layout is a mixed launch with the pass's divisor -- from
// host memory a pipelined host batch of its own, the ids on the device once for both.
int rs_mixed_blocked(const char *fn, const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe, uint8_t *base,
                     int64_t nstripes, int64_t byte_count, int64_t block_bytes, bool host, void *stream) {
    return guarded(fn, [&]() -> int {
        if (!set) throw Error(ECX_E_NULL, "null pattern set");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        // a host batch of no stripes needs no buffers
        if ((!base || !pattern_of_stripe) && (!host || nstripes > 0))
            throw Error(ECX_E_NULL, host ? "null host pointer" : "null device pointer");
        const int n = set->rs->code.n();
        const int64_t block = resolve_block(n, byte_count, block_bytes);
        BlockedPlan plan;
        blocked_plan_or_throw(n, nstripes, byte_count, block, &plan);
        if (plan.count == 0 || set->set->max_rows() == 0) return ECX_OK;  // no bytes, or nothing missing anywhere
        if (!host) {
            launch_apply_mixed_blocked(*set->set, pattern_of_stripe, base, plan, (hipStream_t)stream);
            return ECX_OK;
        }
        const HostMixedIds ids(pattern_of_stripe, nstripes);
        for (int i = 0; i < plan.count; ++i) {
            const BlockedPass &p = plan.pass[i];
            run_host_mixed_batch(*set->set, ids.get(), base + p.offset, p.stripe_stride, p.slot_bytes, n, p.units,
                                 p.slot_bytes, p.divisor);
        }
        return ECX_OK;
    });
}
}  // namespace

int ecx_rs_decode_missing_blocked_batch_mixed(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                              uint8_t *base, int64_t nstripes, int64_t byte_count,
                                              int64_t block_bytes, void *stream) {
    return rs_mixed_blocked(__func__, set, pattern_of_stripe, base, nstripes, byte_count, block_bytes, false, stream);
}

int ecx_rs_decode_missing_blocked_mixed_batch_host(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                                   uint8_t *base, int64_t nstripes, int64_t byte_count,
                                                   int64_t block_bytes) {
    return rs_mixed_blocked(__func__, set, pattern_of_stripe, base, nstripes, byte_count, block_bytes, true, nullptr);
}

int ecx_rs_decode_missing_mixed_batch_host(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                           uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                           int64_t nstripes, int64_t offset, int64_t byte_count) {
    return guarded(__func__, [&]() -> int {
        if (!set) throw Error(ECX_E_NULL, "null pattern set");
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if ((!base || !pattern_of_stripe) && nstripes > 0) throw Error(ECX_E_NULL, "null host pointer");
        if (nstripes == 0 || byte_count == 0 || set->set->max_rows() == 0) return ECX_OK;
        if (stripe_stride < 0 || shard_stride < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative stride");
        const HostMixedIds ids(pattern_of_stripe, nstripes);
        run_host_mixed_batch(*set->set, ids.get(), base + offset, stripe_stride, shard_stride, set->rs->code.n(),
                             nstripes, byte_count, 1);
        return ECX_OK;
    });
}

int ecx_rs_encode_parity(ecx_rs *rs, uint8_t *const *shards, int shard_count, int shard_length, int offset,
                         int byte_count) {
    return guarded(__func__, [&]() -> int {
        check_buffers(rs->code, shards, shard_count, shard_length, offset, byte_count);
        const ecx_map *m = nullptr;
        int st = ecx_rs_encode_map(rs, &m);
        if (st) return st;
        run_host(const_cast<ecx_map *>(m)->cm, shards, shards, offset, byte_count);
        return ECX_OK;
    });
}

int ecx_rs_encode_parity_single(ecx_rs *rs, const uint8_t *shard, uint8_t *output, int input_index,
                                int output_index, int offset, int byte_count) {
    return guarded(__func__, [&]() -> int {
        const RsCode &c = rs->code;
        if (output_index < 0 || output_index >= c.m() || input_index < 0 || input_index >= c.k())
            throw Error(ECX_E_INDEX, "parity row / column index");
        if (offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "invalid counts");
        if (host_exec_wanted(byte_count)) {  // below the per-call crossover: no plan, no device round trip
            if (!shard || !output) throw Error(ECX_E_NULL, "null buffer");
            host_exec_scale(c.parity_row(output_index)[input_index], shard + offset, output + offset, byte_count, true);
            return ECX_OK;
        }
        const std::shared_ptr<CompiledMap> cm = cached_plan(scale_map(c.parity_row(output_index)[input_index], true));
        const uint8_t *ins[2] = {shard, output};
        uint8_t *outs[1] = {output};
        run_host(*cm, ins, outs, offset, byte_count);
        return ECX_OK;
    });
}

int ecx_rs_is_parity_correct(ecx_rs *rs, uint8_t *const *shards, int shard_count, int shard_length, int first_byte,
                             int byte_count, uint8_t *temp_buffer, int temp_length) {
    return guarded(__func__, [&]() -> int {
        check_buffers(rs->code, shards, shard_count, shard_length, first_byte, byte_count);
        if (temp_buffer && (long long)temp_length < (long long)first_byte + byte_count)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "tempBuffer is not big enough");
        return run_host_all_zero(rs_check_plan(rs)->cm, shards, first_byte, byte_count) ? 1 : 0;
    });
}

int ecx_rs_is_parity_correct_batch(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                   int64_t nstripes, int64_t offset, int64_t byte_count, uint8_t *verdict,
                                   void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (nstripes == 0) return ECX_OK;
        if (!base || !verdict) throw Error(ECX_E_NULL, "null device pointer");
        launch_check(rs_check_plan(rs)->cm, base + offset, stripe_stride, shard_stride, verdict, nstripes, byte_count,
                     (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_locate_corrupt_batch(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                int64_t nstripes, int64_t offset, int64_t byte_count, uint8_t *suspect,
                                int32_t *culprit, uint8_t *heal_id, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        check_locatable(rs, heal_id);
        if (nstripes == 0) return ECX_OK;
        if (!base || !suspect || !culprit) throw Error(ECX_E_NULL, "null device pointer");
        launch_locate(rs_check_plan(rs)->cm, *rs_locate_plan(rs), base + offset, stripe_stride, shard_stride, suspect,
                      culprit, heal_id, nstripes, byte_count, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_locate_corrupt2_batch(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                                 int64_t nstripes, int64_t offset, int64_t byte_count, uint8_t *suspect,
                                 int32_t *culprit, uint8_t *heal_id, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        check_locatable2(rs, heal_id);
        if (nstripes == 0) return ECX_OK;
        if (!base || !suspect || !culprit) throw Error(ECX_E_NULL, "null device pointer");
        launch_locate2(rs_check_plan(rs)->cm, *rs_locate_plan(rs), *rs_locate2_plan(rs), base + offset, stripe_stride,
                       shard_stride, suspect, culprit, heal_id, nstripes, byte_count, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_decode_missing(ecx_rs *rs, uint8_t *const *shards, const uint8_t *shard_present, int shard_count,
                          int shard_length, int offset, int byte_count) {
    return guarded(__func__, [&]() -> int {
        check_buffers(rs->code, shards, shard_count, shard_length, offset, byte_count);
        std::vector<bool> present = present_vec(shard_present, rs->code.n());
        const int np = (int)std::count(present.begin(), present.end(), true);
        if (np == rs->code.n()) return ECX_OK;
        if (np < rs->code.k()) throw Error(ECX_E_NOT_ENOUGH_SHARDS, "Not enough shards present");
        ecx_map *m = rs_decode_map(rs, present);
        run_host(m->cm, shards, shards, offset, byte_count);
        return ECX_OK;
    });
}

int ecx_rs_decode_missing_single(ecx_rs *rs, const uint8_t *shard, int shard_index, int index,
                                 const uint8_t *shard_present, uint8_t *const *outputs, int output_count, int offset,
                                 int byte_count, int is_first) {
    (void)shard_index;
    return guarded(__func__, [&]() -> int {
        const RsCode &c = rs->code;
        // row j: out_j (=|^=) D^-1[missing_j][index] * shard; its refusals come first
        LinearMap lm = decode_single_map(c, present_vec(shard_present, c.n()), index, output_count, is_first != 0);
        if (offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "invalid counts");
        if (lm.n_out == 0) return ECX_OK;
        std::vector<const uint8_t *> ins(1, shard);
        ins.insert(ins.end(), outputs, outputs + output_count);
        const std::shared_ptr<CompiledMap> cm = cached_plan(std::move(lm));
        run_host(*cm, ins.data(), outputs, offset, byte_count);
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- maps
int ecx_map_create(const uint8_t *matrix, int n_out, int n_in, const int *in_slot, const int *out_slot,
                   ecx_map **out) {
    return guarded(__func__, [&]() -> int {
        *out = nullptr;
        if (n_out < 0 || n_in <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "map shape");
        LinearMap lm = dense_map(matrix, n_out, n_in);
        if (in_slot) lm.in_slot.assign(in_slot, in_slot + n_in);
        if (out_slot) lm.out_slot.assign(out_slot, out_slot + n_out);
        for (int s : lm.in_slot)
            if (s < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative slot");
        for (int s : lm.out_slot)
            if (s < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative slot");
        *out = new ecx_map(lm.pruned());
        return ECX_OK;
    });
}

void ecx_map_destroy(ecx_map *map) { delete map; }

int ecx_map_info(const ecx_map *map, int *n_out, int *n_in, int *nnz) {
    const LinearMap &m = map->cm.map();
    if (n_out) *n_out = m.n_out;
    if (n_in) *n_in = m.n_in;
    if (nnz) *nnz = m.nnz();
    return ECX_OK;
}

int ecx_map_matrix(const ecx_map *map, uint8_t *matrix, int *in_slot, int *out_slot) {
    const LinearMap &m = map->cm.map();
    if (matrix) std::memcpy(matrix, m.a.data(), m.a.size());
    if (in_slot) std::copy(m.in_slot.begin(), m.in_slot.end(), in_slot);
    if (out_slot) std::copy(m.out_slot.begin(), m.out_slot.end(), out_slot);
    return ECX_OK;
}

int ecx_map_slot_extent(const ecx_map *map, int *max_in_slot, int *max_out_slot) {
    return guarded(__func__, [&]() -> int {
        if (!map) throw Error(ECX_E_NULL, "null map");
        const LinearMap &m = map->cm.map();
        int mi = -1, mo = -1;
        for (int s : m.in_slot) mi = std::max(mi, s);
        for (int s : m.out_slot) mo = std::max(mo, s);
        if (max_in_slot) *max_in_slot = mi;
        if (max_out_slot) *max_out_slot = mo;
        return ECX_OK;
    });
}

int ecx_map_apply_batch(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                        uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                        int64_t byte_count, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!in || !out) throw Error(ECX_E_NULL, "null device pointer");
        launch_apply(const_cast<ecx_map *>(map)->cm, in, in_stripe_stride, in_slot_stride, out, out_stripe_stride,
                     out_slot_stride, nstripes, byte_count, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_map_accumulate_batch(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                             uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                             int64_t byte_count, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!in || !out) throw Error(ECX_E_NULL, "null device pointer");
        launch_apply(const_cast<ecx_map *>(map)->cm, in, in_stripe_stride, in_slot_stride, out, out_stripe_stride,
                     out_slot_stride, nstripes, byte_count, (hipStream_t)stream, true);
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- batched partial sums
int ecx_rs_decode_partial_batch(ecx_rs *rs, const uint8_t *shard_present, int shard_index, const uint8_t *in,
                                int64_t in_stripe_stride, uint8_t *acc, int64_t acc_stripe_stride,
                                int64_t acc_row_stride, int64_t nstripes, int64_t byte_count, int is_first,
                                void *stream) {
    return guarded(__func__, [&]() -> int {
        const RsCode &c = rs->code;
        if (shard_index < 0 || shard_index >= c.n()) throw Error(ECX_E_INDEX, "shard index");
        std::vector<bool> present = present_vec(shard_present, c.n());
        const int np = (int)std::count(present.begin(), present.end(), true);
        if (np < c.k()) throw Error(ECX_E_NOT_ENOUGH_SHARDS, "Not enough shards present");
        if (np == c.n()) return ECX_OK;
        ecx_map *full = rs_decode_map(rs, present);  // rows: the missing shards, data AND parity
        ecx_map *part = rs->maps.get({MapKey::decode_partial, present, shard_index},
                                     [&] { return single_input_map(full->cm.map(), shard_index); });
        launch_apply(part->cm, in, in_stripe_stride, 0, acc, acc_stripe_stride, acc_row_stride, nstripes, byte_count,
                     (hipStream_t)stream, !is_first);
        return ECX_OK;
    });
}

// tests/test_partial_mixed_cpu.py pins the order of the checks.
int ecx_rs_decode_partial_batch_mixed(const ecx_rs_pattern_set *set, const uint8_t *pattern_of_stripe,
                                      const uint8_t *shard_of_stripe, const uint8_t *in, int64_t in_stripe_stride,
                                      int64_t in_shard_stride, uint8_t *acc, int64_t acc_stripe_stride,
                                      int64_t acc_row_stride, int64_t nstripes, int64_t byte_count, int is_first,
                                      void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!set) throw Error(ECX_E_NULL, "null pattern set");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (nstripes == 0 || byte_count == 0 || set->max_missing == 0) return ECX_OK;
        if (!pattern_of_stripe || !shard_of_stripe || !in || !acc) throw Error(ECX_E_NULL, "null device pointer");
        const int n = set->rs->code.n();
        if (!extent_fits({{nstripes, in_stripe_stride}, {n, in_shard_stride}}, byte_count) ||
            !extent_fits({{nstripes, acc_stripe_stride}, {set->max_missing, acc_row_stride}}, byte_count))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative stride, or the batch's extent is beyond int64_t");
        launch_partial_mixed(*set->set, n, pattern_of_stripe, shard_of_stripe, in, in_stripe_stride, in_shard_stride, acc,
                             acc_stripe_stride, acc_row_stride, nstripes, byte_count, is_first != 0, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_encode_partial_batch(ecx_rs *rs, int input_index, const uint8_t *in, int64_t in_stripe_stride,
                                uint8_t *acc, int64_t acc_stripe_stride, int64_t acc_row_stride, int64_t nstripes,
                                int64_t byte_count, int is_first, void *stream) {
    return guarded(__func__, [&]() -> int {
        const RsCode &c = rs->code;
        if (input_index < 0 || input_index >= c.k()) throw Error(ECX_E_INDEX, "data shard index");
        ecx_map *part = rs->maps.get({MapKey::encode_partial, {}, input_index},
                                     [&] { return encode_partial_map(c, input_index); });
        launch_apply(part->cm, in, in_stripe_stride, 0, acc, acc_stripe_stride, acc_row_stride, nstripes, byte_count,
                     (hipStream_t)stream, !is_first);
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- Clay
int ecx_clay_create(int data_units, int parity_units, const int *erased, int n_erased, ecx_clay **out) {
    return ecx_clay_create_shortened(data_units, parity_units, 0, erased, n_erased, out);
}

int ecx_clay_create_shortened(int data_units, int parity_units, int virtual_units, const int *erased, int n_erased,
                              ecx_clay **out) {
    return ecx_clay_create_ex(data_units, parity_units, virtual_units, erased, n_erased, 0, out);
}

int ecx_clay_create_ex(int data_units, int parity_units, int virtual_units, const int *erased, int n_erased, int flags,
                       ecx_clay **out) {
    return guarded(__func__, [&]() -> int {
        if (!out) throw Error(ECX_E_NULL, "null out");
        *out = nullptr;
        if (n_erased < 0 || virtual_units < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "n_erased / virtual_units");
        if (flags & ~ECX_CLAY_IS_TEST) throw Error(ECX_E_ILLEGAL_ARGUMENT, "unknown Clay flags");
        if (n_erased > 0 && !erased) throw Error(ECX_E_NULL, "null erased list");
        const std::vector<int> e(erased, erased + n_erased);  // order matters (the reference's erasedIndexes)
        const bool is_test = (flags & ECX_CLAY_IS_TEST) != 0;
        *out = clay_registry().get(std::make_tuple(data_units, parity_units, virtual_units, e, flags),
                                   [&] { return new ecx_clay(data_units, parity_units, e, virtual_units, is_test); });
        return ECX_OK;
    });
}

void ecx_clay_destroy(ecx_clay *clay) { clay_registry().release(clay); }

int ecx_codec_stats(int *rs_live, int *rs_idle, int *clay_live, int *clay_idle) {
    rs_registry().stats(rs_live, rs_idle);
    clay_registry().stats(clay_live, clay_idle);
    return ECX_OK;
}

int ecx_clay_geometry(const ecx_clay *clay, int *q, int *t, int *alpha) {
    if (q) *q = clay->pl.q();
    if (t) *t = clay->pl.t();
    if (alpha) *alpha = clay->pl.alpha();
    return ECX_OK;
}

int ecx_clay_shape(const ecx_clay *clay, int *nodes, int *n_erased, int *alpha) {
    if (!clay) return ECX_E_NULL;
    if (nodes) *nodes = clay->pl.n_real();
    if (n_erased) *n_erased = (int)clay->pl.erased().size();
    if (alpha) *alpha = clay->pl.alpha();
    return ECX_OK;
}

int ecx_clay_helper_planes(const ecx_clay *clay, int erased_index, int *out) {
    return guarded(__func__, [&]() -> int {
        std::vector<int> h = clay->pl.helper_planes(erased_index);
        std::copy(h.begin(), h.end(), out);
        return (int)h.size();
    });
}

int ecx_clay_perform_coding(ecx_clay *clay, const uint8_t *const *inputs, uint8_t *const *outputs, int buf_size) {
    return guarded(__func__, [&]() -> int {
        if (clay->pl.erased().empty()) return ECX_OK;
        if (buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "buf_size");
        const int w = clay->pl.n_real() * clay->pl.alpha();
        std::vector<bool> present(w);
        for (int j = 0; j < w; ++j) present[j] = inputs[j] != nullptr;
        run_host(clay_coding_map(clay, present)->cm, inputs, outputs, 0, buf_size);
        return ECX_OK;
    });
}

int ecx_clay_decode_single_helper(ecx_clay *clay, const uint8_t *const *helper_coupled, int helper_i,
                                  uint8_t *const *outputs, int erased_index, int buf_size) {
    return guarded(__func__, [&]() -> int {
        if (buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "buf_size");
        const int nh = (int)clay->pl.helper_planes(erased_index).size();
        const int w = nh * clay->pl.n_real();
        std::vector<bool> present(w);
        for (int j = 0; j < w; ++j) present[j] = helper_coupled[j] != nullptr;
        ecx_map *m = clay->maps.get({MapKey::helper_plane, present, erased_index, helper_i}, [&] {
            return clay->pl.decode_single_helper_map(present, helper_i, erased_index, nullptr);
        });
        run_host(m->cm, helper_coupled, outputs, 0, buf_size);
        return ECX_OK;
    });
}

int ecx_clay_map(ecx_clay *clay, const ecx_map **out) {
    return guarded(__func__, [&]() -> int {
        *out = clay_standard_map(clay);
        return ECX_OK;
    });
}

namespace {
// The per-helper-plane repair kernel of a single-erasure step, or nullptr when the
// step's repair has no such program (ClayPlanner::repair_program throws; the reason is
// kept for ecx_clay_rtc_compile_check).
ClayRtc *clay_rtc(ecx_clay *clay) {
    std::lock_guard<std::mutex> lk(clay->mu);
    if (clay->rtc_state == 0) {
        try {
            if (clay->pl.erased().size() != 1) throw Error(ECX_E_ILLEGAL_ARGUMENT, "not a single-node repair");
            clay->rtc.reset(new ClayRtc(clay->pl.repair_program(clay->pl.erased()[0])));
            clay->rtc_state = 1;
        } catch (const Error &e) {
            clay->rtc_state = -1;
            clay->rtc_why = e.what();
        }
    }
    return clay->rtc_state == 1 ? clay->rtc.get() : nullptr;
}
}  // namespace

int ecx_clay_perform_coding_batch(ecx_clay *clay, const uint8_t *in, int64_t in_stripe_stride, int64_t in_sub_stride,
                                  uint8_t *out, int64_t out_stripe_stride, int64_t out_sub_stride, int64_t nstripes,
                                  int64_t buf_size, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (clay->pl.erased().empty()) return ECX_OK;
        if (nstripes < 0 || buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!in || !out) throw Error(ECX_E_NULL, "null device pointer");
        ecx_map *m = clay_standard_map(clay);
        // Single-node repair: the per-helper-plane kernel (clay_rtc.hpp) for the whole
        // 4 KiB chunks of 16-B-aligned layouts whose slot offsets fit 31 bits; the
        // composed-map kernel takes any tail and every other layout.
        int64_t done = 0;
        const char *rtc_kernel = nullptr;
        // auto (1): repairs whose composed map spans several 8-row tiles (alpha > 8), where
        // the composed kernel is bound by vector issue (Clay(10,4): 0.61 -> 0.70 of HBM);
        // Clay(4,2)'s single-tile map is memory-bound and stays on the composed kernel
        // (0.83 there vs 0.63 per plane: profiles/r02_clay_rtc_ab.jsonl).
        const int rtc_mode = tuning().clay_rtc;
        const bool rtc_want = rtc_mode == 2 || (rtc_mode == 1 && m->cm.n_tiles() > 1);
        if (rtc_want && buf_size >= kChunkBytes && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
            in_stripe_stride % 16 == 0 && in_sub_stride % 16 == 0 && out_stripe_stride % 16 == 0 &&
            out_sub_stride % 16 == 0 && in_sub_stride >= 0 && out_sub_stride >= 0) {
            if (ClayRtc *r = clay_rtc(clay)) {
                // first use of the module, its table or the zero page is refused under capture (engine.hpp)
                const LaunchStreamScope scope((hipStream_t)stream);
                // auto: a generated kernel that cannot be compiled or loaded here (no
                // hiprtc, another target) falls back to the composed map; forced (2) throws
                RtcShape sh = rtc_current_shape();
                // slot offsets beyond 31 bits (1 MiB sub-chunks of Clay(10,4)): the plane-group
                // kernel with 64-bit load addresses; the per-plane kernel has no such form
                const bool narrow = (int64_t)r->program().max_in_slot * in_sub_stride + kChunkBytes <= 0x7FFFFFFF;
                if (!narrow) sh.wide = 1;
                if ((narrow || (clay_grp_supported(r->program()) && sh.group)) &&
                    (rtc_mode == 2 || r->available(sh, (hipStream_t)stream))) {
                    done = buf_size / kChunkBytes * kChunkBytes;
                    r->launch(sh, in, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride,
                              nstripes, done / kChunkBytes, (hipStream_t)stream);
                    rtc_kernel = r->kernel_name(sh);
                    int dev = 0;
                    check_hip(hipGetDevice(&dev), "hipGetDevice");
                    note_device_launch(dev, (hipStream_t)stream, nstripes * done * (int64_t)(r->program().max_in_slot + 1));
                }
            }
        }
        if (done < buf_size)
            launch_apply(m->cm, in + done, in_stripe_stride, in_sub_stride, out + done, out_stripe_stride,
                         out_sub_stride, nstripes, buf_size - done, (hipStream_t)stream);
        if (rtc_kernel) set_last_kernel(rtc_kernel);
        return ECX_OK;
    });
}

namespace {
// The codeword test of a geometry, on the registry's codec without erasures: the planner's proof
// runs once, and a refusal is kept with its reason.
ClayCheck *clay_check(ecx_clay *clay) {
    std::lock_guard<std::mutex> lk(clay->mu);
    if (clay->check_state == 0) {
        try {
            clay->check.reset(new ClayCheck(clay_check_program(clay->pl)));
            clay->check_state = 1;
        } catch (const Error &e) {
            clay->check_state = -1;
            clay->check_why = e.what();
        }
    }
    if (clay->check_state != 1) throw Error(ECX_E_ILLEGAL_ARGUMENT, "no Clay parity check for this geometry: " + clay->check_why);
    return clay->check.get();
}

// The program's dense syndrome map as an ordinary check map (rows z * m + p over the real slots).
constexpr int kClayCheckDenseRows = 16;
ecx_map *clay_check_dense_map(ecx_clay *clay, ClayCheck *cc) {
    return clay->maps.get({MapKey::check}, [&] { return cc->program().compose(); });
}

// A reference on the registry's codec of a geometry for the length of one call.
struct ClayRef {
    ClayRef(int k, int m, int v)
        : clay(clay_registry().get(std::make_tuple(k, m, v, std::vector<int>{}, 0), [&] { return new ecx_clay(k, m, {}, v); })) {}
    ~ClayRef() { clay_registry().release(clay); }
    ClayRef(const ClayRef &) = delete;
    ClayRef &operator=(const ClayRef &) = delete;
    ecx_clay *clay;
};
}  // namespace

int ecx_clay_is_parity_correct_batch(int data_units, int parity_units, int virtual_units, const uint8_t *base,
                                     int64_t stripe_stride, int64_t sub_stride, int64_t nstripes, int64_t buf_size,
                                     uint8_t *verdict, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (data_units < 1 || parity_units < 1 || virtual_units < 0 || nstripes < 0 || buf_size < 0)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (nstripes == 0) return ECX_OK;
        if (!base || !verdict) throw Error(ECX_E_NULL, "null device pointer");
        if (stripe_stride < 0 || sub_stride < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative stride");
        const ClayRef ref(data_units, parity_units, virtual_units);  // (refuses what ecx_clay_create_shortened does)
        const ClayPlanner &pl = ref.clay->pl;
        if (!extent_fits({{nstripes, stripe_stride}, {(int64_t)pl.n_real() * pl.alpha(), sub_stride}}, buf_size))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative stride, or the batch's extent is beyond int64_t");
        ClayCheck *cc = clay_check(ref.clay);
        // Geometries whose dense syndrome map has at most 16 rows (Clay(2,2), Clay(4,2)) run it as an
        // ordinary check map on k_gf_check: measured faster there than one workgroup per plane (0.85 of
        // its time on Clay(4,2)), and the simpler path.
        if (pl.m() * pl.alpha() <= kClayCheckDenseRows)
            launch_check(clay_check_dense_map(ref.clay, cc)->cm, base, stripe_stride, sub_stride, verdict, nstripes,
                         buf_size, (hipStream_t)stream);
        else
            launch_clay_check(*cc, base, stripe_stride, sub_stride, verdict, nstripes, buf_size, (hipStream_t)stream);
        return ECX_OK;
    });
}

#if ECX_DIAG
// DIAG only (scripts/clay_check_ab.py): either route forced for any geometry -- dense 1: the
// existing k_gf_check over the program's dense syndrome map, 0: k_clay_check.
extern "C" int ecx_diag_clay_check_route_batch(int dense, int data_units, int parity_units, int virtual_units,
                                               const uint8_t *base, int64_t stripe_stride, int64_t sub_stride,
                                               int64_t nstripes, int64_t buf_size, uint8_t *verdict, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!base || !verdict || nstripes <= 0 || buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "arguments");
        const ClayRef ref(data_units, parity_units, virtual_units);
        ClayCheck *cc = clay_check(ref.clay);
        if (dense)
            launch_check(clay_check_dense_map(ref.clay, cc)->cm, base, stripe_stride, sub_stride, verdict, nstripes,
                         buf_size, (hipStream_t)stream);
        else
            launch_clay_check(*cc, base, stripe_stride, sub_stride, verdict, nstripes, buf_size, (hipStream_t)stream);
        return ECX_OK;
    });
}
#endif

// ---------------------------------------------------------------- Clay pattern sets
// A Clay pattern set (ecx.h): the standard-null-pattern performCoding maps of its erased-node
// lists as one device plan.  `codecs` holds the set's own reference on the codec of each distinct
// list: the maps are the codecs' and live as long as they do.
struct ecx_clay_pattern_set {
    ecx_clay_pattern_set() : codecs(clay_registry()) {}
    RefBundle<ecx_clay, ClayKey> codecs;
    std::unique_ptr<PatternSet> set;  // destroyed in ~: before the references go (declared after them)
    // A generated set (ecx.h): single-node lists of maps too tall for the composed plan, run by
    // k_clay_repair_set (clay_rtc.hpp).  Exactly one of `set` and `gen` is there.
    std::unique_ptr<ClaySetRtc> gen;
    int npatterns = 0, nodes = 0, alpha = 0, max_erased = 0;
    int max_out_slot() const { return gen ? (gen->programs().empty() ? -1 : alpha - 1) : set->max_out_slot(); }
    const std::vector<int> &in_slots() const { return gen ? gen->in_slots() : set->in_slots(); }
    const std::vector<int> &out_slots() const { return gen ? gen->out_slots() : set->out_slots(); }
};

namespace {
const char *const kGeneratedSetNoPartial =
    "a generated pattern set (k_clay_repair_set) has no partial-sum hop: repair its stripes with "
    "ecx_clay_perform_coding_batch_mixed";
}  // namespace

int ecx_clay_pattern_set_create(int data_units, int parity_units, int virtual_units, const int *erased,
                                const int *n_erased, int npatterns, ecx_clay_pattern_set **out) {
    return guarded(__func__, [&]() -> int {
        if (out) *out = nullptr;
        if (!out) throw Error(ECX_E_NULL, "null out pointer");
        if (npatterns < 1 || npatterns > kMixedRecords)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "a pattern set holds 1..256 lists: " + std::to_string(npatterns));
        if (!n_erased) throw Error(ECX_E_NULL, "null list counts");
        if (virtual_units < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "virtual_units");
        int64_t total = 0;
        for (int p = 0; p < npatterns; ++p) {
            if (n_erased[p] < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "list " + std::to_string(p) + " has a negative count");
            total += n_erased[p];
        }
        if (total > 0 && !erased) throw Error(ECX_E_NULL, "null erased lists");
        auto set = std::make_unique<ecx_clay_pattern_set>();
        std::vector<const CompiledMap *> maps;
        // a generated set's bodies: one program per distinct node, and each id's body
        std::vector<ClayRepairProgram> programs;
        std::map<int, int> body_of_node;
        int id_to_body[256];
        std::fill(id_to_body, id_to_body + 256, -1);
        int first_generated = -1, first_composed = -1;
        const int *list = erased;
        for (int p = 0; p < npatterns; list += n_erased[p], ++p) {
            const std::vector<int> e(list, list + n_erased[p]);  // order matters (the reference's erasedIndexes)
            // a list the single step refuses is refused with that step's status (the planner throws)
            ecx_clay *c = set->codecs.get(std::make_tuple(data_units, parity_units, virtual_units, e, 0), [&] {
                return new ecx_clay(data_units, parity_units, e, virtual_units, false);
            });
            const int rows = (int)e.size() * c->pl.alpha();
            auto refuse = [&](const std::string &why) {
                std::string names;
                for (int x : e) names += (names.empty() ? "" : ",") + std::to_string(x);
                throw Error(ECX_E_ILLEGAL_ARGUMENT,
                            "list " + std::to_string(p) + " {" + names + "} has a map of " + std::to_string(rows) +
                                " rows, a pattern set takes at most " + std::to_string(kMixedMaxTiles * kTileRows) + why +
                                ": repair such stripes with ecx_clay_perform_coding_batch, one list per call");
            };
            set->nodes = c->pl.n_real();
            set->alpha = c->pl.alpha();
            set->max_erased = std::max(set->max_erased, (int)e.size());
            if (rows > kMixedMaxTiles * kTileRows) {
                // taller maps run on the generated set kernel, which has single-node bodies only
                if (e.size() != 1) refuse(" (or single-node lists of a q = 4 geometry, on the generated set kernel)");
                ClayRtc *r = clay_rtc(c);
                std::string why = r ? std::string() : c->rtc_why;
                if (!r || !clay_grp_supported(r->program(), &why))
                    refuse(", and the generated set kernel needs q = 4 and t >= 3 (" + why + ")");
                if (first_generated < 0) first_generated = p;
                auto at = body_of_node.find(e[0]);
                if (at == body_of_node.end()) {
                    at = body_of_node.emplace(e[0], (int)programs.size()).first;
                    programs.push_back(r->program());
                }
                id_to_body[p] = at->second;
                continue;
            }
            if (!e.empty() && first_composed < 0) first_composed = p;
            maps.push_back(&clay_standard_map(c)->cm);
        }
        if (first_generated >= 0 && first_composed >= 0)
            throw Error(ECX_E_ILLEGAL_ARGUMENT,
                        "list " + std::to_string(first_generated) + " runs on the generated set kernel and list " +
                            std::to_string(first_composed) + " on the composed-map kernel: a pattern set holds one kind");
        if (first_generated >= 0)
            set->gen = std::make_unique<ClaySetRtc>(std::move(programs), id_to_body);
        else
            set->set = std::make_unique<PatternSet>(maps);
        set->npatterns = npatterns;
        *out = set.release();
        return ECX_OK;
    });
}

void ecx_clay_pattern_set_destroy(ecx_clay_pattern_set *set) {
    if (!set) return;
    set->set.reset();  // the device plans first (hipFree), then the codec references
    set->gen.reset();
    delete set;
}

int ecx_clay_pattern_set_info(const ecx_clay_pattern_set *set, int *npatterns, int *nodes, int *alpha,
                              int *max_erased) {
    if (!set) return ECX_E_NULL;
    if (npatterns) *npatterns = set->npatterns;
    if (nodes) *nodes = set->nodes;
    if (alpha) *alpha = set->alpha;
    if (max_erased) *max_erased = set->max_erased;
    return ECX_OK;
}

namespace {
// The one body of the two mixed Clay batches (ecx.h); tests/test_clay_mixed_cpu.py pins the order of
// its checks.
int clay_mixed_batch(const char *fn, const ecx_clay_pattern_set *set, const uint8_t *pattern_of_stripe,
                     const uint8_t *in, int64_t in_stripe_stride, int64_t in_sub_stride, uint8_t *out,
                     int64_t out_stripe_stride, int64_t out_sub_stride, int64_t nstripes, int64_t buf_size, bool host,
                     void *stream) {
    return guarded(fn, [&]() -> int {
        if (!set) throw Error(ECX_E_NULL, "null pattern set");
        if (nstripes < 0 || buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (nstripes == 0 || buf_size == 0 || set->max_out_slot() < 0) return ECX_OK;
        if (!pattern_of_stripe || !in || !out) throw Error(ECX_E_NULL, host ? "null host pointer" : "null device pointer");
        const int n_in = set->nodes * set->alpha;
        if (in_stripe_stride < 0 || in_sub_stride < 0 || out_stripe_stride < 0 || out_sub_stride < 0)
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative stride");
        if (!extent_fits({{nstripes, in_stripe_stride}, {(int64_t)n_in, in_sub_stride}}, buf_size) ||
            !extent_fits({{nstripes, out_stripe_stride}, {(int64_t)set->max_out_slot() + 1, out_sub_stride}}, buf_size))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "batch extent overflows");
        MapMixedRun run{set->in_slots(), set->out_slots(), nullptr};
        if (ClaySetRtc *g = set->gen.get()) {
            // k_clay_repair_set covers whole 4 KiB chunks of 16-B-aligned layouts, and nothing
            // here can take a tail (the composed kernel cannot run these maps)
            if (buf_size % kChunkBytes != 0)
                throw Error(ECX_E_ILLEGAL_ARGUMENT, "a generated pattern set takes a buf_size that is a multiple of " +
                                                        std::to_string(kChunkBytes) + ": " + std::to_string(buf_size));
            if (!host) {
                const std::pair<const char *, int64_t> aligned[] = {
                    {"in", (int64_t)(uintptr_t)in},           {"out", (int64_t)(uintptr_t)out},
                    {"in_stripe_stride", in_stripe_stride},   {"in_sub_stride", in_sub_stride},
                    {"out_stripe_stride", out_stripe_stride}, {"out_sub_stride", out_sub_stride}};
                for (const auto &a : aligned)
                    if (a.second % 16 != 0)
                        throw Error(ECX_E_ILLEGAL_ARGUMENT,
                                    std::string("a generated pattern set takes bases and strides that are multiples of 16: ") +
                                        a.first + " = " + std::to_string(a.second));
            }
            run.launch = [g](const uint8_t *ids, const uint8_t *pin, int64_t iss, int64_t isl, uint8_t *pout, int64_t oss,
                             int64_t osl, int64_t units, int64_t nbytes, int64_t first_unit, hipStream_t s) {
                RtcShape sh = rtc_current_shape();
                // slot offsets beyond 31 bits: 64-bit load addresses, by ecx_clay_perform_coding_batch's rule
                if ((int64_t)g->max_in_slot() * isl + kChunkBytes > 0x7FFFFFFF) sh.wide = 1;
                g->launch(sh, ids + first_unit, pin, iss, isl, pout, oss, osl, units, nbytes / kChunkBytes, s);
            };
        } else {
            PatternSet *ps = set->set.get();
            run.launch = [ps](const uint8_t *ids, const uint8_t *pin, int64_t iss, int64_t isl, uint8_t *pout,
                              int64_t oss, int64_t osl, int64_t units, int64_t nbytes, int64_t first_unit, hipStream_t s) {
                launch_map_mixed(*ps, ids, pin, iss, isl, pout, oss, osl, units, nbytes, first_unit, s);
            };
        }
        if (host) {
            const HostMixedIds ids(pattern_of_stripe, nstripes);
            run_host_map_mixed_batch(run, ids.get(), in, in_stripe_stride, in_sub_stride, n_in, out, out_stripe_stride,
                                     out_sub_stride, nstripes, buf_size);
        } else if (set->gen) {
            // first use of the module or the zero page is refused under capture (engine.hpp)
            const LaunchStreamScope scope((hipStream_t)stream);
            run.launch(pattern_of_stripe, in, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride,
                       nstripes, buf_size, 0, (hipStream_t)stream);
            int dev = 0;
            check_hip(hipGetDevice(&dev), "hipGetDevice");
            note_device_launch(dev, (hipStream_t)stream, nstripes * buf_size * (int64_t)(set->gen->max_in_slot() + 1));
            set_last_kernel("k_clay_repair_set");
        } else {
            run.launch(pattern_of_stripe, in, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride,
                       nstripes, buf_size, 0, (hipStream_t)stream);
        }
        return ECX_OK;
    });
}
}  // namespace

int ecx_clay_perform_coding_batch_mixed(const ecx_clay_pattern_set *set, const uint8_t *pattern_of_stripe,
                                        const uint8_t *in, int64_t in_stripe_stride, int64_t in_sub_stride,
                                        uint8_t *out, int64_t out_stripe_stride, int64_t out_sub_stride,
                                        int64_t nstripes, int64_t buf_size, void *stream) {
    return clay_mixed_batch(__func__, set, pattern_of_stripe, in, in_stripe_stride, in_sub_stride, out,
                            out_stripe_stride, out_sub_stride, nstripes, buf_size, false, stream);
}

int ecx_clay_perform_coding_mixed_batch_host(const ecx_clay_pattern_set *set, const uint8_t *pattern_of_stripe,
                                             const uint8_t *in, int64_t in_stripe_stride, int64_t in_sub_stride,
                                             uint8_t *out, int64_t out_stripe_stride, int64_t out_sub_stride,
                                             int64_t nstripes, int64_t buf_size) {
    return clay_mixed_batch(__func__, set, pattern_of_stripe, in, in_stripe_stride, in_sub_stride, out,
                            out_stripe_stride, out_sub_stride, nstripes, buf_size, true, nullptr);
}

// tests/test_clay_partial_mixed_cpu.py pins the order of the checks.
int ecx_clay_partial_batch_mixed(const ecx_clay_pattern_set *set, const uint8_t *pattern_of_stripe,
                                 const uint8_t *node_of_stripe, const uint8_t *in, int64_t in_stripe_stride,
                                 int64_t in_node_stride, int64_t in_sub_stride, uint8_t *acc,
                                 int64_t acc_stripe_stride, int64_t acc_sub_stride, int64_t nstripes, int64_t buf_size,
                                 int is_first, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!set) throw Error(ECX_E_NULL, "null pattern set");
        if (set->gen) throw Error(ECX_E_ILLEGAL_ARGUMENT, kGeneratedSetNoPartial);
        if (nstripes < 0 || buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (nstripes == 0 || buf_size == 0 || set->set->max_out_slot() < 0) return ECX_OK;
        if (!pattern_of_stripe || !node_of_stripe || !in || !acc) throw Error(ECX_E_NULL, "null device pointer");
        if (!extent_fits({{nstripes, in_stripe_stride}, {set->nodes, in_node_stride}, {set->alpha, in_sub_stride}},
                         buf_size) ||
            !extent_fits({{nstripes, acc_stripe_stride}, {(int64_t)set->set->max_out_slot() + 1, acc_sub_stride}},
                         buf_size))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative stride, or the batch's extent is beyond int64_t");
        launch_clay_partial_mixed(*set->set, set->nodes, pattern_of_stripe, node_of_stripe, in, in_stripe_stride,
                                  in_node_stride, in_sub_stride, acc, acc_stripe_stride, acc_sub_stride, nstripes,
                                  buf_size, is_first != 0, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_clay_rtc_compile_check(ecx_clay *clay) {
    return guarded(__func__, [&]() -> int {
        ClayRtc *r = clay_rtc(clay);
        if (!r) throw Error(ECX_E_ILLEGAL_ARGUMENT, "no per-helper-plane program: " + clay->rtc_why);
        return (int)rtc_compile_check(clay_rtc_selected_source(r->program(), rtc_current_shape()));
    });
}

int ecx_clay_rtc_source(ecx_clay *clay, char *buf, int len) {
    return guarded(__func__, [&]() -> int {
        ClayRtc *r = clay_rtc(clay);
        if (!r) throw Error(ECX_E_ILLEGAL_ARGUMENT, "no per-helper-plane program: " + clay->rtc_why);
        const std::string src = clay_rtc_selected_source(r->program(), rtc_current_shape());
        if (buf && len > (int)src.size()) std::memcpy(buf, src.c_str(), src.size() + 1);
        return (int)src.size();
    });
}

namespace {
ClaySetRtc &generated_of(const ecx_clay_pattern_set *set) {
    if (!set) throw Error(ECX_E_NULL, "null pattern set");
    if (!set->gen) throw Error(ECX_E_ILLEGAL_ARGUMENT, "not a generated pattern set: its lists run on the composed-map kernel");
    return *set->gen;
}
}  // namespace

// Diagnostic exports of a generated set (prototyped in a comment of include/ecx_tune.h)
extern "C" {
int ecx_clay_pattern_set_generated(const ecx_clay_pattern_set *set);
int ecx_clay_pattern_set_rtc_source(const ecx_clay_pattern_set *set, char *buf, int len);
int ecx_clay_pattern_set_rtc_compile_check(const ecx_clay_pattern_set *set);
int ecx_clay_pattern_set_rtc_resources(const ecx_clay_pattern_set *set, int *vgprs, int *lds_bytes, int *scratch_bytes,
                                       int64_t *code_bytes);
}

int ecx_clay_pattern_set_generated(const ecx_clay_pattern_set *set) {
    if (!set) return ECX_E_NULL;
    return set->gen ? 1 : 0;
}

int ecx_clay_pattern_set_rtc_source(const ecx_clay_pattern_set *set, char *buf, int len) {
    return guarded(__func__, [&]() -> int {
        const std::string src = generated_of(set).source(rtc_current_shape());
        if (buf && len > (int)src.size()) std::memcpy(buf, src.c_str(), src.size() + 1);
        return (int)src.size();
    });
}

int ecx_clay_pattern_set_rtc_compile_check(const ecx_clay_pattern_set *set) {
    return guarded(__func__, [&]() -> int {
        return (int)rtc_compile_check(generated_of(set).source(rtc_current_shape()));
    });
}

int ecx_clay_pattern_set_rtc_resources(const ecx_clay_pattern_set *set, int *vgprs, int *lds_bytes, int *scratch_bytes,
                                       int64_t *code_bytes) {
    return guarded(__func__, [&]() -> int {
        generated_of(set).resources(rtc_current_shape(), vgprs, lds_bytes, scratch_bytes, code_bytes);
        return ECX_OK;
    });
}

int ecx_map_planes_compile_check(const ecx_map *map, int accumulate) {
    return guarded(__func__, [&]() -> int {
        PlanesShape sh;
        const Tuning tu = tuning();
        sh.lookahead = tu.planes_lookahead;
        sh.waves = tu.planes_waves;
        return (int)rtc_compile_check(map_planes_source(map->cm.map(), sh, accumulate != 0));
    });
}

int ecx_map_planes_source(const ecx_map *map, int accumulate, char *buf, int len) {
    return guarded(__func__, [&]() -> int {
        PlanesShape sh;
        const Tuning tu = tuning();
        sh.lookahead = tu.planes_lookahead;
        sh.waves = tu.planes_waves;
        const std::string src = map_planes_source(map->cm.map(), sh, accumulate != 0);
        if (buf && len > (int)src.size()) std::memcpy(buf, src.c_str(), src.size() + 1);
        return (int)src.size();
    });
}

// ---------------------------------------------------------------- LRC
int ecx_lrc_map(const uint8_t *block_present, const ecx_map **out) {
    return guarded(__func__, [&]() -> int {
        if (!out) throw Error(ECX_E_NULL, "null out pointer");
        static const LrcCode code;
        static MapMemo maps;
        if (!block_present) {
            *out = maps.get({MapKey::encode}, [&] { return code.encode_map(); });
            return ECX_OK;
        }
        const std::vector<bool> present = present_vec(block_present, LrcCode::kN);
        *out = maps.get({MapKey::decode, present}, [&] { return code.decode_map(present); });
        return ECX_OK;
    });
}

int ecx_lrc_encode_batch(uint8_t *stripes, int64_t stripe_stride, int64_t block_stride, int64_t nstripes,
                         int64_t block_size, void *stream) {
    const ecx_map *m = nullptr;
    int st = ecx_lrc_map(nullptr, &m);
    if (st) return st;
    return ecx_map_apply_batch(m, stripes, stripe_stride, block_stride, stripes, stripe_stride, block_stride, nstripes,
                               block_size, stream);
}

int ecx_lrc_decode_batch(uint8_t *stripes, int64_t stripe_stride, int64_t block_stride, const uint8_t *block_present,
                         int64_t nstripes, int64_t block_size, void *stream) {
    if (!block_present) return ECX_E_NULL;
    const ecx_map *m = nullptr;
    int st = ecx_lrc_map(block_present, &m);
    if (st) return st;
    if (m->cm.map().n_out == 0) return ECX_OK;  // nothing missing
    return ecx_map_apply_batch(m, stripes, stripe_stride, block_stride, stripes, stripe_stride, block_stride, nstripes,
                               block_size, stream);
}

// ---------------------------------------------------------------- host-memory batches (f1)
int ecx_map_apply_batch_host(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride, int64_t in_slot_stride,
                             uint8_t *out, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                             int64_t byte_count) {
    return guarded(__func__, [&]() -> int {
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!in || !out) throw Error(ECX_E_NULL, "null host pointer");
        run_host_batch(const_cast<ecx_map *>(map)->cm, in, in_stripe_stride, in_slot_stride, out, out_stripe_stride,
                       out_slot_stride, nstripes, byte_count);
        return ECX_OK;
    });
}

int ecx_clay_perform_coding_batch_host(ecx_clay *clay, const uint8_t *in, int64_t in_stripe_stride,
                                       int64_t in_sub_stride, uint8_t *out, int64_t out_stripe_stride,
                                       int64_t out_sub_stride, int64_t nstripes, int64_t buf_size) {
    return guarded(__func__, [&]() -> int {
        if (clay->pl.erased().empty()) return ECX_OK;
        if (nstripes < 0 || buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!in || !out) throw Error(ECX_E_NULL, "null host pointer");
        ecx_map *m = clay_standard_map(clay);
        run_host_batch(m->cm, in, in_stripe_stride, in_sub_stride, out, out_stripe_stride, out_sub_stride, nstripes,
                       buf_size);
        return ECX_OK;
    });
}

int ecx_map_apply_batch_host_devices(const ecx_map *map, const uint8_t *in, int64_t in_stripe_stride,
                                     int64_t in_slot_stride, uint8_t *out, int64_t out_stripe_stride,
                                     int64_t out_slot_stride, int64_t nstripes, int64_t byte_count,
                                     const int *devices, int ndev) {
    return guarded(__func__, [&]() -> int {
        if (!map) throw Error(ECX_E_NULL, "null map");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!in || !out) throw Error(ECX_E_NULL, "null host pointer");
        run_host_batch_devices(const_cast<ecx_map *>(map)->cm, in, in_stripe_stride, in_slot_stride, out,
                               out_stripe_stride, out_slot_stride, nstripes, byte_count, devices, ndev);
        return ECX_OK;
    });
}

int ecx_clay_perform_coding_batch_host_devices(ecx_clay *clay, const uint8_t *in, int64_t in_stripe_stride,
                                               int64_t in_sub_stride, uint8_t *out, int64_t out_stripe_stride,
                                               int64_t out_sub_stride, int64_t nstripes, int64_t buf_size,
                                               const int *devices, int ndev) {
    return guarded(__func__, [&]() -> int {
        if (!clay) throw Error(ECX_E_NULL, "null decoding step");
        if (!devices) throw Error(ECX_E_NULL, "null device list");
        if (ndev <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "empty device list");
        if (clay->pl.erased().empty()) return ECX_OK;
        if (nstripes < 0 || buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (!in || !out) throw Error(ECX_E_NULL, "null host pointer");
        run_host_batch_devices(clay_standard_map(clay)->cm, in, in_stripe_stride, in_sub_stride, out,
                               out_stripe_stride, out_sub_stride, nstripes, buf_size, devices, ndev);
        return ECX_OK;
    });
}

namespace {
int rs_check_host(const char *fn, ecx_rs *rs, const uint8_t *base, int64_t stripe_stride, int64_t shard_stride,
                  int64_t nstripes, int64_t offset, int64_t byte_count, uint8_t *verdict, const int *devices,
                  int ndev, bool multi) {
    return guarded(fn, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (nstripes < 0 || offset < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        if (stripe_stride < 0 || shard_stride < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative stride");
        if (nstripes > 0 && (!base || !verdict)) throw Error(ECX_E_NULL, "null host pointer");
        CompiledMap &cm = rs_check_plan(rs)->cm;
        const uint8_t *in = nstripes > 0 ? base + offset : base;
        if (multi) run_host_check_batch_devices(cm, in, stripe_stride, shard_stride, nstripes, byte_count, verdict,
                                                devices, ndev);
        else run_host_check_batch(cm, in, stripe_stride, shard_stride, nstripes, byte_count, verdict);
        return ECX_OK;
    });
}
}  // namespace

int ecx_rs_is_parity_correct_batch_host(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride,
                                        int64_t shard_stride, int64_t nstripes, int64_t offset,
                                        int64_t byte_count, uint8_t *verdict) {
    return rs_check_host(__func__, rs, base, stripe_stride, shard_stride, nstripes, offset, byte_count, verdict,
                         nullptr, 0, false);
}

int ecx_rs_is_parity_correct_batch_host_devices(ecx_rs *rs, const uint8_t *base, int64_t stripe_stride,
                                                int64_t shard_stride, int64_t nstripes, int64_t offset,
                                                int64_t byte_count, uint8_t *verdict, const int *devices,
                                                int ndev) {
    return rs_check_host(__func__, rs, base, stripe_stride, shard_stride, nstripes, offset, byte_count, verdict,
                         devices, ndev, true);
}

int ecx_rs_is_parity_correct_blocked_batch(ecx_rs *rs, const uint8_t *base, int64_t nstripes, int64_t byte_count,
                                           int64_t block_bytes, uint8_t *verdict, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        const int64_t block = resolve_block(rs->code.n(), byte_count, block_bytes);
        if (nstripes == 0) return ECX_OK;
        if (!base || !verdict) throw Error(ECX_E_NULL, "null device pointer");
        launch_check_blocked(rs_check_plan(rs)->cm, base, rs->code.n(), nstripes, byte_count, block, verdict,
                             (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_locate_corrupt_blocked_batch(ecx_rs *rs, const uint8_t *base, int64_t nstripes, int64_t byte_count,
                                        int64_t block_bytes, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id,
                                        void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        const int64_t block = resolve_block(rs->code.n(), byte_count, block_bytes);
        check_locatable(rs, heal_id);
        if (nstripes == 0) return ECX_OK;
        if (!base || !suspect || !culprit) throw Error(ECX_E_NULL, "null device pointer");
        launch_locate_blocked(rs_check_plan(rs)->cm, *rs_locate_plan(rs), base, rs->code.n(), nstripes, byte_count,
                              block, suspect, culprit, heal_id, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_rs_locate_corrupt2_blocked_batch(ecx_rs *rs, const uint8_t *base, int64_t nstripes, int64_t byte_count,
                                         int64_t block_bytes, uint8_t *suspect, int32_t *culprit, uint8_t *heal_id,
                                         void *stream) {
    return guarded(__func__, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        const int64_t block = resolve_block(rs->code.n(), byte_count, block_bytes);
        check_locatable2(rs, heal_id);
        if (nstripes == 0) return ECX_OK;
        if (!base || !suspect || !culprit) throw Error(ECX_E_NULL, "null device pointer");
        launch_locate2_blocked(rs_check_plan(rs)->cm, *rs_locate_plan(rs), *rs_locate2_plan(rs), base, rs->code.n(),
                               nstripes, byte_count, block, suspect, culprit, heal_id, (hipStream_t)stream);
        return ECX_OK;
    });
}

namespace {
// The blocked check from host memory: each pass of the layout is a pipelined host check
// (host_pipe.cpp) with one verdict byte per unit of the pass; the body pass's go to a temporary
// (1 byte per n * block data bytes) and are folded per stripe here, then ANDed with the tail
// pass's.  With a device list each pass is split over the entries like any host check: the body
// units by ranges, the tails by stripes (by byte ranges where there are fewer stripes than entries).
int rs_check_blocked_host(const char *fn, ecx_rs *rs, const uint8_t *base, int64_t nstripes, int64_t byte_count,
                          int64_t block_bytes, uint8_t *verdict, const int *devices, int ndev, bool multi) {
    return guarded(fn, [&]() -> int {
        if (!rs) throw Error(ECX_E_NULL, "null codec");
        if (multi && !devices) throw Error(ECX_E_NULL, "null device list");
        if (multi && ndev <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "empty device list");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        const int n = rs->code.n();
        const int64_t block = resolve_block(n, byte_count, block_bytes);
        if (nstripes > 0 && (!base || !verdict)) throw Error(ECX_E_NULL, "null host pointer");
        BlockedPlan plan;
        blocked_plan_or_throw(n, nstripes, byte_count, block, &plan);
        if (multi) check_device_list(devices, ndev);  // even for an empty batch
        if (nstripes == 0) return ECX_OK;
        CompiledMap &cm = rs_check_plan(rs)->cm;
        auto check = [&](const BlockedPass &p, uint8_t *v) {
            if (multi) run_host_check_batch_devices(cm, base + p.offset, p.stripe_stride, p.slot_bytes, p.units,
                                                    p.slot_bytes, v, devices, ndev);
            else run_host_check_batch(cm, base + p.offset, p.stripe_stride, p.slot_bytes, p.units, p.slot_bytes, v);
        };
        if (plan.count == 0) {  // no bytes: every stripe passes, through the natural check's own path
            check(BlockedPass{0, 0, 0, nstripes, 1}, verdict);
            return ECX_OK;
        }
        std::vector<uint8_t> unit;
        for (int i = 0; i < plan.count; ++i) {
            const BlockedPass &p = plan.pass[i];
            if (i == 0 && p.divisor == 1) {  // one unit per stripe: straight into the caller's array
                check(p, verdict);
                continue;
            }
            unit.assign((size_t)p.units, 0);
            check(p, unit.data());
            fold_unit_verdicts(unit.data(), p.divisor, i == 0, verdict, nstripes);
        }
        return ECX_OK;
    });
}
}  // namespace

int ecx_rs_is_parity_correct_blocked_batch_host(ecx_rs *rs, const uint8_t *base, int64_t nstripes,
                                                int64_t byte_count, int64_t block_bytes, uint8_t *verdict) {
    return rs_check_blocked_host(__func__, rs, base, nstripes, byte_count, block_bytes, verdict, nullptr, 0, false);
}

int ecx_rs_is_parity_correct_blocked_batch_host_devices(ecx_rs *rs, const uint8_t *base, int64_t nstripes,
                                                        int64_t byte_count, int64_t block_bytes, uint8_t *verdict,
                                                        const int *devices, int ndev) {
    return rs_check_blocked_host(__func__, rs, base, nstripes, byte_count, block_bytes, verdict, devices, ndev, true);
}

int ecx_host_alloc(int64_t nbytes, void **out) {
    return guarded(__func__, [&]() -> int {
        if (!out) throw Error(ECX_E_NULL, "null out pointer");
        if (nbytes < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative size");
        *out = nullptr;
        check_hip(hipHostMalloc(out, (size_t)std::max<int64_t>(nbytes, 1), hipHostMallocDefault), "hipHostMalloc");
        return ECX_OK;
    });
}

int ecx_host_free(void *ptr) {
    return guarded(__func__, [&]() -> int {
        if (ptr) check_hip(hipHostFree(ptr), "hipHostFree");
        return ECX_OK;
    });
}

int ecx_host_register(void *ptr, int64_t nbytes) {
    return guarded(__func__, [&]() -> int {
        if (!ptr) throw Error(ECX_E_NULL, "null pointer");
        if (nbytes <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "non-positive size");
        check_hip(hipHostRegister(ptr, (size_t)nbytes, hipHostRegisterDefault), "hipHostRegister");
        return ECX_OK;
    });
}

int ecx_host_unregister(void *ptr) {
    return guarded(__func__, [&]() -> int {
        if (!ptr) throw Error(ECX_E_NULL, "null pointer");
        check_hip(hipHostUnregister(ptr), "hipHostUnregister");
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- tuning hook (include/ecx_tune.h)
// The keys, their classes and their ranges are tune_table.cpp's rows; here only what the table
// must not do itself: the environment, the tuning lock and the "roctx" atomic.
namespace {
bool env_is_1(const char *name) {
    const char *v = std::getenv(name);
    return v && std::strcmp(v, "1") == 0;
}
}  // namespace

int ecx_tune(const char *key, int value) {
    // ECX_SHAPE_KNOBS is read once, so one library loaded into a JVM cannot be talked into reshaping
    // every other caller's launches later on; ECX_DIAGNOSTIC with every call
    static const bool shape_opt_in = env_is_1("ECX_SHAPE_KNOBS");
    const KnobEnv env{ECX_DIAG != 0, shape_opt_in, env_is_1("ECX_DIAGNOSTIC")};
    const Knob *k = find_knob(key);
    bool ok = false;
    update_tuning([&](Tuning &t) { ok = k && knob_set(t, *k, value, env); });
    if (ok && k->store == KnobStore::external) g_roctx.store(value);  // "roctx"
    return ok ? ECX_OK : ECX_E_ILLEGAL_ARGUMENT;
}

int ecx_tune_value(const char *key, int *value) {
    const Knob *k = find_knob(key);
    if (!value || !k || k->cls != KnobClass::deployment) return ECX_E_ILLEGAL_ARGUMENT;
    if (!knob_get(tuning(), *k, value)) *value = g_roctx.load();  // "roctx"
    return ECX_OK;
}

int ecx_probe_bandwidth(int kind, const uint8_t *src, uint8_t *dst, int64_t nbytes, int nontemporal, void *stream) {
    return guarded(__func__, [&]() -> int {
        launch_probe(kind, src, dst, nbytes, nontemporal != 0, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_map_plan_stats(const ecx_map *map, int *n_tiles, int *n_entries, int *n_groups, int *union_total) {
    return guarded(__func__, [&]() -> int {
        const CompiledMap &cm = map->cm;
        if (n_tiles) *n_tiles = cm.n_tiles();
        if (n_entries) *n_entries = cm.n_tiles() ? cm.n_entries() : 0;
        if (n_groups) *n_groups = cm.n_groups();
        if (union_total) *union_total = cm.union_total();
        return ECX_OK;
    });
}

int ecx_build_diag(void) { return ECX_DIAG ? 1 : 0; }

int ecx_host_exec_isa(void) { return host_exec_isa(); }

int ecx_stripe_range(int64_t nstripes, int parts, int j, int64_t *begin, int64_t *end) {
    if (nstripes < 0 || parts <= 0 || j < 0 || j >= parts || !begin || !end) return ECX_E_ILLEGAL_ARGUMENT;
    stripe_range(nstripes, parts, j, begin, end);
    return ECX_OK;
}

int ecx_map_layout_choice(const ecx_map *map, int64_t slot_pitch, float *median_ms, int n) {
    return guarded(__func__, [&]() -> int {
        if (!map) throw Error(ECX_E_NULL, "null map");
        if (slot_pitch <= 0 || n < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "slot pitch or count");
        std::vector<float> ms;
        const int c = const_cast<ecx_map *>(map)->cm.layout_choice(slot_pitch, median_ms ? &ms : nullptr);
        if (median_ms)
            for (int i = 0; i < n; ++i) median_ms[i] = i < (int)ms.size() ? ms[i] : -1.f;
        if (c < 0) return 0x200;  // none chosen yet (or the layout is not selected per launch)
        const int code = layout_candidate_code(c);
        return code == -1 ? 0x100 : code;  // 0x100 = the static rules' shape
    });
}

int ecx_map_layout_state(const ecx_map *map, int64_t slot_pitch, int *state, int *dropped) {
    return guarded(__func__, [&]() -> int {
        if (!map) throw Error(ECX_E_NULL, "null map");
        if (slot_pitch <= 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "slot pitch");
        int st = -1, dr = 0;
        const int c = const_cast<ecx_map *>(map)->cm.layout_choice(slot_pitch, nullptr, &st, &dr);
        if (state) *state = c < 0 ? -1 : st;
        if (dropped) *dropped = c < 0 ? 0 : dr;
        return ECX_OK;
    });
}

int ecx_map_host_plan(const ecx_map *map, int64_t in_stripe_stride, int64_t in_slot_stride, int64_t out_stripe_stride,
                      int64_t out_slot_stride, int64_t nstripes, int64_t byte_count, int64_t *plan) {
    return guarded(__func__, [&]() -> int {
        if (!map || !plan) throw Error(ECX_E_NULL, "null map or plan");
        if (nstripes < 0 || byte_count < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        const HostBatchPlan hp = plan_host_batch(const_cast<ecx_map *>(map)->cm, in_stripe_stride, in_slot_stride,
                                                 out_stripe_stride, out_slot_stride, nstripes, byte_count);
        const int64_t v[10] = {hp.chunk, hp.nchunks, hp.buffers, hp.h2d_copies, hp.h2d_rows, hp.d2h_copies,
                               hp.d2h_rows, hp.h2d_3d, hp.d2h_3d, hp.slices};
        std::memcpy(plan, v, sizeof(v));
        return ECX_OK;
    });
}

int ecx_clay_pattern_set_host_plan(const ecx_clay_pattern_set *set, int64_t in_stripe_stride, int64_t in_sub_stride,
                                   int64_t out_stripe_stride, int64_t out_sub_stride, int64_t nstripes,
                                   int64_t buf_size, int64_t *plan) {
    return guarded(__func__, [&]() -> int {
        if (!set || !plan) throw Error(ECX_E_NULL, "null pattern set or plan");
        if (nstripes < 0 || buf_size < 0) throw Error(ECX_E_ILLEGAL_ARGUMENT, "negative count");
        int64_t v[7] = {0, 0, 0, 0, 0, 0, 0};
        if (nstripes > 0 && buf_size > 0 && set->max_out_slot() >= 0) {
            const Tuning t = tuning();
            const HostMapMixedPlan mp = make_map_mixed_plan(
                set->in_slots(), set->out_slots(), in_stripe_stride, in_sub_stride, set->nodes * set->alpha,
                out_stripe_stride, out_sub_stride, set->max_out_slot() + 1, nstripes, buf_size, t.host_chunk,
                t.host_buffers);
            const int64_t w[7] = {(int64_t)set->in_slots().size(), (int64_t)set->out_slots().size(), mp.chunk, mp.nchunks,
                                  mp.nb, (int64_t)mp.cin.size(), (int64_t)mp.cout.size()};
            std::memcpy(v, w, sizeof(v));
        }
        std::memcpy(plan, v, sizeof(v));
        return ECX_OK;
    });
}

int ecx_map_launch_plan(const ecx_map *map, uint64_t in_addr, int64_t in_stripe_stride, int64_t in_slot_stride,
                        uint64_t out_addr, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
                        int64_t byte_count, int accumulate, int cand, char *buf, int len) {
    return guarded(__func__, [&]() -> int {
        if (!map) throw Error(ECX_E_NULL, "null map");
        const int pick = layout_candidate_code(cand);
        if (pick == -2) throw Error(ECX_E_ILLEGAL_ARGUMENT, "no such layout candidate");
        const BatchLayout b{(uintptr_t)in_addr, (uintptr_t)out_addr, in_stripe_stride, in_slot_stride, out_stripe_stride,
                            out_slot_stride,    nstripes,            byte_count,       accumulate != 0};
        // no device here: a generated bit-plane kernel the auto rule asks for is taken to build
        const std::string s = describe(choose_launch(map->cm.traits(), tuning(), b, pick, ECX_DIAG != 0,
                                                     {[](void *) { return true; }, nullptr}));
        if (!buf || len < (int)s.size() + 1) return ECX_E_ILLEGAL_ARGUMENT;
        std::memcpy(buf, s.c_str(), s.size() + 1);
        return (int)s.size();
    });
}

int ecx_last_launch_shape(char *buf, int len) {
    const std::string k = last_launch_shape();
    if (!buf || len < (int)k.size() + 1) return ECX_E_ILLEGAL_ARGUMENT;
    std::memcpy(buf, k.c_str(), k.size() + 1);
    return (int)k.size();
}

int ecx_last_kernel(char *buf, int len) {
    const std::string &k = last_kernel();
    if (!buf || len < (int)k.size() + 1) return ECX_E_ILLEGAL_ARGUMENT;
    std::memcpy(buf, k.c_str(), k.size() + 1);
    return (int)k.size();
}

int ecx_map_selftest(const ecx_map *map, uint64_t seed) {
    return guarded(__func__, [&]() -> int {
        const CompiledMap &cm = map->cm;
        const LinearMap &m = cm.map();
        const int64_t len = 97;  // ragged on purpose
        const int nin = cm.max_in_slot() + 1, nout = cm.max_out_slot() + 1;
        std::vector<uint8_t> in((size_t)std::max(1, nin) * len), ref((size_t)std::max(1, nout) * len, 0);
        uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
        for (uint8_t &b : in) {
            x ^= x << 13;
            x ^= x >> 7;
            x ^= x << 17;
            b = (uint8_t)x;
        }
        const Field &f = Field::get();
        for (int o = 0; o < m.n_out; ++o)
            for (int j = 0; j < m.n_in; ++j) {
                const uint8_t c = m.at(o, j);
                if (!c) continue;
                for (int64_t i = 0; i < len; ++i)
                    ref[(size_t)m.out_slot[o] * len + i] ^= f.mul(c, in[(size_t)m.in_slot[j] * len + i]);
            }
        auto check = [&](const std::vector<uint8_t> &got, const char *what) {
            for (int o = 0; o < m.n_out; ++o)
                if (!std::equal(got.begin() + (size_t)m.out_slot[o] * len, got.begin() + (size_t)(m.out_slot[o] + 1) * len,
                                ref.begin() + (size_t)m.out_slot[o] * len))
                    throw Error(ECX_E_ILLEGAL_ARGUMENT, what);
        };
        for (bool via_unions : {false, true}) {
            std::vector<uint8_t> got(ref.size(), 0);
            cm.emulate(in.data(), got.data(), len, via_unions);
            check(got, via_unions ? "plan (union view) differs from the map" : "plan (slot view) differs from the map");
        }
        // The padded arrays the device receives, at both ring depths, with the split
        // tables read as k_gf_apply reads them (SGPRs only, or low dwords from LDS).
        for (int depth : {4, 8, 10, 12, 20}) {
            const HostPlan hp = cm.padded_plan(depth);
            if (cm.n_wide_tiles() > 0 && depth <= 8) {  // wide tiles run at depth 4 / 8
                std::vector<uint8_t> got(ref.size(), 0);
                cm.emulate_wide(hp, in.data(), got.data(), len);
                check(got, "padded plan (wide tiles) differs from the map");
            }
            for (bool tlds : {false, true}) {
                std::vector<uint8_t> got(ref.size(), 0);
                cm.emulate_padded(hp, in.data(), got.data(), len, tlds, depth);
                check(got, tlds ? "padded plan (LDS tables) differs from the map" : "padded plan differs from the map");
            }
        }
        // The bit-sliced kernel's arithmetic (bits.hpp, shared with apply_bits.hip) over
        // its padded entries at both of its ring depths, on one whole 4 KiB chunk.
        const int64_t blen = kChunkBytes;
        std::vector<uint8_t> bin((size_t)std::max(1, nin) * blen), bref((size_t)std::max(1, nout) * blen, 0);
        for (uint8_t &b : bin) {
            x ^= x << 13;
            x ^= x >> 7;
            x ^= x << 17;
            b = (uint8_t)x;
        }
        for (int o = 0; o < m.n_out; ++o)
            for (int j = 0; j < m.n_in; ++j) {
                const uint8_t c = m.at(o, j);
                if (!c) continue;
                for (int64_t i = 0; i < blen; ++i)
                    bref[(size_t)m.out_slot[o] * blen + i] ^= f.mul(c, bin[(size_t)m.in_slot[j] * blen + i]);
            }
        for (int depth : {2, 4}) {
            if (!ECX_DIAG) break;  // bit-sliced entries exist in the diagnostic build only
            std::vector<uint8_t> got(bref.size(), 0);
            cm.emulate_bits(cm.padded_plan(depth), bin.data(), got.data(), blen);
            for (int o = 0; o < m.n_out; ++o)
                if (!std::equal(got.begin() + (size_t)m.out_slot[o] * blen, got.begin() + (size_t)(m.out_slot[o] + 1) * blen,
                                bref.begin() + (size_t)m.out_slot[o] * blen))
                    throw Error(ECX_E_ILLEGAL_ARGUMENT, "bit-sliced plan differs from the map");
        }
        return ECX_OK;
    });
}

// ---------------------------------------------------------------- synthetic data / verification
int ecx_fill_random(uint8_t *dst, int64_t nbytes, uint64_t seed, void *stream) {
    return guarded(__func__, [&]() -> int {
        launch_fill_random(dst, nbytes, seed, (hipStream_t)stream);
        return ECX_OK;
    });
}

int ecx_count_mismatch(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t nrows,
                       int64_t row_bytes, uint64_t *d_count, void *stream) {
    return guarded(__func__, [&]() -> int {
        launch_count_mismatch(a, a_stride, b, b_stride, nrows, row_bytes, d_count, (hipStream_t)stream);
        return ECX_OK;
    });
}
