// api_core_check.cpp -- what the C ABI owns and decides besides its launches, on the CPU: the
// caches of csrc/codec_cache.hpp and the maps and rules of csrc/api_maps.cpp, built with gf.cpp and
// codes.cpp and no ROCm include path (tests/test_api_core_native.py).
//
// The caches hold an element that counts its constructions and records its destructions, so every
// claim is about objects, not about the caches' own counters: which pointer a key gives, how many
// are alive, which were destroyed, in which order and when.  The maps are expanded into dense
// matrices over their slots and compared with definitions computed here from RsCode::matrix() and
// Field::mul alone.  `api_core_check threads` runs the threaded section only (ThreadSanitizer).
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../repair-pipelining_amd/csrc/api_maps.hpp"
#include "../../repair-pipelining_amd/csrc/codec_cache.hpp"

using namespace ecx;

static std::atomic<long> g_checks{0};
#define REQUIRE(c)                                                              \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
            std::_Exit(1);                                                      \
        }                                                                       \
    } while (0)

// ---------------------------------------------------------------- the counted element
struct Obj;
using Reg = RefRegistry<Obj, int>;

static std::atomic<int> g_made{0}, g_gone{0};
static std::mutex g_log_mu;
static std::vector<int> g_destroyed;  // keys, in order of destruction

struct Obj {
    explicit Obj(int k, Reg *back = nullptr) : key(k), back(back) { ++g_made; }
    ~Obj() {
        if (back) {  // comes back to the registry that is destroying it
            int live = -1, idle = -1;
            back->stats(&live, &idle);
            REQUIRE(live >= 0 && idle >= 0);
        }
        ++g_gone;
        std::lock_guard<std::mutex> lk(g_log_mu);
        g_destroyed.push_back(key);
    }
    const int key;
    Reg *const back;
};

static Obj *get(Reg &r, int key) {
    return r.get(key, [&] { return new Obj(key); });
}

struct Stats {
    int live, idle;
    bool operator==(const Stats &o) const { return live == o.live && idle == o.idle; }
};
static Stats stats(Reg &r) {
    Stats s{-1, -1};
    r.stats(&s.live, &s.idle);
    return s;
}

// a pointer to storage that has been freed: whoever reads through it is caught by AddressSanitizer
static Obj *dangling() {
    void *p = std::malloc(sizeof(Obj));
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    std::free(p);
    return reinterpret_cast<Obj *>(addr);
}

// ---------------------------------------------------------------- RefRegistry
static void check_registry() {
    {
        Reg r(8, 3);
        const int made0 = g_made, gone0 = g_gone;
        Obj *a = get(r, 1), *b = get(r, 1);
        REQUIRE(a == b && a->key == 1 && g_made == made0 + 1);
        REQUIRE((stats(r) == Stats{1, 0}));
        Obj *c = get(r, 2);
        REQUIRE(c != a && (stats(r) == Stats{2, 0}));
        r.release(a);
        REQUIRE((stats(r) == Stats{2, 0}));  // b still holds key 1
        r.release(b);
        REQUIRE((stats(r) == Stats{1, 1}) && g_gone == gone0);
        r.release(b);  // a second release of a released pointer
        REQUIRE((stats(r) == Stats{1, 1}) && g_gone == gone0);
        r.release(nullptr);
        r.release(dangling());  // never issued: ignored, not read
        REQUIRE((stats(r) == Stats{1, 1}) && g_gone == gone0);
        Obj *again = get(r, 1);  // revival: the same object, no longer idle
        REQUIRE(again == a && g_made == made0 + 2);  // (keys 1 and 2, nothing built since)
        REQUIRE((stats(r) == Stats{2, 0}));
        r.release(again);
        REQUIRE((stats(r) == Stats{1, 1}));  // one release parks it: the earlier second release took nothing
        r.release(c);
        REQUIRE((stats(r) == Stats{0, 2}) && g_gone == gone0);

        // a make() that throws registers nothing
        bool thrown = false;
        try {
            r.get(55, []() -> Obj * { throw std::runtime_error("invalid geometry"); });
        } catch (const std::runtime_error &) {
            thrown = true;
        }
        REQUIRE(thrown && (stats(r) == Stats{0, 2}) && g_made == made0 + 2);
        Obj *d = get(r, 55);  // the key was absent: built now
        REQUIRE(d->key == 55 && g_made == made0 + 3 && (stats(r) == Stats{1, 2}));
        r.release(d);
    }
    {
        // 10 distinct keys released: 3 stay idle, the 7 least recently released are destroyed, once each
        Reg r(8, 3);
        { std::lock_guard<std::mutex> lk(g_log_mu); g_destroyed.clear(); }
        const int made0 = g_made, gone0 = g_gone;
        std::vector<Obj *> p;
        for (int k = 0; k < 8; ++k) p.push_back(get(r, k));
        REQUIRE((stats(r) == Stats{8, 0}));
        const std::vector<int> order = {5, 0, 7, 2, 6, 1, 4, 3, 8, 9};  // of release
        for (int i = 0; i < 8; ++i) r.release(p[(size_t)order[(size_t)i]]);
        REQUIRE((stats(r) == Stats{0, 3}) && g_gone == gone0 + 5);
        for (int k : {8, 9}) r.release(get(r, k));
        REQUIRE((stats(r) == Stats{0, 3}) && g_made == made0 + 10 && g_gone == gone0 + 7);
        REQUIRE(g_destroyed == std::vector<int>(order.begin(), order.begin() + 7));
        for (int k : {3, 8, 9}) r.release(get(r, k));  // the three kept ones are revived,
        REQUIRE(g_made == made0 + 10);
        r.release(get(r, 4));  // an evicted one is built again
        REQUIRE(g_made == made0 + 11);
    }
    {
        // the 9th distinct live key is a private object: not registered, destroyed by its release
        Reg r(8, 3);
        std::vector<Obj *> p;
        for (int k = 0; k < 8; ++k) p.push_back(get(r, k));
        const int made0 = g_made, gone0 = g_gone;
        Obj *x = get(r, 100), *y = get(r, 100);
        REQUIRE(x != y && x->key == 100 && g_made == made0 + 2);
        REQUIRE((stats(r) == Stats{8, 0}));
        const uintptr_t x_addr = reinterpret_cast<uintptr_t>(x);
        r.release(x);
        REQUIRE(g_gone == gone0 + 1 && (stats(r) == Stats{8, 0}));
        r.release(reinterpret_cast<Obj *>(x_addr));  // again: ignored
        REQUIRE(g_gone == gone0 + 1);
        r.release(y);
        REQUIRE(g_gone == gone0 + 2);
        REQUIRE(get(r, 3) == p[3]);  // the shared ones are as they were
        r.release(p[3]);
        for (Obj *o : p) r.release(o);
        REQUIRE((stats(r) == Stats{0, 3}));
    }
    {
        // a destructor that calls back into the registry: evicted and private objects are destroyed
        // outside the lock, or this never returns (no idle objects kept: every last release evicts)
        Reg r(2, 0);
        const int gone0 = g_gone;
        auto make = [&](int k) { return r.get(k, [&] { return new Obj(k, &r); }); };
        Obj *a = make(1), *b = make(2), *priv = make(3);
        r.release(priv);
        r.release(a);
        r.release(b);
        REQUIRE(g_gone == gone0 + 3 && (stats(r) == Stats{0, 0}));
    }
}

// ---------------------------------------------------------------- LruCache
using Lru = LruCache<int, Obj>;
static std::shared_ptr<Obj> lru_get(Lru &c, int key, size_t cap) {
    return c.get(key, cap, [&] { return std::make_shared<Obj>(key); });
}

static void check_lru() {
    Lru c;
    const int made0 = g_made, gone0 = g_gone;
    std::shared_ptr<Obj> a = lru_get(c, 1, 2), b = lru_get(c, 2, 2);
    REQUIRE(g_made == made0 + 2 && c.size() == 2);
    REQUIRE(lru_get(c, 1, 2) == a && g_made == made0 + 2);  // a hit: the same object, and now the most recent
    Obj *const a_raw = a.get();
    a.reset();
    std::shared_ptr<Obj> d = lru_get(c, 3, 2);  // evicts the least recently used: 2, not 1
    REQUIRE(c.size() == 2 && g_made == made0 + 3);
    REQUIRE(g_gone == gone0);  // b is still held: evicted, alive
    REQUIRE(b->key == 2);
    { std::lock_guard<std::mutex> lk(g_log_mu); g_destroyed.clear(); }
    b.reset();
    REQUIRE(g_gone == gone0 + 1 && g_destroyed == std::vector<int>{2});
    REQUIRE(lru_get(c, 1, 2).get() == a_raw && g_made == made0 + 3);  // 1 was protected by its hit
    REQUIRE(lru_get(c, 2, 2)->key == 2 && g_made == made0 + 4);       // 2 is built again (3 leaves)
    REQUIRE(g_gone == gone0 + 1);                                     // d holds 3
    d.reset();
    REQUIRE(g_gone == gone0 + 2);

    // cap 0: a fresh object per call, nothing stored
    std::shared_ptr<Obj> x = lru_get(c, 7, 0), y = lru_get(c, 7, 0);
    REQUIRE(x != y && g_made == made0 + 6 && c.size() == 2);
    REQUIRE(lru_get(c, 7, 2) != x && g_made == made0 + 7);  // (neither had been kept)
    x.reset();
    y.reset();

    // a smaller cap evicts on the next insert
    REQUIRE(c.size() == 2);
    const int gone1 = g_gone;
    std::shared_ptr<Obj> z = lru_get(c, 9, 1);
    REQUIRE(c.size() == 1 && g_gone == gone1 + 2);
    REQUIRE(lru_get(c, 9, 1) == z);

    // a racing builder: the key arrives while this call builds outside the lock -- the one that
    // is in the cache wins, the second object is dropped
    const int made2 = g_made, gone2 = g_gone;
    std::shared_ptr<Obj> inner;
    std::shared_ptr<Obj> outer = c.get(11, 2, [&] {
        inner = lru_get(c, 11, 2);
        return std::make_shared<Obj>(11);
    });
    REQUIRE(inner && outer == inner && g_made == made2 + 2 && g_gone == gone2 + 1 && c.size() == 2);
    REQUIRE(lru_get(c, 11, 2) == inner && lru_get(c, 9, 2) == z);
}

// ---------------------------------------------------------------- Memo
static void check_memo() {
    struct Key {
        std::vector<uint8_t> present;
        int index;
        bool operator<(const Key &o) const { return std::tie(present, index) < std::tie(o.present, o.index); }
    };
    Memo<Key, Obj> m;
    const int made0 = g_made;
    int calls = 0;
    auto get = [&](const Key &k) { return m.get(k, [&] { ++calls; return k.index; }); };
    Obj *a = get({{1, 0, 1}, 4}), *b = get({{1, 0, 1}, 5}), *c = get({{1, 1, 1}, 4});
    REQUIRE(a != b && a != c && b != c && a->key == 4 && b->key == 5 && calls == 3);
    REQUIRE(get({{1, 0, 1}, 4}) == a && get({{1, 1, 1}, 4}) == c && calls == 3 && g_made == made0 + 3);
    bool thrown = false;
    try {
        m.get(Key{{}, 9}, []() -> int { throw std::runtime_error("no such map"); });
    } catch (const std::runtime_error &) {
        thrown = true;
    }
    REQUIRE(thrown && get({{}, 9})->key == 9 && calls == 4);  // a throw left the key without a value
}

// ---------------------------------------------------------------- threads
static void check_threads() {
    constexpr int kThreads = 8, kOps = 2000, kKeys = 5;
    {
        Reg r(8, 3);
        const int made0 = g_made, gone0 = g_gone;
        // who holds a reference on which key right now (counted down BEFORE the release, so a
        // positive count always means a live object): every such get must give that one pointer
        std::mutex mu;
        Obj *held[kKeys] = {};
        int holders[kKeys] = {};
        std::vector<std::thread> ts;
        for (int t = 0; t < kThreads; ++t)
            ts.emplace_back([&, t] {
                std::mt19937 rng(1234u + (unsigned)t);
                for (int i = 0; i < kOps; ++i) {
                    const int k = (int)(rng() % kKeys);
                    Obj *p = get(r, k);
                    REQUIRE(p->key == k);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (holders[k]++ > 0) REQUIRE(held[k] == p);
                        held[k] = p;
                    }
                    if (rng() % 4 == 0) {  // a second reference of this thread's own
                        Obj *q = get(r, k);
                        REQUIRE(q == p);
                        r.release(q);
                    }
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        --holders[k];
                    }
                    r.release(p);
                }
            });
        for (std::thread &t : ts) t.join();
        const Stats s = stats(r);
        REQUIRE(s.live == 0 && s.idle == 3);
        REQUIRE(g_made - made0 == g_gone - gone0 + s.live + s.idle);
        // no two registered objects share a key: every key gives one pointer, idle or newly built
        std::vector<Obj *> p;
        for (int k = 0; k < kKeys; ++k) p.push_back(get(r, k));
        for (int k = 0; k < kKeys; ++k) REQUIRE(get(r, k) == p[(size_t)k]);
        REQUIRE((stats(r) == Stats{kKeys, 0}));
        REQUIRE(g_made - made0 == g_gone - gone0 + kKeys);
        for (int k = 0; k < kKeys; ++k) {
            r.release(p[(size_t)k]);
            r.release(p[(size_t)k]);
        }
    }
    {
        Lru c;
        const int made0 = g_made, gone0 = g_gone;
        std::vector<std::thread> ts;
        for (int t = 0; t < kThreads; ++t)
            ts.emplace_back([&, t] {
                std::mt19937 rng(99u + (unsigned)t);
                std::shared_ptr<Obj> keep;  // held across calls: evicted values stay alive
                for (int i = 0; i < kOps; ++i) {
                    const int k = (int)(rng() % kKeys);
                    std::shared_ptr<Obj> v = lru_get(c, k, 2);
                    REQUIRE(v && v->key == k);
                    if (keep) REQUIRE(keep->key >= 0 && keep->key < kKeys);
                    if (rng() % 3 == 0) keep = v;
                }
            });
        for (std::thread &t : ts) t.join();
        REQUIRE(c.size() == 2);
        REQUIRE(g_made - made0 == g_gone - gone0 + (int)c.size());
        // the two entries are two keys: each of them hits, the other three build
        int hits = 0;
        for (int k = 0; k < kKeys; ++k) {
            const int before = g_made;
            lru_get(c, k, kKeys + 2);
            hits += g_made == before;
        }
        REQUIRE(hits == 2 && c.size() == (size_t)kKeys);
    }
}

// ---------------------------------------------------------------- maps
// `m` over `rows` output and `cols` input slots, as a dense rows x cols matrix
static std::vector<uint8_t> dense_of(const LinearMap &m, int rows, int cols) {
    REQUIRE((int)m.in_slot.size() == m.n_in && (int)m.out_slot.size() == m.n_out);
    REQUIRE(m.a.size() == (size_t)m.n_in * m.n_out);
    std::vector<uint8_t> d((size_t)rows * cols, 0);
    std::vector<int> seen_in((size_t)cols, 0), seen_out((size_t)rows, 0);
    for (int j = 0; j < m.n_in; ++j) REQUIRE(m.in_slot[j] >= 0 && m.in_slot[j] < cols && !seen_in[(size_t)m.in_slot[j]]++);
    for (int o = 0; o < m.n_out; ++o) REQUIRE(m.out_slot[o] >= 0 && m.out_slot[o] < rows && !seen_out[(size_t)m.out_slot[o]]++);
    for (int o = 0; o < m.n_out; ++o)
        for (int j = 0; j < m.n_in; ++j) d[(size_t)m.out_slot[o] * cols + m.in_slot[j]] = m.at(o, j);
    return d;
}

using Shards = std::vector<std::vector<uint8_t>>;
// rows of the dense matrix `d` (rows x cols) applied to the shards
static Shards apply(const std::vector<uint8_t> &d, int rows, int cols, const Shards &in) {
    const Field &f = Field::get();
    Shards out((size_t)rows, std::vector<uint8_t>(in[0].size(), 0));
    for (int o = 0; o < rows; ++o)
        for (int j = 0; j < cols; ++j)
            for (size_t i = 0; i < in[0].size(); ++i) out[(size_t)o][i] ^= f.mul(d[(size_t)o * cols + j], in[(size_t)j][i]);
    return out;
}

static bool all_zero(const Shards &s) {
    for (const auto &row : s)
        for (uint8_t b : row)
            if (b) return false;
    return true;
}

static void check_rs_maps(int k, int m) {
    const RsCode c(k, m);
    const Matrix &gen = c.matrix();
    const int n = k + m;
    std::mt19937 rng(7u * (unsigned)k + (unsigned)m);

    // the check map is [parityRows | I], entry for entry
    const LinearMap chk = rs_check_map(c);
    REQUIRE(chk.n_out == m);
    for (int p = 0; p < m; ++p) REQUIRE(chk.out_slot[(size_t)p] == p);
    const std::vector<uint8_t> cd = dense_of(chk, m, n);
    for (int p = 0; p < m; ++p)
        for (int j = 0; j < n; ++j)
            REQUIRE(cd[(size_t)p * n + j] == (j < k ? gen.at(k + p, j) : (j == k + p ? 1 : 0)));
    for (int j = 0; j < chk.n_in; ++j) {  // pruned: no column of zeros
        bool any = false;
        for (int p = 0; p < m; ++p) any = any || chk.at(p, j);
        REQUIRE(any);
    }

    // a codeword (random data extended by encode_map) checks to zero in every row; one flipped byte in
    // any one shard does not
    const size_t len = 37;
    Shards word((size_t)n, std::vector<uint8_t>(len));
    for (int j = 0; j < k; ++j)
        for (uint8_t &b : word[(size_t)j]) b = (uint8_t)rng();
    const std::vector<uint8_t> enc = dense_of(c.encode_map(), n, n);
    const Shards coded = apply(enc, n, n, word);
    for (int p = 0; p < m; ++p) word[(size_t)(k + p)] = coded[(size_t)(k + p)];
    REQUIRE(all_zero(apply(cd, m, n, word)));
    for (int s = 0; s < n; ++s) {
        Shards bad = word;
        bad[(size_t)s][rng() % len] ^= (uint8_t)(1u << (rng() % 8));
        REQUIRE(!all_zero(apply(cd, m, n, bad)));
    }
    // checkSomeShards' map is the same construction over the caller's rows
    REQUIRE(map_key(check_map(gen.row(k), m, k)) == map_key(chk));

    // the encode-partial map of every input: that column of the parity rows
    for (int j = 0; j < k; ++j) {
        const LinearMap ep = encode_partial_map(c, j);
        REQUIRE(ep.n_in == 1 && ep.n_out == m && ep.in_slot == std::vector<int>{0} && (int)ep.a.size() == m);
        for (int p = 0; p < m; ++p) REQUIRE(ep.out_slot[(size_t)p] == p && ep.a[(size_t)p] == gen.at(k + p, j));
    }

    // single_input_map of a decode map: the column of the requested shard, zero for one it does not read
    for (const std::vector<int> &erased : {std::vector<int>{0}, std::vector<int>{1, k}}) {
        std::vector<bool> present((size_t)n, true);
        for (int e : erased) present[(size_t)e] = false;
        const LinearMap dm = c.decode_map(present);
        REQUIRE(dm.n_out == (int)erased.size());
        const std::vector<uint8_t> dd = dense_of(dm, n, n);
        for (int s = 0; s < n; ++s) {
            const LinearMap sm = single_input_map(dm, s);
            REQUIRE(sm.n_in == 1 && sm.in_slot == std::vector<int>{0} && sm.n_out == dm.n_out);
            bool reads = false;
            for (int o = 0; o < dm.n_out; ++o) {
                REQUIRE(sm.out_slot[(size_t)o] == o);
                REQUIRE(sm.a[(size_t)o] == dd[(size_t)dm.out_slot[(size_t)o] * n + s]);
                reads = reads || sm.a[(size_t)o];
            }
            if (!present[(size_t)s]) REQUIRE(!reads);
        }
    }
}

static int thrown_code(const RsCode &c, const std::vector<bool> &present, int index, int output_count) {
    try {
        decode_single_map(c, present, index, output_count, true);
    } catch (const Error &e) {
        return e.code;
    }
    return ECX_OK;
}

// decodeMissingSingle over every one- and two-erasure data pattern of RS(4,2)
static void check_decode_single() {
    const RsCode c(4, 2);
    const Matrix &gen = c.matrix();
    const Field &f = Field::get();
    const int k = 4, n = 6;
    for (int mask = 1; mask < (1 << k); ++mask) {
        std::vector<int> missing;
        for (int i = 0; i < k; ++i)
            if (mask >> i & 1) missing.push_back(i);
        if (missing.size() > 2) continue;
        std::vector<bool> present((size_t)n, true);
        for (int i : missing) present[(size_t)i] = false;
        std::vector<int> used;  // decodeMissing's rows: the first k present shards
        for (int i = 0; i < n && (int)used.size() < k; ++i)
            if (present[(size_t)i]) used.push_back(i);
        for (int is_first : {0, 1})
            for (int outputs = 0; outputs <= (int)missing.size(); ++outputs) {
                // row j over index 0..k-1 is a row of D^-1: times the used rows it is a unit vector
                std::vector<std::vector<uint8_t>> row((size_t)outputs, std::vector<uint8_t>((size_t)k));
                for (int index = 0; index < k; ++index) {
                    const LinearMap lm = decode_single_map(c, present, index, outputs, is_first != 0);
                    REQUIRE(lm.n_out == outputs);
                    const std::vector<uint8_t> d = dense_of(lm, outputs, 1 + outputs);
                    for (int j = 0; j < outputs; ++j) {
                        REQUIRE(lm.out_slot[(size_t)j] == j);
                        row[(size_t)j][(size_t)index] = d[(size_t)j * (1 + outputs)];
                        for (int x = 0; x < outputs; ++x)  // the identity on input 1 + j, unless first
                            REQUIRE(d[(size_t)j * (1 + outputs) + 1 + x] == (x == j && !is_first ? 1 : 0));
                    }
                }
                for (int j = 0; j < outputs; ++j)
                    for (int col = 0; col < k; ++col) {
                        uint8_t sum = 0;
                        for (int index = 0; index < k; ++index) sum ^= f.mul(row[(size_t)j][(size_t)index], gen.at(used[(size_t)index], col));
                        REQUIRE(sum == (col == missing[(size_t)j] ? 1 : 0));
                    }
            }
    }
    // its refusals, in the export's order
    const std::vector<bool> one = {true, false, true, true, true, true};
    const std::vector<bool> few = {true, false, false, false, true, true};
    REQUIRE(thrown_code(c, few, -1, 9) == ECX_E_SINGULAR);  // fewer than k present, whatever else is wrong
    REQUIRE(thrown_code(c, one, -1, 3) == ECX_E_INDEX);     // more outputs than parity rows
    REQUIRE(thrown_code(c, one, -1, 2) == ECX_E_NULL);      // more outputs than missing data shards, before the index
    REQUIRE(thrown_code(c, one, -1, 1) == ECX_E_INDEX);
    REQUIRE(thrown_code(c, one, k, 1) == ECX_E_INDEX);
    REQUIRE(thrown_code(c, one, k, 0) == ECX_E_INDEX);
    REQUIRE(thrown_code(c, one, k - 1, 1) == ECX_OK);
}

static LinearMap map_of(int n_out, int n_in, std::vector<uint8_t> a, std::vector<int> in, std::vector<int> out) {
    LinearMap m;
    m.n_out = n_out;
    m.n_in = n_in;
    m.a = std::move(a);
    m.in_slot = std::move(in);
    m.out_slot = std::move(out);
    return m;
}

static void check_rules() {
    // dense_map, scale_map, present_vec
    const uint8_t six[6] = {1, 2, 3, 4, 5, 6};
    const LinearMap dm = dense_map(six, 2, 3);
    REQUIRE(dm.n_out == 2 && dm.n_in == 3 && dm.a == std::vector<uint8_t>(six, six + 6));
    REQUIRE(dm.in_slot == (std::vector<int>{0, 1, 2}) && dm.out_slot == (std::vector<int>{0, 1}));
    const LinearMap set = scale_map(29, false), acc = scale_map(29, true);
    REQUIRE(set.n_out == 1 && set.n_in == 2 && set.a == (std::vector<uint8_t>{29, 0}));  // the zero column stays
    REQUIRE(acc.a == (std::vector<uint8_t>{29, 1}) && acc.in_slot == (std::vector<int>{0, 1}) && acc.out_slot == std::vector<int>{0});
    const uint8_t flags[4] = {1, 0, 200, 0};
    REQUIRE(present_vec(flags, 4) == (std::vector<bool>{true, false, true, false}));

    // the plan cache's key tells maps apart by one coefficient, one slot, and by shape alone
    const LinearMap base = map_of(2, 2, {1, 2, 3, 4}, {0, 1}, {0, 1});
    REQUIRE(map_key(base) == map_key(map_of(2, 2, {1, 2, 3, 4}, {0, 1}, {0, 1})));
    REQUIRE(map_key(base) != map_key(map_of(2, 2, {1, 2, 3, 5}, {0, 1}, {0, 1})));
    REQUIRE(map_key(base) != map_key(map_of(2, 2, {1, 2, 3, 4}, {0, 2}, {0, 1})));
    REQUIRE(map_key(base) != map_key(map_of(2, 2, {1, 2, 3, 4}, {0, 1}, {0, 2})));
    // 1x2 and 2x1 with the same coefficient bytes and the same slot numbers one after the other
    REQUIRE(map_key(map_of(1, 2, {8, 9}, {3, 4}, {4})) != map_key(map_of(2, 1, {8, 9}, {3}, {4, 4})));
    REQUIRE(map_key(map_of(1, 4, {1, 2, 3, 4}, {0, 1, 2, 3}, {0})) != map_key(map_of(4, 1, {1, 2, 3, 4}, {0}, {1, 2, 3, 0})));

    REQUIRE(recommended_pitch(0) == 0);
    REQUIRE(recommended_pitch(1) == 4096);
    REQUIRE(recommended_pitch(4095) == 4096);
    REQUIRE(recommended_pitch(4096) == 4096);
    REQUIRE(recommended_pitch(4097) == 12288);
    REQUIRE(recommended_pitch(8192) == 12288);
    REQUIRE(recommended_pitch(200000) == 200704);
    REQUIRE(recommended_pitch(4194304) == 4198400);

    const int64_t big = std::numeric_limits<int64_t>::max();
    REQUIRE(extent_fits({{4, 100}, {6, 10}}, 10));
    REQUIRE(!extent_fits({{4, -1}}, 10));
    REQUIRE(!extent_fits({{4, 100}, {0, -1}}, 10));  // a negative stride even where nothing is counted
    REQUIRE(!extent_fits({{big / 2, 4}}, 0));        // the product leaves int64_t
    REQUIRE(!extent_fits({{2, big}}, 1));            // the sum does
    REQUIRE(extent_fits({{2, big}}, 0));
    REQUIRE(!extent_fits({{2, big / 2 + 1}, {2, big / 2 + 1}}, 0));
    REQUIRE(extent_fits({{0, big}, {1, big}}, 10));  // no stripes, one stripe: no stride is taken

    // 7 stripes x 6 flags, 3 distinct rows: first-seen order, ids, and refusal at cap 2
    const uint8_t A[6] = {1, 1, 0, 1, 1, 1}, B[6] = {1, 1, 1, 1, 1, 1}, C[6] = {0, 1, 1, 1, 0, 1};
    const uint8_t *rows[7] = {B, A, B, C, A, C, B};
    std::vector<uint8_t> present;
    for (const uint8_t *r : rows)
        for (int i = 0; i < 6; ++i) present.push_back(r[i] ? (uint8_t)(1 + 40 * i) : 0);  // any non-zero is present
    std::vector<uint8_t> patterns(3 * 6, 0xee), ids(7, 0xee);
    REQUIRE(index_patterns(6, present.data(), 7, patterns.data(), 3, ids.data()) == 3);
    REQUIRE(ids == (std::vector<uint8_t>{0, 1, 0, 2, 1, 2, 0}));
    REQUIRE(!std::memcmp(&patterns[0], B, 6) && !std::memcmp(&patterns[6], A, 6) && !std::memcmp(&patterns[12], C, 6));
    int code = ECX_OK;
    try {
        index_patterns(6, present.data(), 7, patterns.data(), 2, ids.data());
    } catch (const Error &e) {
        code = e.code;
    }
    REQUIRE(code == ECX_E_ILLEGAL_ARGUMENT);
    REQUIRE(index_patterns(6, present.data(), 3, patterns.data(), 2, ids.data()) == 2);  // two rows fit
    REQUIRE(index_patterns(6, present.data(), 0, patterns.data(), 1, ids.data()) == 0);

    // the verdict fold: divisor 3 over 4 stripes, one failing unit in stripe 2
    std::vector<uint8_t> unit(12, 1);
    unit[2 * 3 + 1] = 0;
    std::vector<uint8_t> verdict = {0, 7, 0, 0};  // a first pass overwrites whatever was there
    fold_unit_verdicts(unit.data(), 3, true, verdict.data(), 4);
    REQUIRE(verdict == (std::vector<uint8_t>{1, 1, 0, 1}));
    verdict = {1, 0, 1, 1};  // a later pass keeps an earlier 0
    fold_unit_verdicts(unit.data(), 3, false, verdict.data(), 4);
    REQUIRE(verdict == (std::vector<uint8_t>{1, 0, 0, 1}));
    unit.assign(12, 1);
    fold_unit_verdicts(unit.data(), 3, false, verdict.data(), 4);
    REQUIRE(verdict == (std::vector<uint8_t>{1, 0, 0, 1}));
}

int main(int argc, char **argv) {
    alarm(180);  // a deadlock ends here, not at the driver's timeout
    if (argc > 1 && std::string(argv[1]) == "threads") {
        check_threads();
    } else {
        check_registry();
        check_lru();
        check_memo();
        check_threads();
        check_rs_maps(4, 2);
        check_rs_maps(5, 5);
        check_rs_maps(17, 3);
        check_decode_single();
        check_rules();
    }
    REQUIRE(g_made == g_gone);  // everything the caches owned is gone with them
    std::printf("api_core_check: ok (%ld checks)\n", g_checks.load());
    return 0;
}
