// tune_table_check.cpp -- the ecx_tune knob table (csrc/tune_table.cpp), on the CPU: built from that
// one file with no ROCm include path (tests/test_tune_table_native.py).
//
// It asserts that the names are unique and found by name; that the deployment and lab classes are
// the lists named here; that every row accepts its own default (what knob_get reads from a
// default-constructed Tuning) in the diagnostic library; that knob_get after knob_set returns the
// value set, for the deployment keys; that a refused set leaves the Tuning as it was; and what is
// stored for the `!= 0` keys and the `<< 10` keys (INT_MAX KiB without overflow).
//
// With --dump <diag> <opt_in> <diagnostic> (0 / 1 each) it prints the table's own grid for that
// environment, as scripts/record_tune_grid.py records the library's: first the values, then per key
//   name default_status default_value get_status  { accepted value_read_back }
// with the caller's side of ecx_tune / ecx_tune_value (csrc/ecx_api.cpp) restated in tune() / get().
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../repair-pipelining_amd/csrc/tune_table.hpp"

using namespace ecx;

static long g_checks = 0;
#define REQUIRE(c)                                                              \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static const char *const kDeployment[] = {"host_chunk_kib", "host_buffers", "host_gather_kib", "host_zero_copy",
                                          "host_contexts", "host_exec_kib", "roctx", "plan_cache", "layout_select"};
static const char *const kLab[] = {"bitslice", "lds_lut", "wave_groups", "rtc_units", "rtc_persist", "rtc_diag",
                                   "occ_lds", "units"};

static std::vector<int> grid_values() {
    std::vector<int> v{INT_MIN};
    for (int i = -3; i <= 69; ++i) v.push_back(i);
    for (int x : {127, 128, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, (1 << 20) - 1, 1 << 20, (1 << 20) + 1,
                  1 << 21, INT_MAX})
        v.push_back(x);
    return v;
}

// ecx_tune and ecx_tune_value as ecx_api.cpp builds them on the table (status 0 / -1); "roctx" lives
// with the caller
struct Library {
    Tuning t;
    int roctx = 0;
    KnobEnv env;
    int tune(const char *key, int value) {
        const Knob *k = find_knob(key);
        if (!k || !knob_set(t, *k, value, env)) return -1;
        if (k->store == KnobStore::external) roctx = value;
        return 0;
    }
    int get(const char *key, int *value) const {
        const Knob *k = find_knob(key);
        if (!k || k->cls != KnobClass::deployment) return -1;
        if (!knob_get(t, *k, value)) *value = roctx;
        return 0;
    }
};

static int dump(bool diag, bool opt_in, bool diagnostic) {
    const std::vector<int> values = grid_values();
    std::printf("values");
    for (int v : values) std::printf(" %d", v);
    std::printf("\n");
    int count = 0;
    const Knob *table = knob_table(&count);
    std::vector<std::string> keys;
    for (int i = 0; i < count; ++i) keys.push_back(table[i].name);
    keys.push_back("no_such_knob");
    keys.push_back("");
    Library lib{Tuning{}, 0, KnobEnv{diag, opt_in, diagnostic}};
    for (const std::string &key : keys) {
        int v = 0;
        const int st = lib.get(key.c_str(), &v);
        std::printf("key \"%s\" %d %d", key.c_str(), st, st ? 0 : v);
        for (int x : values) {
            const int set = lib.tune(key.c_str(), x);
            int r = 0;
            if (lib.get(key.c_str(), &r) != st) return 1;
            std::printf(" %d %d", set == 0, st ? 0 : r);
        }
        std::printf("\n");
    }
    return 0;
}

template <size_t N>
static std::set<std::string> names(const char *const (&list)[N]) {
    return std::set<std::string>(list, list + N);
}

int main(int argc, char **argv) {
    if (argc == 5 && std::strcmp(argv[1], "--dump") == 0)
        return dump(argv[2][0] == '1', argv[3][0] == '1', argv[4][0] == '1');
    int count = 0;
    const Knob *table = knob_table(&count);
    const KnobEnv lab{true, false, true}, product{false, false, false};
    std::set<std::string> seen, deployment, labs;
    for (int i = 0; i < count; ++i) {
        const Knob &k = table[i];
        REQUIRE(seen.insert(k.name).second);
        REQUIRE(find_knob(k.name) == &k);
        if (k.cls == KnobClass::deployment) deployment.insert(k.name);
        if (k.cls == KnobClass::lab) labs.insert(k.name);
        // the compiled-in default is a value the key takes, and setting it changes nothing
        Tuning t;
        int dflt = 0, back = -77;
        if (knob_get(t, k, &dflt)) {
            REQUIRE(knob_set(t, k, dflt, lab));
            REQUIRE(knob_get(t, k, &back) && back == dflt);
        } else {
            REQUIRE(k.store == KnobStore::external && knob_set(t, k, 0, lab));
        }
        // one home per row
        REQUIRE((k.store == KnobStore::kib) == (k.wide != nullptr));
        REQUIRE((k.store == KnobStore::value || k.store == KnobStore::flag) == (k.field != nullptr));
        REQUIRE(k.n_only >= 0 && k.n_only <= (int)(sizeof(k.only) / sizeof(k.only[0])));
    }
    REQUIRE(deployment == names(kDeployment) && deployment.size() == 9);
    REQUIRE(labs == names(kLab) && labs.size() == 8);
    REQUIRE(find_knob(nullptr) == nullptr && find_knob("") == nullptr && find_knob("no_such_knob") == nullptr);
    REQUIRE(find_knob("depth ") == nullptr && find_knob("dept") == nullptr);

    // the deployment keys read back what was set, in the product library without any opt-in
    for (const char *name : kDeployment) {
        const Knob &k = *find_knob(name);
        if (k.store == KnobStore::external) continue;
        for (int v : grid_values()) {
            Tuning t;
            int before = 0, after = -77;
            REQUIRE(knob_get(t, k, &before));
            if (knob_set(t, k, v, product)) {
                REQUIRE(knob_get(t, k, &after) && after == (k.store == KnobStore::flag ? v != 0 : v));
            } else {  // refused: untouched
                REQUIRE(knob_get(t, k, &after) && after == before);
            }
        }
    }
    // the stored fields
    {
        Tuning t;
        for (const char *name : {"store_scope", "chunk_major", "host_zero_copy", "rtc_group"})
            for (int v : {INT_MIN, -1, 0, 1, 2, INT_MAX}) {
                int got = -77;
                REQUIRE(knob_set(t, *find_knob(name), v, lab) && knob_get(t, *find_knob(name), &got) && got == (v != 0));
            }
        REQUIRE(knob_set(t, *find_knob("store_scope"), 7, lab) && t.store_scope == 1);
        REQUIRE(knob_set(t, *find_knob("host_zero_copy"), 0, product) && t.host_zero_copy == 0);
        REQUIRE(knob_set(t, *find_knob("host_chunk_kib"), INT_MAX, product) && t.host_chunk == (int64_t)INT_MAX * 1024);
        REQUIRE(knob_set(t, *find_knob("host_chunk_kib"), 1, product) && t.host_chunk == 1024);
        REQUIRE(!knob_set(t, *find_knob("host_chunk_kib"), 0, product) && t.host_chunk == 1024);
        REQUIRE(knob_set(t, *find_knob("host_gather_kib"), INT_MAX, product) &&
                t.host_gather_max == (int64_t)INT_MAX * 1024);
        REQUIRE(knob_set(t, *find_knob("host_gather_kib"), 0, product) && t.host_gather_max == 0);
        REQUIRE(!knob_set(t, *find_knob("host_gather_kib"), -1, product));
        REQUIRE(knob_set(t, *find_knob("host_exec_kib"), 1 << 20, product) && t.host_exec_max == (int64_t)1 << 30);
        REQUIRE(!knob_set(t, *find_knob("host_exec_kib"), (1 << 20) + 1, product) && t.host_exec_max == (int64_t)1 << 30);
        REQUIRE(knob_set(t, *find_knob("depth"), 24, lab) && t.depth == 24);
        REQUIRE(!knob_set(t, *find_knob("depth"), 6, lab) && t.depth == 24);
    }
    // the classes and the two gates, over the four environments
    for (int e = 0; e < 8; ++e) {
        const KnobEnv env{(e & 1) != 0, (e & 2) != 0, (e & 4) != 0};
        Tuning t;
        REQUIRE(knob_set(t, *find_knob("plan_cache"), 7, env));
        REQUIRE(knob_set(t, *find_knob("nontemporal"), 2, env) == (env.diag_build || env.shape_opt_in));
        REQUIRE(knob_set(t, *find_knob("bitslice"), 1, env) == env.diag_build);
        REQUIRE(knob_set(t, *find_knob("rtc_lookahead"), 15, env) == (env.diag_build || env.shape_opt_in));
        REQUIRE(knob_set(t, *find_knob("rtc_lookahead"), 16, env) == (env.diag_build && env.diagnostic_env));
        REQUIRE(knob_set(t, *find_knob("rtc_diag"), 0, env) == env.diag_build);
        REQUIRE(knob_set(t, *find_knob("rtc_diag"), 1, env) == (env.diag_build && env.diagnostic_env));
    }
    std::printf("tune_table_check: ok (%d keys, %ld checks)\n", count, g_checks);
    return 0;
}
