// tune_table.cpp -- the ecx_tune keys, one row each, in include/ecx_tune.h's order (tune_table.hpp).
#include "tune_table.hpp"

#include <climits>
#include <cstring>
#include <initializer_list>

namespace ecx {
namespace {
using T = Tuning;
constexpr KnobClass kDeploy = KnobClass::deployment, kShape = KnobClass::shape, kLab = KnobClass::lab;

constexpr Knob range(const char *name, KnobClass cls, int lo, int hi, int T::*f, KnobGate gate = KnobGate::none) {
    return {name, cls, KnobStore::value, lo, hi, {}, 0, f, nullptr, gate};
}
constexpr Knob only(const char *name, KnobClass cls, std::initializer_list<int> values, int T::*f) {
    Knob k = range(name, cls, 0, 0, f);
    for (int v : values) k.only[k.n_only++] = v;
    return k;
}
constexpr Knob flag(const char *name, KnobClass cls, int T::*f) {
    return {name, cls, KnobStore::flag, INT_MIN, INT_MAX, {}, 0, f, nullptr, KnobGate::none};
}
constexpr Knob kib(const char *name, int lo, int hi, int64_t T::*f) {
    return {name, kDeploy, KnobStore::kib, lo, hi, {}, 0, nullptr, f, KnobGate::none};
}

constexpr Knob kTable[] = {
    only("depth", kShape, {0, 2, 4, 8, 10, 12, 16, 20, 24}, &T::depth),
    range("nontemporal", kShape, 0, 2, &T::nontemporal),
    range("xcd_group", kShape, 0, 3, &T::xcd_group),
    range("xcd_run", kShape, 1, 4096, &T::xcd_run),
    range("xcd_misaligned", kShape, 0, 1, &T::xcd_misaligned),
    range("lds_tables", kShape, 0, 2, &T::lds_tables),
    flag("store_scope", kShape, &T::store_scope),
    flag("chunk_major", kShape, &T::chunk_major),
    range("stagger", kShape, 0, 64, &T::stagger),
    only("block_threads", kShape, {0, 64, 256}, &T::block_threads),
    range("small_tiles", kShape, 0, 2, &T::small_tiles),
    range("plan_cache", kDeploy, 0, 4096, &T::plan_cache),
    only("skew_chunks", kShape, {0, 1, 2, 4}, &T::skew_chunks),
    range("layout_select", kDeploy, 0, 1, &T::layout_select),
    range("wide_tiles", kShape, 0, 2, &T::wide_tiles),
    range("clay_rtc", kShape, 0, 2, &T::clay_rtc),
    range("rtc_lookahead", kShape, 0, 31, &T::rtc_lookahead, KnobGate::lookahead_bit4),
    range("rtc_waves", kShape, 2, 4, &T::rtc_waves),
    flag("rtc_group", kShape, &T::rtc_group),
    range("rtc_sched", kShape, 0, 2, &T::rtc_sched),
    range("rtc_wide", kShape, 0, 1, &T::rtc_wide),
    range("rtc_nt", kShape, 0, 15, &T::rtc_nt),
    range("rtc_xcd", kShape, 0, 4, &T::rtc_xcd),
    range("map_planes", kShape, 0, 2, &T::map_planes),
    range("planes_lookahead", kShape, 0, 15, &T::planes_lookahead),
    range("planes_waves", kShape, 1, 4, &T::planes_waves),
    range("host_contexts", kDeploy, 0, 1, &T::host_contexts),
    {"roctx", kDeploy, KnobStore::external, 0, 1, {}, 0, nullptr, nullptr, KnobGate::none},
    kib("host_chunk_kib", 1, INT_MAX, &T::host_chunk),
    range("host_buffers", kDeploy, 1, 8, &T::host_buffers),
    kib("host_gather_kib", 0, INT_MAX, &T::host_gather_max),
    kib("host_exec_kib", 0, 1 << 20, &T::host_exec_max),
    flag("host_zero_copy", kDeploy, &T::host_zero_copy),
    range("wave_groups", kLab, 0, 2, &T::wave_groups),
    range("occ_lds", kLab, -1, 65536, &T::occ_lds),
    range("bitslice", kLab, 0, 2, &T::bitslice),
    range("lds_lut", kLab, 0, 2, &T::lds_lut),
    range("rtc_diag", kLab, 0, 31, &T::rtc_diag, KnobGate::nonzero),
    range("rtc_units", kLab, 1, 2, &T::rtc_units),
    only("units", kLab, {1, 2, 4}, &T::units),
    range("rtc_persist", kLab, 0, 8, &T::rtc_persist),
};

bool accepts(const Knob &k, int value) {
    if (k.n_only == 0) return value >= k.lo && value <= k.hi;
    for (int i = 0; i < k.n_only; ++i)
        if (k.only[i] == value) return true;
    return false;
}
}  // namespace

const Knob *knob_table(int *count) {
    *count = (int)(sizeof(kTable) / sizeof(kTable[0]));
    return kTable;
}

const Knob *find_knob(const char *name) {
    for (const Knob &k : kTable)
        if (name && std::strcmp(k.name, name) == 0) return &k;
    return nullptr;
}

bool knob_set(Tuning &t, const Knob &k, int value, const KnobEnv &env) {
    if (k.cls == KnobClass::lab && !env.diag_build) return false;
    if (k.cls != KnobClass::deployment && !env.diag_build && !env.shape_opt_in) return false;
    if (!accepts(k, value)) return false;
    if (k.gate == KnobGate::lookahead_bit4 && (value & 16) && !(env.diag_build && env.diagnostic_env)) return false;
    if (k.gate == KnobGate::nonzero && value != 0 && !env.diagnostic_env) return false;
    if (k.store == KnobStore::value) t.*k.field = value;
    else if (k.store == KnobStore::flag) t.*k.field = value != 0;
    else if (k.store == KnobStore::kib) t.*k.wide = (int64_t)value << 10;
    return true;
}

bool knob_get(const Tuning &t, const Knob &k, int *value) {
    if (k.store == KnobStore::external) return false;
    *value = k.store == KnobStore::kib ? (int)(t.*k.wide >> 10) : t.*k.field;
    return true;
}

}  // namespace ecx
