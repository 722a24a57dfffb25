// tune_table.hpp -- the ecx_tune keys (include/ecx_tune.h) as one table: a key's class, the values
// it accepts and where its value lives.  No HIP header and no environment: the caller passes what it
// read (tests/native/tune_table_check.cpp drives every environment from one program).
#pragma once

#include "tuning.hpp"

namespace ecx {

// deployment: what a production caller may set, always accepted and the only keys ecx_tune_value
// answers.  shape: changes a kernel's launch shape (same results, other speed): the diagnostic
// library, or a process that opted in with ECX_SHAPE_KNOBS=1.  lab: the measured-and-rejected
// kernels and builds: the diagnostic library only.
enum class KnobClass { deployment, shape, lab };
// value: field = v.  flag: field = (v != 0), any v.  kib: wide = v << 10.  external: checked here,
// kept by the caller ("roctx": an atomic every ABI call reads without the tuning lock).
enum class KnobStore { value, flag, kib, external };
// Values whose builds do not compute the repair.  lookahead_bit4: bit 4 needs the diagnostic library
// and ECX_DIAGNOSTIC=1.  nonzero: any value but 0 needs ECX_DIAGNOSTIC=1.
enum class KnobGate { none, lookahead_bit4, nonzero };

struct Knob {
    const char *name;
    KnobClass cls;
    KnobStore store;
    int lo, hi;            // accepts lo..hi, or, where n_only > 0, only[0 .. n_only)
    int only[9], n_only;
    int Tuning::*field;    // value, flag
    int64_t Tuning::*wide;  // kib
    KnobGate gate;
};

struct KnobEnv {
    bool diag_build, shape_opt_in, diagnostic_env;  // make DIAG=1, ECX_SHAPE_KNOBS=1, ECX_DIAGNOSTIC=1
};

const Knob *knob_table(int *count);
const Knob *find_knob(const char *name);  // null for an unknown or a null name
// Sets the key's field; false = refused (the class, the range or the gate), `t` as it was.
bool knob_set(Tuning &t, const Knob &k, int value, const KnobEnv &env);
// The key's value in ecx_tune's units; false for an external key.
bool knob_get(const Tuning &t, const Knob &k, int *value);

}  // namespace ecx
