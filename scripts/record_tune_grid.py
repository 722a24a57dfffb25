#!/usr/bin/env python3
"""Record what ecx_tune accepts and what ecx_tune_value reads back, over a grid of keys and values.

For every key include/ecx_tune.h documents, plus "no_such_knob" and "", the script reads
ecx_tune_value before any set (the compiled-in default), then tries every value of VALUES in
ascending order through ecx_tune and reads ecx_tune_value after each try.  Per key it records

    {"default": [status, value], "accepted": [values ecx_tune took], "get": the getter's status,
     "read": [the value read back after each try]}          ("read" only where the getter answers)

in a fresh process per mode (the library reads ECX_SHAPE_KNOBS once):

    product        libecx.so, ECX_SHAPE_KNOBS unset
    product_shape  libecx.so, ECX_SHAPE_KNOBS=1
    diag           libecx_diag.so (make DIAG=1), ECX_DIAGNOSTIC unset
    diag_env       libecx_diag.so, ECX_DIAGNOSTIC=1

No device is touched.  The script uses nothing but the two calls, so it runs unchanged against any
build of the library; tests/test_tune_table_native.py compares the committed recording
(tests/golden/tune_grid.json.gz) with the knob table's own grid and with the built library.

    python scripts/record_tune_grid.py --out tests/golden/tune_grid.json.gz
"""
import argparse
import gzip
import json
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "repair-pipelining_amd"
INT_MAX, INT_MIN = 2**31 - 1, -2**31
VALUES = sorted(list(range(-3, 70)) + [127, 128, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537,
                                       2**20 - 1, 2**20, 2**20 + 1, 2**21, INT_MAX, INT_MIN])
# mode -> (library, ECX_SHAPE_KNOBS, ECX_DIAGNOSTIC); the table's --dump takes the same three as 0 / 1
MODES = {
    "product": ("libecx.so", False, False),
    "product_shape": ("libecx.so", True, False),
    "diag": ("libecx_diag.so", False, False),
    "diag_env": ("libecx_diag.so", False, True),
}


def documented_keys():
    """The keys of include/ecx_tune.h's comment, in its order, then the two that are none."""
    text = (ROOT / "include" / "ecx_tune.h").read_text()
    keys = re.findall(r'^ \*   (?:\[DIAG\] )?"(\w+)" ', text, re.M)
    assert len(keys) == len(set(keys)), keys
    return keys + ["no_such_knob", ""]


def grid():
    """This process's library over the grid (ECX_LIB_PATH and the environment as they are)."""
    import ctypes
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    import rpamd
    lib = rpamd.load().lib()
    tune, tune_value = lib.ecx_tune, lib.ecx_tune_value
    tune.argtypes, tune.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    tune_value.argtypes, tune_value.restype = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)], ctypes.c_int
    out = {}

    def get(key):
        v = ctypes.c_int(-77)
        st = tune_value(key, ctypes.byref(v))
        return st, (v.value if st == 0 else None)

    for name in documented_keys():
        key = name.encode()
        rec = {"default": list(get(key)), "accepted": [], "get": None, "read": []}
        for v in VALUES:
            if tune(key, v) == 0:
                rec["accepted"].append(v)
            st, val = get(key)
            assert rec["get"] in (None, st), (name, v, st)
            rec["get"] = st
            rec["read"].append(val)
        assert rec["get"] == rec["default"][0], name
        if rec["get"] != 0:
            del rec["read"]
        out[name] = rec
    return out


def mode_env(mode, env=None):
    """The environment of a fresh process for `mode`."""
    libname, shape, diagnostic = MODES[mode]
    e = {k: v for k, v in (os.environ if env is None else env).items()
         if k not in ("ECX_SHAPE_KNOBS", "ECX_DIAGNOSTIC", "ECX_LIB_PATH")}
    e["ECX_LIB_PATH"] = str(PKG / libname)
    if shape:
        e["ECX_SHAPE_KNOBS"] = "1"
    if diagnostic:
        e["ECX_DIAGNOSTIC"] = "1"
    return e


def run_mode(mode):
    """grid() of a fresh process in `mode`."""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=mode_env(mode),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def read_fixture(path):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help="print this process's grid as one JSON line")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(grid(), separators=(",", ":")))
        return
    if not args.out:
        ap.error("--out is required")
    for mode, (libname, _, _) in MODES.items():
        if not (PKG / libname).exists():
            sys.exit("%s is not built (make -C repair-pipelining_amd%s)" % (libname, " DIAG=1" if "diag" in libname else ""))
    rec = {"values": VALUES, "keys": documented_keys(), "modes": {m: run_mode(m) for m in MODES}}
    text = json.dumps(rec, separators=(",", ":"), sort_keys=True)
    with open(args.out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as f:
        f.write(text.encode())
    print("recorded %d keys x %d values in %d modes: %d bytes of JSON, %d in %s" %
          (len(rec["keys"]), len(VALUES), len(MODES), len(text), os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
