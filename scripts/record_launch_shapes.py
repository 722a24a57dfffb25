#!/usr/bin/env python3
"""Record the launch shape the library chooses over a grid of maps, batch layouts and knobs.

One JSON line per case: the inputs and the string ecx.last_launch_shape() reports after the
real launch.  The script uses nothing but tune, apply_batch, accumulate_batch and
last_launch_shape, so it runs unchanged against any build of the library (ECX_LIB_PATH); two
builds choose the same shapes exactly when their files are byte-identical.  The file recorded
on an MI355X is committed under tests/golden/, and tests/test_planner.py replays every line
through GfMap.launch_plan on the CPU (replay() below; the diagnostic library's lines are
replayed by the `diag`-marked test of tests/test_gpu_parity.py).

    python scripts/record_launch_shapes.py --out shapes.jsonl           # the loaded library
    ECX_LIB_PATH=.../libecx_diag.so python scripts/record_launch_shapes.py --out shapes.jsonl --append

A call that launches no full-chunk kernel (an unaligned layout, a shard under one chunk) leaves
the string of the call before it: the lines are in launch order and the replay carries that
state (replay() below).  The product library runs the full cross product of the layout axes and
every knob value on every map over four layouts; the diagnostic library, whose layout rules are
the same code, runs a corner of the grid, every knob and its own knobs.  The file is committed
gzip-compressed (tests/golden/launch_shapes.jsonl.gz: `gzip -n -9` of this script's output).
"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NBYTES = (64, 1072, 4000, 4096, 8176, 8208, 16384, 65536, 200000)
OFFSETS = (0, 16, 1)
PITCH_KINDS = ("r16", "pad", "200704", "4m")
MAX_BUFFER = 24 << 30  # a cell whose three stripes would need more runs one stripe

# one at a time from the defaults, over every value include/ecx_tune.h documents
KNOBS = (
    ("depth", (2, 4, 8, 10, 12, 16, 20, 24)),
    ("nontemporal", (0, 2)),
    ("store_scope", (1,)),
    ("small_tiles", (0, 1)),
    ("wide_tiles", (0, 2)),
    ("lds_tables", (0, 2)),
    ("block_threads", (64, 256)),
    ("skew_chunks", (0, 2, 4)),
    ("xcd_group", (1, 2, 3)),
    ("xcd_misaligned", (0,)),
    ("stagger", (1, 2, 3, 8, 64)),
    ("chunk_major", (1,)),
    ("map_planes", (0, 2)),
)
# the lab kernels' knobs: the diagnostic library only
KNOBS_DIAG = (
    ("wave_groups", (1, 2)),
    ("bitslice", (1, 2)),
    ("lds_lut", (1, 2)),
    ("units", (2, 4)),
    ("occ_lds", (-1, 4096)),
)
KNOB_DEFAULTS = {"depth": 0, "nontemporal": 1, "store_scope": 0, "small_tiles": 2, "wide_tiles": 1, "lds_tables": 1,
                 "block_threads": 0, "skew_chunks": 1, "xcd_group": 0, "xcd_misaligned": 1, "stagger": 0,
                 "chunk_major": 0, "map_planes": 1}
KNOB_DEFAULTS_DIAG = {"wave_groups": 0, "bitslice": 0, "lds_lut": 0, "units": 1, "occ_lds": 0}
KNOB_LAYOUTS = ((8208, "r16", 16), (200000, "r16", 0), (8208, "4m", 0), (200000, "4m", 0))
KNOB_LAYOUTS_DIAG = ((8208, "r16", 16), (200000, "4m", 0))
CAND_CALLS = 7 * 5


def build_maps(ecx):
    """name -> GfMap of the grid's maps (host-only: no device is touched)."""
    import numpy as np
    rs124, rs173, rs42 = (ecx.ReedSolomon.create(k, m) for k, m in ((12, 4), (17, 3), (4, 2)))
    clay = {e: ecx.ClayCodeErasureDecodingStep(list(e), 4, 2) for e in ((1,), (4, 5), (0, 3))}
    clay104 = ecx.ClayCodeErasureDecodingStep([3], 10, 4, virtualUnits=2)
    maps = {
        "rs124_dec01": rs124.decode_map([False, False] + [True] * 14),
        "rs173_enc": rs173.encode_map(),
        "rs42_enc": rs42.encode_map(),
        "lrc_rep0": ecx.LRCErasureCode.map([False] + [True] * 15),
        "lrc_enc": ecx.LRCErasureCode.map(),
        "clay42_rep1": clay[(1,)].map(),
        "clay42_enc45": clay[(4, 5)].map(),
        "clay42_rep03": clay[(0, 3)].map(),
        "clay104_rep3": clay104.map(),
        "partial1": ecx.GfMap.from_matrix(np.array([[3], [7]], np.uint8)),
    }
    maps["_owners"] = (rs124, rs173, rs42, clay, clay104)
    return maps


def pitch_of(kind, nbytes):
    return {"r16": (nbytes + 15) // 16 * 16, "pad": nbytes + 4096 + 48, "200704": 200704, "4m": 4 << 20}[kind]


def layout(gmap, case):
    """(in offset, in stripe stride, slot pitch, out offset or None for in place, out stripe stride, slot pitch,
    bytes of the input buffer, bytes of the output buffer) of a recorded case."""
    mi, mo = gmap.max_slots()
    p = pitch_of(case["p"], case["n"])
    if case["ip"]:
        slots = max(mi, mo) + 1
        return case["o"], slots * p, p, None, slots * p, p, case["S"] * slots * p + 4096, 0
    return (case["o"], (mi + 1) * p, p, case["o"], (mo + 1) * p, p, case["S"] * (mi + 1) * p + 4096,
            case["S"] * (mo + 1) * p + 4096)


def cases(map_names, diag):
    """The grid, in launch order (without the candidate path: candidate_case)."""
    out = []

    def add(name, n, p, o, ip, acc, S, k=""):
        out.append({"map": name, "n": n, "p": p, "o": o, "ip": ip, "acc": acc, "S": S, "k": k, "diag": diag})

    if diag:  # the layout rules are the product library's: a corner of the grid, every combination
        for name in map_names:
            for n, p, o in KNOB_LAYOUTS_DIAG:
                for combo in range(8):
                    add(name, n, p, o, combo & 1, (combo >> 1) & 1, 3 if combo & 4 else 1)
    else:  # the full cross product
        for name in map_names:
            for n in NBYTES:
                for p in PITCH_KINDS:
                    for o in OFFSETS:
                        for combo in range(8):
                            add(name, n, p, o, combo & 1, (combo >> 1) & 1, 3 if combo & 4 else 1)
    # the bit-plane auto threshold: nstripes * (nbytes / 4096) * used inputs >= 16384
    for S in (64, 63):
        add("clay42_rep03", 32768, "r16", 0, 0, 0, S)
    for key, values in KNOBS + (KNOBS_DIAG if diag else ()):
        for v in values:
            for name in map_names:
                for n, p, o in (KNOB_LAYOUTS_DIAG if diag else KNOB_LAYOUTS):
                    add(name, n, p, o, 0, 0, 3, "%s=%d" % (key, v))
    return out


def candidate_case(gmap, diag):
    """The per-layout candidate path: a batch of >= 256 MiB of input at a 4 MiB pitch."""
    n_in = gmap.info()["n_in"]
    S = max(4, -(-(256 << 20) // (n_in * (4 << 20))))
    return {"map": "rs124_dec01", "n": 4 << 20, "p": "4m", "o": 0, "ip": 1, "acc": 0, "S": S, "k": "", "diag": diag}


def read_lines(path):
    """The recorded cases of a .jsonl or .jsonl.gz file."""
    import gzip
    with (gzip.open if str(path).endswith(".gz") else open)(path, "rt") as f:
        return [json.loads(l) for l in f]


def plan_of(gmap, case, cand=0):
    """GfMap.launch_plan for a recorded case, without a device: the case's layout at made-up
    addresses with the recorded alignment (in place, or two buffers far apart)."""
    io, iss, isl, oo, oss, osl, _, _ = layout(gmap, case)
    inp = (1 << 40) + io
    out = inp if oo is None else (1 << 44) + oo
    return gmap.launch_plan(inp, iss, isl, out, oss, osl, case["S"], case["n"], bool(case["acc"]), cand)


def replay(ecx, lines, plan=plan_of):
    """Check every line recorded from the loaded library's kind (`diag`) against
    plan(gmap, case, cand) -> GfMap.launch_plan's string; returns how many were checked.  A
    call that leaves no kernel of record keeps the string of the call before it, and so does a
    `refused` one (a forced shape without a kernel instance: the launch threw before it ran)."""
    lines = [r for r in lines if r["diag"] == int(ecx.is_diag())]
    maps = build_maps(ecx)
    last_knob, state = None, ""
    try:
        for r in lines:
            if r["k"] != last_knob:
                set_knob(ecx, r["k"])
                last_knob = r["k"]
            # the candidate path: call i of a fresh layout explores candidate i mod 7
            got = plan(maps[r["map"]], r, r["call"] % 7 if "call" in r else 0)
            assert isinstance(got, str), r
            if not r.get("refused"):
                state = got or state
            assert state == r["shape"], (r, got)
    finally:
        set_knob(ecx, "")
    return len(lines)


def set_knob(ecx, k):
    """Every knob of the grid back to its default, then the case's one."""
    for key, v in dict(KNOB_DEFAULTS, **(KNOB_DEFAULTS_DIAG if ecx.is_diag() else {})).items():
        ecx.tune(key, v)
    if k:
        key, _, v = k.partition("=")
        ecx.tune(key, int(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--append", action="store_true", help="append to --out (the second library of a pair)")
    args = ap.parse_args()
    import rpamd
    import torch
    ecx = rpamd.load(shape_knobs=True)
    diag = int(ecx.is_diag())
    maps = build_maps(ecx)
    names = [k for k in maps if not k.startswith("_")]
    bufs = {}

    def buffer(tag, nbytes):
        if bufs.get(tag) is None or bufs[tag].numel() < nbytes:
            bufs[tag] = None
            bufs[tag] = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        return bufs[tag].data_ptr()

    def run(gmap, case):
        if case["S"] == 3 and layout(gmap, case)[6] > MAX_BUFFER:
            case = dict(case, S=1)
        io, iss, isl, oo, oss, osl, in_bytes, out_bytes = layout(gmap, case)
        inp = buffer("in", in_bytes) + io
        out = inp if oo is None else buffer("out", out_bytes) + oo
        f = gmap.accumulate_batch if case["acc"] else gmap.apply_batch
        try:
            f(inp, iss, isl, out, oss, osl, case["S"], case["n"])
        except ecx.EcxError as e:  # a forced shape no kernel instance exists for: refused, nothing faulted
            if e.code != -1:
                raise
            return dict(case, shape=ecx.last_launch_shape(), refused=1)
        return dict(case, shape=ecx.last_launch_shape())

    lines = []
    last_knob = None
    for i, case in enumerate(cases(names, diag)):
        if case["k"] != last_knob:
            set_knob(ecx, case["k"])
            last_knob = case["k"]
        lines.append(run(maps[case["map"]], case))
        if i % 256 == 255:
            torch.cuda.synchronize()
    set_knob(ecx, "")
    fresh = build_maps(ecx)  # a map no layout has been selected for
    cand = candidate_case(fresh["rs124_dec01"], diag)
    for i in range(0 if diag else CAND_CALLS):  # the selection is the same code in both libraries
        lines.append(dict(run(fresh["rs124_dec01"], cand), call=i))
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        for rec in lines:
            f.write(json.dumps(rec, separators=(",", ":")) + "\n")
    print("recorded %d cases (diag=%d), %d distinct shapes, %d bytes in %s" %
          (len(lines), diag, len({r["shape"] for r in lines}), os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
