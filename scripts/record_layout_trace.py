#!/usr/bin/env python3
"""Record what the per-layout launch-shape selection decided BEFORE its rules became
csrc/layout_select.cpp: tests/golden/layout_trace.txt.gz.

Recorded from commit c04b685ab33a7d06bd6130ba2ccde1097e2ccf24, the last one whose selection lived
in CompiledMap (engine.cpp harvest / next_layout_pick / fill_layout_probe / cancel_layout_probe /
layout_choice).  The text of those five functions, of their constants and of the LayoutSel struct
is lifted out of that commit with `git show`, unaltered, and compiled against the fake events of
scripts/layout_trace_driver.cpp, which runs a fixed set of seeded scripts through it and prints one
line per operation (the format is in that file's header).  tests/native/layout_select_check.cpp
replays the operations against LayoutTable and requires identical lines, so the tie-breaks and the
order of the tests of a pick are the recorded commit's.

    python scripts/record_layout_trace.py            # rewrites tests/golden/layout_trace.txt.gz

The fixture is written only if the run covers every branch listed in coverage() below.
"""
import argparse
import gzip
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
COMMIT = "c04b685ab33a7d06bd6130ba2ccde1097e2ccf24"
CSRC = "repair-pipelining_amd/csrc/"
FIXTURE = ROOT / "tests" / "golden" / "layout_trace.txt.gz"
MAX_LAYOUTS = 64  # kMaxLayouts of the recorded commit

# what is lifted: (file, first line starts with, last line is)
FUNCS = [(CSRC + "engine.cpp", "void CompiledMap::harvest(", "}"),
         (CSRC + "engine.cpp", "int CompiledMap::next_layout_pick(", "}"),
         (CSRC + "engine.cpp", "void CompiledMap::fill_layout_probe(", "}"),
         (CSRC + "engine.cpp", "void CompiledMap::cancel_layout_probe(", "}"),
         (CSRC + "engine.cpp", "int CompiledMap::layout_choice(", "}")]
CONSTS = [(CSRC + "engine.cpp", "constexpr float kLayoutMargin", None),
          (CSRC + "engine.cpp", "constexpr size_t kMaxLayouts", None),
          (CSRC + "engine.cpp", "constexpr int kLayoutMaxDropped", None),
          (CSRC + "engine.cpp", "constexpr int64_t kLayoutRevalidate", None),
          (CSRC + "engine.cpp", "float median_of(", "}")]
CLASS = [(CSRC + "engine.hpp", "    enum LayoutState {", "                       kLayoutContended = 4 };"),
         (CSRC + "engine.hpp", "    struct LayoutSel {", "    };")]
RULES = [(CSRC + "launch_rules.hpp", "constexpr int kLayoutCand[]", None),
         (CSRC + "launch_rules.hpp", "constexpr int kLayoutNCand", None),
         (CSRC + "kernels.hip", "constexpr int kLayoutSamples", None)]


def lift(sources, spec):
    """The lines of `file` from the one that starts with `first` through the next that equals `last`."""
    file, first, last = spec
    if file not in sources:
        sources[file] = subprocess.run(["git", "-C", str(ROOT), "show", f"{COMMIT}:{file}"], check=True,
                                       capture_output=True, text=True).stdout.split("\n")
    lines = sources[file]
    begin = [i for i, l in enumerate(lines) if l.startswith(first)]
    assert len(begin) == 1, (file, first, begin)
    end = begin[0] if last is None else next(i for i in range(begin[0], len(lines)) if lines[i] == last)
    return "\n".join(lines[begin[0]:end + 1]) + "\n"


def record():
    sources = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        (tmp / "parent_rules.inc").write_text("".join(lift(sources, s) for s in RULES))
        (tmp / "parent_class.inc").write_text("".join(lift(sources, s) for s in CLASS))
        (tmp / "parent_funcs.inc").write_text("namespace {\n" + "".join(lift(sources, s) for s in CONSTS) + "}\n" +
                                              "".join(lift(sources, s) for s in FUNCS))
        exe = tmp / "layout_trace_driver"
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(tmp), "-o", str(exe),
                        str(ROOT / "scripts" / "layout_trace_driver.cpp")], check=True)
        return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout


def coverage(trace):
    """What the recorded run exercised, from its own lines: name -> seen."""
    seen = {f"state {s}": False for s in range(5)}
    seen.update({k: False for k in (
        "re-validation keeps a non-static shape", "re-validation replaces a non-static shape",
        "re-validation keeps a static shape", "re-validation replaces a static shape",
        "contended layout", "all in flight while exploring", "all in flight while re-validating",
        "cancel between reserve and fill", "failed probe", "probe reported after the choice", "key past the limit",
        "times inside the margin", "times outside the margin", "two layouts at one pitch")})
    for line in trace.splitlines():
        op, _, readout = line.partition(" | ")
        op, readout = op.split(), readout.split()
        if op[0] == "S":
            keys, picked, last, reserved, late = {}, [], {}, set(), set()
            continue
        if op[0] == "K":
            keys[int(op[1])] = op[2:]
            if sum(k[0] == op[2] for k in keys.values()) > 1:
                seen["two layouts at one pitch"] = True
            continue
        k = int(op[1])
        choice, state = (int(readout[0]), int(readout[1])) if readout[0] != "-1" else (-1, 0)
        if choice >= 0:
            seen[f"state {state}"] = True
            med = [float.fromhex(m) for m in readout[3:]]
            for m in med[1:]:  # a shape faster than the static rules: by less than the 2 % margin, or more
                if 0 < m < med[0]:
                    seen["times inside the margin" if m >= 0.98 * med[0] else "times outside the margin"] = True
        else:
            seen["state 0"] = True
        if op[0] == "P":
            cand, ticket = int(op[2]), int(op[3])
            if k not in picked:
                picked.append(k)
            past = picked.index(k) >= MAX_LAYOUTS
            if past:
                assert (cand, ticket, choice) == (0, 0, -1), line
                seen["key past the limit"] = True
            elif not ticket and choice < 0:
                seen["all in flight while exploring"] = True
            elif not ticket and state == 2:
                seen["all in flight while re-validating"] = True
            # shared pitches: the read-out may be the other layout's, so outcomes are read off unshared ones
            shared = sum(v[0] == keys[k][0] for v in keys.values()) > 1
            before = last.get(k)
            if not shared and before and before[1] == 2 and state == 3:
                kept = "keeps" if choice == before[0] else "replaces"
                seen[f"re-validation {kept} a {'static' if before[0] == 0 else 'non-static'} shape"] = True
            if state == 4:
                seen["contended layout"] = True
            if k in late:
                seen["probe reported after the choice"] = True
            if ticket:
                reserved.add(ticket)
            last[k] = (choice, state)
        elif op[0] == "X" and int(op[2]) in reserved:
            seen["cancel between reserve and fill"] = True
        elif op[0] == "F":
            reserved.discard(int(op[2]))
        elif op[0] == "D":
            if op[3] == "f":
                seen["failed probe"] = True
            if choice >= 0 and state != 2:
                late.add(k)
    return seen


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", type=Path, default=FIXTURE)
    args = ap.parse_args()
    trace = record()
    seen = coverage(trace)
    # A kept static choice whose runner-up is itself (no re-validation) needs a layout with a single
    # candidate; the library always passes kLayoutNCand = 7, where the runner-up is another shape,
    # so the recorded code cannot reach it and it is not required.
    missing = [k for k, v in seen.items() if not v]
    print(f"{len(trace.splitlines())} lines from {COMMIT[:7]}; covered: {', '.join(k for k, v in seen.items() if v)}")
    if missing:
        sys.exit("NOT written, the run does not cover: " + ", ".join(missing))
    with open(args.out, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as z:
        z.write(trace.encode())
    print(f"wrote {args.out} ({args.out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
