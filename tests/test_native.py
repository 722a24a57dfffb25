"""Host-only native checks under AddressSanitizer + UndefinedBehaviorSanitizer:
the planner (gf.cpp, codes.cpp) compiled with g++ together with
tests/native/planner_check.cpp, which round-trips codewords through the
composed RS / Clay / shortened-Clay / LRC maps with a dense host application.
(GPU sanitizers are not available; the sanitizers cover host code only.)"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.timeout(300)
def test_planner_round_trips_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "planner_check"
    srcs = [ROOT / "tests" / "native" / "planner_check.cpp", ROOT / "repair-pipelining_amd" / "csrc" / "gf.cpp",
            ROOT / "repair-pipelining_amd" / "csrc" / "codes.cpp"]
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-o", str(exe)] + [str(s) for s in srcs], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "planner_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_host_executor_under_asan_ubsan(tmp_path):
    """The per-call host executor (host_exec.cpp, ecx_tune "host_exec_kib") at every
    instruction-set level this CPU has -- AVX-512BW + GFNI affine multiplies, AVX2 nibble
    tables, scalar product rows -- against Field::mul and a dense application: every product,
    random maps at every vector / block boundary, aliasing outputs, the all-zero check."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "host_exec_check"
    srcs = [ROOT / "tests" / "native" / "host_exec_check.cpp", ROOT / "repair-pipelining_amd" / "csrc" / "host_exec.cpp",
            ROOT / "repair-pipelining_amd" / "csrc" / "gf.cpp", ROOT / "repair-pipelining_amd" / "csrc" / "codes.cpp"]
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-o", str(exe)] + [str(s) for s in srcs], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_exec_check: ok" in r.stdout
    assert "isa 2: not on this CPU" not in r.stdout or "isa 1: not on this CPU" not in r.stdout


@pytest.mark.timeout(300)
def test_launch_rules_invariants_under_asan_ubsan(tmp_path):
    """The launch rules (csrc/launch_rules.cpp: which kernels a batch launches, in what shape) are
    plain C++ with no HIP header: built here from that one file, with no ROCm include path, and
    walked over a dense grid of synthetic map traits x batch layouts x knobs by
    tests/native/launch_rules_check.cpp, which asserts for every plan that the launches tile the
    shard's chunks exactly once, that only byte-safe launches touch bytes outside full aligned
    chunks (but for a fused tail, and that only when no output is read), and that no kernel is
    chosen on a layout it cannot address."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "launch_rules_check"
    srcs = [ROOT / "tests" / "native" / "launch_rules_check.cpp",
            ROOT / "repair-pipelining_amd" / "csrc" / "launch_rules.cpp"]
    subprocess.run([gxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-o", str(exe)] + [str(s) for s in srcs],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "launch_rules_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_layout_selection_rules_and_recorded_trace_under_asan_ubsan(tmp_path):
    """The per-layout launch-shape decisions (csrc/layout_select.cpp: which candidate a call runs,
    when it is timed, what is kept) are plain C++ with no HIP header: built here from that one file,
    with no ROCm include path, and driven by tests/native/layout_select_check.cpp -- seeded random
    scripts of picks, reports (clean, contaminated, failed) and cancels with the selection's
    invariants asserted after every operation, then tests/golden/layout_trace.txt.gz, the decisions
    recorded by scripts/record_layout_trace.py from the code the table was split out of, replayed
    line for line."""
    import gzip
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "layout_select_check"
    srcs = [ROOT / "tests" / "native" / "layout_select_check.cpp",
            ROOT / "repair-pipelining_amd" / "csrc" / "layout_select.cpp"]
    subprocess.run([gxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-o", str(exe)] + [str(s) for s in srcs],
                   check=True)
    trace = tmp_path / "layout_trace.txt"
    trace.write_bytes(gzip.decompress((ROOT / "tests" / "golden" / "layout_trace.txt.gz").read_bytes()))
    r = subprocess.run([str(exe), str(trace)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "layout_select_check: ok" in r.stdout
    assert f"{len(trace.read_text().splitlines())} trace lines replayed" in r.stdout


UNIT_ORDER_BEGIN = "// Logical work index of this workgroup"
UNIT_ORDER_END = "// One output tile over the workgroup's"


def unit_order_slice(apply_hpp: str) -> str:
    """The text of logical_block and unit_of, comments included, as it stands in csrc/apply.hpp."""
    a, b = apply_hpp.index(UNIT_ORDER_BEGIN), apply_hpp.index(UNIT_ORDER_END)
    text = apply_hpp[a:b]
    assert a < b and text.count("__device__ __forceinline__") == 2, "apply.hpp: logical_block / unit_of moved"
    assert "uint32_t logical_block(int xcd_group, uint32_t n_tiles, uint32_t run)" in text
    assert "void unit_of(uint32_t u, uint32_t nc, uint32_t nst, int chunk_major, uint32_t G," in text
    return text


@pytest.mark.timeout(300)
def test_unit_orders_are_bijections_under_asan_ubsan(tmp_path):
    """Which (stripe, chunk, tile) a workgroup of the composed-map kernels computes (csrc/apply.hpp
    logical_block and unit_of) is decided from blockIdx.x and gridDim.x inside the device functions.
    Their text is cut out of apply.hpp unchanged and compiled on the host by
    tests/native/unit_order_check.cpp, with blockIdx / gridDim as variables the check sets: it walks
    every grid size 1..4096 the launcher can produce over 1, 2, 3, 5 and 32 tiles, every xcd_group,
    xcd_run 1 / 3 / 8 / 4096, 1..9 chunks, the staggers and chunk_major, and asserts that the
    workgroups hit every (tile, stripe, chunk) exactly once -- a mapping that does not leaves stale
    bytes in the output."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "unit_order_check"
    (tmp_path / "unit_order_slice.inc").write_text(
        unit_order_slice((ROOT / "repair-pipelining_amd" / "csrc" / "apply.hpp").read_text()))
    subprocess.run([gxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-I", str(tmp_path), "-o", str(exe),
                    str(ROOT / "tests" / "native" / "unit_order_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unit_order_check: ok" in r.stdout
