"""The partial-sum plan of a Clay pattern set (csrc/clay_partial_plan.cpp: the tiled plan cut by
input node into [256][n][T] tile records, and the host interpreter that reads the plan as
k_gf_map_partial_mixed does) is plain C++ with no HIP header: built here from that file,
csrc/mixed_plan.cpp (the tiled plan it starts from), csrc/codes.cpp (the planner's repair maps) and
csrc/gf.cpp (the field), with no ROCm include path, together with
tests/native/clay_partial_plan_check.cpp, and run as a program of its own -- once as an ordinary
build and, where the compiler has them, once under AddressSanitizer + UndefinedBehaviorSanitizer
(host code only, as tests/test_partial_plan_native.py).  The check prints the largest entry count
of a (list, node, tile) record per geometry; DESIGN.md section 4.7.4 quotes those lines."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "repair-pipelining_amd" / "csrc"
SRCS = [ROOT / "tests" / "native" / "clay_partial_plan_check.cpp", CSRC / "clay_partial_plan.cpp",
        CSRC / "mixed_plan.cpp", CSRC / "codes.cpp", CSRC / "gf.cpp"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
GEOMETRIES = ["Clay(4,2) n=6 alpha=8 lists=22", "Clay(4,2) n=6 alpha=8 lists=6", "Clay(2,2) n=4 alpha=4",
              "Clay(3,3) n=6 alpha=9", "Clay(6,2) n=8 alpha=16"]


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    return gxx


def _build_and_run(gxx, exe, extra):
    subprocess.run([gxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror"] + extra + ["-o", str(exe)] +
                   [str(s) for s in SRCS], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clay_partial_plan_check: ok" in r.stdout
    for g in GEOMETRIES:  # the largest per-record entry count of every geometry is reported
        assert re.search(re.escape(g) + r".*largest \(list, node, tile\) record \d+ entries", r.stdout), r.stdout


@pytest.mark.timeout(300)
def test_clay_partial_plan(tmp_path):
    _build_and_run(_gxx(), tmp_path / "clay_partial_plan_check", [])


@pytest.mark.timeout(300)
def test_clay_partial_plan_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "clay_partial_plan_check_san", SANITIZE)
