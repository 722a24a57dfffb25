"""The Clay codeword-test program (clay_check_program, csrc/clay_check_plan.cpp: the per-plane
syndrome form, its dense map and the two proofs it must pass before anyone may run it) is plain
C++ with no HIP header: built here from that file, csrc/codes.cpp (the planner) and csrc/gf.cpp
(the field), with no ROCm include path, together with tests/native/clay_check_plan_check.cpp, and run as a program of its
own -- once as an ordinary build and, where the compiler has them, once under AddressSanitizer +
UndefinedBehaviorSanitizer (host code only, as tests/test_clay_partial_plan_native.py).  The check
prints what the proof of each geometry cost; DESIGN.md section 4.9 quotes those lines."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "repair-pipelining_amd" / "csrc"
SRCS = [ROOT / "tests" / "native" / "clay_check_plan_check.cpp", CSRC / "clay_check_plan.cpp", CSRC / "codes.cpp",
        CSRC / "gf.cpp"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
GEOMETRIES = ["Clay(2,2) n_real=4 alpha=4", "Clay(4,2) n_real=6 alpha=8", "Clay(6,3) n_real=9 alpha=27",
              "Clay(12,4) n_real=16 alpha=256", "Clay(10,4) v=2 n_real=14 alpha=256"]


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
    assert "clay_check_plan_check: ok" in r.stdout
    for g in GEOMETRIES:  # every geometry proved itself and reported its cost
        assert re.search(re.escape(g) + r": proved in \d+ ms, widest row \d+ of \d+", r.stdout), r.stdout


@pytest.mark.timeout(300)
def test_clay_check_plan(tmp_path):
    _build_and_run(_gxx(), tmp_path / "clay_check_plan_check", [])


@pytest.mark.timeout(300)
def test_clay_check_plan_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "clay_check_plan_check_san", SANITIZE)
