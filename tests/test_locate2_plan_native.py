"""The pair plan of an RS code (csrc/locate2_plan.cpp: C(n,2) pairs with m - 2 test rows each, cut
into tiles of exactly m entry records in syndrome order, the pair-member table, and the host
interpreter that reads both plans as k_gf_locate2 does, with the wave shortcut and without) is plain
C++ with no HIP header: built here from that file, csrc/locate_plan.cpp, csrc/codes.cpp and
csrc/gf.cpp, with no ROCm include path, together with tests/native/locate2_plan_check.cpp, and run as
a program of its own -- once as an ordinary build and, where the compiler has them, once under
AddressSanitizer + UndefinedBehaviorSanitizer (host code only, as tests/test_locate_plan_native.py)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "repair-pipelining_amd" / "csrc"
SRCS = [ROOT / "tests" / "native" / "locate2_plan_check.cpp", CSRC / "locate2_plan.cpp", CSRC / "locate_plan.cpp",
        CSRC / "codes.cpp", CSRC / "gf.cpp"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


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
    assert "locate2_plan_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_locate2_plan(tmp_path):
    _build_and_run(_gxx(), tmp_path / "locate2_plan_check", [])


@pytest.mark.timeout(300)
def test_locate2_plan_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "locate2_plan_check_san", SANITIZE)
