"""The locate plan of an RS code (csrc/locate_plan.cpp: n candidates with m - 1 test rows each, cut
into tiles of exactly m entry records in syndrome order, and the host interpreter that reads the
plan as k_gf_locate does) is plain C++ with no HIP header: built here from that file, csrc/codes.cpp
(the codec's parity rows) and csrc/gf.cpp (the field), with no ROCm include path, together with
tests/native/locate_plan_check.cpp, and run as a program of its own -- once as an ordinary build
and, where the compiler has them, once under AddressSanitizer + UndefinedBehaviorSanitizer (host
code only, as tests/test_partial_plan_native.py)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "repair-pipelining_amd" / "csrc"
SRCS = [ROOT / "tests" / "native" / "locate_plan_check.cpp", CSRC / "locate_plan.cpp", CSRC / "codes.cpp",
        CSRC / "gf.cpp"]
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
    assert "locate_plan_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_locate_plan(tmp_path):
    _build_and_run(_gxx(), tmp_path / "locate_plan_check", [])


@pytest.mark.timeout(300)
def test_locate_plan_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "locate_plan_check_san", SANITIZE)
