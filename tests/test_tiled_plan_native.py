"""The tiled plan of a pattern set (csrc/mixed_plan.cpp build_tiled_plan: [256][T] tile records for
maps of up to 8 tiles, each tile's entries padded to the set's load-ring depth, and the
out-of-place host interpreter that reads the plan as k_gf_map_mixed does) is plain C++ with no HIP
header: built here from that file and csrc/gf.cpp, with no ROCm include path, together with
tests/native/tiled_plan_check.cpp, and run as a program of its own -- once as an ordinary build
and, where the compiler has them, once under AddressSanitizer + UndefinedBehaviorSanitizer (host
code only, as tests/test_mixed_plan_native.py)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "repair-pipelining_amd" / "csrc"
SRCS = [ROOT / "tests" / "native" / "tiled_plan_check.cpp", CSRC / "mixed_plan.cpp", CSRC / "gf.cpp"]
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
    assert "tiled_plan_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_tiled_plan(tmp_path):
    _build_and_run(_gxx(), tmp_path / "tiled_plan_check", [])


@pytest.mark.timeout(300)
def test_tiled_plan_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "tiled_plan_check_san", SANITIZE)
