"""The split of a mixed decode's pass into launches (csrc/mixed_launch.hpp: per launch its units,
the id of its first unit's stripe and the VerdictDiv the kernel divides with) is plain C++ with no
HIP header: built here with no ROCm include path from tests/native/mixed_launch_check.cpp, and run
as a program of its own -- once as an ordinary build and, where the compiler has them, once under
AddressSanitizer + UndefinedBehaviorSanitizer (host code only, as
tests/test_blocked_layout_native.py)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRCS = [ROOT / "tests" / "native" / "mixed_launch_check.cpp"]
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
    assert "mixed_launch_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_mixed_launch_split(tmp_path):
    _build_and_run(_gxx(), tmp_path / "mixed_launch_check", [])


@pytest.mark.timeout(300)
def test_mixed_launch_split_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "mixed_launch_check_san", SANITIZE)
