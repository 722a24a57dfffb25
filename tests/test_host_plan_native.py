"""The plans of the host-memory batches (csrc/host_plan.cpp: the runs of a stripe's used slots, the
folded 2D, 3D and plain copies that move them, the chunking rule and its 160-row floor, column
slices, the mixed decode's in-place plan, stripe_range and the column split over a device list)
are plain C++ with no HIP header: built here from that one file, with no ROCm include path,
together with tests/native/host_plan_check.cpp -- which expands every plan into the rows it moves
and compares them with the definition, byte for byte -- and run as a program of its own, once as
an ordinary build and, where the compiler has them, once under AddressSanitizer +
UndefinedBehaviorSanitizer (host code only, as tests/test_native.py).  tests/test_host_plan.py
pins the same fixed cases through the library."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRCS = [ROOT / "tests" / "native" / "host_plan_check.cpp",
        ROOT / "repair-pipelining_amd" / "csrc" / "host_plan.cpp"]
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
    assert "host_plan_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_host_plan(tmp_path):
    _build_and_run(_gxx(), tmp_path / "host_plan_check", [])


@pytest.mark.timeout(300)
def test_host_plan_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "host_plan_check_san", SANITIZE)
