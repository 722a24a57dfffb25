"""What the C ABI owns and decides besides its launches is plain C++ with no HIP header: the codec
registry, the per-call plan cache and the per-codec map tables (csrc/codec_cache.hpp, header-only),
and the coefficient maps and small rules of the per-call, partial-sum, layout and check exports
(csrc/api_maps.cpp).  Built here with gf.cpp and codes.cpp and no ROCm include path, together with
tests/native/api_core_check.cpp -- which counts the objects the caches own and compares every map
with a definition it computes from the generator matrix -- and run as a program of its own: once
as an ordinary build, once under AddressSanitizer + UndefinedBehaviorSanitizer, and its threaded
section once under ThreadSanitizer, where the compiler has them (host code only, as
tests/test_native.py).  The program ends itself if a cache deadlocks."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "repair-pipelining_amd" / "csrc"
SRCS = [ROOT / "tests" / "native" / "api_core_check.cpp", CSRC / "api_maps.cpp", CSRC / "gf.cpp", CSRC / "codes.cpp"]
ASAN_UBSAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
TSAN = ["-fsanitize=thread", "-fno-omit-frame-pointer"]


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    return gxx


def _require(gxx, tmp_path, flags, what):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip(f"this compiler has no {what}")
    if subprocess.run([str(tmp_path / "probe")], capture_output=True, timeout=60).returncode != 0:
        pytest.skip(f"an empty program does not start under the {what} here")


def _build_and_run(gxx, exe, extra, args=()):
    subprocess.run([gxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-pthread"] + extra + ["-o", str(exe)] +
                   [str(s) for s in SRCS], check=True)
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "api_core_check: ok" in r.stdout


@pytest.mark.timeout(300)
def test_api_core(tmp_path):
    _build_and_run(_gxx(), tmp_path / "api_core_check", [])


@pytest.mark.timeout(300)
def test_api_core_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    _require(gxx, tmp_path, ASAN_UBSAN, "address / undefined sanitizers")
    _build_and_run(gxx, tmp_path / "api_core_check_san", ASAN_UBSAN)


@pytest.mark.timeout(300)
def test_api_core_threads_under_tsan(tmp_path):
    gxx = _gxx()
    _require(gxx, tmp_path, TSAN, "thread sanitizer")
    _build_and_run(gxx, tmp_path / "api_core_check_tsan", TSAN, ["threads"])
