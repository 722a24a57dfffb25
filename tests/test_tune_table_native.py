"""The ecx_tune knob table (csrc/tune_table.cpp: every key's class, accepted values and storage) is
plain C++ with no HIP header: built here from that one file, with no ROCm include path, together
with tests/native/tune_table_check.cpp, and run as a program of its own -- once as an ordinary
build and, where the compiler has them, once under AddressSanitizer + UndefinedBehaviorSanitizer
(host code only, as tests/test_native.py).  tests/golden/tune_grid.json.gz is what ecx_tune and
ecx_tune_value answered over a grid of keys and values before the table existed, recorded by
scripts/record_tune_grid.py from the product and the diagnostic library: the table's own grid
(--dump) must equal it in all four modes, and so must the built product library's."""
import importlib.util
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRCS = [ROOT / "tests" / "native" / "tune_table_check.cpp",
        ROOT / "repair-pipelining_amd" / "csrc" / "tune_table.cpp"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
FIXTURE = ROOT / "tests" / "golden" / "tune_grid.json.gz"


def load_recorder():
    spec = importlib.util.spec_from_file_location("record_tune_grid", ROOT / "scripts" / "record_tune_grid.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    return gxx


def _build(gxx, exe, extra):
    subprocess.run([gxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror"] + extra + ["-o", str(exe)] +
                   [str(s) for s in SRCS], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([str(exe)] + list(args), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _parse_dump(text):
    """The --dump of tune_table_check as (values, the recorder's per-key records)."""
    lines = text.splitlines()
    assert lines[0].startswith("values ")
    values = [int(x) for x in lines[0].split()[1:]]
    out = {}
    for line in lines[1:]:
        tag, name, rest = line.split('"')
        assert tag == "key "
        f = [int(x) for x in rest.split()]
        st, dflt, tries = f[0], f[1], f[2:]
        assert len(tries) == 2 * len(values), name
        rec = {"default": [st, dflt if st == 0 else None], "get": st,
               "accepted": [v for v, a in zip(values, tries[0::2]) if a]}
        if st == 0:
            rec["read"] = tries[1::2]
        assert name not in out
        out[name] = rec
    return values, out


def _check_table(exe):
    assert "tune_table_check: ok" in _run(exe)
    rec = load_recorder()
    fixture = rec.read_fixture(FIXTURE)
    assert fixture["values"] == rec.VALUES and fixture["keys"] == rec.documented_keys()
    assert sorted(fixture["modes"]) == sorted(rec.MODES)
    for mode, (libname, shape, diagnostic) in rec.MODES.items():
        values, got = _parse_dump(_run(exe, "--dump", str(int("diag" in libname)), str(int(shape)),
                                       str(int(diagnostic))))
        assert values == fixture["values"], mode
        want = fixture["modes"][mode]
        assert sorted(got) == sorted(want), mode
        for key in want:
            assert got[key] == want[key], (mode, key)


@pytest.mark.timeout(300)
def test_tune_table(tmp_path):
    _check_table(_build(_gxx(), tmp_path / "tune_table_check", []))


@pytest.mark.timeout(300)
def test_tune_table_under_asan_ubsan(tmp_path):
    gxx = _gxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("this compiler has no address / undefined sanitizers")
    _check_table(_build(gxx, tmp_path / "tune_table_check_san", SANITIZE))


@pytest.mark.timeout(600)
def test_library_answers_the_recorded_grid():
    """The built product library's ecx_tune / ecx_tune_value over the same grid, in a fresh process
    without and with ECX_SHAPE_KNOBS=1 (the library reads it once): what was recorded."""
    rec = load_recorder()
    fixture = rec.read_fixture(FIXTURE)
    for mode in ("product", "product_shape"):
        got = rec.run_mode(mode)
        assert sorted(got) == sorted(fixture["modes"][mode]) == sorted(fixture["keys"]), mode
        for key, want in fixture["modes"][mode].items():
            assert got[key] == want, (mode, key)
