"""The Clay codeword check through the generated JNI forwarder (jni/ecx_jni.c) over the fake JNIEnv
(tests/jni_harness.py; no JDK here): clayIsParityCorrectBatch takes a geometry and device addresses
(longs) only, so nothing is pinned; negative counts are IllegalArgumentException, null addresses
NullPointerException, an empty batch touches nothing, before a device is needed.  On the GPU one
Clay(4,2) pool through the forwarder gives the verdicts of tests/clay_check_cases.py."""
import re

import pytest

import clay_check_cases as C
from jni_harness import Jni, ROOT

OK, ILL, NUL = 0, -1, -6


@pytest.fixture(scope="module")
def jni():
    j = Jni()
    yield j
    j.free_all()


@pytest.fixture
def J(jni):
    jni.reset()
    yield jni
    c = jni.counters()
    assert c["pins_now"] == 0 and c["pins"] == c["unpins"], c
    assert c["violations"] == 0 and c["calls_while_pinned"] == 0, c


def test_forwarder_argument_rules(J):
    """clayIsParityCorrectBatch(dataUnits, parityUnits, virtualUnits, base, stripeStride, subStride,
    nstripes, bufSize, verdict, stream): one forwarder for the export, nothing pinned."""
    assert "clayIsParityCorrectBatch" in J.sigs
    f = lambda **kw: J.call("clayIsParityCorrectBatch", kw.get("k", 4), kw.get("m", 2), kw.get("v", 0),  # noqa: E731
                            kw.get("base", 4096), kw.get("ss", 48 * 64), kw.get("sub", 64), kw.get("S", 2),
                            kw.get("B", 64), kw.get("verdict", 8192), 0)
    assert f(S=-1) == ILL and f(B=-1) == ILL
    assert f(k=0) == ILL and f(m=0) == ILL and f(v=-1) == ILL
    assert f(S=0, base=0, verdict=0, ss=-1) == OK  # an empty batch touches nothing
    assert f(base=0) == NUL and f(verdict=0) == NUL
    assert f(ss=-1) == ILL and f(sub=-1) == ILL
    assert f(ss=1 << 62, S=4) == ILL                # the extent is beyond int64_t
    assert f(k=9, m=9) == ILL and f(k=5, m=2) == ILL  # more than 8 parity units; seven nodes on a 2 x 3 grid
    assert J.counters()["pins"] == 0


def test_wrapper_uses_the_native_and_keeps_addresses_in_the_package():
    """EcxClayParityCheck is a thin wrapper over the native: the call that takes device addresses is
    package-private, close() is idempotent and releases the codec once."""
    src = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxClayParityCheck.java").read_text()
    for native in ("clayIsParityCorrectBatch", "clayCreateShortened", "clayGeometry", "clayDestroy"):
        assert "EcxNative.%s(" % native in src, native
    assert re.search(r"\n    void isParityCorrectBatch\(long base,", src), "package-private: no access modifier"
    assert "public void isParityCorrectBatch(" not in src and "public int[] geometry()" in src
    close = re.search(r"public synchronized void close\(\) \{(.*?)\n    \}", src, flags=re.S).group(1)
    assert "if (clay == 0)" in close and "clay = 0;" in close
    assert close.index("clay = 0;") < close.index("EcxNative.clayDestroy(")


@pytest.mark.gpu
def test_check_through_the_forwarder(J, ecx):
    """Clay(4,2), the 48 sub-chunk sites at 4096 + 16 bytes (a vector body and a byte-safe tail)."""
    import torch
    B = C.CHUNK + 16
    case = C.subchunk_case(4, 2, 0, B)
    flat, view, stride = C.device_pool(case, torch)
    S = case.nstripes
    verdict = torch.full((S + 16,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert J.call("clayIsParityCorrectBatch", 4, 2, 0, view.data_ptr(), stride, case.pitch, S, B, verdict.data_ptr(),
                  0) == OK
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == case.want.tolist() + [9] * 16
