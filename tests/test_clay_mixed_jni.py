"""The Clay pattern-set exports through the generated JNI forwarders (jni/ecx_jni.c) over the fake
JNIEnv (tests/jni_harness.py; no JDK here): the two int[] arguments of the create -- the list counts
and the lists back to back -- are read with GetIntArrayRegion and never pinned; a count array shorter
than npatterns, a list array shorter than the counts add up to, a negative count, a handle of 0 and
null arrays are refused before the export.  Both batch calls take addresses (longs) only, so they
have nothing to pin; the host form's native is package-private."""
import re

import numpy as np
import pytest

from jni_harness import Jni, ROOT

OK, ILL, IDX, NUL = 0, -1, -5, -6


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


def _create(J, lists, k=4, m=2, v=0, erased=..., counts=..., npatterns=None, out=...):
    flat = np.array([e for lst in lists for e in lst], np.int32)
    cnt = np.array([len(lst) for lst in lists], np.int32)
    h = np.zeros(1, np.int64)
    st = J.call("clayPatternSetCreate", k, m, v, J.array(flat if erased is ... else erased),
                J.array(cnt if counts is ... else counts), len(lists) if npatterns is None else npatterns,
                J.array(h if out is ... else out))
    return st, int(h[0])


def test_clay_pattern_set_create_argument_checks(J):
    lists = [[1], [0, 3], [], [5]]
    assert _create(J, lists, counts=np.array([1, 2, 0], np.int32))[0] == IDX          # counts shorter than npatterns
    assert _create(J, lists, erased=np.array([1, 0, 3], np.int32))[0] == IDX          # lists shorter than their sum
    assert _create(J, lists, counts=np.array([1, 2, -1, 1], np.int32))[0] == ILL      # a negative count
    assert _create(J, lists, npatterns=-1)[0] == ILL
    assert _create(J, lists, erased=None)[0] == NUL and _create(J, lists, counts=None)[0] == NUL
    assert _create(J, lists, out=None)[0] == NUL
    assert _create(J, lists, out=np.zeros(0, np.int64))[0] == IDX
    assert J.counters()["pins"] == 0
    # the export's own refusals come through: 0 lists, an out-of-range node, more than 64 rows
    assert _create(J, lists, npatterns=0) == (ILL, 0)
    assert _create(J, [[1], [6]])[0] < 0
    assert _create(J, [[0, 1, 2]], k=6, m=3) == (ILL, 0)
    # a valid call: neither int[] was pinned; info reads the set back
    st, h = _create(J, lists)
    assert st == OK and h != 0 and J.counters()["pins"] == 0
    n, nodes, alpha, erased = (np.zeros(1, np.int32) for _ in range(4))
    assert J.call("clayPatternSetInfo", h, J.array(n), J.array(nodes), J.array(alpha), J.array(erased)) == OK
    assert (n[0], nodes[0], alpha[0], erased[0]) == (4, 6, 8, 2)
    assert J.call("clayPatternSetInfo", h, None, None, None, J.array(erased)) == OK        # each may be null
    assert J.call("clayPatternSetInfo", h, J.array(np.zeros(0, np.int32)), None, None, None) == IDX
    assert J.call("clayPatternSetInfo", 0, J.array(n), J.array(nodes), J.array(alpha), J.array(erased)) == NUL
    # longer arrays than needed are fine: only the counted part is read
    st, h2 = _create(J, lists, erased=np.array([1, 0, 3, 5, 9, 9], np.int32))
    assert st == OK
    J.call("clayPatternSetDestroy", h2)
    # the device batch: addresses only; a handle of 0, null addresses and negative counts never reach a device
    args = (16, 4096, 48 * 64, 64, 8192, 16 * 64, 64)
    assert J.call("clayPerformCodingBatchMixed", 0, *args, 1, 64, 0) == NUL
    assert J.call("clayPerformCodingBatchMixed", h, *args, -1, 64, 0) == ILL
    assert J.call("clayPerformCodingBatchMixed", h, *args, 1, -1, 0) == ILL
    assert J.call("clayPerformCodingBatchMixed", h, 0, *args[1:], 1, 64, 0) == NUL
    assert J.call("clayPerformCodingBatchMixed", h, 16, 0, *args[2:], 1, 64, 0) == NUL
    assert J.call("clayPerformCodingBatchMixed", h, *args[:4], 0, 16 * 64, 64, 1, 64, 0) == NUL
    assert J.call("clayPerformCodingBatchMixed", h, *args, 0, 64, 0) == OK                  # empty batch
    # the host plan: seven longs
    plan = np.zeros(7, np.int64)
    assert J.call("clayPatternSetHostPlan", h, 48 * 64, 64, 16 * 64, 64, 5, 64, J.array(plan)) == OK
    assert plan[1] == 16 and plan[2] * plan[3] >= 5
    assert J.call("clayPatternSetHostPlan", h, 48 * 64, 64, 16 * 64, 64, 5, 64, J.array(plan[:6].copy())) == IDX
    assert J.call("clayPatternSetHostPlan", h, 48 * 64, 64, 16 * 64, 64, 5, 64, None) == NUL
    assert J.call("clayPatternSetHostPlan", 0, 48 * 64, 64, 16 * 64, 64, 5, 64, J.array(plan)) == NUL
    assert J.call("clayPatternSetHostPlan", h, 48 * 64, 64, 16 * 64, 64, -5, 64, J.array(plan)) == ILL
    J.call("clayPatternSetDestroy", h)
    J.call("clayPatternSetDestroy", 0)


def test_clay_mixed_host_native_is_package_private_and_checks_its_counts(J):
    """The host form takes raw host addresses, so its native is package-private like the other
    mixed host batches (no ByteBuffer form yet); the forwarder refuses a handle of 0 and negative
    counts, and an empty batch returns before any device work."""
    java = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxNative.java").read_text()
    assert re.search(r"\n    static native int clayPerformCodingMixedBatchHost\(", java)
    assert "public static native int clayPerformCodingMixedBatchHost" not in java
    st, h = _create(J, [[1], [0, 3], []])
    assert st == OK
    buf = np.zeros(64, np.uint8)
    p = int(buf.ctypes.data)
    args = (p, p, 48, 1, p, 16, 1)
    assert J.call("clayPerformCodingMixedBatchHost", 0, *args, 1, 1) == NUL
    assert J.call("clayPerformCodingMixedBatchHost", h, *args, -1, 1) == ILL
    assert J.call("clayPerformCodingMixedBatchHost", h, *args, 1, -1) == ILL
    assert J.call("clayPerformCodingMixedBatchHost", h, 0, *args[1:], 1, 1) == NUL   # the export's own: null ids
    assert J.call("clayPerformCodingMixedBatchHost", h, *args, 0, 1) == OK
    assert J.call("clayPerformCodingMixedBatchHost", h, 0, 0, 48, 1, 0, 16, 1, 1, 0) == OK
    assert (buf == 0).all() and J.counters()["pins"] == 0
    J.call("clayPatternSetDestroy", h)


def test_no_int_array_of_the_create_is_pinned():
    src = (ROOT / "jni" / "ecx_jni.c").read_text()
    body = re.search(r"JNICALL Java_\w+_clayPatternSetCreate\(.*?\n\}", src, flags=re.S).group(0)
    assert body.count("GetIntArrayRegion") == 2 and "PIN(" not in body
    assert body.index("array_check(env, n_erased") < body.index("int_array_sum(env, n_erased")


def test_clay_mixed_repair_wrapper_uses_the_pattern_set_natives():
    """EcxClayMixedRepair is a thin wrapper: it flattens the lists, forwards the batch calls (the host
    form package-private, as it takes raw addresses), and close() frees the set exactly once."""
    src = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxClayMixedRepair.java").read_text()
    for native in ("clayPatternSetCreate", "clayPatternSetDestroy", "clayPatternSetInfo", "clayPerformCodingBatchMixed",
                   "clayPerformCodingMixedBatchHost"):
        assert "EcxNative.%s(" % native in src, native
    assert re.search(r"\n    void performCodingBatchHost\(", src)  # package-private, like the native it calls
    close = re.search(r"public synchronized void close\(\) \{(.*?)\n    \}", src, flags=re.S).group(1)
    assert "set = 0;" in close and close.index("set = 0;") < close.index("EcxNative.clayPatternSetDestroy(")
    assert "if (s != 0)" in close
