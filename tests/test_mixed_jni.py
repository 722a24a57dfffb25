"""The pattern-set exports through the generated JNI forwarders (jni/ecx_jni.c) over the fake
JNIEnv (tests/jni_harness.py; no JDK here): a `patterns` array shorter than npatterns * n flags,
or `present` / `patterns` / `ids` arrays shorter than the index helper will touch, are refused
before anything is pinned, the way the other forwarders refuse short arrays
(ArrayIndexOutOfBoundsException); a handle of 0 and null arrays are NullPointerException; valid
calls reach the exports and return their results through the Java arrays.  The batch call takes
device addresses (longs) only, so it has nothing to pin."""
import re

import numpy as np
import pytest

from jni_harness import Jni, ROOT

OK, ILL, NSH, IDX, NUL = 0, -1, -2, -5, -6


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


def _rs(J, k, m):
    h = np.zeros(1, np.int64)
    assert J.call("rsCreate", k, m, J.array(h)) == OK and h[0]
    return int(h[0])


def test_pattern_set_create_argument_checks(J):
    rs = _rs(J, 4, 2)
    try:
        pats = np.ones(3 * 6, np.uint8)
        pats[6 + 2] = 0
        pats[12 + 0] = pats[12 + 5] = 0
        out = np.zeros(1, np.int64)
        assert J.call("rsPatternSetCreate", rs, J.array(pats[:17]), 3, J.array(out)) == IDX   # short patterns
        assert J.call("rsPatternSetCreate", rs, J.array(pats), 4, J.array(out)) == IDX        # more rows than flags
        assert J.call("rsPatternSetCreate", rs, None, 3, J.array(out)) == NUL
        assert J.call("rsPatternSetCreate", 0, J.array(pats), 3, J.array(out)) == NUL          # handle 0
        assert J.call("rsPatternSetCreate", rs, J.array(pats), -1, J.array(out)) == ILL
        assert J.call("rsPatternSetCreate", rs, J.array(pats), 3, J.array(np.zeros(0, np.int64))) == IDX
        assert J.call("rsPatternSetCreate", rs, J.array(pats), 3, None) == NUL
        assert J.counters()["pins"] == 0 and out[0] == 0  # rejected before the export
        # the export's own refusals come through: 0 patterns, too few shards present
        assert J.call("rsPatternSetCreate", rs, J.array(pats), 0, J.array(out)) == ILL
        few = pats.copy()
        few[6:9] = 0
        assert J.call("rsPatternSetCreate", rs, J.array(few), 3, J.array(out)) == NSH
        assert out[0] == 0
        # a valid call returns the handle, and info reads it back
        assert J.call("rsPatternSetCreate", rs, J.array(pats), 3, J.array(out)) == OK and out[0] != 0
        st = int(out[0])
        n, shards, missing = (np.zeros(1, np.int32) for _ in range(3))
        assert J.call("rsPatternSetInfo", st, J.array(n), J.array(shards), J.array(missing)) == OK
        assert (n[0], shards[0], missing[0]) == (3, 6, 2)
        assert J.call("rsPatternSetInfo", st, None, None, J.array(missing)) == OK              # each may be null
        assert J.call("rsPatternSetInfo", st, J.array(np.zeros(0, np.int32)), None, None) == IDX
        assert J.call("rsPatternSetInfo", 0, J.array(n), J.array(shards), J.array(missing)) == NUL
        # the batch call: addresses only; a handle of 0, null addresses and negative counts never reach a device
        assert J.call("rsDecodeMissingBatchMixed", 0, 16, 4096, 6 * 64, 64, 1, 0, 64, 0) == NUL
        assert J.call("rsDecodeMissingBatchMixed", st, 0, 4096, 6 * 64, 64, 1, 0, 64, 0) == NUL
        assert J.call("rsDecodeMissingBatchMixed", st, 16, 0, 6 * 64, 64, 1, 0, 64, 0) == NUL
        assert J.call("rsDecodeMissingBatchMixed", st, 16, 4096, 6 * 64, 64, -1, 0, 64, 0) == ILL
        assert J.call("rsDecodeMissingBatchMixed", st, 16, 4096, 6 * 64, 64, 0, 0, 64, 0) == OK  # empty batch
        J.call("rsPatternSetDestroy", st)
        J.call("rsPatternSetDestroy", 0)
    finally:
        J.call("rsDestroy", rs)


def test_index_patterns_argument_checks(J):
    present = np.array([[1, 1, 0, 1], [1, 1, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1], [1, 1, 1, 1]], np.uint8)
    S, n = present.shape
    flat = present.reshape(-1)
    patterns, count, ids = np.zeros(256 * n, np.uint8), np.zeros(1, np.int32), np.full(S, 9, np.uint8)
    call = lambda pres=flat, pats=patterns, cap=256, cnt=count, ids_=ids, shards=n, nstripes=S: J.call(  # noqa: E731
        "rsIndexPatterns", shards, J.array(pres) if pres is not None else None, nstripes,
        J.array(pats) if pats is not None else None, cap, J.array(cnt) if cnt is not None else None,
        J.array(ids_) if ids_ is not None else None)
    assert call(pres=flat[:-1]) == IDX                      # present shorter than nstripes * shards
    assert call(pats=patterns[:256 * n - 1]) == IDX         # patterns shorter than cap * shards
    assert call(pats=patterns[:3 * n], cap=4) == IDX
    assert call(ids_=ids[:S - 1]) == IDX                    # ids shorter than nstripes
    assert call(cnt=np.zeros(0, np.int32)) == IDX
    assert call(pres=None) == NUL and call(pats=None) == NUL and call(cnt=None) == NUL and call(ids_=None) == NUL
    assert call(nstripes=-1) == ILL and call(shards=-1) == ILL and call(cap=-1) == ILL
    assert J.counters()["pins"] == 0 and (ids == 9).all()   # nothing above reached the export
    assert call(cap=2, pats=patterns[:2 * n]) == ILL        # the export's own: 3 distinct rows, room for 2
    assert call(cap=0) == ILL
    assert call() == OK
    assert count[0] == 3 and list(ids) == [0, 1, 0, 2, 1]
    assert np.array_equal(patterns[:3 * n].reshape(3, n), present[[0, 1, 3]])
    assert call(cap=3, pats=patterns[:3 * n]) == OK         # exactly enough room


def test_mixed_decode_wrapper_uses_the_pattern_set_natives():
    """EcxMixedDecode is a thin wrapper: it creates the set from the flattened flags, forwards the
    batch call, and close() frees the set and its codec reference exactly once."""
    src = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxMixedDecode.java").read_text()
    for native in ("rsPatternSetCreate", "rsPatternSetDestroy", "rsPatternSetInfo", "rsDecodeMissingBatchMixed",
                   "rsIndexPatterns"):
        assert "EcxNative.%s(" % native in src, native
    close = re.search(r"public synchronized void close\(\) \{(.*?)\n    \}", src, flags=re.S).group(1)
    assert "set = 0;" in close and "rs = 0;" in close
    assert close.index("set = 0;") < close.index("EcxNative.rsPatternSetDestroy(")
    assert "if (s != 0)" in close and "if (h != 0)" in close
