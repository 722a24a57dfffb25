"""ecx_clay_partial_batch_mixed through its generated JNI forwarder (jni/ecx_jni.c) over the fake
JNIEnv (tests/jni_harness.py; no JDK here).  The call takes addresses (longs) only, so it pins
nothing: a handle of 0 and negative counts are refused by the forwarder, null addresses and an
extent beyond int64_t by the export, and an empty batch needs no buffers.  One GPU case runs the
forwarder on device addresses against ClayPatternSet.partialBatchMixed."""
import re

import numpy as np
import pytest

from jni_harness import Jni, ROOT

OK, ILL, IDX, NUL = 0, -1, -5, -6
NATIVE = "clayPartialBatchMixed"
LISTS = [[1], [0, 3], [], [5]]


@pytest.fixture(scope="module")
def jni(ecx):
    ecx.lib()  # libecx.so through the package first: it then shares torch's HIP runtime, and so does the harness
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


def _set(J, lists, k=4, m=2):
    flat = np.array([e for lst in lists for e in lst], np.int32)
    cnt = np.array([len(lst) for lst in lists], np.int32)
    h = np.zeros(1, np.int64)
    assert J.call("clayPatternSetCreate", k, m, 0, J.array(flat), J.array(cnt), len(lists), J.array(h)) == OK and h[0]
    return int(h[0])


def test_forwarder_argument_rules(J):
    st = _set(J, LISTS)
    empty = _set(J, [[], []])
    pins = J.counters()["pins"]
    try:
        # (set, ids, nodeOfStripe, in, inStripeStride, inNodeStride, inSubStride, acc, accStripeStride,
        #  accSubStride, nstripes, bufSize, isFirst, stream)
        good = [st, 16, 32, 4096, 512, 0, 64, 8192, 1024, 64, 1, 64, 1, 0]
        assert J.call(NATIVE, 0, *good[1:]) == NUL                                  # handle 0
        assert J.call(NATIVE, 0, *good[1:10], -1, 64, 1, 0) == NUL                  # the handle first
        assert J.call(NATIVE, *good[:10], -1, 64, 1, 0) == ILL
        assert J.call(NATIVE, *good[:10], 1, -64, 1, 0) == ILL
        assert J.call(NATIVE, st, 0, 0, 0, 512, 0, 64, 0, 1024, 64, -1, 64, 1, 0) == ILL   # counts before pointers
        for slot in (1, 2, 3, 7):                                                   # a null address among the four
            args = list(good)
            args[slot] = 0
            assert J.call(NATIVE, *args) == NUL, slot
        for slot in (4, 5, 6, 8, 9):                                                # a negative stride
            args = list(good)
            args[slot] = -16
            assert J.call(NATIVE, *args) == ILL, slot
        assert J.call(NATIVE, st, 16, 32, 4096, 2**40, 0, 64, 8192, 1024, 64, 2**62, 64, 1, 0) == ILL  # the extent
        assert J.call(NATIVE, st, 16, 32, 4096, 512, 2**62, 64, 8192, 1024, 64, 1, 64, 1, 0) == ILL
        assert J.call(NATIVE, st, 0, 0, 0, 512, 0, 64, 0, 1024, 64, 0, 64, 1, 0) == OK      # empty: no buffers
        assert J.call(NATIVE, st, 0, 0, 0, 512, 0, 64, 0, 1024, 64, 1, 0, 0, 0) == OK
        assert J.call(NATIVE, empty, 0, 0, 0, 512, 0, 64, 0, 1024, 64, 3, 64, 1, 0) == OK   # every list empty
        assert J.counters()["pins"] == pins  # addresses only: nothing to pin
    finally:
        J.call("clayPatternSetDestroy", st)
        J.call("clayPatternSetDestroy", empty)


def test_wrapper_and_native_declarations():
    """EcxClayMixedRepair.partialBatch forwards to the generated native beside its repair methods;
    the forwarder hands the export exactly its parameters, in order."""
    java = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxClayMixedRepair.java").read_text()
    assert "EcxNative.%s(handle(), patternOfStripe, nodeOfStripe, in, inStripeStride," % NATIVE in java
    assert java.index("public void performCodingBatch(") < java.index("public void partialBatch(") < \
        java.index("public int[] info()")
    native = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxNative.java").read_text()
    decl = re.search(r"public static native int %s\((.*?)\);" % NATIVE, native).group(1)
    assert [p.split()[0] for p in decl.split(", ")] == ["long"] * 12 + ["int", "long"]
    c = (ROOT / "jni" / "ecx_jni.c").read_text()
    body = c[c.index("/* ecx_clay_partial_batch_mixed */"):]
    body = body[:body.index("\n}\n")]
    assert "PIN(" not in body
    call = re.search(r"ecx_clay_partial_batch_mixed\((.*)\);", body).group(1)
    names = re.findall(r"\)\(?(?:intptr_t\))?(\w+)(?:,|$)", call)
    assert names == ["set", "pattern_of_stripe", "node_of_stripe", "in", "in_stripe_stride", "in_node_stride",
                     "in_sub_stride", "acc", "acc_stripe_stride", "acc_sub_stride", "nstripes", "buf_size", "is_first",
                     "stream"], names
    header = (ROOT / "include" / "ecx.h").read_text()
    comment = header[:header.index("int ecx_clay_partial_batch_mixed(")].rsplit("/*", 1)[1]
    assert "ClayCoordinator.kt:265-319" in comment and "ClayCodeNode.kt:165-233" in comment


@pytest.mark.gpu
def test_forwarder_on_the_gpu_equals_the_python_method(J, ecx):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    S, B, alpha, rows = 5, 4096 + 48, 8, 16
    ids = [1, 0, 3, 2, 1]
    node_of = [2, 0, 4, 5, 3]
    inp = torch.empty((S, alpha, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(inp, inp.numel(), 9500)
    fill = torch.empty((S, rows, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(fill, fill.numel(), 9501)
    dev_ids = torch.tensor(ids, dtype=torch.uint8, device="cuda")
    dev_node_of = torch.tensor(node_of, dtype=torch.uint8, device="cuda")
    st = _set(J, LISTS)
    try:
        with ecx.ClayPatternSet(LISTS, 4, 2) as ps:
            for first in (1, 0):
                got, ref = fill.clone(), fill.clone()
                assert J.call(NATIVE, st, dev_ids.data_ptr(), dev_node_of.data_ptr(), inp.data_ptr(), alpha * B, 0, B,
                              got.data_ptr(), rows * B, B, S, B, first, 0) == OK
                ps.partialBatchMixed(dev_ids, dev_node_of, inp, alpha * B, 0, B, ref, rows * B, B, S, B, bool(first))
                torch.cuda.synchronize()
                assert torch.equal(got, ref), first
                assert not torch.equal(got, fill)
                assert torch.equal(got[3], fill[3])  # the empty list leaves its stripe alone
    finally:
        J.call("clayPatternSetDestroy", st)
