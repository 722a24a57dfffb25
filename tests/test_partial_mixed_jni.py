"""ecx_rs_decode_partial_batch_mixed through its generated JNI forwarder (jni/ecx_jni.c) over the
fake JNIEnv (tests/jni_harness.py; no JDK here).  The call takes addresses (longs) only, so it pins
nothing: a handle of 0 and negative counts are refused by the forwarder, null addresses by the
export, and an empty batch needs no buffers.  One GPU case runs the forwarder on device addresses
against the uniform decodePartialBatch."""
import re

import numpy as np
import pytest

from jni_harness import Jni, ROOT

OK, ILL, IDX, NUL = 0, -1, -5, -6
NATIVE = "rsDecodePartialBatchMixed"


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


def _set(J, k, m, pats):
    h = np.zeros(1, np.int64)
    assert J.call("rsCreate", k, m, J.array(h)) == OK and h[0]
    out = np.zeros(1, np.int64)
    flat = np.ascontiguousarray(pats, np.uint8).reshape(-1)
    assert J.call("rsPatternSetCreate", int(h[0]), J.array(flat), len(pats), J.array(out)) == OK and out[0]
    return int(h[0]), int(out[0])


def test_forwarder_argument_rules(J):
    pats = np.ones((2, 6), np.uint8)
    pats[1, 2] = pats[1, 5] = 0
    rs, st = _set(J, 4, 2, pats)
    pins = J.counters()["pins"]  # creating the set pinned its flags
    try:
        # (set, ids, shardOfStripe, in, inStripeStride, inShardStride, acc, accStripeStride, accRowStride,
        #  nstripes, byteCount, isFirst, stream)
        assert J.call(NATIVE, 0, 16, 32, 4096, 64, 0, 8192, 128, 64, 1, 64, 1, 0) == NUL      # handle 0
        assert J.call(NATIVE, 0, 16, 32, 4096, 64, 0, 8192, 128, 64, -1, 64, 1, 0) == NUL     # the handle first
        assert J.call(NATIVE, st, 16, 32, 4096, 64, 0, 8192, 128, 64, -1, 64, 1, 0) == ILL
        assert J.call(NATIVE, st, 16, 32, 4096, 64, 0, 8192, 128, 64, 1, -64, 1, 0) == ILL
        assert J.call(NATIVE, st, 0, 0, 0, 64, 0, 0, 128, 64, -1, 64, 1, 0) == ILL             # counts before pointers
        for slot in (1, 2, 3, 6):                                                             # a null address among the four
            args = [st, 16, 32, 4096, 64, 0, 8192, 128, 64, 1, 64, 1, 0]
            args[slot] = 0
            assert J.call(NATIVE, *args) == NUL, slot
        assert J.call(NATIVE, st, 16, 32, 4096, 2**40, 0, 8192, 128, 64, 2**62, 64, 1, 0) == ILL  # the extent
        assert J.call(NATIVE, st, 0, 0, 0, 64, 0, 0, 128, 64, 0, 64, 1, 0) == OK               # empty: no buffers
        assert J.call(NATIVE, st, 0, 0, 0, 64, 0, 0, 128, 64, 1, 0, 0, 0) == OK
        assert J.counters()["pins"] == pins  # addresses only: nothing to pin
    finally:
        J.call("rsPatternSetDestroy", st)
        J.call("rsDestroy", rs)


def test_wrapper_and_native_declarations():
    """EcxMixedDecode.decodePartialBatch forwards to the generated native beside its decode
    methods; the forwarder hands the export exactly its parameters, in order."""
    java = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxMixedDecode.java").read_text()
    assert "EcxNative.%s(handle(), patternOfStripe, shardOfStripe, in, inStripeStride," % NATIVE in java
    assert java.index("public void decodeMissingBatch(") < java.index("public void decodePartialBatch(") < \
        java.index("public int[] info()")
    native = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxNative.java").read_text()
    decl = re.search(r"static native int %s\((.*?)\);" % NATIVE, native).group(1)
    assert [p.split()[0] for p in decl.split(", ")] == ["long"] * 11 + ["int", "long"]
    c = (ROOT / "jni" / "ecx_jni.c").read_text()
    body = c[c.index("/* ecx_rs_decode_partial_batch_mixed */"):]
    body = body[:body.index("\n}\n")]
    call = re.search(r"ecx_rs_decode_partial_batch_mixed\((.*)\);", body).group(1)
    names = re.findall(r"\)\(?(?:intptr_t\))?(\w+)(?:,|$)", call)
    assert names == ["set", "pattern_of_stripe", "shard_of_stripe", "in", "in_stripe_stride", "in_shard_stride", "acc",
                     "acc_stripe_stride", "acc_row_stride", "nstripes", "byte_count", "is_first", "stream"], names
    header = (ROOT / "include" / "ecx.h").read_text()
    comment = header[:header.index("int ecx_rs_decode_partial_batch_mixed(")].rsplit("/*", 1)[1]
    assert "ReedSolomon.java:288-333" in comment


@pytest.mark.gpu
def test_forwarder_on_the_gpu_equals_the_uniform_call(J, ecx):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    k, m, S, L = 4, 2, 5, 4096 + 48
    n = k + m
    pats = np.ones((3, n), np.uint8)
    pats[0, 1] = 0
    pats[1, 0] = pats[1, 5] = 0
    ids = [1, 0, 2, 1, 0]
    shard_of = [3, 0, 2, 5, 4]
    inp = torch.empty((S, L), dtype=torch.uint8, device="cuda")
    ecx.fill_random(inp, inp.numel(), 8500)
    fill = torch.empty((S, 2, L), dtype=torch.uint8, device="cuda")
    ecx.fill_random(fill, fill.numel(), 8501)
    dev_ids = torch.tensor(ids, dtype=torch.uint8, device="cuda")
    dev_shard_of = torch.tensor(shard_of, dtype=torch.uint8, device="cuda")
    rs = ecx.ReedSolomon.create(k, m)
    jrs, st = _set(J, k, m, pats)
    try:
        for first in (1, 0):
            got, ref = fill.clone(), fill.clone()
            assert J.call(NATIVE, st, dev_ids.data_ptr(), dev_shard_of.data_ptr(), inp.data_ptr(), L, 0,
                          got.data_ptr(), 2 * L, L, S, L, first, 0) == OK
            for s in range(S):
                rs.decodePartialBatch(pats[ids[s]], shard_of[s], inp[s:], L, ref[s:], 2 * L, L, 1, L, bool(first))
            torch.cuda.synchronize()
            assert torch.equal(got, ref), first
            assert not torch.equal(got, fill)
    finally:
        J.call("rsPatternSetDestroy", st)
        J.call("rsDestroy", jrs)
