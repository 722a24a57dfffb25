"""The blocked and the host-memory mixed decodes (include/ecx.h:
ecx_rs_decode_missing_blocked_batch_mixed, ecx_rs_decode_missing_mixed_batch_host,
ecx_rs_decode_missing_blocked_mixed_batch_host) where no GPU is needed: that the exports exist,
the status of every argument rule that holds before any device work and the order of those rules,
the empty host batch, the status without a device (no CPU fallback), the Python methods' own
refusals, and the device export's generated JNI forwarder over the fake JNIEnv.  The decodes
themselves are tests/test_mixed_blocked.py and tests/test_mixed_host.py.
RS(4,2), 3 stripes of 100-byte shards."""
import numpy as np
import pytest

OK, ILL, IDX, NUL, DEV = 0, -1, -5, -6, -10
K, M, S, L = 4, 2, 3, 100
N = K + M
BLOCKED, HOST, BLOCKED_HOST = ("ecx_rs_decode_missing_blocked_batch_mixed", "ecx_rs_decode_missing_mixed_batch_host",
                               "ecx_rs_decode_missing_blocked_mixed_batch_host")


def _has_device(ecx):
    try:
        return ecx.device_count() > 0
    except ecx.EcxError:
        return False


@pytest.fixture
def batch(ecx):
    rs = ecx.ReedSolomon.create(K, M)
    pats = np.ones((3, N), np.uint8)
    pats[1, 5] = 0
    pats[2, 0] = 0
    base = np.arange(S * N * L, dtype=np.uint32).astype(np.uint8)
    ids = np.array([1, 2, 0], np.uint8)
    with rs.patternSet(pats) as ps, rs.patternSet(np.ones((2, N), np.uint8)) as whole:
        yield rs, ps, whole, base, base.copy(), ids


def test_the_three_exports_exist(ecx):
    lib = ecx.lib()
    for name in (BLOCKED, HOST, BLOCKED_HOST):
        assert callable(getattr(lib, name)), name


def test_blocked_device_form_argument_rules_in_order(ecx, batch):
    """Null set; then negative counts; then null base / ids (also for an empty batch: the device
    form has no empty-batch exemption); then the block and the extent; then the empty batch."""
    rs, ps, whole, base, before, ids = batch
    f = getattr(ecx.lib(), BLOCKED)
    b, i = base.ctypes.data, ids.ctypes.data
    assert f(None, i, b, S, L, 0, None) == NUL
    assert f(None, None, None, -1, -1, -1, None) == NUL            # the set first
    assert f(ps._h, i, b, -1, L, 0, None) == ILL
    assert f(ps._h, i, b, S, -1, 0, None) == ILL
    assert f(ps._h, None, None, -1, L, -1, None) == ILL            # the counts before the pointers
    assert f(ps._h, i, None, S, L, 0, None) == NUL
    assert f(ps._h, None, b, S, L, 0, None) == NUL
    assert f(ps._h, i, None, 0, L, 0, None) == NUL
    assert f(ps._h, None, b, S, 0, 0, None) == NUL
    assert f(ps._h, i, None, S, L, -64, None) == NUL               # the pointers before the block
    assert f(ps._h, i, b, S, L, -64, None) == ILL
    assert f(ps._h, i, b, 0, L, -64, None) == ILL                  # the block before the empty batch
    assert f(ps._h, i, b, 2**62, 2**40, 4096, None) == ILL         # the extent does not fit int64_t
    assert f(ps._h, i, b, 2**62, 2**40, 0, None) == ILL
    assert f(ps._h, i, b, 0, L, 0, None) == OK
    assert f(ps._h, i, b, S, 0, 32, None) == OK
    assert f(whole._h, i, b, S, L, 32, None) == OK                 # nothing missing anywhere: nothing enqueued
    assert (base == before).all()


@pytest.mark.parametrize("form", [HOST, BLOCKED_HOST])
def test_host_forms_argument_rules_in_order(ecx, batch, form):
    """As the device form, but a host batch of no stripes needs no buffers."""
    rs, ps, whole, base, before, ids = batch
    g = getattr(ecx.lib(), form)
    if form == HOST:
        f = lambda st, i, b, s, c, blk=0, off=0: g(st, i, b, N * L, L, s, off, c)  # noqa: E731
    else:
        f = lambda st, i, b, s, c, blk=0, off=0: g(st, i, b, s, c, blk)           # noqa: E731
    b, i = base.ctypes.data, ids.ctypes.data
    assert f(None, i, b, S, L) == NUL
    assert f(None, None, None, -1, -1) == NUL
    assert f(ps._h, i, b, -1, L) == ILL
    assert f(ps._h, i, b, S, -1) == ILL
    assert f(ps._h, None, None, -1, L) == ILL
    if form == HOST:
        assert f(ps._h, i, b, S, L, off=-1) == ILL
    assert f(ps._h, i, None, S, L) == NUL
    assert f(ps._h, None, b, S, L) == NUL
    assert f(ps._h, None, None, 0, L) == OK                        # empty: no buffers needed
    assert f(ps._h, None, None, 0, 0) == OK
    assert f(ps._h, i, b, S, 0) == OK
    if form == BLOCKED_HOST:
        assert f(ps._h, i, None, S, L, blk=-64) == NUL
        assert f(ps._h, i, b, S, L, blk=-64) == ILL
        assert f(ps._h, None, None, 0, L, blk=-64) == ILL
        assert f(ps._h, i, b, 2**62, 2**40, blk=4096) == ILL
    assert f(whole._h, i, b, S, L) == OK                           # nothing missing anywhere: no device needed
    assert (base == before).all()


def test_no_gpu_mixed_batches_fail_loudly(ecx, batch):
    """Without a HIP device a batch with work returns ECX_E_DEVICE from all three exports (no CPU
    fallback) and leaves the bytes alone."""
    if _has_device(ecx):
        pytest.skip("a device is present")
    rs, ps, whole, base, before, ids = batch
    lib = ecx.lib()
    b, i = base.ctypes.data, ids.ctypes.data
    # (the device form is handed host addresses: it must fail before it would launch anything)
    for blk in (0, 32):
        assert getattr(lib, BLOCKED)(ps._h, i, b, S, L, blk, None) == DEV
        assert getattr(lib, BLOCKED_HOST)(ps._h, i, b, S, L, blk) == DEV
    assert getattr(lib, HOST)(ps._h, i, b, N * L, L, S, 0, L) == DEV
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBatchMixedHost(base, ps, ids, N * L, L, S, 0, L)
    assert e.value.code == DEV
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBlockedBatchMixedHost(base, ps, ids, S, L)
    assert e.value.code == DEV
    assert (base == before).all()


def test_python_methods_refuse_a_closed_set_and_short_buffers(ecx, batch):
    rs, ps, whole, base, before, ids = batch
    import torch
    dev_like, dev_ids = torch.zeros(S * N * L, dtype=torch.uint8), torch.zeros(S, dtype=torch.uint8)
    # a stripe too many for the buffer, then ids too few (CPU tensors stand in for the device
    # form: the extents are checked before the device pointers are taken)
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBlockedBatchMixed(dev_like, ps, dev_ids, S + 1, L)
    assert e.value.code == IDX and "base" in str(e.value)
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBlockedBatchMixed(dev_like, ps, torch.zeros(S - 1, dtype=torch.uint8), S, L)
    assert e.value.code == IDX and "ids" in str(e.value)
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBlockedBatchMixedHost(base, ps, ids, S + 1, L)
    assert e.value.code == IDX and "base" in str(e.value)
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBlockedBatchMixedHost(base, ps, np.zeros(S - 1, np.uint8), S, L)
    assert e.value.code == IDX and "ids" in str(e.value)
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBatchMixedHost(base, ps, ids, N * L, L, S + 1, 0, L)
    assert e.value.code == IDX and "shards" in str(e.value)
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBatchMixedHost(base, ps, ids, N * L, L, S, 1, L)      # the window runs past the end
    assert e.value.code == IDX
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBatchMixedHost(base, ps, np.zeros(S - 1, np.uint8), N * L, L, S, 0, L)
    assert e.value.code == IDX and "ids" in str(e.value)
    other = ecx.ReedSolomon.create(5, 2)
    for call in (lambda: other.decodeMissingBlockedBatchMixed(dev_like, ps, dev_ids, 1, L),
                 lambda: other.decodeMissingBatchMixedHost(base, ps, ids, 7 * L, L, 1, 0, L),
                 lambda: other.decodeMissingBlockedBatchMixedHost(base, ps, ids, 1, L)):
        with pytest.raises(ecx.EcxError) as e:
            call()
        assert e.value.code == ILL
    ps.close()
    for call in (lambda: rs.decodeMissingBlockedBatchMixed(dev_like, ps, dev_ids, S, L),
                 lambda: rs.decodeMissingBatchMixedHost(base, ps, ids, N * L, L, S, 0, L),
                 lambda: rs.decodeMissingBlockedBatchMixedHost(base, ps, ids, S, L)):
        with pytest.raises(ecx.EcxError) as e:
            call()
        assert e.value.code == NUL and "closed" in str(e.value)
    assert (base == before).all()


def test_jni_forwarder_of_the_device_export():
    """Over the fake JNIEnv: a handle of 0 is NullPointerException, a negative count
    IllegalArgumentException, null addresses NullPointerException -- none reaches a device -- and
    an empty batch is a no-op.  The two host natives are package-private raw-address natives."""
    from jni_harness import Jni, ROOT
    J = Jni()
    try:
        J.reset()
        h = np.zeros(1, np.int64)
        assert J.call("rsCreate", K, M, J.array(h)) == OK and h[0]
        rs = int(h[0])
        pats = np.ones(2 * N, np.uint8)
        pats[N + 1] = 0
        out = np.zeros(1, np.int64)
        assert J.call("rsPatternSetCreate", rs, J.array(pats), 2, J.array(out)) == OK and out[0]
        st = int(out[0])
        pins = J.counters()["pins"]
        assert J.call("rsDecodeMissingBlockedBatchMixed", 0, 16, 4096, S, L, 0, 0) == NUL
        assert J.call("rsDecodeMissingBlockedBatchMixed", st, 16, 4096, -1, L, 0, 0) == ILL
        assert J.call("rsDecodeMissingBlockedBatchMixed", st, 16, 4096, S, -1, 0, 0) == ILL
        assert J.call("rsDecodeMissingBlockedBatchMixed", 0, 16, 4096, -1, L, 0, 0) == NUL   # the handle first
        assert J.call("rsDecodeMissingBlockedBatchMixed", st, 0, 4096, S, L, 0, 0) == NUL
        assert J.call("rsDecodeMissingBlockedBatchMixed", st, 16, 0, S, L, 0, 0) == NUL
        assert J.call("rsDecodeMissingBlockedBatchMixed", st, 16, 4096, S, L, -64, 0) == ILL
        assert J.call("rsDecodeMissingBlockedBatchMixed", st, 16, 4096, 0, L, 0, 0) == OK
        # the host natives: the same refusals, and the empty batch with null addresses
        assert J.call("rsDecodeMissingMixedBatchHost", 0, 16, 4096, N * L, L, S, 0, L) == NUL
        assert J.call("rsDecodeMissingMixedBatchHost", st, 16, 4096, N * L, L, -1, 0, L) == ILL
        assert J.call("rsDecodeMissingMixedBatchHost", st, 0, 0, N * L, L, 0, 0, L) == OK
        assert J.call("rsDecodeMissingBlockedMixedBatchHost", 0, 16, 4096, S, L, 0) == NUL
        assert J.call("rsDecodeMissingBlockedMixedBatchHost", st, 16, 4096, S, -1, 0) == ILL
        assert J.call("rsDecodeMissingBlockedMixedBatchHost", st, 0, 0, 0, L, 0) == OK
        c = J.counters()
        assert c["pins"] == pins and c["violations"] == 0, c       # addresses only: nothing to pin
        J.call("rsPatternSetDestroy", st)
        J.call("rsDestroy", rs)
    finally:
        J.free_all()
    java = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxNative.java").read_text()
    assert "    public static native int rsDecodeMissingBlockedBatchMixed(" in java
    for native in ("rsDecodeMissingMixedBatchHost", "rsDecodeMissingBlockedMixedBatchHost"):
        assert ("(no ByteBuffer form yet; INTEGRATION.md). */\n    static native int %s(" % native) in java, native
    wrapper = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxMixedDecode.java").read_text()
    assert "    public void decodeMissingBlockedBatch(long patternOfStripe, long base, long nstripes, long byteCount," in wrapper
    assert "\n    void decodeMissingBatchHost(" in wrapper and "\n    void decodeMissingBlockedBatchHost(" in wrapper
