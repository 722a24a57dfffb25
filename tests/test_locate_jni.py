"""The corrupt-shard locate through the generated JNI forwarders (jni/ecx_jni.c) over the fake
JNIEnv (tests/jni_harness.py; no JDK here): both natives take device addresses (longs) only, so
nothing is pinned; a handle of 0 and null addresses are NullPointerException, negative counts
IllegalArgumentException, before a device is needed.  On the GPU one RS(4,2) batch through the
forwarder equals the oracle's brute force (tests/locate_cases.py)."""
import re

import numpy as np
import pytest

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


def _rs(J, k, m):
    h = np.zeros(1, np.int64)
    assert J.call("rsCreate", k, m, J.array(h)) == OK and h[0]
    return int(h[0])


def test_locate_forwarders_argument_rules(J):
    """rsLocateCorruptBatch(rs, base, stripeStride, shardStride, nstripes, offset, byteCount,
    suspect, culprit, healId, stream) and rsLocateCorruptBlockedBatch(rs, base, nstripes, byteCount,
    blockBytes, suspect, culprit, healId, stream): one forwarder per export, nothing pinned."""
    assert "rsLocateCorruptBatch" in J.sigs and "rsLocateCorruptBlockedBatch" in J.sigs
    rs, rs1 = _rs(J, 4, 2), _rs(J, 4, 1)
    try:
        nat = lambda **kw: J.call("rsLocateCorruptBatch", kw.get("rs", rs), kw.get("base", 4096), 6 * 64, 64,  # noqa: E731
                                  kw.get("S", 2), kw.get("off", 0), kw.get("L", 64), kw.get("su", 8192),
                                  kw.get("cu", 12288), kw.get("he", 16384), 0)
        blk = lambda **kw: J.call("rsLocateCorruptBlockedBatch", kw.get("rs", rs), kw.get("base", 4096),  # noqa: E731
                                  kw.get("S", 2), kw.get("L", 64), kw.get("blk", 0), kw.get("su", 8192),
                                  kw.get("cu", 12288), kw.get("he", 16384), 0)
        for f in (nat, blk):
            assert f(rs=0) == NUL
            assert f(S=-1) == ILL and f(L=-1) == ILL
            assert f(base=0) == NUL and f(su=0) == NUL and f(cu=0) == NUL
            assert f(S=0, base=0, su=0, cu=0, he=0) == OK  # an empty batch touches nothing
            assert f(rs=rs1) == ILL                        # m = 1: every column matches every syndrome
        assert nat(off=-1) == ILL and blk(blk=-1) == ILL
        assert J.counters()["pins"] == 0
    finally:
        J.call("rsDestroy", rs)
        J.call("rsDestroy", rs1)


def test_locate_wrapper_uses_the_locate_natives():
    """EcxCorruptLocate is a thin wrapper over the two natives and releases its codec once."""
    src = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxCorruptLocate.java").read_text()
    for native in ("rsLocateCorruptBatch", "rsLocateCorruptBlockedBatch", "rsDestroy"):
        assert "EcxNative.%s(" % native in src, native
    assert "public void locateCorrupt(" in src and "public void locateCorruptBlocked(" in src
    close = re.search(r"public synchronized void close\(\) \{(.*?)\n    \}", src, flags=re.S).group(1)
    assert "if (rs == 0)" in close and "rs = 0;" in close
    assert close.index("rs = 0;") < close.index("EcxNative.rsDestroy(")


@pytest.mark.gpu
def test_locate_through_the_forwarder_vs_oracle(J, ecx):
    """RS(4,2), four stripes of 5,000 B: clean, data shard 2 corrupt, parity shard 5 corrupt, two
    shards corrupt.  The forwarder's outputs equal the oracle's brute force."""
    import torch

    from locate_cases import expectations, valid_stripes
    k, m, L, S = 4, 2, 5000, 4
    n = k + m
    nat = valid_stripes(k, m, S, L, 9900)
    bad = nat.copy()
    for s, i, byte in ((1, 2, 0), (2, 5, L - 1), (3, 0, 10), (3, 4, 4500)):
        bad[s, i, byte] ^= 0x18
    want_s, want_c, want_h = expectations(k, m, bad, 0, L)
    assert want_c.tolist() == [-1, 2, 5, -2]
    pool = torch.from_numpy(bad).cuda()
    su = torch.full((S * n,), 9, dtype=torch.uint8, device="cuda")
    cu = torch.full((S,), -77, dtype=torch.int32, device="cuda")
    he = torch.full((S,), 9, dtype=torch.uint8, device="cuda")
    rs = _rs(J, k, m)
    try:
        torch.cuda.synchronize()
        assert J.call("rsLocateCorruptBatch", rs, pool.data_ptr(), n * L, L, S, 0, L, su.data_ptr(), cu.data_ptr(),
                      he.data_ptr(), 0) == OK
        torch.cuda.synchronize()
        assert cu.cpu().tolist() == want_c.tolist() and he.cpu().tolist() == want_h.tolist()
        assert su.cpu().tolist() == want_s.reshape(-1).tolist()
        assert J.call("rsLocateCorruptBatch", rs, pool.data_ptr(), n * L, L, S, 0, L, su.data_ptr(), cu.data_ptr(),
                      0, 0) == OK  # heal ids not wanted
        torch.cuda.synchronize()
        assert cu.cpu().tolist() == want_c.tolist()
    finally:
        J.call("rsDestroy", rs)
