"""The two-shard locate through the generated JNI forwarders (jni/ecx_jni.c) over the fake JNIEnv
(tests/jni_harness.py; no JDK here), as tests/test_locate_jni.py: both natives take device addresses
(longs) only, so nothing is pinned; a handle of 0 and null addresses are NullPointerException,
negative counts and codes the export refuses IllegalArgumentException, before a device is needed.
On the GPU one RS(2,4) batch through the forwarder equals the oracle's brute force
(tests/locate2_cases.py)."""
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


def test_locate2_forwarders_argument_rules(J):
    """rsLocateCorrupt2Batch and rsLocateCorrupt2BlockedBatch take the parameters of the single-shard
    pair: one forwarder per export, nothing pinned."""
    assert "rsLocateCorrupt2Batch" in J.sigs and "rsLocateCorrupt2BlockedBatch" in J.sigs
    rs, rs3, rs23 = _rs(J, 2, 4), _rs(J, 4, 3), _rs(J, 19, 4)
    try:
        nat = lambda **kw: J.call("rsLocateCorrupt2Batch", kw.get("rs", rs), kw.get("base", 4096), 6 * 64, 64,  # noqa: E731
                                  kw.get("S", 2), kw.get("off", 0), kw.get("L", 64), kw.get("su", 8192),
                                  kw.get("cu", 12288), kw.get("he", 16384), 0)
        blk = lambda **kw: J.call("rsLocateCorrupt2BlockedBatch", kw.get("rs", rs), kw.get("base", 4096),  # noqa: E731
                                  kw.get("S", 2), kw.get("L", 64), kw.get("blk", 0), kw.get("su", 8192),
                                  kw.get("cu", 12288), kw.get("he", 16384), 0)
        for f in (nat, blk):
            assert f(rs=0) == NUL
            assert f(S=-1) == ILL and f(L=-1) == ILL
            assert f(base=0) == NUL and f(su=0) == NUL and f(cu=0) == NUL
            assert f(S=0, base=0, su=0, cu=0, he=0) == OK  # an empty batch touches nothing
            assert f(rs=rs3) == ILL                        # m = 3: two errors need 2 * 2 <= m
            assert f(rs=rs23, S=0) == ILL                  # n = 23: the heal ids do not fit a byte
            assert f(rs=rs23, S=0, he=0) == OK
        assert nat(off=-1) == ILL and blk(blk=-1) == ILL
        assert J.counters()["pins"] == 0
    finally:
        for h in (rs, rs3, rs23):
            J.call("rsDestroy", h)


def test_locate_wrapper_uses_the_locate2_natives():
    """EcxCorruptLocate forwards locateCorrupt2 / locateCorrupt2Blocked to the two natives, mirrors
    the export's refusals and offers the patterns and the pair index that go with the heal ids."""
    src = (ROOT / "jni" / "com" / "backblaze" / "erasure" / "ecx" / "EcxCorruptLocate.java").read_text()
    for native in ("rsLocateCorrupt2Batch", "rsLocateCorrupt2BlockedBatch"):
        assert "EcxNative.%s(" % native in src, native
    for method in ("public void locateCorrupt2(", "public void locateCorrupt2Blocked(",
                   "public boolean[][] doubleLossPatterns()", "public int pairIndex(int i, int j)"):
        assert method in src, method
    check = re.search(r"private void checkArguments2\(.*?\n    \}", src, flags=re.S).group(0)
    for refusal in ("parityCount < 4", "shardCount > 64", "healId != 0 && shardCount > 22", "nstripes < 0 || byteCount < 0"):
        assert refusal in check, refusal
    assert check.index("negative count") < check.index("parityCount < 4") < check.index("null device address")


@pytest.mark.gpu
def test_locate2_through_the_forwarder_vs_oracle(J, ecx):
    """RS(2,4), five stripes of 5,000 B: clean, data shard 1 corrupt, parity shards 2 and 5 corrupt at
    one byte, shards 0 and 4 in different chunks, three shards.  The forwarder's outputs equal the
    oracle's brute force."""
    import torch

    from locate2_cases import expectations2
    from locate_cases import valid_stripes
    k, m, L, S = 2, 4, 5000, 5
    n, width = 6, 21
    nat = valid_stripes(k, m, S, L, 9950)
    bad = nat.copy()
    for s, i, byte in ((1, 1, 0), (2, 2, 77), (2, 5, 77), (3, 0, 10), (3, 4, 4500), (4, 0, 1), (4, 1, 2), (4, 3, 3)):
        bad[s, i, byte] ^= 0x18
    want_s, want_c, want_h = expectations2(k, m, bad, 0, L)
    assert want_c.tolist() == [[-1, -1], [1, -1], [2, 5], [0, 4], [-2, -2]]
    pool = torch.from_numpy(bad).cuda()
    su = torch.full((S * width,), 9, dtype=torch.uint8, device="cuda")
    cu = torch.full((2 * S,), -77, dtype=torch.int32, device="cuda")
    he = torch.full((S,), 9, dtype=torch.uint8, device="cuda")
    rs = _rs(J, k, m)
    try:
        torch.cuda.synchronize()
        assert J.call("rsLocateCorrupt2Batch", rs, pool.data_ptr(), n * L, L, S, 0, L, su.data_ptr(), cu.data_ptr(),
                      he.data_ptr(), 0) == OK
        torch.cuda.synchronize()
        assert cu.cpu().tolist() == want_c.reshape(-1).tolist() and he.cpu().tolist() == want_h.tolist()
        assert su.cpu().tolist() == want_s.reshape(-1).tolist()
        assert J.call("rsLocateCorrupt2Batch", rs, pool.data_ptr(), n * L, L, S, 0, L, su.data_ptr(), cu.data_ptr(),
                      0, 0) == OK  # heal ids not wanted
        torch.cuda.synchronize()
        assert cu.cpu().tolist() == want_c.reshape(-1).tolist()
    finally:
        J.call("rsDestroy", rs)
