"""Pattern sets on the host (include/ecx.h: ecx_rs_pattern_set_*, ecx_rs_index_patterns,
ecx_rs_decode_missing_batch_mixed): everything that is decided before the first HIP call -- the
pattern index, every status code, the set's info, and that creating and destroying sets touches no
device.  The library loads without a GPU; the decode itself is tests/test_mixed_decode.py."""
import ctypes

import numpy as np
import pytest

ILL, NOT_ENOUGH, NULL = -1, -2, -6


def _index_by_numpy(present):
    """numpy.unique's distinct rows, re-sorted by first appearance, and each row's index."""
    uniq, first, inverse = np.unique(present, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # position in `uniq` of the p-th pattern to appear
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    return uniq[order], rank[np.asarray(inverse).reshape(-1)]


@pytest.mark.parametrize("shape", ["7x6", "1000x16"])
def test_index_patterns_matches_numpy_unique(ecx, shape):
    rng = np.random.default_rng(11)
    if shape == "7x6":
        present = (rng.random((7, 6)) < 0.7).astype(np.uint8)
        present[3] = present[0]  # one pattern certainly repeats
    else:
        five = (rng.random((5, 16)) < 0.8).astype(np.uint8)
        assert len(np.unique(five, axis=0)) == 5
        present = five[rng.integers(0, 5, 1000)]
    want_patterns, want_ids = _index_by_numpy(present)
    patterns, ids = ecx.index_patterns(present)
    assert patterns.dtype == np.uint8 and ids.dtype == np.uint8
    assert np.array_equal(patterns, want_patterns)
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(patterns[ids], present)
    # any non-zero flag means present; the patterns come back as 0 / 1
    scaled, ids2 = ecx.index_patterns(present * 7)
    assert np.array_equal(scaled, want_patterns) and np.array_equal(ids2, want_ids)


def test_index_patterns_status_codes(ecx):
    lib = ecx.lib()
    f = lib.ecx_rs_index_patterns
    present = np.eye(6, dtype=np.uint8)  # 6 distinct rows
    patterns, ids, count = np.zeros((256, 6), np.uint8), np.zeros(6, np.uint8), ctypes.c_int(-9)
    args = lambda **kw: [kw.get("shards", 6), kw.get("present", present.ctypes.data), kw.get("nstripes", 6),
                         kw.get("patterns", patterns.ctypes.data), kw.get("cap", 256),
                         kw.get("count", ctypes.byref(count)), kw.get("ids", ids.ctypes.data)]
    assert f(*args()) == 0 and count.value == 6 and list(ids) == list(range(6))
    assert f(*args(cap=6)) == 0
    assert f(*args(cap=5)) == ILL                     # more distinct rows than cap
    assert b"distinct" in lib.ecx_last_error()
    assert f(*args(cap=0)) == ILL and f(*args(cap=257)) == ILL and f(*args(cap=-1)) == ILL
    assert f(*args(nstripes=-1)) == ILL
    assert f(*args(shards=0)) == ILL and f(*args(shards=-3)) == ILL
    assert f(*args(present=None)) == NULL
    assert f(*args(patterns=None)) == NULL
    assert f(*args(count=None)) == NULL
    assert f(*args(ids=None)) == NULL
    assert f(*args(nstripes=0)) == 0 and count.value == 0
    with pytest.raises(ecx.EcxError) as e:
        ecx.index_patterns(present, cap=3)
    assert e.value.code == ILL


def _create(lib, rs_handle, patterns, npatterns=None):
    h = ctypes.c_void_p(0xDEAD)
    pats = np.ascontiguousarray(patterns, np.uint8)
    st = lib.ecx_rs_pattern_set_create(rs_handle, pats.ctypes.data, len(pats) if npatterns is None else npatterns,
                                       ctypes.byref(h))
    return st, h


def test_pattern_set_create_status_codes(ecx):
    lib = ecx.lib()
    rs = ecx.ReedSolomon.create(4, 2)
    ok = np.ones((3, 6), np.uint8)
    ok[1, 2] = 0
    ok[2, [0, 5]] = 0
    st, h = _create(lib, rs._h, ok)
    assert st == 0 and h.value
    lib.ecx_rs_pattern_set_destroy(h)
    # null codec, list or out pointer
    st, h = _create(lib, None, ok)
    assert st == NULL and not h.value               # *out is cleared on failure
    assert lib.ecx_rs_pattern_set_create(rs._h, None, 3, ctypes.byref(h)) == NULL
    assert lib.ecx_rs_pattern_set_create(rs._h, ok.ctypes.data, 3, None) == NULL
    # npatterns outside 1..256
    for bad in (0, -1, 257):
        st, h = _create(lib, rs._h, np.ones((257, 6), np.uint8), bad)
        assert st == ILL and not h.value, bad
    # fewer than k present
    few = ok.copy()
    few[1, [0, 1, 2]] = 0
    st, h = _create(lib, rs._h, few)
    assert st == NOT_ENOUGH and not h.value
    # more than 8 missing with k still present: the message sends the caller to the uniform batch
    wide = ecx.ReedSolomon.create(4, 10)
    nine = np.ones((2, 14), np.uint8)
    nine[1, 5:14] = 0
    st, h = _create(lib, wide._h, nine)
    assert st == ILL and not h.value
    assert b"ecx_rs_decode_missing_batch" in lib.ecx_last_error()
    nine[1, 5] = 1  # exactly 8 missing is a pattern like any other
    st, h = _create(lib, wide._h, nine)
    assert st == 0
    lib.ecx_rs_pattern_set_destroy(h)
    lib.ecx_rs_pattern_set_destroy(None)            # as free(NULL)
    # the Python wrapper raises the same codes
    with pytest.raises(ecx.EcxError) as e:
        rs.patternSet(few)
    assert e.value.code == NOT_ENOUGH
    with pytest.raises(ecx.EcxError) as e:
        rs.patternSet(np.ones((2, 5), np.uint8))        # wrong number of flags per pattern
    assert e.value.code == ILL
    with pytest.raises(ecx.EcxError) as e:
        rs.patternSet(np.ones((0, 6), np.uint8))
    assert e.value.code == ILL


def test_pattern_set_info(ecx):
    rs = ecx.ReedSolomon.create(12, 4)
    pats = np.ones((5, 16), np.uint8)
    pats[1, 3] = 0
    pats[2, [0, 15]] = 0
    pats[3, [1, 2, 3, 14]] = 0
    pats[4] = pats[1]                                   # duplicates are allowed
    with rs.patternSet(pats) as ps:
        assert ps.info() == (5, 16, 4)
        lib = ecx.lib()
        n, mm = ctypes.c_int(), ctypes.c_int()
        assert lib.ecx_rs_pattern_set_info(ps._h, None, ctypes.byref(n), None) == 0 and n.value == 16
        assert lib.ecx_rs_pattern_set_info(ps._h, None, None, ctypes.byref(mm)) == 0 and mm.value == 4
        assert lib.ecx_rs_pattern_set_info(None, None, None, None) == NULL
    ps.close()                                          # idempotent
    with pytest.raises(ecx.EcxError) as e:
        ps.info()
    assert e.value.code == NULL
    with rs.patternSet(np.ones((1, 16), np.uint8)) as none_missing:
        assert none_missing.info() == (1, 16, 0)
    with rs.patternSet(np.ones((256, 16), np.uint8)) as full:
        assert full.info() == (256, 16, 0)


def test_decode_missing_batch_mixed_argument_checks(ecx):
    """Null set, ids or base: NullPointerException; negative counts: IllegalArgumentException;
    an empty batch is a no-op -- all before any device is touched."""
    lib = ecx.lib()
    f = lib.ecx_rs_decode_missing_batch_mixed
    rs = ecx.ReedSolomon.create(4, 2)
    pats = np.ones((2, 6), np.uint8)
    pats[1, 0] = 0
    with rs.patternSet(pats) as ps:
        assert f(None, 16, 4096, 6 * 64, 64, 1, 0, 64, None) == NULL
        assert f(ps._h, None, 4096, 6 * 64, 64, 1, 0, 64, None) == NULL
        assert f(ps._h, 16, None, 6 * 64, 64, 1, 0, 64, None) == NULL
        assert f(ps._h, 16, 4096, 6 * 64, 64, -1, 0, 64, None) == ILL
        assert f(ps._h, 16, 4096, 6 * 64, 64, 1, -1, 64, None) == ILL
        assert f(ps._h, 16, 4096, 6 * 64, 64, 1, 0, -64, None) == ILL
        assert f(ps._h, 16, 4096, 6 * 64, 64, 0, 0, 64, None) == 0
        assert f(ps._h, 16, 4096, 6 * 64, 64, 1, 0, 0, None) == 0
        # the wrapper checks the extents of the shards and of the ids first (CPU tensors stand in:
        # the layout check runs before the device pointers are taken)
        import torch
        shards, ids = torch.zeros((3, 6, 64), dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8)
        with pytest.raises(ecx.EcxError) as e:
            rs.decodeMissingBatchMixed(shards, ps, ids, 6 * 64, 64, 4, 0, 64)   # one stripe too many
        assert e.value.code == -5
        with pytest.raises(ecx.EcxError) as e:
            rs.decodeMissingBatchMixed(shards, ps, torch.zeros(2, dtype=torch.uint8), 6 * 64, 64, 3, 0, 64)
        assert e.value.code == -5 and "ids" in str(e.value)
        other = ecx.ReedSolomon.create(5, 2)
        with pytest.raises(ecx.EcxError) as e:
            other.decodeMissingBatchMixed(shards, ps, ids, 7 * 64, 64, 1, 0, 64)
        assert e.value.code == ILL
    with pytest.raises(ecx.EcxError) as e:
        rs.decodeMissingBatchMixed(shards, ps, ids, 6 * 64, 64, 3, 0, 64)       # closed
    assert e.value.code == NULL


def test_create_and_destroy_many_sets_without_a_device(ecx):
    """A set uploads nothing until its first batch call, so creating and destroying sets makes
    no device call: 100 rounds leave the process and the codec registry as they were."""
    lib = ecx.lib()
    stats = lib.ecx_codec_stats
    stats.argtypes, stats.restype = [ctypes.POINTER(ctypes.c_int)] * 4, ctypes.c_int

    def live():
        v = [ctypes.c_int() for _ in range(4)]
        assert stats(*[ctypes.byref(x) for x in v]) == 0
        return v[0].value

    rs = ecx.ReedSolomon.create(17, 3)
    before = live()
    rng = np.random.default_rng(5)
    for i in range(100):
        pats = np.ones((1 + i % 7, 20), np.uint8)
        for row in pats:
            row[rng.choice(20, int(rng.integers(0, 4)), replace=False)] = 0
        ps = rs.patternSet(pats)
        assert ps.info()[:2] == (len(pats), 20)
        ps.close()
    assert live() == before
    # a set keeps its codec alive after the caller's own reference is gone
    lonely = ecx.ReedSolomon.create(23, 5)
    ps = lonely.patternSet(np.ones((1, 28), np.uint8))
    lib.ecx_rs_destroy(lonely._h)
    lonely._h = None
    assert ps.info() == (1, 28, 0)
    ps.close()
