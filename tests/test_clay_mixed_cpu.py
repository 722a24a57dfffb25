"""Clay pattern sets on the host (include/ecx.h: ecx_clay_pattern_set_*,
ecx_clay_perform_coding_batch_mixed, ecx_clay_perform_coding_mixed_batch_host): everything that is
decided before the first HIP call -- the create refusals, info(), index_erased, the status codes of
the two batch calls and their order, and the plan of the host form -- runs without a device.  The
repair itself is tests/test_clay_mixed.py."""
import ctypes
import itertools

import numpy as np
import pytest

OK, ILL, NSH, IDX, NULL = 0, -1, -2, -5, -6
LISTS42 = [[i] for i in range(6)] + [list(c) for c in itertools.combinations(range(6), 2)] + [[]]


def _create(lib, k, m, lists, v=0, npatterns=None):
    flat = np.ascontiguousarray([e for lst in lists for e in lst] + [0], np.int32)
    counts = np.ascontiguousarray([len(lst) for lst in lists] + [0], np.int32)
    h = ctypes.c_void_p()
    st = lib.ecx_clay_pattern_set_create(k, m, v, flat.ctypes.data, counts.ctypes.data,
                                         len(lists) if npatterns is None else npatterns, ctypes.byref(h))
    return st, h


def test_create_status_codes(ecx):
    lib = ecx.lib()
    st, h = _create(lib, 4, 2, LISTS42)
    assert st == OK and h.value
    lib.ecx_clay_pattern_set_destroy(h)
    lib.ecx_clay_pattern_set_destroy(None)  # as free(NULL)
    # 1..256 lists
    assert _create(lib, 4, 2, [[1]], npatterns=0)[0] == ILL
    st, h = _create(lib, 4, 2, [[s % 6] for s in range(257)])
    assert st == ILL and not h.value and "1..256" in ecx.lib().ecx_last_error().decode()
    st, h = _create(lib, 4, 2, [[s % 6] for s in range(256)])  # duplicates are allowed
    assert st == OK
    lib.ecx_clay_pattern_set_destroy(h)
    # a list the single step refuses: that step's own status
    for k, m, lst in ((4, 2, [6]), (4, 2, [-1]), (4, 2, [0, 1, 2]), (5, 2, [0])):
        er = np.ascontiguousarray(lst, np.int32)
        h1 = ctypes.c_void_p()
        single = lib.ecx_clay_create_ex(k, m, 0, er.ctypes.data, len(lst), 0, ctypes.byref(h1))
        if single == OK:  # refused by the step's map, not by its constructor
            hm = ctypes.c_void_p()
            single = lib.ecx_clay_map(h1, ctypes.byref(hm))
            lib.ecx_clay_destroy(h1)
        assert single < 0, (k, m, lst)
        st, h = _create(lib, k, m, [[0] if k == 4 else [1], lst])
        assert st == single and not h.value, (k, m, lst, st, single)
    # a list of more than 64 rows: Clay(6,3) with three nodes has 81
    st, h = _create(lib, 6, 3, [[0], [0, 1, 2]])
    msg = lib.ecx_last_error().decode()
    assert st == ILL and not h.value
    assert "list 1" in msg and "81 rows" in msg and "ecx_clay_perform_coding_batch" in msg, msg
    # Clay(6,3) with two nodes (54 rows, 7 tiles) fits
    st, h = _create(lib, 6, 3, [[0], [4, 8]])
    assert st == OK
    lib.ecx_clay_pattern_set_destroy(h)
    # null pointers
    counts = np.array([1], np.int32)
    assert lib.ecx_clay_pattern_set_create(4, 2, 0, None, counts.ctypes.data, 1, ctypes.byref(h)) == NULL
    assert lib.ecx_clay_pattern_set_create(4, 2, 0, counts.ctypes.data, None, 1, ctypes.byref(h)) == NULL
    assert lib.ecx_clay_pattern_set_create(4, 2, 0, counts.ctypes.data, counts.ctypes.data, 1, None) == NULL
    neg = np.array([-1], np.int32)
    assert lib.ecx_clay_pattern_set_create(4, 2, 0, counts.ctypes.data, neg.ctypes.data, 1, ctypes.byref(h)) == ILL


def test_set_holds_one_codec_reference_per_distinct_list(ecx):
    lib = ecx.lib()

    def clay_live():
        v = [ctypes.c_int() for _ in range(4)]
        assert lib.ecx_codec_stats(*[ctypes.byref(x) for x in v]) == OK
        return v[2].value

    before = clay_live()
    # (virtualUnits 1 of Clay(3,2): a geometry no other test holds, so the counts are this test's)
    with ecx.ClayPatternSet([[0], [1], [0], [], [1, 2], [0]], 3, 2, 1) as ps:
        assert clay_live() == before + 4  # {0}, {1}, {}, {1,2}
        assert ps.info() == (6, 5, 8, 2)
    assert clay_live() == before


def test_info_and_close(ecx):
    with ecx.ClayPatternSet(LISTS42, 4, 2) as ps:
        assert ps.info() == (22, 6, 8, 2)
        assert (ps.numTotalUnits, ps.subPacketSize, ps.maxErased) == (6, 8, 2)
        lib = ecx.lib()
        n, a = ctypes.c_int(), ctypes.c_int()
        assert lib.ecx_clay_pattern_set_info(ps._h, None, ctypes.byref(n), ctypes.byref(a), None) == OK
        assert (n.value, a.value) == (6, 8)
        assert lib.ecx_clay_pattern_set_info(None, None, None, None, None) == NULL
    ps.close()  # idempotent
    with pytest.raises(ecx.EcxError):
        ps.info()
    assert ecx.ClayPatternSet([[0]], 2, 2).info() == (1, 4, 4, 1)
    assert ecx.ClayPatternSet([[2], [4]], 3, 3).info() == (2, 6, 9, 1)
    assert ecx.ClayPatternSet([[]], 4, 2).info() == (1, 6, 8, 0)


def test_package_exports_the_new_names(ecx):
    assert "ClayPatternSet" in ecx.__all__ and "index_erased" in ecx.__all__
    for name in ("info", "host_plan", "performCodingBatchMixed", "performCodingBatchMixedHost", "close"):
        assert callable(getattr(ecx.ClayPatternSet, name)), name


def test_index_erased(ecx):
    lists, ids = ecx.index_erased([[1], [4], [1], [0, 2], [], [2, 0], [4]])
    assert lists == [(1,), (4,), (0, 2), (), (2, 0)]  # first appearance; the order of a list's nodes matters
    assert ids.dtype == np.uint8 and list(ids) == [0, 1, 0, 2, 3, 4, 1]
    assert ecx.index_erased([])[0] == [] and len(ecx.index_erased([])[1]) == 0
    many = [[i, j] for i in range(20) for j in range(20) if i != j][:257]
    with pytest.raises(ecx.EcxError):
        ecx.index_erased(many)
    lists, ids = ecx.index_erased(many[:256])
    assert len(lists) == 256 and list(ids) == list(range(256))
    # the lists feed the set, the ids the batch call
    lists, ids = ecx.index_erased([[s % 6] for s in range(13)])
    with ecx.ClayPatternSet(lists, 4, 2) as ps:
        assert ps.info() == (6, 6, 8, 1)
    assert list(ids) == [s % 6 for s in range(13)]


@pytest.mark.parametrize("fn", ["ecx_clay_perform_coding_batch_mixed", "ecx_clay_perform_coding_mixed_batch_host"])
def test_batch_status_codes_and_their_order(ecx, fn):
    """Neither form touches a device before its checks are done (this machine may have none)."""
    lib = ecx.lib()
    f = getattr(lib, fn)
    host = fn.endswith("_host")
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data

    def call(h, ids=p, inp=p, iss=48, isl=1, out=p, oss=16, osl=1, S=1, B=1):
        args = [h, ids, inp, iss, isl, out, oss, osl, S, B]
        return f(*args) if host else f(*(args + [None]))

    with ecx.ClayPatternSet(LISTS42, 4, 2) as ps, ecx.ClayPatternSet([[], []], 4, 2) as empty:
        h = ps._h
        # 1. a null set, before anything else
        assert call(None, S=-1, ids=None) == NULL
        # 2. negative counts, before the empty batch and before the pointers
        assert call(h, S=-1, ids=None) == ILL and call(h, B=-1, inp=None) == ILL
        assert call(h, S=-1, B=0) == ILL and call(h, S=0, B=-1) == ILL
        # 3. nothing to do: no buffer is looked at, no stride, no device
        assert call(h, S=0, ids=None, inp=None, out=None, iss=-1) == OK
        assert call(h, B=0, ids=None, inp=None, out=None, osl=-1) == OK
        assert call(empty._h, ids=None, inp=None, out=None, iss=-1, S=5, B=5) == OK
        # 4. a null pointer among the three, before the strides
        assert call(h, ids=None, iss=-1) == NULL and call(h, inp=None, isl=-1) == NULL
        assert call(h, out=None, oss=-1) == NULL
        # 5. negative strides and extents beyond int64
        for kw in ({"iss": -1}, {"isl": -1}, {"oss": -1}, {"osl": -1}):
            assert call(h, **kw) == ILL, kw
        big = (1 << 62)
        assert call(h, S=4, iss=big) == ILL and call(h, S=4, oss=big) == ILL
        assert call(h, isl=big) == ILL and call(h, osl=big) == ILL
        assert call(h, S=3, iss=1 << 61, B=1 << 62) == ILL
    assert (buf == 0).all()


def test_python_extent_checks_are_those_of_the_uniform_batch(ecx):
    """_check_batch: the layout must fit the buffers, as for performCodingBatch."""
    B, S = 64, 3
    inp, out = np.zeros(S * 48 * B, np.uint8), np.zeros(S * 16 * B, np.uint8)
    ids = np.zeros(S, np.uint8)
    with ecx.ClayPatternSet(LISTS42, 4, 2) as ps:
        for kw in ({"inp": inp[1:]}, {"out": out[1:]}, {"ids": ids[1:]}):
            a = {"inp": inp, "out": out, "ids": ids, **kw}
            with pytest.raises(ecx.EcxError) as err:
                ps.performCodingBatchMixedHost(a["inp"], 48 * B, B, a["out"], 16 * B, B, a["ids"], S, B)
            assert err.value.code == IDX, kw
        with pytest.raises(ecx.EcxError) as err:
            ps.performCodingBatchMixedHost(inp, -1, B, out, 16 * B, B, ids, S, B)
        assert err.value.code == ILL
    with ecx.ClayPatternSet([[1], [4]], 4, 2) as ps:  # single nodes: 8 output slots are enough
        with pytest.raises(ecx.EcxError) as err:
            ps.performCodingBatchMixedHost(inp, 48 * B, B, np.zeros(S * 8 * B - 1, np.uint8), 8 * B, B, ids, S, B)
        assert err.value.code == IDX


class chunk_kib:
    def __init__(self, ecx, kib):
        self.ecx, self.kib = ecx, kib

    def __enter__(self):
        self.was = self.ecx.tune_value("host_chunk_kib")
        self.ecx.tune("host_chunk_kib", self.kib)

    def __exit__(self, *exc):
        self.ecx.tune("host_chunk_kib", self.was)


def test_host_plan_of_the_host_form(ecx):
    """ecx_clay_pattern_set_host_plan: the union of the lists' input slots goes up, output slots
    0 .. maxErased*alpha - 1 come back, and chunks carry host_chunk_kib of input."""
    B, S = 4096, 24
    zero = dict.fromkeys(("slots_up", "slots_down", "chunk", "chunks", "buffers", "h2d_copies", "d2h_copies"), 0)
    with ecx.ClayPatternSet(LISTS42, 4, 2) as ps:
        with chunk_kib(ecx, 16):  # 16 KiB < one stripe's 48 * 4 KiB: a stripe per chunk, a ring of 3 sets
            plan = ps.host_plan(48 * B, B, 16 * B, B, S, B)
            assert plan == {"slots_up": 48, "slots_down": 16, "chunk": 1, "chunks": 24, "buffers": 3, "h2d_copies": 1,
                            "d2h_copies": 1}, plan
        with chunk_kib(ecx, 1024):  # 1 MiB / (48 * 4 KiB) = 5 stripes per chunk
            plan = ps.host_plan(48 * B, B, 16 * B, B, S, B)
            assert (plan["chunk"], plan["chunks"]) == (5, 5), plan
            # padded pitches: a copy per slot run instead of one per stripe side
            plan = ps.host_plan(48 * (B + 64), B + 64, 16 * (B + 64), B + 64, S, B)
            assert (plan["slots_up"], plan["slots_down"]) == (48, 16) and plan["h2d_copies"] >= 1, plan
        assert ps.host_plan(48 * B, B, 16 * B, B, 0, B) == zero and ps.host_plan(48 * B, B, 16 * B, B, S, 0) == zero
    # single nodes 1 and 4 (one column of the grid): each reads 20 sub-chunks, the union is smaller than 48
    with ecx.ClayPatternSet([[1], [4]], 4, 2) as ps, chunk_kib(ecx, 16):
        plan = ps.host_plan(48 * B, B, 8 * B, B, S, B)
        one = ecx.ClayCodeErasureDecodingStep([1], 4, 2).map().info()["n_in"]
        assert one == 20 and one < plan["slots_up"] < 48 and plan["slots_down"] == 8, plan
        assert plan["chunk"] == 1 and plan["chunks"] == S
    with ecx.ClayPatternSet([[1]], 4, 2) as ps:
        assert ps.host_plan(48 * B, B, 8 * B, B, S, B)["slots_up"] == 20
    with ecx.ClayPatternSet([[], []], 4, 2) as ps:
        assert ps.host_plan(48 * B, B, 8 * B, B, S, B) == zero
    lib = ecx.lib()
    out = np.zeros(7, np.int64)
    assert lib.ecx_clay_pattern_set_host_plan(None, 1, 1, 1, 1, 1, 1, out.ctypes.data) == NULL
    with ecx.ClayPatternSet([[1]], 4, 2) as ps:
        assert lib.ecx_clay_pattern_set_host_plan(ps._h, 1, 1, 1, 1, 1, 1, None) == NULL
        assert lib.ecx_clay_pattern_set_host_plan(ps._h, 1, 1, 1, 1, -1, 1, out.ctypes.data) == ILL
