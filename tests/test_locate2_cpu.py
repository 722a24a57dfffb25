"""The two-shard locate (include/ecx.h: ecx_rs_locate_corrupt2_batch,
ecx_rs_locate_corrupt2_blocked_batch) where no GPU is needed: the argument rules that hold before
any device work, in the order of ecx_rs_locate_corrupt_batch; the binding table rows and the
version; pair_index / pair_of; doubleLossPatternSet's row order; and that the brute-force
expectations of every GPU shape hold all three kinds of stripe."""
import ctypes

import numpy as np
import pytest

import locate2_cases as C

OK, ILL, IDX, NUL, DEV = 0, -1, -5, -6, -10


def _has_device(ecx):
    try:
        return ecx.device_count() > 0
    except ecx.EcxError:
        return False


def _calls(ecx):
    """Both exports as f(rs, base, nstripes, byte_count, suspect, culprit, heal, extra) -> status;
    `extra` is the natural form's offset, the blocked form's block."""
    lib = ecx.lib()
    return {
        "ecx_rs_locate_corrupt2_batch":
            lambda r, b, s, c, su, cu, he, x=0: lib.ecx_rs_locate_corrupt2_batch(r, b, 6 * 128, 128, s, x, c, su, cu, he, None),
        "ecx_rs_locate_corrupt2_blocked_batch":
            lambda r, b, s, c, su, cu, he, x=0: lib.ecx_rs_locate_corrupt2_blocked_batch(r, b, s, c, x, su, cu, he, None),
    }


def test_locate2_argument_rules(ecx):
    """A null codec is ECX_E_NULL; then a negative count (offset, block) is ECX_E_ILLEGAL_ARGUMENT;
    then m < 4, m > 8, n > 64 and heal ids for n > 22 are; then an empty batch is ECX_OK with null
    pointers; then a null base, suspect or culprit is ECX_E_NULL -- a null heal_id is not.
    Nothing is written."""
    rs = ecx.ReedSolomon.create(2, 4)
    S, L = 3, 100
    base = np.zeros(S * 6 * 128, np.uint8)
    su, cu, he = np.full(S * 21, 7, np.uint8), np.full(2 * S, 7, np.int32), np.full(S, 7, np.uint8)
    b, s_, c_, h_ = base.ctypes.data, su.ctypes.data, cu.ctypes.data, he.ctypes.data
    for name, f in _calls(ecx).items():
        assert f(None, b, S, L, s_, c_, h_) == NUL, name
        assert f(None, b, -1, L, s_, c_, h_) == NUL, name              # the codec first
        assert f(rs._h, b, -1, L, s_, c_, h_) == ILL, name
        assert f(rs._h, b, S, -1, s_, c_, h_) == ILL, name
        assert f(rs._h, b, S, L, s_, c_, h_, -1) == ILL, name           # offset / block
        assert f(rs._h, None, -1, L, None, None, None) == ILL, name     # counts before pointers
        assert f(rs._h, None, 0, L, None, None, None) == OK, name       # an empty batch touches nothing
        assert f(rs._h, None, S, L, s_, c_, h_) == NUL, name
        assert f(rs._h, b, S, L, None, c_, h_) == NUL, name
        assert f(rs._h, b, S, L, s_, None, h_) == NUL, name
        for k, m in ((4, 3), (4, 2), (4, 9), (61, 4)):  # m < 4; m > 8; n = 65
            r = ecx.ReedSolomon.create(k, m)
            assert f(r._h, b, S, L, s_, c_, None) == ILL, (name, k, m)
            assert f(r._h, None, 0, L, None, None, None) == ILL, (name, k, m)  # the codec, before the batch
        wide = ecx.ReedSolomon.create(19, 4)  # n = 23: 23 + 253 = 276 ids do not fit a byte
        assert f(wide._h, None, 0, L, None, None, h_) == ILL, name
        assert f(wide._h, None, 0, L, None, None, None) == OK, name
        fits = ecx.ReedSolomon.create(18, 4)  # n = 22: 22 + 231 = 253
        assert f(fits._h, None, 0, L, None, None, h_) == OK, name
        assert f(ecx.ReedSolomon.create(60, 4)._h, None, 0, L, None, None, None) == OK, name  # n = 64
        # with everything in order the call reaches the device -- or reports that there is none
        if not _has_device(ecx):
            assert f(rs._h, b, S, L, s_, c_, h_) == DEV, name
            assert f(rs._h, b, S, L, s_, c_, None) == DEV, name
    assert (su == 7).all() and (cu == 7).all() and (he == 7).all() and not base.any()


def test_locate2_python_mirror_checks_extents(ecx):
    """locateCorrupt2Batch / locateCorrupt2BlockedBatch refuse a short buffer with ECX_E_INDEX before
    the library is called, with or without a device: suspect rows are n + C(n,2) bytes, culprits two
    int32 per stripe."""
    rs = ecx.ReedSolomon.create(2, 4)
    S, L, n = 3, 100, 6
    base = np.zeros(S * n * L, np.uint8)
    su, cu, he = np.zeros(S * 21, np.uint8), np.zeros(2 * S, np.int32), np.zeros(S, np.uint8)
    import torch
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    for args in ((t(base)[1:], t(su), t(cu), t(he)), (t(base), t(su)[1:], t(cu), t(he)),
                 (t(base), t(su), t(cu)[1:], t(he)), (t(base), t(su), t(cu), t(he)[1:])):
        for call in (lambda bb, a, c, h: rs.locateCorrupt2Batch(bb, n * L, L, S, 0, L, a, c, h),
                     lambda bb, a, c, h: rs.locateCorrupt2BlockedBatch(bb, S, L, a, c, h)):
            with pytest.raises(ecx.EcxError) as e:
                call(*args)
            assert e.value.code == IDX


def test_locate2_binding_rows_and_version(ecx):
    """The ctypes table binds both exports with the header's parameter lists; the library is 1.09."""
    from importlib import import_module
    rows = import_module(ecx.__name__ + "._lib").SIGNATURES
    I, P, I64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert rows["ecx_rs_locate_corrupt2_batch"] == (I, [P, P, I64, I64, I64, I64, I64, P, P, P, P])
    assert rows["ecx_rs_locate_corrupt2_blocked_batch"] == (I, [P, P, I64, I64, I64, P, P, P, P])
    lib = ecx.lib()
    for name in ("ecx_rs_locate_corrupt2_batch", "ecx_rs_locate_corrupt2_blocked_batch"):
        assert getattr(lib, name).argtypes == rows[name][1]
    assert lib.ecx_version() >= 109


def test_pair_index_round_trip(ecx):
    """pair_index is the place in lexicographic order, pair_of its inverse, for every n up to 64."""
    for n in (2, 3, 6, 16, 22, 64):
        pairs = C.pairs_of(n)
        assert [ecx.pair_index(n, i, j) for i, j in pairs] == list(range(len(pairs)))
        assert [ecx.pair_of(n, p) for p in range(len(pairs))] == pairs
    for bad in ((6, 3, 3), (6, 4, 2), (6, -1, 2), (6, 2, 6)):
        with pytest.raises(ValueError):
            ecx.pair_index(*bad)
    for bad in ((6, -1), (6, 15)):
        with pytest.raises(ValueError):
            ecx.pair_of(*bad)


def test_double_loss_pattern_set_row_order(ecx, monkeypatch):
    """doubleLossPatternSet() is the n single-loss patterns in shard order, then the C(n,2) pair-loss
    patterns in pair order: n + C(n,2) patterns, at most two shards missing."""
    rs = ecx.ReedSolomon.create(2, 4)
    with rs.doubleLossPatternSet() as ps:
        assert ps.info() == (21, 6, 2)
    seen = []
    monkeypatch.setattr(type(rs), "patternSet", lambda self, p: seen.append(np.asarray(p)) or "set")
    assert rs.doubleLossPatternSet() == "set"
    want = [[int(x != j) for x in range(6)] for j in range(6)]
    want += [[int(x not in (i, j)) for x in range(6)] for i, j in C.pairs_of(6)]
    assert len(seen) == 1 and seen[0].tolist() == want


@pytest.mark.parametrize("k,m,L,first,count,P", C.SHAPES)
def test_gpu_shapes_hold_every_kind_of_stripe(k, m, L, first, count, P):
    """By the oracle alone, each shape of tests/test_locate2.py has at least 2 stripes whose culprit is
    a single shard, 5 whose culprit is a pair and 1 with nobody: a device answering "nobody"
    everywhere cannot pass.  The stripes the case table promises are what it promises."""
    n = k + m
    _, _, (want_s, want_c, want_h), _ = C.fourteen_stripes(k, m, L, first, count, P)
    single, pair, nobody = C.kinds(want_c)
    print(f"RS({k},{m}) L={L}: {single} single, {pair} pair, {nobody} nobody; culprit={want_c.tolist()}")
    assert single >= 2 and pair >= 5 and nobody >= 1
    assert want_c[[0, 12]].tolist() == [[-1, -1]] * 2 and want_s[[0, 12]].all()
    assert want_c[1].tolist() == [0, -1] and want_c[2].tolist() == [n - 1, -1]
    assert want_s[1].sum() == n and want_s[2].sum() == n  # the shard and the n - 1 pairs with it
    assert want_c[3:11].tolist() == [[0, 1], [k - 1, k], [k, n - 1], [1, k + 1], [0, n - 2], [1, k + 2], [0, k],
                                     [0, n - 2]]
    assert (want_s[3:11].sum(axis=1) == 1).all()
    assert want_c[11].tolist() == [-2, -2] and want_c[13].tolist() == [-2, -2]
    pairs = C.pairs_of(n)
    for s in range(3, 11):
        assert want_h[s] == n + pairs.index(tuple(want_c[s].tolist()))
    assert want_h[[0, 11, 12, 13]].tolist() == [255] * 4 and want_h[1] == 0 and want_h[2] == n - 1
