"""The corrupt-shard locate (include/ecx.h: ecx_rs_locate_corrupt_batch,
ecx_rs_locate_corrupt_blocked_batch) where no GPU is needed: the argument rules that hold before any
device work, in the order of ecx_rs_is_parity_correct_batch; the status without a device (no CPU
fallback); the binding table rows; and singleLossPatternSet."""
import ctypes

import numpy as np
import pytest

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
        "ecx_rs_locate_corrupt_batch":
            lambda r, b, s, c, su, cu, he, x=0: lib.ecx_rs_locate_corrupt_batch(r, b, 6 * 128, 128, s, x, c, su, cu, he, None),
        "ecx_rs_locate_corrupt_blocked_batch":
            lambda r, b, s, c, su, cu, he, x=0: lib.ecx_rs_locate_corrupt_blocked_batch(r, b, s, c, x, su, cu, he, None),
    }


def test_locate_argument_rules(ecx):
    """A null codec is ECX_E_NULL; then a negative count (offset, block) is ECX_E_ILLEGAL_ARGUMENT;
    then m < 2, m > 8 and heal ids for n > 255 are; then an empty batch is ECX_OK with null
    pointers; then a null base, suspect or culprit is ECX_E_NULL -- a null heal_id is not.
    Nothing is written."""
    rs = ecx.ReedSolomon.create(4, 2)
    S, L = 3, 100
    base = np.zeros(S * 6 * 128, np.uint8)
    su, cu, he = np.full(S * 6, 7, np.uint8), np.full(S, 7, np.int32), np.full(S, 7, np.uint8)
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
        for k, m in ((4, 1), (4, 9), (1, 1)):
            r = ecx.ReedSolomon.create(k, m)
            assert f(r._h, b, S, L, s_, c_, h_) == ILL, (name, k, m)
            assert f(r._h, None, 0, L, None, None, None) == ILL, (name, k, m)  # the codec, before the batch
        wide = ecx.ReedSolomon.create(250, 6)  # n = 256: no byte names shard 255 AND "no pattern"
        assert f(wide._h, None, 0, L, None, None, h_) == ILL, name
        assert f(wide._h, None, 0, L, None, None, None) == OK, name
        # with everything in order the call reaches the device -- or reports that there is none
        if not _has_device(ecx):
            assert f(rs._h, b, S, L, s_, c_, h_) == DEV, name
            assert f(rs._h, b, S, L, s_, c_, None) == DEV, name
    assert (su == 7).all() and (cu == 7).all() and (he == 7).all() and not base.any()


def test_locate_python_mirror_checks_extents(ecx):
    """locateCorruptBatch / locateCorruptBlockedBatch refuse a short buffer with ECX_E_INDEX before
    the library is called, with or without a device."""
    rs = ecx.ReedSolomon.create(4, 2)
    S, L, n = 3, 100, 6
    base = np.zeros(S * n * L, np.uint8)
    su, cu, he = np.zeros(S * n, np.uint8), np.zeros(S, np.int32), np.zeros(S, np.uint8)
    import torch
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    for args in ((t(base)[1:], t(su), t(cu), t(he)), (t(base), t(su)[1:], t(cu), t(he)),
                 (t(base), t(su), t(cu)[1:], t(he)), (t(base), t(su), t(cu), t(he)[1:])):
        for call in (lambda bb, a, c, h: rs.locateCorruptBatch(bb, n * L, L, S, 0, L, a, c, h),
                     lambda bb, a, c, h: rs.locateCorruptBlockedBatch(bb, S, L, a, c, h)):
            with pytest.raises(ecx.EcxError) as e:
                call(*args)
            assert e.value.code == IDX


def test_locate_binding_rows(ecx):
    """The ctypes table binds both exports with the header's parameter lists."""
    from importlib import import_module
    rows = import_module(ecx.__name__ + "._lib").SIGNATURES
    I, P, I64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert rows["ecx_rs_locate_corrupt_batch"] == (I, [P, P, I64, I64, I64, I64, I64, P, P, P, P])
    assert rows["ecx_rs_locate_corrupt_blocked_batch"] == (I, [P, P, I64, I64, I64, P, P, P, P])
    lib = ecx.lib()
    for name in ("ecx_rs_locate_corrupt_batch", "ecx_rs_locate_corrupt_blocked_batch"):
        assert getattr(lib, name).argtypes == rows[name][1]
    assert lib.ecx_version() >= 108


def test_single_loss_pattern_set(ecx, monkeypatch):
    """singleLossPatternSet() is patternSet(1 - eye(n)): n patterns, shard order, one shard each."""
    rs = ecx.ReedSolomon.create(4, 2)
    with rs.singleLossPatternSet() as ps:
        assert ps.info() == (6, 6, 1)
    seen = []
    monkeypatch.setattr(type(rs), "patternSet", lambda self, p: seen.append(np.asarray(p)) or "set")
    assert rs.singleLossPatternSet() == "set"
    assert len(seen) == 1 and (seen[0] == 1 - np.eye(6, dtype=np.uint8)).all()
