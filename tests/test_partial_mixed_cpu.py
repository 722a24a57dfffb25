"""ecx_rs_decode_partial_batch_mixed (include/ecx.h) where no GPU is needed: that the export
exists, the status of every argument rule that holds before any device work and the order of those
rules, the status without a device (no CPU fallback), and the Python method's own refusals.  The
hop itself is tests/test_partial_mixed.py.  RS(4,2), 3 stripes of 100-byte shards."""
import numpy as np
import pytest

OK, ILL, IDX, NUL, DEV = 0, -1, -5, -6, -10
K, M, S, L = 4, 2, 3, 100
N = K + M
ROWS = 2
NAME = "ecx_rs_decode_partial_batch_mixed"


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
    pats[2, 0] = pats[2, 3] = 0
    inp = np.arange(S * L, dtype=np.uint32).astype(np.uint8)
    acc = np.full(S * ROWS * L, 0xA5, np.uint8)
    ids = np.array([1, 2, 0], np.uint8)
    shard_of = np.array([0, 1, 2], np.uint8)
    with rs.patternSet(pats) as ps, rs.patternSet(np.ones((2, N), np.uint8)) as whole:
        yield rs, ps, whole, inp, acc, ids, shard_of


def test_the_export_exists(ecx):
    assert callable(getattr(ecx.lib(), NAME))


def test_argument_rules_in_order(ecx, batch):
    """Null set; then negative counts; then the empty batch and the set that misses nothing, which
    need no buffers and no device; then a null pointer among the four; then the extent."""
    rs, ps, whole, inp, acc, ids, shard_of = batch
    g = getattr(ecx.lib(), NAME)

    def f(st, i, sh, x, a, s=S, c=L, in_ss=L, in_sh=0, acc_ss=ROWS * L, acc_rs=L, first=1):
        return g(st, i, sh, x, in_ss, in_sh, a, acc_ss, acc_rs, s, c, first, None)

    i, sh, x, a = ids.ctypes.data, shard_of.ctypes.data, inp.ctypes.data, acc.ctypes.data
    assert f(None, i, sh, x, a) == NUL
    assert f(None, None, None, None, None, s=-1, c=-1) == NUL          # the set first
    assert f(ps._h, i, sh, x, a, s=-1) == ILL
    assert f(ps._h, i, sh, x, a, c=-1) == ILL
    assert f(ps._h, None, None, None, None, s=-1) == ILL               # the counts before the pointers
    assert f(ps._h, None, None, None, None, s=0, c=-1) == ILL          # and before the empty batch
    assert f(ps._h, None, None, None, None, s=0) == OK                 # empty: no buffers needed
    assert f(ps._h, None, None, None, None, c=0) == OK
    assert f(ps._h, None, None, None, None, s=0, in_ss=-1, acc_rs=2**62) == OK   # nor a look at the strides
    assert f(whole._h, None, None, None, None) == OK                   # nothing missing anywhere
    assert f(whole._h, i, sh, x, a, s=2**62, c=2**40, in_ss=2**40) == OK
    for k in range(4):                                                 # a null pointer among the four
        args = [i, sh, x, a]
        args[k] = None
        assert f(ps._h, *args) == NUL, k
        assert f(ps._h, *args, s=2**62, in_ss=2**40) == NUL, k         # the pointers before the extent
    assert f(ps._h, i, sh, x, a, s=2**62, in_ss=2**40) == ILL          # extents beyond int64_t
    assert f(ps._h, i, sh, x, a, s=2**62, acc_ss=2**40) == ILL
    assert f(ps._h, i, sh, x, a, in_sh=2**62) == ILL                   # (n - 1) * in_shard_stride
    assert f(ps._h, i, sh, x, a, acc_rs=2**63 - 50) == ILL             # (rows - 1) * acc_row_stride + byte_count
    assert f(ps._h, i, sh, x, a, c=2**63 - 1, in_ss=1) == ILL
    for name in ("in_ss", "in_sh", "acc_ss", "acc_rs"):
        assert f(ps._h, i, sh, x, a, **{name: -16}) == ILL, name
    assert (acc == 0xA5).all()


def test_without_a_device_a_hop_with_work_fails_loudly(ecx, batch):
    """No CPU fallback: ECX_E_DEVICE, and the accumulator keeps its bytes."""
    if _has_device(ecx):
        pytest.skip("a device is present")
    rs, ps, whole, inp, acc, ids, shard_of = batch
    g = getattr(ecx.lib(), NAME)
    # (handed host addresses: it must fail before it would launch anything)
    for first in (1, 0):
        assert g(ps._h, ids.ctypes.data, shard_of.ctypes.data, inp.ctypes.data, L, 0, acc.ctypes.data, ROWS * L, L,
                 S, L, first, None) == DEV
    assert (acc == 0xA5).all()


def test_python_method_refusals(ecx, batch):
    rs, ps, whole, inp, acc, ids, shard_of = batch
    other = ecx.ReedSolomon.create(3, 1)
    with pytest.raises(ecx.EcxError) as e:
        other.decodePartialBatchMixed(ps, 0, 0, 0, L, 0, 0, ROWS * L, L, S, L, True)
    assert e.value.code == ILL and "another code" in str(e.value)
    with pytest.raises(TypeError):  # host arrays are not device tensors
        rs.decodePartialBatchMixed(ps, ids, shard_of, inp, L, 0, acc, ROWS * L, L, S, L, True)
    with pytest.raises(ecx.EcxError) as e:
        rs.decodePartialBatchMixed(ps, 0, 0, 0, -L, 0, 0, ROWS * L, L, S, L, True)
    assert e.value.code == ILL and "negative stride" in str(e.value)
    ps.close()
    with pytest.raises(ecx.EcxError) as e:
        rs.decodePartialBatchMixed(ps, 0, 0, 0, L, 0, 0, ROWS * L, L, S, L, True)
    assert e.value.code == NUL and "closed" in str(e.value)
