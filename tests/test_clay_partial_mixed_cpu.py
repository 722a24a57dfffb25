"""ecx_clay_partial_batch_mixed (include/ecx.h) where no GPU is needed: that the export exists, the
status of every argument rule that holds before any device work and the order of those rules, a set
whose lists are all empty, the status without a device (no CPU fallback), and the Python method's
own refusals, a closed set among them.  The hop itself is tests/test_clay_partial_mixed.py.
Clay(4,2), 3 stripes of 100-byte sub-chunks, one helper's planes back to back."""
import numpy as np
import pytest

OK, ILL, IDX, NUL, DEV = 0, -1, -5, -6, -10
K, M, S, B = 4, 2, 3, 100
N, ALPHA = K + M, 8
ROWS = 2 * ALPHA
NAME = "ecx_clay_partial_batch_mixed"


def _has_device(ecx):
    try:
        return ecx.device_count() > 0
    except ecx.EcxError:
        return False


@pytest.fixture
def batch(ecx):
    inp = np.arange(S * ALPHA * B, dtype=np.uint32).astype(np.uint8)
    acc = np.full(S * ROWS * B, 0xA5, np.uint8)
    ids = np.array([1, 2, 0], np.uint8)
    node_of = np.array([0, 1, 2], np.uint8)
    with ecx.ClayPatternSet([[1], [5], [0, 3]], K, M) as ps, ecx.ClayPatternSet([[], []], K, M) as empty:
        yield ps, empty, inp, acc, ids, node_of


def test_the_export_exists(ecx):
    assert callable(getattr(ecx.lib(), NAME))
    assert callable(ecx.ClayPatternSet.partialBatchMixed)


def test_argument_rules_in_order(ecx, batch):
    """Null set; then negative counts; then the empty batch and the set whose lists are all empty,
    which need no buffers and no device; then a null pointer among the four; then the extent."""
    ps, empty, inp, acc, ids, node_of = batch
    g = getattr(ecx.lib(), NAME)

    def f(st, i, nd, x, a, s=S, c=B, in_ss=ALPHA * B, in_ns=0, in_sub=B, acc_ss=ROWS * B, acc_sub=B, first=1):
        return g(st, i, nd, x, in_ss, in_ns, in_sub, a, acc_ss, acc_sub, s, c, first, None)

    i, nd, x, a = ids.ctypes.data, node_of.ctypes.data, inp.ctypes.data, acc.ctypes.data
    assert f(None, i, nd, x, a) == NUL
    assert f(None, None, None, None, None, s=-1, c=-1) == NUL          # the set first
    assert f(ps._h, i, nd, x, a, s=-1) == ILL
    assert f(ps._h, i, nd, x, a, c=-1) == ILL
    assert f(ps._h, None, None, None, None, s=-1) == ILL               # the counts before the pointers
    assert f(ps._h, None, None, None, None, s=0, c=-1) == ILL          # and before the empty batch
    assert f(ps._h, None, None, None, None, s=0) == OK                 # empty: no buffers needed
    assert f(ps._h, None, None, None, None, c=0) == OK
    assert f(ps._h, None, None, None, None, s=0, in_ss=-1, acc_sub=2**62) == OK   # nor a look at the strides
    assert f(empty._h, None, None, None, None) == OK                   # every list empty
    assert f(empty._h, None, None, None, None, first=0) == OK
    assert f(empty._h, i, nd, x, a, s=2**62, c=2**40, in_ss=2**40) == OK
    for k in range(4):                                                 # a null pointer among the four
        args = [i, nd, x, a]
        args[k] = None
        assert f(ps._h, *args) == NUL, k
        assert f(ps._h, *args, s=2**62, in_ss=2**40) == NUL, k         # the pointers before the extent
    assert f(ps._h, i, nd, x, a, s=2**62, in_ss=2**40) == ILL          # extents beyond int64_t
    assert f(ps._h, i, nd, x, a, s=2**62, acc_ss=2**40) == ILL
    assert f(ps._h, i, nd, x, a, in_ns=2**62) == ILL                   # (n - 1) * in_node_stride
    assert f(ps._h, i, nd, x, a, in_sub=2**62) == ILL                  # (alpha - 1) * in_sub_stride
    assert f(ps._h, i, nd, x, a, acc_sub=2**63 - 50) == ILL            # (rows - 1) * acc_sub_stride + buf_size
    assert f(ps._h, i, nd, x, a, c=2**63 - 1, in_ss=1) == ILL
    for name in ("in_ss", "in_ns", "in_sub", "acc_ss", "acc_sub"):
        assert f(ps._h, i, nd, x, a, **{name: -16}) == ILL, name
    assert (acc == 0xA5).all()


def test_without_a_device_a_hop_with_work_fails_loudly(ecx, batch):
    """No CPU fallback: ECX_E_DEVICE, and the accumulator keeps its bytes."""
    if _has_device(ecx):
        pytest.skip("a device is present")
    ps, empty, inp, acc, ids, node_of = batch
    g = getattr(ecx.lib(), NAME)
    # (handed host addresses: it must fail before it would launch anything)
    for first in (1, 0):
        assert g(ps._h, ids.ctypes.data, node_of.ctypes.data, inp.ctypes.data, ALPHA * B, 0, B, acc.ctypes.data,
                 ROWS * B, B, S, B, first, None) == DEV
    assert (acc == 0xA5).all()


def test_python_method_refusals(ecx, batch):
    ps, empty, inp, acc, ids, node_of = batch
    with pytest.raises(TypeError):  # host arrays are not device tensors
        ps.partialBatchMixed(ids, node_of, inp, ALPHA * B, 0, B, acc, ROWS * B, B, S, B, True)
    for strides in ((-B, 0, B, ROWS * B, B), (ALPHA * B, -B, B, ROWS * B, B), (ALPHA * B, 0, -B, ROWS * B, B),
                    (ALPHA * B, 0, B, -ROWS * B, B), (ALPHA * B, 0, B, ROWS * B, -B)):
        with pytest.raises(ecx.EcxError) as e:
            ps.partialBatchMixed(0, 0, 0, strides[0], strides[1], strides[2], 0, strides[3], strides[4], S, B, True)
        assert e.value.code == ILL and "negative stride" in str(e.value), strides
    # a set whose lists are all empty needs no buffers
    empty.partialBatchMixed(0, 0, 0, ALPHA * B, 0, B, 0, ROWS * B, B, S, B, True)
    ps.close()
    with pytest.raises(ecx.EcxError) as e:
        ps.partialBatchMixed(0, 0, 0, ALPHA * B, 0, B, 0, ROWS * B, B, S, B, True)
    assert e.value.code == NUL and "closed" in str(e.value)
