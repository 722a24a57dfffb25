"""The six blocked RS apply exports (encode / decode x device, host, host over a device list) where
no GPU is needed: the argument rules that hold before any device work and their order, and their
status without a device (no CPU fallback), as tests/test_blocked_check_cpu.py for the check family.
RS(4,2), 3 stripes of 100-byte shards, the recommended block (0) and a block of 32."""
import numpy as np
import pytest

OK, ILL, FEW, NUL, DEV = 0, -1, -2, -6, -10
K, M, S, L = 4, 2, 3, 100
N = K + M
BLOCKS = (0, 32)
DEVICE, HOST, DEVICES = ("ecx_rs_%s_blocked_batch", "ecx_rs_%s_blocked_batch_host",
                         "ecx_rs_%s_blocked_batch_host_devices")
ENC, DEC = "encode_parity", "decode_missing"


def _has_device(ecx):
    try:
        return ecx.device_count() > 0
    except ecx.EcxError:
        return False


def _exports(ecx):
    """The six exports as (name, form, decodes, f(rs, present, base, nstripes, byte_count, block, devs, ndev) -> status);
    the encode forms take no `present`, only the _devices forms the list."""
    lib = ecx.lib()
    out = []
    for form in (DEVICE, HOST, DEVICES):
        for op in (ENC, DEC):
            g = getattr(lib, form % op)

            def f(rs, present, base, s, c, blk, devs=None, nd=0, g=g, form=form, op=op):
                args = (rs,) + ((present,) if op == DEC else ()) + (base, s, c, blk)
                return g(*args + {DEVICE: (None,), HOST: (), DEVICES: (devs, nd)}[form])
            out.append((form % op, form, op == DEC, f))
    assert len(out) == 6
    return out


@pytest.fixture
def batch(ecx):
    rs = ecx.ReedSolomon.create(K, M)
    base = np.arange(S * N * L, dtype=np.uint32).astype(np.uint8)
    masks = {"one": np.array([1, 0, 1, 1, 1, 1], np.uint8), "few": np.array([1, 0, 0, 1, 1, 0], np.uint8),
             "all": np.ones(N, np.uint8)}
    return rs, base, base.copy(), masks, np.zeros(2, np.int32)


def test_blocked_apply_argument_rules(ecx, batch):
    """Before any device work, for each of the six exports: a negative count or block is
    ECX_E_ILLEGAL_ARGUMENT; a null base with stripes is ECX_E_NULL, and without stripes still for
    the device forms, while the host forms take it as the empty batch; the host forms refuse a null
    codec, the _devices forms a null, empty or negative list, and the list before the counts.  The
    decode forms look the map up before the block: too few shards is ECX_E_NOT_ENOUGH_SHARDS even
    with a negative block, and with every shard present they return before any pass -- but not
    before the block and, in the _devices form, the device list are checked.  Nothing is written."""
    rs, base, before, masks, devs = batch
    b, d = base.ctypes.data, devs.ctypes.data
    one, few, every = (masks[k].ctypes.data for k in ("one", "few", "all"))
    has_device = _has_device(ecx)
    for name, form, decodes, f in _exports(ecx):
        for blk in BLOCKS:
            where = (name, blk)
            assert f(rs._h, one, b, -1, L, blk, d, 1) == ILL, where
            assert f(rs._h, one, b, S, -1, blk, d, 1) == ILL, where
            assert f(rs._h, one, None, S, L, blk, d, 1) == NUL, where
            if form == DEVICE:
                assert f(rs._h, one, None, 0, L, blk) == NUL, where
            elif form == HOST:  # an empty batch: no pass, no device needed
                assert f(rs._h, one, None, 0, L, blk) == OK, where
            else:  # the list is looked at even for an empty batch
                assert f(rs._h, one, None, 0, L, blk, d, 1) == (OK if has_device else DEV), where
            if form != DEVICE:
                assert f(None, one, b, S, L, blk, d, 1) == NUL, where
            if form == DEVICES:
                assert f(rs._h, one, b, S, L, blk, None, 1) == NUL, where
                assert f(rs._h, one, b, S, L, blk, d, 0) == ILL, where
                assert f(rs._h, one, b, S, L, blk, d, -1) == ILL, where
                assert f(rs._h, one, b, -1, L, blk, None, 1) == NUL, where   # the list before the counts
                assert f(rs._h, one, b, -1, L, blk, d, 0) == ILL, where
                assert f(None, one, b, S, L, blk, None, 1) == NUL, where
            if decodes:
                assert f(rs._h, few, b, S, L, blk, d, 1) == FEW, where
                assert f(rs._h, few, b, 0, L, blk, d, 1) == FEW, where
                assert f(rs._h, few, b, -1, L, blk, d, 1) == ILL, where       # the counts before the map
                assert f(rs._h, few, None, S, L, blk, d, 1) == NUL, where     # and the base
                for s in (0, S):  # all present: nothing to do, whatever the batch
                    want = OK if form != DEVICES or has_device else DEV
                    assert f(rs._h, every, b, s, L, blk, d, 1) == want, where + (s,)
        assert f(rs._h, one, b, S, L, -64, d, 1) == ILL, name
        if decodes:
            assert f(rs._h, few, b, S, L, -64, d, 1) == FEW, name     # the map lookup comes before the block
            assert f(rs._h, every, b, S, L, -64, d, 1) == ILL, name   # the block before the all-present return
    assert (base == before).all()


def test_no_gpu_blocked_apply_fails_loudly(ecx, batch):
    """Without a HIP device a valid call of any of the six exports returns ECX_E_DEVICE (no CPU
    fallback) and leaves the bytes alone."""
    if _has_device(ecx):
        pytest.skip("a device is present")
    rs, base, before, masks, devs = batch
    for name, form, decodes, f in _exports(ecx):
        for blk in BLOCKS:
            # (the device forms are handed host addresses: they must fail before they would launch anything)
            assert f(rs._h, masks["one"].ctypes.data, base.ctypes.data, S, L, blk, devs.ctypes.data, 2) == DEV, (name, blk)
    assert (base == before).all()
    with pytest.raises(ecx.EcxError) as e:
        rs.encodeParityBlockedBatchHost(base, S, L)
    assert e.value.code == DEV
    assert (base == before).all()
