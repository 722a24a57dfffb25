"""The blocked parity check's entry points where no GPU is needed: their status codes without a
device (no CPU fallback, as tests/test_abi.py::test_no_gpu_fails_loudly), the argument rules that
hold before any device work, and the generated JNI forwarders' argument rules over the fake JNIEnv
(as tests/test_jni_runtime.py)."""
import numpy as np
import pytest

from jni_harness import Jni

OK, ILL, IDX, NUL, DEV = 0, -1, -5, -6, -10
EXPORTS = ("ecx_rs_is_parity_correct_blocked_batch", "ecx_rs_is_parity_correct_blocked_batch_host",
           "ecx_rs_is_parity_correct_blocked_batch_host_devices")


def _has_device(ecx):
    try:
        return ecx.device_count() > 0
    except ecx.EcxError:
        return False


def _calls(ecx, rs, base, verdict, devs):
    """The three exports as f(rs, base, nstripes, byte_count, block, verdict) -> status."""
    lib = ecx.lib()
    return {
        EXPORTS[0]: lambda r, b, s, c, blk, v: lib.ecx_rs_is_parity_correct_blocked_batch(r, b, s, c, blk, v, None),
        EXPORTS[1]: lambda r, b, s, c, blk, v: lib.ecx_rs_is_parity_correct_blocked_batch_host(r, b, s, c, blk, v),
        EXPORTS[2]: lambda r, b, s, c, blk, v: lib.ecx_rs_is_parity_correct_blocked_batch_host_devices(
            r, b, s, c, blk, v, devs.ctypes.data, len(devs)),
    }


def test_blocked_check_argument_rules(ecx):
    """Before any device work, for each of the three exports: a null codec is ECX_E_NULL; a negative
    count or block is ECX_E_ILLEGAL_ARGUMENT; a null base or verdict with stripes to check is
    ECX_E_NULL; the _devices form refuses a null or empty list.  Nothing is written."""
    rs = ecx.ReedSolomon.create(4, 2)
    S, L = 3, 100
    base, verdict = np.zeros(S * 6 * L, np.uint8), np.full(S, 7, np.uint8)
    devs = np.zeros(2, np.int32)
    b, v = base.ctypes.data, verdict.ctypes.data
    for name, f in _calls(ecx, rs, base, verdict, devs).items():
        assert f(None, b, S, L, 0, v) == NUL, name
        assert f(rs._h, b, -1, L, 0, v) == ILL, name
        assert f(rs._h, b, S, -1, 0, v) == ILL, name
        assert f(rs._h, b, S, L, -64, v) == ILL, name
        assert f(rs._h, None, S, L, 0, v) == NUL, name
        assert f(rs._h, b, S, L, 0, None) == NUL, name
    lib = ecx.lib()
    g = lib.ecx_rs_is_parity_correct_blocked_batch_host_devices
    assert g(rs._h, b, S, L, 0, v, None, 1) == NUL
    assert g(rs._h, b, S, L, 0, v, devs.ctypes.data, 0) == ILL
    assert g(rs._h, b, S, L, 0, v, devs.ctypes.data, -1) == ILL
    assert (verdict == 7).all() and not base.any()
    # an empty batch touches nothing, null buffers included (the device form and the one-GPU host form
    # need no device for it)
    assert lib.ecx_rs_is_parity_correct_blocked_batch(rs._h, None, 0, L, 0, None, None) == OK
    assert lib.ecx_rs_is_parity_correct_blocked_batch_host(rs._h, None, 0, L, 0, None) == OK
    assert (verdict == 7).all()
    # the Python mirror checks both extents first: ECX_E_INDEX with or without a device
    for call in (lambda bb, vv: rs.isParityCorrectBlockedBatchHost(bb, S, L, vv),
                 lambda bb, vv: rs.isParityCorrectBlockedBatchHostDevices(bb, S, L, vv, [0])):
        for bb, vv in ((base[1:], verdict), (base, verdict[1:])):
            with pytest.raises(ecx.EcxError) as e:
                call(bb, vv)
            assert e.value.code == IDX
    assert (verdict == 7).all()


def test_no_gpu_blocked_check_fails_loudly(ecx):
    """Without a HIP device the three exports return ECX_E_DEVICE (no CPU fallback) and leave the
    verdicts alone."""
    if _has_device(ecx):
        pytest.skip("a device is present")
    rs = ecx.ReedSolomon.create(4, 2)
    S, L = 3, 100
    base, verdict = np.zeros(S * 6 * L, np.uint8), np.full(S, 7, np.uint8)
    devs = np.zeros(1, np.int32)
    for name, f in _calls(ecx, rs, base, verdict, devs).items():
        # (the device form is handed host addresses: it must fail before it would launch anything)
        assert f(rs._h, base.ctypes.data, S, L, 0, verdict.ctypes.data) == DEV, name
        assert f(rs._h, base.ctypes.data, S, L, 32, verdict.ctypes.data) == DEV, name
    assert (verdict == 7).all()
    with pytest.raises(ecx.EcxError) as e:
        rs.isParityCorrectBlockedBatchHost(base, S, L, verdict)
    assert e.value.code == DEV
    # the device list is looked at even for an empty batch: no device, no list to check it against
    assert ecx.lib().ecx_rs_is_parity_correct_blocked_batch_host_devices(
        rs._h, None, 0, L, 0, None, devs.ctypes.data, 1) == DEV


# ---------------------------------------------------------------- JNI forwarders (fake JNIEnv)
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


def test_blocked_check_forwarders_argument_rules(J, ecx):
    """rsIsParityCorrectBlockedBatch / ...Host / ...HostDevices: one forwarder per export; a null
    rs is the NullPointerException status; the device list is a copied int[] whose length must
    cover ndev -- a short array or a negative ndev is the IllegalArgumentException status, a null
    one the NullPointerException status -- and nothing is pinned.  With a device the host forms
    report the oracle-checked verdicts of a small blocked batch; without one, ECX_E_DEVICE."""
    for n in ("rsIsParityCorrectBlockedBatch", "rsIsParityCorrectBlockedBatchHost",
              "rsIsParityCorrectBlockedBatchHostDevices"):
        assert n in J.sigs, n
    k, m, S, L, blk = 4, 2, 3, 1000, 256
    n = k + m
    h = np.zeros(1, np.int64)
    assert J.call("rsCreate", k, m, J.array(h)) == OK and h[0] != 0
    rs = int(h[0])
    try:
        import oracle as O
        import torch
        nat = np.zeros((S, n, L), np.uint8)
        nat[:, :k] = np.random.default_rng(62).integers(0, 256, (S, k, L), dtype=np.uint8)
        for s in range(S):
            O.ReedSolomon(k, m).encode_parity([nat[s, i] for i in range(n)], 0, L)
        buf = ecx.blocked_pack(torch.from_numpy(nat), blk).numpy()
        buf[-1] ^= 0x40  # the last byte of the batch: stripe S - 1's tail
        before = buf.copy()
        verdict = np.full(S + 8, 7, np.uint8)
        b, v = buf.ctypes.data, verdict.ctypes.data
        J.reset()
        assert J.call("rsIsParityCorrectBlockedBatch", 0, b, S, L, blk, v, 0) == NUL
        assert J.call("rsIsParityCorrectBlockedBatchHost", 0, b, S, L, blk, v) == NUL
        assert J.call("rsIsParityCorrectBlockedBatchHostDevices", 0, b, S, L, blk, v, J.ints([0]), 1) == NUL
        dev = lambda devs, nd, **kw: J.call("rsIsParityCorrectBlockedBatchHostDevices", rs, b, kw.get("S", S),  # noqa: E731
                                            kw.get("L", L), kw.get("blk", blk), v, devs, nd)
        assert dev(J.ints([0]), 2) == ILL          # the array is shorter than ndev
        assert dev(J.ints([]), 1) == ILL
        assert dev(J.ints([0]), -1) == ILL
        assert dev(None, 1) == NUL
        assert dev(J.ints([0]), 0) == ILL          # an empty list (the export's own rule)
        assert dev(J.ints([0]), 1, S=-1) == ILL and dev(J.ints([0]), 1, L=-1) == ILL
        assert dev(J.ints([0]), 1, blk=-1) == ILL
        host = lambda **kw: J.call("rsIsParityCorrectBlockedBatchHost", rs, b, kw.get("S", S), kw.get("L", L),  # noqa: E731
                                   kw.get("blk", blk), v)
        assert host(S=-1) == ILL and host(L=-1) == ILL and host(blk=-1) == ILL
        assert J.call("rsIsParityCorrectBlockedBatchHost", rs, 0, S, L, blk, v) == NUL
        assert J.call("rsIsParityCorrectBlockedBatchHost", rs, b, S, L, blk, 0) == NUL
        assert J.counters()["pins"] == 0 and (verdict == 7).all() and (buf == before).all()
        assert host(S=0) == OK and (verdict == 7).all()
        st = host()
        assert st == (OK if _has_device(ecx) else DEV), st
        if st == OK:
            assert verdict.tolist() == [1] * (S - 1) + [0] + [7] * 8
            verdict[:] = 7
            assert dev(J.ints([0, 0]), 2) == OK
            assert verdict.tolist() == [1] * (S - 1) + [0] + [7] * 8
        assert (buf == before).all()
    finally:
        J.call("rsDestroy", rs)
