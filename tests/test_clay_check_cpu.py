"""The Clay codeword check without a device: the pools of tests/clay_check_cases.py are what they
promise (the oracle agrees with the expected verdicts stripe by stripe), a numpy model of the check
program -- decouple with (3, 2), fold into the plane code's m syndromes -- gives the same verdicts,
and ecx_clay_is_parity_correct_batch keeps the argument rules that are decided before the device is
touched (include/ecx.h)."""
import ctypes

import numpy as np
import pytest

import clay_check_cases as C
import oracle as O

ILL, NUL = -1, -6

# (name, builder): the cases of tests/test_clay_check.py small enough to re-encode on the CPU, and
# the covering-plane set of the shortened Clay(10,4) at 16 bytes instead of all its 3,584 sites
CASES = {
    "clay42_vector": lambda: C.subchunk_case(4, 2, 0, 4096),
    "clay42_safe": lambda: C.subchunk_case(4, 2, 0, 48),
    "clay63": lambda: C.subchunk_case(6, 3, 0, 4096),
    "clay104_cover_16": lambda: C.subchunk_case(10, 4, 2, 16, 16, True),
    "clay42_body_tail": lambda: C.byte_case(4, 2, 0, 4096 + 16, 4096 + 16),
    "clay42_ragged_tail": lambda: C.byte_case(4, 2, 0, 8192 + 5, 8192 + 5),
    "clay42_padded": lambda: C.byte_case(4, 2, 0, 1000, 1024),
    "clay42_odd_pitch": lambda: C.byte_case(4, 2, 0, 1001, 1011),
    "clay33_vector": lambda: C.subchunk_case(3, 3, 0, 4096),
    "clay33_ragged_tail": lambda: C.byte_case(3, 3, 0, 8192 + 5, 8192 + 16),
    "clay33_odd_pitch": lambda: C.byte_case(3, 3, 0, 1001, 1011),
    "clay124": C.clay124_case,
}


def model_verdicts(case, pair=(3, 2), z_partner=True):
    """The check program on the host pool: for every plane z, U(z, j) = C(z, j) for a dot node, else
    pair[0] * C(z, j) ^ pair[1] * C(z', j') (a virtual node's C is zero), and the syndromes
    S(z, p) = sum_j P[p][j] U(z, j) ^ U(z, k + v + p); a stripe passes when all are zero."""
    k, m, v, B = case.k, case.m, case.v, case.B
    q, t, alpha, nr = C.geometry(k, m, v)
    mt = O.mul_table()
    P = O.ReedSolomon(k + v, m).parity_rows
    pool = case.host_pool()[:, :, :B]
    S = pool.shape[0]
    zero = np.zeros((S, B), np.uint8)

    def sub(z, u):
        r = C.real_of(u, k, v)
        return zero if r is None else pool[:, z * nr + r]

    bad = np.zeros(S, bool)
    for z in range(alpha):
        dig = C.zvec(z, q, t)
        U = []
        for u in range(k + v + m):
            x, y = u % q, u // q
            if dig[y] == x:
                U.append(sub(z, u))
            else:
                zz = z + (x - dig[y]) * q ** (t - 1 - y) if z_partner else z
                U.append(mt[pair[0]][sub(z, u)] ^ mt[pair[1]][sub(zz, dig[y] + q * y)])
        for p in range(m):
            syn = U[k + v + p].copy()
            for j in range(k + v):
                syn ^= mt[P[p][j]][U[j]]
            bad |= syn.any(axis=1)
    return (~bad).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_verdicts_are_the_oracles(name):
    """Stripe by stripe, re-encoding the data nodes with the oracle and comparing with the stored
    parity gives the verdict the builder expects; every case has failing and passing stripes."""
    case = CASES[name]()
    got = C.oracle_verdicts(case)
    assert got.tolist() == case.want.tolist()
    assert 0 < int(case.want.sum()) < case.nstripes


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "clay124"))
def test_model_of_the_program_gives_the_same_verdicts(name):
    case = CASES[name]()
    assert model_verdicts(case).tolist() == case.want.tolist()


def test_model_with_the_pair_swapped_or_the_own_plane_fails_clean_stripes():
    """What the planner's proof and the GPU mutants rest on: with (2, 3), or with the partner read
    from plane z instead of z', clean stripes no longer pass."""
    case = C.subchunk_case(4, 2, 0, 48)
    clean = case.want == 1
    assert not model_verdicts(case, pair=(2, 3))[clean].any()
    assert not model_verdicts(case, z_partner=False)[clean].any()


def test_covering_planes_and_unit_rounds():
    """The plane set of the Clay(10,4) vector case holds planes 0 and 255 and, for every digit
    position and value, a plane with that digit; the unit rounds probe every (stripe, chunk, plane)
    once, each time in a dot node, which no other plane's workgroup reads."""
    planes = C.covering_planes(4, 4)
    assert 0 in planes and 255 in planes and len(planes) <= 20
    assert all(any(C.zvec(z, 4, 4)[y] == x for z in planes) for y in range(4) for x in range(4))
    _, _, alpha, nr = C.geometry(10, 4, 2)
    virtual_partner = [(z, n) for z in planes for n in range(nr)
                       if not C.is_dot(10, 4, 2, z, n) and C.partner(10, 4, 2, z, n)[1] is None]
    assert virtual_partner, "the case holds sites whose partner is virtual"
    for S in (9, 17, 65):
        rounds = C.unit_rounds(2, 2, 0, 2 * C.CHUNK, S)
        assert len(rounds) == 2 * 4 + 1
        for sites in rounds:
            assert len({s for s, *_ in sites}) == len(sites)
            assert all(C.is_dot(2, 2, 0, z, node) for _, z, node, _, _ in sites)
    # a dot node is nobody's partner
    for z in range(8):
        for n in range(6):
            if not C.is_dot(4, 2, 0, z, n):
                zz, nn = C.partner(4, 2, 0, z, n)
                assert not C.is_dot(4, 2, 0, zz, nn)


# ---------------------------------------------------------------- the ABI's argument rules
def _call(ecx, k, m, v, base, ss, sub, S, B, verdict):
    return ecx.lib().ecx_clay_is_parity_correct_batch(k, m, v, base, ss, sub, S, B, verdict, None)


def test_abi_argument_rules_without_a_device(ecx):
    """In the header's order: negative counts, nstripes == 0 (nothing touched, not even null
    pointers), null pointers, negative strides and extents beyond int64_t, then the geometry."""
    A = 1 << 20  # a non-null address no rule below dereferences
    big = (1 << 62)
    for args in ((-1, 2, 0, A, 48, 1, 1, 1, A), (4, 0, 0, A, 48, 1, 1, 1, A), (4, 2, -1, A, 48, 1, 1, 1, A),
                 (4, 2, 0, A, 48, 1, -1, 1, A), (4, 2, 0, A, 48, 1, 1, -1, A)):
        assert _call(ecx, *args) == ILL, args
    assert _call(ecx, 4, 2, 0, None, -5, -5, 0, 16, None) == 0          # nstripes == 0: ECX_OK, nothing touched
    assert _call(ecx, 9, 9, 0, None, 0, 0, 0, 16, None) == 0
    assert _call(ecx, 4, 2, 0, None, 48 * 16, 16, 1, 16, A) == NUL
    assert _call(ecx, 4, 2, 0, A, 48 * 16, 16, 1, 16, None) == NUL
    assert _call(ecx, 4, 2, 0, A, -48 * 16, 16, 1, 16, A) == ILL
    assert _call(ecx, 4, 2, 0, A, 48 * 16, -16, 1, 16, A) == ILL
    assert _call(ecx, 4, 2, 0, A, big, 16, 4, 16, A) == ILL             # (nstripes - 1) * stride overflows
    assert b"int64_t" in ecx.lib().ecx_last_error()
    assert _call(ecx, 4, 2, 0, A, 48 * 16, big, 1, 16, A) == ILL
    # geometries: more parity units than accumulator rows; nodes that do not fill the grid; a
    # sub-packetization the planner refuses at create
    for k, m, v, word in ((9, 9, 0, b"parity_units"), (5, 2, 0, b"grid"), (40, 2, 0, b"")):
        assert _call(ecx, k, m, v, A, 1 << 30, 16, 1, 16, A) == ILL, (k, m, v)
        assert word in ecx.lib().ecx_last_error()


def test_binding_row_wrapper_and_version(ecx):
    from importlib import import_module
    rows = import_module(ecx.__name__ + "._lib").SIGNATURES
    I, P, I64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert rows["ecx_clay_is_parity_correct_batch"] == (I, [I, I, I, P, I64, I64, I64, I64, P, P])
    assert ecx.lib().ecx_version() >= 110
    assert ecx.ClayParityCheck(4, 2).geometry() == (2, 3, 8, 6)
    assert ecx.ClayParityCheck(10, 4, 2).geometry() == (4, 4, 256, 14)
    assert ecx.ClayParityCheck(6, 3).geometry() == (3, 3, 27, 9)
    with pytest.raises(ecx.EcxError) as e:  # the wrapper refuses a layout beyond the buffer before the call
        chk = ecx.ClayParityCheck(4, 2)
        chk.isParityCorrectBatch(np.zeros(10, np.uint8), 48 * 16, 16, 1, 16, np.zeros(1, np.uint8))
    assert e.value.code == -5


def test_wrapper_holds_the_codec_until_close(ecx):
    """The proved program and its device records live with the geometry's shared codec: the Python
    object keeps a reference on it from construction to close() (idempotent), as a captured graph
    needs, and a closed object refuses the call."""
    lib = ecx.lib()
    lib.ecx_codec_stats.argtypes = [ctypes.POINTER(ctypes.c_int)] * 4
    lib.ecx_codec_stats.restype = ctypes.c_int

    def clay_live():
        v = [ctypes.c_int() for _ in range(4)]
        assert lib.ecx_codec_stats(*[ctypes.byref(x) for x in v]) == 0
        return v[2].value

    before = clay_live()
    chk = ecx.ClayParityCheck(7, 7)  # a geometry nothing else here holds
    assert clay_live() == before + 1
    again = ecx.ClayParityCheck(7, 7)  # the same shared codec
    assert clay_live() == before + 1
    again.close()
    assert clay_live() == before + 1
    chk.close()
    chk.close()
    assert clay_live() == before
    with pytest.raises(ecx.EcxError):
        chk.isParityCorrectBatch(1 << 20, 0, 0, 1, 0, 1 << 20)
