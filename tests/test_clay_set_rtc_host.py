"""performCodingBatchMixedHost of a generated set (ecx_clay_perform_coding_mixed_batch_host over
k_clay_repair_set; host_pipe.cpp run_host_map_mixed_batch): Clay(10,4) stripes that lost different
nodes repaired from HOST memory, pageable and pinned, against the device form of the same batch.

The zero rule: output slots 0..255 come back for every stripe; a stripe whose id names no list or
the empty list gets zeros there where the host buffer held 0x5A.  Host bytes outside the returned
slots -- the caller's slots 256 and 257, the gaps of the padded pitch, the guards -- keep 0x5A."""
import numpy as np
import pytest

import clay_set_rtc_cases as T
from clay_rtc_sweep_cases import GUARD, SENTINEL

pytestmark = pytest.mark.gpu

K, M, V, A = 10, 4, 2, 256
OUT_SLOTS = A + 2


@pytest.fixture(scope="module")
def case(ecx):
    """The set, the batch's host input and the device form's output (stripe x alpha x B)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with ecx.ClayPatternSet([list(x) for x in T.LISTS104], K, M, V) as ps:
        lay = T.layout(K, M, V)
        got, kern = T.run_mixed(ecx, torch, ps, K, M, V, T.IDS104, lay, 8600)
        assert kern == "k_clay_repair_set"
        dev_form = got[GUARD:len(got) - GUARD].reshape(T.S, A, T.B)
        flat_in = T.device_input(ecx, torch, K, M, V, lay, 8600).cpu().numpy()[GUARD:]
        flat_in.setflags(write=False)
        yield ps, lay, flat_in, dev_form


@pytest.mark.parametrize("pinned", [False, True])
def test_host_form_matches_the_device_form_with_the_zero_rule(ecx, case, pinned):
    ps, lay, flat_in, dev_form = case
    hlay = T.layout(K, M, V, out_pad=64, out_slots=OUT_SLOTS)
    size = GUARD + T.out_bytes(hlay) + GUARD
    if pinned:
        hin, hout = ecx.HostBuffer(flat_in.size), ecx.HostBuffer(size)
        inp, out = hin.array, hout.array
    else:
        inp, out = np.empty(flat_in.size, np.uint8), np.empty(size, np.uint8)
    inp[:] = flat_in
    out[:] = SENTINEL
    ids = np.array(T.IDS104, np.uint8)
    ps.performCodingBatchMixedHost(inp, lay.in_stripe, lay.in_sub, out[GUARD:len(out) - GUARD], hlay.out_stripe,
                                   hlay.out_sub, ids, T.S, T.B)
    assert (inp == flat_in).all() and tuple(ids) == T.IDS104
    want = np.full(size, SENTINEL, np.uint8)
    for s, pid in enumerate(T.IDS104):
        repaired = pid < len(T.LISTS104) and T.LISTS104[pid]
        for z in range(A):
            at = GUARD + s * hlay.out_stripe + z * hlay.out_sub
            want[at:at + T.B] = dev_form[s, z] if repaired else 0
    T.assert_same(np.asarray(out), want, hlay, ("host", pinned))
    # the rule itself, spelled out: id 255 (stripe 3) and the empty list (stripe 6)
    for s in (3, 6):
        base = GUARD + s * hlay.out_stripe
        for z in range(OUT_SLOTS):
            sub = out[base + z * hlay.out_sub:base + z * hlay.out_sub + T.B]
            assert (sub == (0 if z < A else SENTINEL)).all(), (s, z)
