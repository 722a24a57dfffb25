"""performCodingBatchMixedHost (ecx_clay_perform_coding_mixed_batch_host; host_pipe.cpp
run_host_map_mixed_batch): the Clay repair with a list per stripe from HOST memory, pageable and
pinned, with the pipeline cut into several chunks (host_chunk_kib 16) and at the default, bit-exact
against the oracle's performCoding (ClayCodeErasureDecodingStep.java:53-107) per stripe.

The zero rule: output slots 0 .. maxErased*alpha - 1 come back for every stripe, and the part a
stripe's own list does not write -- slots 8..15 of a single-node stripe of Clay(4,2), every slot of
a stripe whose id names no list or the empty list -- comes back 0x00 where the host buffer held
0x5A.  Host bytes outside the returned slots and past buf_size keep 0x5A."""
import numpy as np
import pytest

from clay_mixed_cases import GUARD, IDS42, LISTS42, SENTINEL, expected_output, layout, make_input
from test_mixed_host import chunk_kib

pytestmark = pytest.mark.gpu

K, M = 4, 2
# 18 output slots per stripe on the host: the set returns 16, slots 16 and 17 are the caller's own
OUT_SLOTS = 18
LAYOUTS = {
    "chunks_and_rest": layout(4096 + 48, 48, OUT_SLOTS, out_pitch=4096 + 64),
    "byte_safe_odd_strides": layout(1001, 48, OUT_SLOTS, in_pitch=1003, out_pitch=1005, in_extra=1, out_extra=3),
}


@pytest.fixture(autouse=True)
def _device():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


@pytest.mark.parametrize("kib", [16, None])
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_host_clay_mixed_matches_the_oracle_with_the_zero_rule(ecx, name, pinned, kib):
    lay, S = LAYOUTS[name], len(IDS42)
    flat_in = make_input(K, M, S, lay, 4600 + lay.B)
    want = expected_output(K, M, LISTS42, IDS42, lay, OUT_SLOTS, flat_in, unwritten=(0, 16))
    if pinned:
        hin, hout = ecx.HostBuffer(flat_in.size), ecx.HostBuffer(want.size)
        inp, out = hin.array, hout.array
    else:
        inp, out = np.empty(flat_in.size, np.uint8), np.empty(want.size, np.uint8)
    inp[:] = flat_in
    out[:] = SENTINEL
    ids = np.array(IDS42, np.uint8)
    with ecx.ClayPatternSet(LISTS42, K, M) as ps, chunk_kib(ecx, kib):
        ps.performCodingBatchMixedHost(inp, lay.in_stripe, lay.in_sub, out[GUARD:], lay.out_stripe, lay.out_sub, ids, S,
                                       lay.B)
    assert (inp == flat_in).all() and list(ids) == IDS42
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]} (stripe {(bad[0] - GUARD) // lay.out_stripe})"
    # the rule itself, spelled out on one stripe of each kind
    for s, erased in ((1, 1), (4, 0), (7, 0)):  # ids 0 (a single node), 255 (no list), 21 (the empty list)
        base = GUARD + s * lay.out_stripe
        for slot in range(OUT_SLOTS):
            sub = out[base + slot * lay.out_sub:base + slot * lay.out_sub + lay.B]
            if erased * 8 <= slot < 16:
                assert (sub == 0).all(), (s, slot)
            elif slot >= 16:
                assert (sub == SENTINEL).all(), (s, slot)


def test_host_clay_mixed_single_node_set_returns_eight_slots(ecx):
    """A set of single-node lists returns slots 0..7 only: slots 8 and up of the host buffer keep
    their bytes, and a stripe without a list gets eight slots of zeros."""
    lists, ids = [[i] for i in range(6)], [4, 1, 255, 0, 3, 5, 2, 1]
    lay, S = layout(4096 + 48, 48, 10, out_pitch=4096 + 64), len(ids)
    flat_in = make_input(K, M, S, lay, 4700)
    want = expected_output(K, M, lists, ids, lay, 10, flat_in, unwritten=(0, 8))
    out = np.full(want.size, SENTINEL, np.uint8)
    with ecx.ClayPatternSet(lists, K, M) as ps, chunk_kib(ecx, 16):
        ps.performCodingBatchMixedHost(flat_in.copy(), lay.in_stripe, lay.in_sub, out[GUARD:], lay.out_stripe,
                                       lay.out_sub, np.array(ids, np.uint8), S, lay.B)
    assert (out == want).all()
