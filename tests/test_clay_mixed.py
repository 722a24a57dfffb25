"""performCodingBatchMixed on the GPU (k_gf_map_mixed, csrc/apply_map_mixed.hip): a batch of Clay
stripes that lost different nodes, repaired out of place in one call, bit-exact against the oracle's
performCoding (ClayCodeErasureDecodingStep.java:53-107) run per stripe with that stripe's own list.

tests/clay_mixed_cases.py has the lists, the ids and the expected output buffer.  The output buffer
is prefilled with 0x5A and compared whole, so the slots a stripe's list does not write (slots 8..15
of a single-node stripe of Clay(4,2), every slot of a stripe whose id names no list or the empty
list), the gaps between slots and the guard bytes are checked to keep the sentinel."""
import numpy as np
import pytest

from clay_mixed_cases import GUARD, IDS42, LISTS42, SENTINEL, alpha_of, expected_output, layout, make_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# what a set whose tiles all have 20 entries runs at its own choice: depth 8, as every tile has at
# least 12 entries (a depth-20 instance did not beat it: DESIGN.md 4.7.3)
OWN_CHOICE_20 = "k_gf_map_mixed<false, 8, 8>"


class depth_knob:
    """ecx_tune depth for the length of a with block (0 = each set's own choice)."""

    def __init__(self, ecx, depth):
        self.ecx, self.depth = ecx, depth

    def __enter__(self):
        self.ecx.tune("depth", self.depth)

    def __exit__(self, *exc):
        self.ecx.tune("depth", 0)


def run_mixed(ecx, torch, k, m, lists, ids, lay, out_slots, flat_in):
    """The mixed call over the case's input -> (whole output buffer on the host, kernel of record)."""
    S = len(ids)
    inp = torch.from_numpy(flat_in.copy()).cuda()
    out = torch.full((2 * GUARD + (S - 1) * lay.out_stripe + (out_slots - 1) * lay.out_sub + lay.B,), SENTINEL,
                     dtype=torch.uint8, device="cuda")
    dev_ids = torch.tensor(ids, dtype=torch.uint8, device="cuda")
    with ecx.ClayPatternSet(lists, k, m) as ps:
        ps.performCodingBatchMixed(inp, lay.in_stripe, lay.in_sub, out[GUARD:], lay.out_stripe, lay.out_sub, dev_ids, S,
                                   lay.B)
        torch.cuda.synchronize()
        kernel = ecx.last_kernel()
    assert (inp.cpu().numpy() == flat_in).all(), "the input changed"
    return out.cpu().numpy(), kernel


# Clay(4,2): 48 input slots, 16 output slots.  One chunk; full chunks and a rest; byte-safe on odd
# strides; an input pitch larger than buf_size
SIZES42 = {
    "one_chunk": layout(4096, 48, 16, out_pitch=4096 + 64),
    "chunks_and_rest": layout(2 * 4096 + 48, 48, 16, out_pitch=2 * 4096 + 48 + 16),
    "byte_safe_odd_strides": layout(1001, 48, 16, in_pitch=1003, out_pitch=1005, in_extra=1, out_extra=3),
    "wide_input_pitch": layout(4096, 48, 16, in_pitch=2 * 4096, out_pitch=4096 + 64),
}


@pytest.mark.parametrize("size", list(SIZES42))
def test_clay42_all_lists_match_the_oracle_and_the_uniform_calls(ecx, torch_dev, size):
    """All 21 one- and two-node lists plus the empty list: two tiles per pattern (16 rows), records
    without a tile for the single-node lists, out of place.  Wrong multi-tile records or wrong
    out-of-place addressing fail here."""
    torch = torch_dev
    k, m, lay = 4, 2, SIZES42[size]
    flat_in = make_input(k, m, len(IDS42), lay, 4200 + lay.B)
    want = expected_output(k, m, LISTS42, IDS42, lay, 16, flat_in)
    got, kernel = run_mixed(ecx, torch, k, m, LISTS42, IDS42, lay, 16, flat_in)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]} (stripe {(bad[0] - GUARD) // lay.out_stripe})"
    if size != "byte_safe_odd_strides":  # byte-safe launches are not noted
        # every tile of every list has exactly 20 entries (a pair: 40 over two tiles): the set's
        # own depth is the uniform set's
        assert kernel == OWN_CHOICE_20, kernel
    # the same bytes as one uniform performCodingBatch per stripe -- all a caller could do before
    inp = torch.from_numpy(flat_in.copy()).cuda()
    out = torch.full((want.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    for s, pid in enumerate(IDS42):
        if pid < len(LISTS42) and LISTS42[pid]:
            ecx.ClayCodeErasureDecodingStep(LISTS42[pid], k, m).performCodingBatch(
                inp[s * lay.in_stripe:], lay.in_stripe, lay.in_sub, out[GUARD + s * lay.out_stripe:], lay.out_stripe,
                lay.out_sub, 1, lay.B)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == got).all()


def test_clay42_single_nodes_at_every_depth(ecx, torch_dev):
    """Single nodes only: one tile per pattern and every record has exactly 20 entries.  The forced
    depths 4 and 8 (20 padded to 24) and the set's own choice give identical bytes, the oracle's."""
    torch = torch_dev
    k, m = 4, 2
    lists = [[i] for i in range(6)]
    ids = [4, 1, 5, 0, 255, 3, 2, 1, 4]
    lay = layout(4096 + 48, 48, 8, out_pitch=4096 + 64)
    flat_in = make_input(k, m, len(ids), lay, 4301)
    want = expected_output(k, m, lists, ids, lay, 8, flat_in)
    kernels = {}
    for depth in (4, 8, 0):
        with depth_knob(ecx, depth):
            got, kernels[depth] = run_mixed(ecx, torch, k, m, lists, ids, lay, 8, flat_in)
        assert (got == want).all(), depth
    assert kernels[4] == "k_gf_map_mixed<false, 4, 8>" and kernels[8] == "k_gf_map_mixed<false, 8, 8>", kernels
    assert kernels[0] == OWN_CHOICE_20, kernels


# (k, m, lists, ids, kernel of record): B = 4096 + 48 and at most 9 stripes
SMALL = {
    # alpha 4: 4 rows, the ROWS 4 instance; 6 entries per list: depth 4
    "clay22_single_nodes": (2, 2, [[0], [1], [2], [3]], [2, 0, 255, 3, 1, 0, 2], "k_gf_map_mixed<false, 4, 4>"),
    # alpha 9: 9 rows, a second tile of one row
    "clay33_single_nodes": (3, 3, [[0], [1], [2], [3], [4], [5]], [3, 0, 5, 255, 1, 4, 2, 0],
                            "k_gf_map_mixed<false, 4, 8>"),
    # alpha 16: 2 tiles for a single node, 4 for a pair, and the empty list: ragged tile counts
    "clay62_nodes_and_pairs": (6, 2, [[0], [3], [7], [0, 1], [2, 7], []], [3, 0, 4, 255, 1, 5, 2, 4, 0],
                               "k_gf_map_mixed<false, 8, 8>"),
}


@pytest.mark.parametrize("case", list(SMALL))
def test_other_geometries_match_the_oracle(ecx, torch_dev, case):
    k, m, lists, ids, kernel_want = SMALL[case]
    a = alpha_of(k, m)
    n_in, out_slots = (k + m) * a, max(len(e) for e in lists) * a
    B = 4096 + 48
    lay = layout(B, n_in, out_slots, out_pitch=B + 16)
    flat_in = make_input(k, m, len(ids), lay, 4400 + k)
    want = expected_output(k, m, lists, ids, lay, out_slots, flat_in)
    with ecx.ClayPatternSet(lists, k, m) as ps:
        assert ps.info() == (len(lists), k + m, a, max(len(e) for e in lists))
    got, kernel = run_mixed(ecx, torch_dev, k, m, lists, ids, lay, out_slots, flat_in)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}"
    assert kernel == kernel_want, kernel
