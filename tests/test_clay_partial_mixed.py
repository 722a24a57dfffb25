"""ClayPatternSet.partialBatchMixed on the GPU (k_gf_map_partial_mixed,
csrc/apply_clay_partial_mixed.hip): one hop of the pipelined Clay repair chain
(ClayCoordinator.kt:265-319, ClayCodeNode.kt:165-233) in which both the erased-node list and the
node this helper holds differ from stripe to stripe.

Placement is rotated: helper j holds node (j + s) mod n of stripe s.  The inputs are random bytes,
not codewords, and the erased nodes' slots hold garbage (tests/clay_mixed_cases.py, reused
unchanged).  (i) The hops of all n helpers in chain order, the first assigning, into an accumulator
prefilled with a sentinel, must give the oracle's performCoding per stripe
(ClayCodeErasureDecodingStep.java:53-107) and keep the sentinel everywhere else: the buffer is
compared whole.  (ii) Each helper's hop alone, assigning and accumulating over a random
accumulator, must be bit-identical, stripe by stripe, to the uniform GfMap call with the columns of
that helper's node of the list's map -- the zero map for a node the list erased.  (iii) Node bytes
that are no node and ids without a list leave their stripes untouched in both modes."""
import functools
from collections import namedtuple

import numpy as np
import pytest

from clay_mixed_cases import GUARD, IDS42, LISTS42, SENTINEL, alpha_of, expected_output, layout, make_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# A hop's layouts: buf_size, the helper-local plane pitch and stripe pad, the accumulator's row
# pitch and stripe pad; `full` addresses the node inside the full plane-major stripe instead
Shape = namedtuple("Shape", "B in_pitch in_extra acc_pitch acc_extra full")

SHAPES42 = {
    "one_chunk": Shape(4096, 4096, 0, 4096 + 64, 0, False),
    "chunks_and_rest_aligned16": Shape(2 * 4096 + 100, 2 * 4096 + 112, 16, 2 * 4096 + 128, 32, False),
    "byte_safe_odd_strides": Shape(1001, 1003, 1, 1005, 3, False),
    "full_stripe_addressing": Shape(4096, 4096, 0, 4096 + 64, 0, True),
}


def node_of(j, s, n):
    return (j + s) % n


class Case:
    """One geometry, its lists and ids, one shape: the full plane-major input (host), the
    expected accumulator after the whole chain, and each helper's device input and strides."""

    def __init__(self, torch, k, m, lists, ids, shape, seed):
        self.k, self.m, self.n, self.a = k, m, k + m, alpha_of(k, m)
        self.lists, self.ids, self.S, self.shape = lists, ids, len(ids), shape
        self.rows = max(len(e) for e in lists) * self.a
        B = shape.B
        # the full stripes (plane-major, slot z*n + node) with the shape's plane pitch
        self.lay = layout(B, self.n * self.a, self.rows, in_pitch=shape.in_pitch, out_pitch=shape.acc_pitch,
                          in_extra=shape.in_extra, out_extra=shape.acc_extra)
        self.flat_in = make_input(k, m, self.S, self.lay, seed)
        self.want_chain = expected_output(k, m, lists, ids, self.lay, self.rows, self.flat_in)
        self.acc_size = self.want_chain.size
        self.dev_ids = torch.tensor(ids, dtype=torch.uint8, device="cuda")
        self.full_dev = torch.from_numpy(self.flat_in.copy()).cuda()

    def helper(self, torch, j):
        """(device input, in_stripe_stride, in_node_stride, in_sub_stride, device node bytes)."""
        nodes = np.array([node_of(j, s, self.n) for s in range(self.S)], np.uint8)
        dev_nodes = torch.from_numpy(nodes).cuda()
        sh, lay = self.shape, self.lay
        if sh.full:
            return self.full_dev, lay.in_stripe, lay.in_sub, self.n * lay.in_sub, dev_nodes
        stripe = self.a * sh.in_pitch + sh.in_extra
        loc = np.full((self.S - 1) * stripe + (self.a - 1) * sh.in_pitch + sh.B, 0xEE, np.uint8)
        for s in range(self.S):
            for z in range(self.a):
                src = s * lay.in_stripe + (z * self.n + int(nodes[s])) * lay.in_sub
                loc[s * stripe + z * sh.in_pitch:s * stripe + z * sh.in_pitch + sh.B] = self.flat_in[src:src + sh.B]
        return torch.from_numpy(loc).cuda(), stripe, 0, sh.in_pitch, dev_nodes

    def hop(self, ps, torch, j, acc, is_first, nodes=None, ids=None):
        inp, iss, ins, isub, dev_nodes = self.helper(torch, j)
        ps.partialBatchMixed(self.dev_ids if ids is None else ids, dev_nodes if nodes is None else nodes, inp, iss, ins,
                             isub, acc[GUARD:], self.lay.out_stripe, self.lay.out_sub, self.S, self.shape.B, is_first)


@functools.lru_cache(maxsize=None)
def _list_matrix(k, m, erased):
    import rpamd
    ecx = rpamd.load(shape_knobs=True)
    return ecx.ClayCodeErasureDecodingStep(list(erased), k, m).map().matrix()


@functools.lru_cache(maxsize=None)
def _node_map(k, m, erased, node):
    """The uniform map of the columns of `node` of the list's repair map: input slot = plane.
    None for a node the list does not read (the zero map)."""
    import rpamd
    ecx = rpamd.load(shape_knobs=True)
    n = k + m
    mat, ins, outs = _list_matrix(k, m, erased)
    cols = [j for j, slot in enumerate(ins) if int(slot) % n == node and np.asarray(mat)[:, j].any()]
    if not cols:
        return None
    return ecx.GfMap.from_matrix(np.ascontiguousarray(np.asarray(mat)[:, cols]), in_slot=[int(ins[j]) // n for j in cols],
                                 out_slot=[int(o) for o in outs])


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_maps():
    """The cached uniform maps are freed with the module, while the library is still loaded."""
    yield
    _node_map.cache_clear()
    _list_matrix.cache_clear()


def check_chain(ecx, torch, case):
    """(i): all helpers in chain order, the first assigning."""
    with ecx.ClayPatternSet(case.lists, case.k, case.m) as ps:
        acc = torch.full((case.acc_size,), SENTINEL, dtype=torch.uint8, device="cuda")
        for j in range(case.n):
            case.hop(ps, torch, j, acc, j == 0)
        torch.cuda.synchronize()
        shape = ecx.last_launch_shape()
    got = acc.cpu().numpy()
    bad = np.flatnonzero(got != case.want_chain)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]} (stripe {(bad[0] - GUARD) // case.lay.out_stripe})"
    assert (case.full_dev.cpu().numpy() == case.flat_in).all(), "the input changed"
    return shape


def check_each_helper_against_uniform_calls(ecx, torch, case):
    """(ii): every helper alone, both modes, over a random accumulator."""
    rng = np.random.default_rng(case.shape.B)
    start = rng.integers(0, 256, case.acc_size, dtype=np.uint8)
    lay, B = case.lay, case.shape.B
    with ecx.ClayPatternSet(case.lists, case.k, case.m) as ps:
        for j in range(case.n):
            inp, iss, ins, isub, _ = case.helper(torch, j)
            for first in (True, False):
                got = torch.from_numpy(start.copy()).cuda()
                case.hop(ps, torch, j, got, first)
                ref = torch.from_numpy(start.copy()).cuda()
                for s, pid in enumerate(case.ids):
                    erased = case.lists[pid] if pid < len(case.lists) else []
                    if not erased:
                        continue
                    node = node_of(j, s, case.n)
                    gm = _node_map(case.k, case.m, tuple(erased), node)
                    dst = ref[GUARD + s * lay.out_stripe:]
                    if gm is None:  # the zero map: zeros when assigning, nothing when accumulating
                        if first:
                            for r in range(len(erased) * case.a):
                                dst[r * lay.out_sub:r * lay.out_sub + B] = 0
                        continue
                    src = inp[s * iss + node * ins:]
                    (gm.apply_batch if first else gm.accumulate_batch)(src, iss, isub, dst, lay.out_stripe, lay.out_sub, 1, B)
                torch.cuda.synchronize()
                g, r = got.cpu().numpy(), ref.cpu().numpy()
                bad = np.flatnonzero(g != r)
                assert bad.size == 0, (f"helper {j} first={first}: {bad.size} bytes differ, first at {bad[0]} "
                                       f"(stripe {(bad[0] - GUARD) // lay.out_stripe})")


@pytest.mark.parametrize("shape", list(SHAPES42))
def test_clay42_chain_of_six_helpers_matches_the_oracle(ecx, torch_dev, shape):
    case = Case(torch_dev, 4, 2, LISTS42, IDS42, SHAPES42[shape], 5200 + SHAPES42[shape].B)
    launch = check_chain(ecx, torch_dev, case)
    if shape != "byte_safe_odd_strides":
        # pairs read 8 planes of a node, single nodes 4: the plan's own depth is 4; 16 rows in two tiles of 8
        assert launch.startswith("k_gf_map_partial_mixed<false, 4, 8>"), launch


@pytest.mark.parametrize("shape", list(SHAPES42))
def test_clay42_each_helper_equals_the_uniform_calls(ecx, torch_dev, shape):
    case = Case(torch_dev, 4, 2, LISTS42, IDS42, SHAPES42[shape], 5200 + SHAPES42[shape].B)
    check_each_helper_against_uniform_calls(ecx, torch_dev, case)


# (k, m, lists, ids, kernel of record): B = 4096 + 16 and at most 9 stripes
SMALL = {
    # alpha 4: single nodes only, 4 rows: the ROWS 4 instance
    "clay22_single_nodes": (2, 2, [[0], [1], [2], [3]], [2, 0, 255, 3, 1, 0, 2], "k_gf_map_partial_mixed<false, 4, 4>"),
    # alpha 9: 9 rows, a second tile of one row; pairs: 18 rows in three tiles
    "clay33_nodes_and_pairs": (3, 3, [[0], [1], [2], [3], [4], [5], [1, 4]], [3, 0, 5, 255, 6, 1, 4, 2, 6],
                               "k_gf_map_partial_mixed<false, 4, 8>"),
    # alpha 16: 2 tiles for a single node, 4 for a pair, and the empty list: ragged tile counts
    "clay62_nodes_and_pairs": (6, 2, [[0], [3], [7], [0, 1], [2, 7], []], [3, 0, 4, 255, 1, 5, 2, 4, 0],
                               "k_gf_map_partial_mixed<false, 4, 8>"),
}


@pytest.mark.parametrize("case_name", list(SMALL))
def test_other_geometries(ecx, torch_dev, case_name):
    k, m, lists, ids, kernel_want = SMALL[case_name]
    B = 4096 + 16
    case = Case(torch_dev, k, m, lists, ids, Shape(B, B, 0, B + 16, 0, False), 5300 + k)
    launch = check_chain(ecx, torch_dev, case)
    assert launch.startswith(kernel_want), launch
    check_each_helper_against_uniform_calls(ecx, torch_dev, case)


def test_forced_depth_8_gives_the_same_bytes(ecx, torch_dev):
    """ecx_tune depth 8 runs the depth-8 plan (records padded to 8) on the depth-8 instance."""
    case = Case(torch_dev, 4, 2, LISTS42, IDS42, SHAPES42["chunks_and_rest_aligned16"], 5200 + 8292)
    ecx.tune("depth", 8)
    try:
        launch = check_chain(ecx, torch_dev, case)
    finally:
        ecx.tune("depth", 0)
    assert launch.startswith("k_gf_map_partial_mixed<false, 8, 8>"), launch


@pytest.mark.parametrize("shape", ["one_chunk", "byte_safe_odd_strides"])
def test_bytes_that_name_nothing_leave_their_stripes_untouched(ecx, torch_dev, shape):
    """(iii): node bytes >= n and ids >= npatterns, in both modes; the other stripes of the same
    launch are written as usual."""
    torch = torch_dev
    case = Case(torch, 4, 2, LISTS42, IDS42, SHAPES42[shape], 5200 + SHAPES42[shape].B)
    S, n, lay = case.S, case.n, case.lay
    rng = np.random.default_rng(77)
    start = rng.integers(0, 256, case.acc_size, dtype=np.uint8)
    nodes = np.array([node_of(2, s, n) for s in range(S)], np.uint8)
    ids = np.array(IDS42, np.uint8)
    bad_node = {1: 6, 5: 7, 9: 255, 13: 128}   # stripe -> a byte that is no node
    bad_id = {2: 22, 6: 23, 10: 254, 14: 100}  # stripe -> an id past the set's 22 lists
    for s, v in bad_node.items():
        nodes[s] = v
    for s, v in bad_id.items():
        ids[s] = v
    untouched = set(bad_node) | set(bad_id) | {s for s, p in enumerate(IDS42) if p >= len(LISTS42) or not LISTS42[p]}
    with ecx.ClayPatternSet(LISTS42, 4, 2) as ps:
        for first in (True, False):
            acc = torch.from_numpy(start.copy()).cuda()
            case.hop(ps, torch, 2, acc, first, nodes=torch.from_numpy(nodes).cuda(), ids=torch.from_numpy(ids).cuda())
            ref = torch.from_numpy(start.copy()).cuda()
            case.hop(ps, torch, 2, ref, first)  # the same hop with the case's own bytes
            torch.cuda.synchronize()
            got, plain = acc.cpu().numpy(), ref.cpu().numpy()
            want = plain.copy()
            for s in untouched:
                lo = GUARD + s * lay.out_stripe
                hi = min(case.acc_size, lo + lay.out_stripe)
                want[lo:hi] = start[lo:hi]
            assert (got == want).all(), first
            written = [s for s in range(S) if s not in untouched]
            assert any((plain[GUARD + s * lay.out_stripe:GUARD + (s + 1) * lay.out_stripe] !=
                        start[GUARD + s * lay.out_stripe:GUARD + (s + 1) * lay.out_stripe]).any() for s in written)
