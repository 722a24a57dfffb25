"""decodePartialBatchMixed on the GPU (k_gf_partial_mixed, csrc/apply_partial_mixed.hip): one hop of
the pipelined partial-sum chain with a pattern id AND a helper shard index per stripe, in one
launch.

The nine stripes and IDS of tests/mixed_cases.py (id 255, a pattern with nothing missing, a
duplicate pattern) under rotated placement: node j holds shard (j + s) mod n of stripe s.  The
stripes are random bytes, not codewords, so the sum over all n nodes' hops equals the oracle's
decodeMissing (ReedSolomon.java:189-286) only if every hop multiplied exactly the shard the
reference reads with exactly its coefficient; the nodes that hold a stripe's missing shard hold
garbage and must add nothing.  The accumulator's rows lie further apart than they are long and
guard bytes surround it: everything no row covers must keep its sentinel."""
import functools

import numpy as np
import pytest

from mixed_cases import IDS, S, oracle_case, patterns_of

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = 0xA5
# (k, m, L, in_stride - L, row_stride - L, stripe_stride - rows * row_stride)
SHAPES = [
    (4, 2, 4096, 0, 16, 0),             # one full chunk
    (12, 4, 4096, 0, 16, 32),
    (17, 3, 4096, 0, 16, 0),
    (4, 2, 2 * 4096 + 100, 12, 28, 0),  # full chunks plus a rest, 16-B aligned strides
    (12, 4, 1001, 2, 5, 1),             # odd strides: byte-safe only
    (5, 5, 4096, 0, 16, 0),             # five missing: the 8-row instance
]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def missing_of(pats, pid):
    return [] if pid >= len(pats) else [i for i, f in enumerate(pats[pid]) if not f]


class Case:
    """The node-local inputs of one shape under rotated placement and the accumulator's layout."""

    def __init__(self, torch, k, m, L, in_pad, row_pad, stripe_pad):
        self.k, self.m, self.n, self.L = k, m, k + m, L
        n = self.n
        self.pats = patterns_of(k, m)
        self.rows = int((self.pats == 0).sum(axis=1).max())
        self.before, self.want = oracle_case(k, m, L)
        self.in_stride = L + in_pad
        self.row_stride = L + row_pad
        self.stripe_stride = self.rows * self.row_stride + stripe_pad
        self.shard_of = np.array([[(j + s) % n for s in range(S)] for j in range(n)], np.uint8)
        self.nodes = []
        for j in range(n):
            host = np.zeros((S, self.in_stride), np.uint8)
            for s in range(S):
                host[s, :L] = self.before[s, self.shard_of[j, s]]
            self.nodes.append(torch.from_numpy(host).cuda())
        self.dev_shard_of = torch.from_numpy(self.shard_of).cuda()
        self.dev_ids = torch.tensor(IDS, dtype=torch.uint8, device="cuda")
        self.acc_bytes = S * self.stripe_stride

    def new_acc(self, torch, fill=None):
        host = np.full(GUARD + self.acc_bytes + GUARD, SENTINEL, np.uint8)
        if fill is not None:
            host[GUARD:GUARD + self.acc_bytes] = fill
        return torch.from_numpy(host).cuda()

    def hop(self, rs, ps, j, acc, is_first, shard_of=None, ids=None):
        rs.decodePartialBatchMixed(ps, self.dev_ids if ids is None else ids,
                                   self.dev_shard_of[j] if shard_of is None else shard_of, self.nodes[j],
                                   self.in_stride, 0, acc[GUARD:], self.stripe_stride, self.row_stride, S, self.L,
                                   is_first)

    def row(self, s, o):
        lo = GUARD + s * self.stripe_stride + o * self.row_stride
        return slice(lo, lo + self.L)


@functools.lru_cache(maxsize=None)
def case_of(shape):
    import torch
    return Case(torch, *shape)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "rs%d_%d_L%d" % s[:3])
def test_chain_sum_over_all_nodes_is_the_oracles_decode(ecx, torch_dev, shape):
    torch = torch_dev
    c = case_of(shape)
    rs = ecx.ReedSolomon.create(c.k, c.m)
    acc = c.new_acc(torch)
    with rs.patternSet(c.pats) as ps:
        assert ps.info() == (len(c.pats), c.n, c.rows)
        for j in range(c.n):
            c.hop(rs, ps, j, acc, j == 0)
        torch.cuda.synchronize()
        shape_of_record = ecx.last_launch_shape()
    got = acc.cpu().numpy()
    want = np.full_like(got, SENTINEL)  # rows past the missing count, untouched stripes, gaps, guards
    rebuilt = 0
    for s, pid in enumerate(IDS):
        for o, shard in enumerate(missing_of(c.pats, pid)):
            want[c.row(s, o)] = c.want[s, shard]
            rebuilt += 1
    assert rebuilt > 0
    if not (got == want).all():
        for s, pid in enumerate(IDS):
            for o in range(c.rows):
                assert (got[c.row(s, o)] == want[c.row(s, o)]).all(), f"stripe {s} (pattern id {pid}) row {o}"
        assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), "guard bytes changed"
        pytest.fail("bytes between the rows changed")
    # the launch of record: the full-chunk instance where the layout has one
    if c.L >= 4096 and c.in_stride % 16 == 0 and c.row_stride % 16 == 0 and c.stripe_stride % 16 == 0:
        assert shape_of_record == "k_gf_partial_mixed<false, %d>" % (4 if c.rows <= 4 else 8), shape_of_record


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4], SHAPES[5]], ids=lambda s: "rs%d_%d_L%d" % s[:3])
@pytest.mark.parametrize("is_first", [True, False])
def test_every_hop_equals_the_uniform_call_stripe_by_stripe(ecx, torch_dev, shape, is_first):
    """The definition of correct: bit-identical, stripe by stripe, to
    decodePartialBatch(pattern, index) -- over an accumulator of random bytes, so an assignment and
    an accumulation differ, and with every node's index, also the ones a pattern does not read."""
    torch = torch_dev
    c = case_of(shape)
    rs = ecx.ReedSolomon.create(c.k, c.m)
    fill = np.random.default_rng(c.L + c.n).integers(0, 256, c.acc_bytes, dtype=np.uint8)
    with rs.patternSet(c.pats) as ps:
        for j in range(c.n):
            got, ref = c.new_acc(torch, fill), c.new_acc(torch, fill)
            c.hop(rs, ps, j, got, is_first)
            for s, pid in enumerate(IDS):
                if pid >= len(c.pats):
                    continue
                rs.decodePartialBatch(c.pats[pid], int(c.shard_of[j, s]), c.nodes[j][s:], c.in_stride,
                                      ref[GUARD + s * c.stripe_stride:], c.stripe_stride, c.row_stride, 1, c.L,
                                      is_first)
            torch.cuda.synchronize()
            assert torch.equal(got, ref), f"node {j}"


def test_shards_read_out_of_a_full_pool_equal_the_node_local_form(ecx, torch_dev):
    """in_shard_stride = L over the whole [S][n][L] pool: one GPU runs every node's hop."""
    torch = torch_dev
    c = case_of(SHAPES[3])
    rs = ecx.ReedSolomon.create(c.k, c.m)
    pool = torch.from_numpy(c.before.copy()).cuda()
    local, pooled = c.new_acc(torch), c.new_acc(torch)
    with rs.patternSet(c.pats) as ps:
        for j in range(c.n):
            c.hop(rs, ps, j, local, j == 0)
            rs.decodePartialBatchMixed(ps, c.dev_ids, c.dev_shard_of[j], pool, c.n * c.L, c.L, pooled[GUARD:],
                                       c.stripe_stride, c.row_stride, S, c.L, j == 0)
        torch.cuda.synchronize()
    assert torch.equal(local, pooled)
    assert not (local.cpu().numpy()[GUARD:-GUARD] == SENTINEL).all()


@pytest.mark.parametrize("is_first", [True, False])
def test_a_shard_byte_that_is_no_shard_leaves_its_stripe_untouched(ecx, torch_dev, is_first):
    torch = torch_dev
    c = case_of(SHAPES[3])
    rs = ecx.ReedSolomon.create(c.k, c.m)
    j = 1
    shard_of = c.dev_shard_of[j].clone()
    off = [0, 4, 7]  # stripes whose patterns do miss something (ids 3, 6, 2)
    assert all(missing_of(c.pats, IDS[s]) for s in off)
    shard_of[off] = 200
    got, ref = c.new_acc(torch), c.new_acc(torch)
    with rs.patternSet(c.pats) as ps:
        c.hop(rs, ps, j, got, is_first, shard_of=shard_of)
        c.hop(rs, ps, j, ref, is_first)
        torch.cuda.synchronize()
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    for s in range(S):
        lo, hi = GUARD + s * c.stripe_stride, GUARD + (s + 1) * c.stripe_stride
        if s in off:
            assert (got[lo:hi] == SENTINEL).all(), s
        else:
            assert (got[lo:hi] == ref[lo:hi]).all(), s
    if is_first:
        assert any((ref[GUARD + s * c.stripe_stride:GUARD + (s + 1) * c.stripe_stride] != SENTINEL).any() for s in off)
    assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
