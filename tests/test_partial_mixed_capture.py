"""decodePartialBatchMixed under stream capture: a fresh set's first partial call on a capturing
stream is refused -- the upload of its partial-sum plan allocates and copies -- and leaves no node
behind; after one call outside capture a chain of four hops captures as kernel nodes only, and
replays over changed data, changed ids AND changed shard bytes equal eager calls: both byte arrays
are read on the device at replay time."""
import pytest

from mixed_cases import IDS, S
from test_mixed_decode import KERNEL, capturing, node_types
from test_partial_mixed import GUARD, SHAPES, case_of

pytestmark = pytest.mark.gpu
ECX_E_DEVICE = -10
HOPS = 4


def test_partial_mixed_chain_under_stream_capture(ecx):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = case_of(SHAPES[3])  # RS(4,2), two full chunks and a 100-B rest: two launches per hop
    rs = ecx.ReedSolomon.create(c.k, c.m)
    # buffers of this test's own: the replays scribble over them
    nodes = [c.nodes[j].clone() for j in range(HOPS)]
    shard_of = c.dev_shard_of[:HOPS].clone()
    ids = c.dev_ids.clone()
    acc = c.new_acc(torch)

    def chain(ps, acc, nodes, ids, shard_of):
        for j in range(HOPS):
            rs.decodePartialBatchMixed(ps, ids, shard_of[j], nodes[j], c.in_stride, 0, acc[GUARD:], c.stripe_stride,
                                       c.row_stride, S, c.L, j == 0)

    with rs.patternSet(c.pats) as ps:
        g0 = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g0):
            with pytest.raises(ecx.EcxError) as err:
                chain(ps, acc, nodes, ids, shard_of)
        assert err.value.code == ECX_E_DEVICE and "once outside the capture" in str(err.value), str(err.value)
        assert node_types(g0) == []
        assert torch.equal(acc, c.new_acc(torch))

        chain(ps, acc, nodes, ids, shard_of)  # outside capture: the plan becomes resident
        torch.cuda.synchronize()
        first = acc.clone()

        g = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g):
            chain(ps, acc, nodes, ids, shard_of)
        types = node_types(g)
        assert len(types) == 2 * HOPS and set(types) == {KERNEL}, types
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(acc, first)
        for r, seed in enumerate((8401, 8402, 8403)):
            for j, t in enumerate(nodes):
                ecx.fill_random(t, t.numel(), seed + 16 * j)
            ids.copy_(torch.tensor(IDS[r + 1:] + IDS[:r + 1], dtype=torch.uint8))  # rotated: every stripe changes
            shard_of.copy_((shard_of + (r + 1)) % c.n)
            if r == 2:
                shard_of[2, 5] = 200  # no shard: that hop skips stripe 5
            acc.copy_(c.new_acc(torch))
            eager = acc.clone()
            g.replay()
            torch.cuda.synchronize()
            chain(ps, eager, nodes, ids, shard_of)
            torch.cuda.synchronize()
            assert torch.equal(acc, eager), seed
            assert not torch.equal(acc, first)
        del g, g0
