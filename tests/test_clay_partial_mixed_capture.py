"""ClayPatternSet.partialBatchMixed under stream capture: a fresh set's first hop on a capturing
stream is refused -- the upload of its partial-sum plan allocates and copies -- and leaves no node
behind; after one warm call outside capture one hop captures as kernel nodes only (the full chunks
and the byte-safe rest), and three replays over changed data, changed ids AND changed node bytes
equal eager calls: both byte arrays are read on the device at replay time."""
import pytest

from clay_mixed_cases import GUARD, IDS42, LISTS42
from test_clay_partial_mixed import SHAPES42, Case
from test_mixed_decode import KERNEL, capturing, node_types

pytestmark = pytest.mark.gpu
ECX_E_DEVICE = -10


def test_clay_partial_mixed_hop_under_stream_capture(ecx):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    # Clay(4,2), two full chunks and a 100-B rest: two launches per hop
    c = Case(torch, 4, 2, LISTS42, IDS42, SHAPES42["chunks_and_rest_aligned16"], 5200 + 8292)
    S, n, lay, B = c.S, c.n, c.lay, c.shape.B
    inp, iss, ins, isub, nodes = c.helper(torch, 3)
    # buffers of this test's own: the replays scribble over them
    inp, nodes, ids = inp.clone(), nodes.clone(), c.dev_ids.clone()

    def new_acc():
        t = torch.empty(c.acc_size, dtype=torch.uint8, device="cuda")
        ecx.fill_random(t, t.numel(), 9100)
        return t

    def hop(ps, acc):
        ps.partialBatchMixed(ids, nodes, inp, iss, ins, isub, acc[GUARD:], lay.out_stripe, lay.out_sub, S, B, False)

    acc = new_acc()
    with ecx.ClayPatternSet(LISTS42, 4, 2) as ps:
        g0 = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g0):
            with pytest.raises(ecx.EcxError) as err:
                hop(ps, acc)
        assert err.value.code == ECX_E_DEVICE and "once outside the capture" in str(err.value), str(err.value)
        assert node_types(g0) == []
        assert torch.equal(acc, new_acc())

        hop(ps, acc)  # the warm call: the plans become resident
        torch.cuda.synchronize()
        first = acc.clone()
        assert not torch.equal(first, new_acc())

        acc.copy_(new_acc())
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g):
            hop(ps, acc)
        types = node_types(g)
        assert len(types) == 2 and set(types) == {KERNEL}, types
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(acc, first)
        for r, seed in enumerate((9401, 9402, 9403)):
            ecx.fill_random(inp, inp.numel(), seed)
            ids.copy_(torch.tensor(IDS42[r + 1:] + IDS42[:r + 1], dtype=torch.uint8))  # rotated: every stripe changes
            nodes.copy_((nodes + (r + 1)) % n)
            if r == 2:
                nodes[5] = 200  # no node: the hop skips stripe 5
            acc.copy_(new_acc())
            eager = acc.clone()
            g.replay()
            torch.cuda.synchronize()
            hop(ps, eager)
            torch.cuda.synchronize()
            assert torch.equal(acc, eager), seed
            assert not torch.equal(acc, first)
        del g, g0
