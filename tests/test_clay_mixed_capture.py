"""performCodingBatchMixed under stream capture (csrc/apply_map_mixed.hip launch_map_mixed): a fresh
set's first call on a capturing stream is refused -- its plan upload allocates and copies -- and
leaves no node behind; after one eager call the same call captures as kernel nodes only, and
replays over changed data and changed ids equal the eager results."""
import pytest

from clay_mixed_cases import GUARD, IDS42, LISTS42, SENTINEL, expected_output, layout, make_input
from test_mixed_decode import ECX_E_DEVICE, KERNEL, capturing, node_types

pytestmark = pytest.mark.gpu


def test_clay_mixed_under_stream_capture(ecx):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    k, m, S = 4, 2, len(IDS42)
    lay = layout(4096 + 48, 48, 16, out_pitch=4096 + 64)  # a full chunk and a byte-safe rest: two launches
    flat_in = make_input(k, m, S, lay, 4500)
    want = expected_output(k, m, LISTS42, IDS42, lay, 16, flat_in)
    inp = torch.from_numpy(flat_in.copy()).cuda()
    out = torch.full((want.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    dev_ids = torch.tensor(IDS42, dtype=torch.uint8, device="cuda")
    with ecx.ClayPatternSet(LISTS42, k, m) as ps:
        def call(o):
            ps.performCodingBatchMixed(inp, lay.in_stripe, lay.in_sub, o[GUARD:], lay.out_stripe, lay.out_sub, dev_ids,
                                       S, lay.B)

        g0 = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g0):
            with pytest.raises(ecx.EcxError) as err:
                call(out)
        assert err.value.code == ECX_E_DEVICE and "once outside the capture" in str(err.value), str(err.value)
        assert node_types(g0) == []
        assert (out == SENTINEL).all()

        call(out)  # outside capture: the plans and the zero page become resident
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == want).all()

        g = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g):
            call(out)
        types = node_types(g)
        assert len(types) == 2 and set(types) == {KERNEL}, types
        # three replays: over changed data, and over changed ids (the kernel reads them on the device)
        for seed, roll in ((4501, 0), (4502, 5), (4503, 11)):
            ecx.fill_random(inp, inp.numel(), seed)
            dev_ids.copy_(torch.tensor(IDS42[roll:] + IDS42[:roll], dtype=torch.uint8))
            out.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            eager = torch.full_like(out, SENTINEL)
            call(eager)
            torch.cuda.synchronize()
            assert torch.equal(out, eager), seed
            assert not (eager == SENTINEL).all()
        # and on the case's own input and ids the replay gives the oracle's bytes
        inp.copy_(torch.from_numpy(flat_in.copy()))
        dev_ids.copy_(torch.tensor(IDS42, dtype=torch.uint8))
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == want).all()
        del g, g0
