"""performCodingBatchMixed of a generated set under stream capture (clay_rtc.cpp ClaySetRtc): a fresh
set's first call on a capturing stream is refused -- it would compile and load k_clay_repair_set --
and leaves no node behind; after one eager call the same call captures as exactly one kernel node,
and replays over changed data and changed ids (the kernel reads them on the device) equal the
oracle."""
import pytest

import clay_set_rtc_cases as T
from clay_rtc_sweep_cases import GUARD, SENTINEL
from test_mixed_decode import ECX_E_DEVICE, KERNEL, capturing, node_types

pytestmark = pytest.mark.gpu


def test_generated_set_under_stream_capture(ecx):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    k, m, v = 10, 4, 2
    lists, ids0 = T.LISTS_LAYOUT, T.IDS_LAYOUT
    lay = T.layout(k, m, v)
    inp = T.device_input(ecx, torch, k, m, v, lay, 8500)
    out = torch.full((GUARD + T.out_bytes(lay) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    dev_ids = torch.tensor(ids0, dtype=torch.uint8, device="cuda")
    with ecx.ClayPatternSet([list(x) for x in lists], k, m, v) as ps:
        def call():
            ps.performCodingBatchMixed(inp[GUARD:], lay.in_stripe, lay.in_sub, out[GUARD:len(out) - GUARD],
                                       lay.out_stripe, lay.out_sub, dev_ids, T.S, lay.B)

        g0 = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g0):
            with pytest.raises(ecx.EcxError) as err:
                call()
        assert err.value.code == ECX_E_DEVICE and "once outside the capture" in str(err.value), str(err.value)
        assert node_types(g0) == []
        assert (out == SENTINEL).all()

        call()  # outside capture: the kernel and the zero page become resident
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == T.expected_output(k, m, v, lists, ids0, lay, 8500)).all()

        g = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g):
            call()
        assert node_types(g) == [KERNEL]
        for seed, roll in ((8501, 0), (8502, 2), (8503, 5)):
            ids = ids0[roll:] + ids0[:roll]
            ecx.fill_random(inp, inp.numel(), seed)
            dev_ids.copy_(torch.tensor(ids, dtype=torch.uint8))
            out.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            T.assert_same(out.cpu().numpy(), T.expected_output(k, m, v, lists, ids, lay, seed), lay, (seed, roll))
        del g, g0
