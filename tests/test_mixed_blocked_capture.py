"""decodeMissingBlockedBatchMixed under stream capture (as tests/test_mixed_decode.py has it for the
natural layout): a fresh set's first call on a capturing stream is refused -- its plan upload
allocates and copies -- and leaves no node behind, of either pass; after one call outside capture
the same call captures as kernel nodes only, and replays over changed data AND changed ids equal
eager calls: the ids are read on the device at replay time, through the divisor."""
import pytest

from mixed_cases import IDS, S, block_of, oracle_case, pack, patterns_of
from test_mixed_decode import KERNEL, capturing, node_types

pytestmark = pytest.mark.gpu
ECX_E_DEVICE = -10


def test_blocked_mixed_decode_under_stream_capture(ecx):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    k, m, L, block_arg = 17, 3, 200000, 0     # 6 x 32 KiB blocks and a 3,392-B tail: both passes
    n = k + m
    block = block_of(ecx, k, m, L, block_arg)
    before, want = oracle_case(k, m, L)
    packed = pack(ecx, before, block)
    buf = torch.from_numpy(packed.copy()).cuda()
    dev_ids = torch.tensor(IDS, dtype=torch.uint8, device="cuda")
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(patterns_of(k, m)) as ps:
        def call(b, ids):
            rs.decodeMissingBlockedBatchMixed(b, ps, ids, S, L, block_arg)

        g0 = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g0):
            with pytest.raises(ecx.EcxError) as err:
                call(buf, dev_ids)
        assert err.value.code == ECX_E_DEVICE and "once outside the capture" in str(err.value), str(err.value)
        assert node_types(g0) == []
        assert (buf.cpu().numpy() == packed).all()

        call(buf, dev_ids)  # outside capture: the plan becomes resident
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == pack(ecx, want, block)).all()

        g = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g):
            call(buf, dev_ids)
        types = node_types(g)
        # the body's full chunks, and the tail's byte-safe launch (3,392 B: no full chunk)
        assert len(types) == 2 and set(types) == {KERNEL}, types
        for r, seed in enumerate((8201, 8202, 8203)):
            ecx.fill_random(buf, buf.numel(), seed)  # whatever the last run left is gone
            dev_ids.copy_(torch.tensor(IDS[r + 1:] + IDS[:r + 1], dtype=torch.uint8))  # rotated: every stripe changes
            eager, eager_ids = buf.clone(), dev_ids.clone()
            g.replay()
            torch.cuda.synchronize()
            call(eager, eager_ids)
            torch.cuda.synchronize()
            assert torch.equal(buf, eager), seed
        # and on the case's own input and ids the replay gives the oracle's bytes
        buf.copy_(torch.from_numpy(packed.copy()))
        dev_ids.copy_(torch.tensor(IDS, dtype=torch.uint8))
        g.replay()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == pack(ecx, want, block)).all()
        del g, g0
