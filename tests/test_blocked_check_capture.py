"""isParityCorrectBlockedBatch under stream capture, by the protocol of tests/test_gpu_capture.py
(its helpers are imported, the file is not edited): the call runs once eagerly, is captured on one
stream, the graph holds kernel nodes only (k_set_verdicts, the body pass, the tail pass -- a
memset node replays with the value 0 from its second replay on, test_gpu_capture.py), and three
replays follow the data as it changes between them."""
import numpy as np
import pytest

import oracle as O
from test_gpu_capture import _refused, capture, kernels_only, node_types

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_replay_of_blocked_parity_check(ecx, torch_dev):
    """RS(17,3), L = 200,000 (6 blocks of 32 KiB + a 3,392-B tail), five stripes made valid by the
    oracle.  Replays: valid data -> all 1; the last byte of stripe 2's last body block of the last
    parity shard flipped -> only stripe 2 is 0; the byte restored -> all 1 again."""
    torch = torch_dev
    k, m, L, S = 17, 3, 200000, 5
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    b, full, tail = rs.blockedLayout(L)
    assert (b, full, tail) == (32768, 6, 3392)
    rng = np.random.default_rng(8100)
    nat = np.zeros((S, n, L), np.uint8)
    nat[:, :k] = rng.integers(0, 256, (S, k, L), dtype=np.uint8)
    for s in range(S):
        O.ReedSolomon(k, m).encode_parity([nat[s, i] for i in range(n)], 0, L)
    flat = ecx.blocked_pack(torch.from_numpy(nat).cuda(), b)
    verdict = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")

    def call():
        rs.isParityCorrectBlockedBatch(flat, S, L, verdict)

    call()  # once outside the capture
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [1] * S + [GUARD] * 16
    g = capture(torch, call)
    types = node_types(g)
    assert kernels_only(types, 3) and len(types) == 3, types  # k_set_verdicts, body, tail
    # stripe 2, block row full - 1, shard n - 1, last byte of the block
    at = 2 * full * n * b + (full - 1) * n * b + (n - 1) * b + b - 1
    for flipped, want in ((False, [1] * S), (True, [1, 1, 0, 1, 1]), (False, [1] * S), (True, [1, 1, 0, 1, 1])):
        verdict.fill_(GUARD)
        if flipped:
            flat[at] ^= 0x81
        before = flat.clone()
        g.replay()
        torch.cuda.synchronize()
        assert verdict.cpu().tolist() == want + [GUARD] * 16, (flipped, verdict.cpu().tolist())
        assert torch.equal(flat, before)
        if flipped:
            shards = ecx.blocked_unpack(flat, S, n, L, b, first=2, count=1).cpu().numpy()[0]
            assert not O.ReedSolomon(k, m).is_parity_correct([shards[i].copy() for i in range(n)], 0, L)
            flat[at] ^= 0x81


def test_first_blocked_check_inside_a_capture_is_refused(ecx, torch_dev):
    """A codec whose check map has never run on this device: its first blocked check on a
    capturing stream is refused with ECX_E_DEVICE before anything is enqueued -- the capture ends
    valid and empty -- and after one eager call the same call captures as kernel nodes."""
    torch = torch_dev
    k, m, L, S = 23, 3, 8192 + 100, 3
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    flat = torch.zeros(S * n * L, dtype=torch.uint8, device="cuda")
    verdict = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")

    def call():
        rs.isParityCorrectBlockedBatch(flat, S, L, verdict, 4096)

    _refused(ecx, torch, call)
    torch.cuda.synchronize()
    assert (verdict.cpu().numpy() == GUARD).all()
    call()
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [1] * S + [GUARD] * 16
    g = capture(torch, call)
    assert kernels_only(node_types(g), 3)
    flat[S * n * L - 1] ^= 1  # the last byte of the batch: stripe S - 1's tail
    g.replay()
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [1] * (S - 1) + [0] + [GUARD] * 16
