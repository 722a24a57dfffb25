"""locateCorruptBatch under stream capture, by the protocol of tests/test_gpu_capture.py (its helpers
are imported, the file is not edited): the call runs once eagerly, is captured on one stream, the
graph holds kernel nodes only (k_set_suspects, the pass, k_fold_suspects -- a memset node replays
with the value 0 from its second replay on), and three replays follow the corruption as it moves."""
import numpy as np
import pytest

from locate_cases import GUARD, expectations, valid_stripes
from test_gpu_capture import _refused, capture, kernels_only, node_types

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_replay_of_locate(ecx, torch_dev):
    """RS(12,4), L = 2 chunks + 48 B, five stripes.  Replays: shard 3 of stripe 1 corrupt; then
    shard 15 of stripe 4 in the tail window as well as two shards of stripe 0; then everything
    restored.  Each replay equals the oracle, so k_set_suspects keeps setting 1s: a suspect cleared
    by one replay is back for the next."""
    torch = torch_dev
    k, m, L, S = 12, 4, 2 * 4096 + 48, 5
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    nat = valid_stripes(k, m, S, L, 9700)
    pool = torch.from_numpy(nat).cuda()
    suspect = torch.full((S * n + 16,), GUARD, dtype=torch.uint8, device="cuda")
    culprit = torch.full((S + 4,), -77, dtype=torch.int32, device="cuda")
    heal = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")

    def call():
        rs.locateCorruptBatch(pool, n * L, L, S, 0, L, suspect, culprit, heal)

    call()  # once outside the capture
    torch.cuda.synchronize()
    assert culprit.cpu().tolist() == [-1] * S + [-77] * 4
    g = capture(torch, call)
    types = node_types(g)
    assert kernels_only(types, 3) and len(types) == 3, types  # k_set_suspects, k_gf_locate, k_fold_suspects
    rounds = ([(1, 3, 17)], [(4, 15, L - 1), (0, 2, 5), (0, 7, 4096 + 9)], [])
    for flips in rounds:
        bad = nat.copy()
        for s, i, byte in flips:
            bad[s, i, byte] ^= 0x42
        want_s, want_c, want_h = expectations(k, m, bad, 0, L)
        pool.copy_(torch.from_numpy(bad))
        before = pool.clone()
        suspect.fill_(GUARD)
        culprit.fill_(-77)
        heal.fill_(GUARD)
        g.replay()
        torch.cuda.synchronize()
        assert culprit.cpu().tolist() == want_c.tolist() + [-77] * 4, flips
        assert suspect.cpu().tolist() == want_s.reshape(-1).tolist() + [GUARD] * 16, flips
        assert heal.cpu().tolist() == want_h.tolist() + [GUARD] * 16, flips
        assert torch.equal(pool, before)
    assert want_c.tolist() == [-1] * S  # the last round is clean again


def test_first_locate_inside_a_capture_is_refused(ecx, torch_dev):
    """A codec that has never run on this device: its first locate on a capturing stream is refused
    with ECX_E_DEVICE before anything is enqueued -- the capture ends valid and empty -- and after
    one eager call the same call captures as kernel nodes.  So is the first locate of a codec whose
    check map is resident but whose locate plan is not."""
    torch = torch_dev
    for k, m, warm_check in ((22, 5, False), (21, 6, True)):
        L, S = 4096 + 100, 3
        n = k + m
        rs = ecx.ReedSolomon.create(k, m)
        pool = torch.zeros(S * n * L, dtype=torch.uint8, device="cuda")
        suspect = torch.full((S * n + 16,), GUARD, dtype=torch.uint8, device="cuda")
        culprit = torch.full((S + 4,), -77, dtype=torch.int32, device="cuda")
        if warm_check:  # the check map and the zero page are resident, the locate plan is not
            rs.isParityCorrectBatch(pool, n * L, L, S, 0, L, suspect[:S])
            torch.cuda.synchronize()
            suspect.fill_(GUARD)

        def call():
            rs.locateCorruptBatch(pool, n * L, L, S, 0, L, suspect, culprit)

        _refused(ecx, torch, call)
        torch.cuda.synchronize()
        assert (suspect.cpu().numpy() == GUARD).all() and (culprit.cpu().numpy() == -77).all()
        call()
        torch.cuda.synchronize()
        assert culprit.cpu().tolist() == [-1] * S + [-77] * 4
        g = capture(torch, call)
        assert kernels_only(node_types(g), 3)
        pool[S * n * L - 1] ^= 1  # the last byte of the batch: the last parity shard of stripe S - 1
        g.replay()
        torch.cuda.synchronize()
        assert culprit.cpu().tolist() == [-1] * (S - 1) + [n - 1] + [-77] * 4
