"""locateCorrupt2Batch under stream capture, by the protocol of tests/test_gpu_capture.py (its helpers
are imported, the file is not edited): the call runs once eagerly, is captured on one stream, the
graph holds kernel nodes only (k_set_suspects, the pass, k_fold_suspects2), and three replays follow
the corruption as it moves from a single shard to a pair to clean.  The project's default queue
settings throughout."""
import numpy as np
import pytest

from locate2_cases import expectations2
from locate_cases import GUARD, valid_stripes
from test_gpu_capture import _refused, capture, kernels_only, node_types

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_replay_of_locate2(ecx, torch_dev):
    """RS(2,4), L = 2 chunks + 48 B, five stripes.  Replays: shard 3 of stripe 1 corrupt; then shards
    0 and 5 of stripe 4, one in the tail window, as well as shard 2 of stripe 0; then everything
    restored.  Each replay equals the oracle, so k_set_suspects keeps setting 1s: a suspect cleared
    by one replay is back for the next."""
    torch = torch_dev
    k, m, L, S = 2, 4, 2 * 4096 + 48, 5
    n, width = 6, 21
    rs = ecx.ReedSolomon.create(k, m)
    nat = valid_stripes(k, m, S, L, 9750)
    pool = torch.from_numpy(nat).cuda()
    suspect = torch.full((S * width + 16,), GUARD, dtype=torch.uint8, device="cuda")
    culprit = torch.full((2 * S + 4,), -77, dtype=torch.int32, device="cuda")
    heal = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")

    def call():
        rs.locateCorrupt2Batch(pool, n * L, L, S, 0, L, suspect, culprit, heal)

    call()  # once outside the capture
    torch.cuda.synchronize()
    assert culprit.cpu().tolist() == [-1] * (2 * S) + [-77] * 4
    g = capture(torch, call)
    types = node_types(g)
    assert kernels_only(types, 3) and len(types) == 3, types  # k_set_suspects, k_gf_locate2, k_fold_suspects2
    rounds = ([(1, 3, 17)], [(4, 5, L - 1), (4, 0, 9), (0, 2, 4096 + 9)], [])
    wants = ([[-1, -1], [3, -1], [-1, -1], [-1, -1], [-1, -1]],
             [[2, -1], [-1, -1], [-1, -1], [-1, -1], [0, 5]], [[-1, -1]] * S)
    for flips, promised in zip(rounds, wants):
        bad = nat.copy()
        for s, i, byte in flips:
            bad[s, i, byte] ^= 0x42
        want_s, want_c, want_h = expectations2(k, m, bad, 0, L)
        assert want_c.tolist() == promised
        pool.copy_(torch.from_numpy(bad))
        before = pool.clone()
        suspect.fill_(GUARD)
        culprit.fill_(-77)
        heal.fill_(GUARD)
        g.replay()
        torch.cuda.synchronize()
        assert culprit.cpu().tolist() == want_c.reshape(-1).tolist() + [-77] * 4, flips
        assert suspect.cpu().tolist() == want_s.reshape(-1).tolist() + [GUARD] * 16, flips
        assert heal.cpu().tolist() == want_h.tolist() + [GUARD] * 16, flips
        assert torch.equal(pool, before)


def test_first_locate2_inside_a_capture_is_refused(ecx, torch_dev):
    """A codec that has never run on this device: its first locate2 on a capturing stream is refused
    with ECX_E_DEVICE before anything is enqueued -- the capture ends valid and empty -- and after
    one eager call the same call captures as kernel nodes.  So is the first locate2 of a codec whose
    check map and locate plan are resident (one locateCorruptBatch) but whose pair plan is not."""
    torch = torch_dev
    for k, m, warm_single in ((20, 5, False), (19, 6, True)):  # codes no other test runs on a device
        L, S = 4096 + 100, 3
        n = k + m
        width = n + n * (n - 1) // 2
        rs = ecx.ReedSolomon.create(k, m)
        pool = torch.zeros(S * n * L, dtype=torch.uint8, device="cuda")
        suspect = torch.full((S * width + 16,), GUARD, dtype=torch.uint8, device="cuda")
        culprit = torch.full((2 * S + 4,), -77, dtype=torch.int32, device="cuda")
        if warm_single:  # the check map, the zero page and the locate plan are resident, the pair plan is not
            rs.locateCorruptBatch(pool, n * L, L, S, 0, L, suspect[:S * n], culprit[:S])
            torch.cuda.synchronize()
            suspect.fill_(GUARD)
            culprit.fill_(-77)

        def call():
            rs.locateCorrupt2Batch(pool, n * L, L, S, 0, L, suspect, culprit)

        _refused(ecx, torch, call)
        torch.cuda.synchronize()
        assert (suspect.cpu().numpy() == GUARD).all() and (culprit.cpu().numpy() == -77).all()
        call()
        torch.cuda.synchronize()
        assert culprit.cpu().tolist() == [-1] * (2 * S) + [-77] * 4
        g = capture(torch, call)
        assert kernels_only(node_types(g), 3)
        pool[S * n * L - 1] ^= 1  # the last byte of the batch: the last parity shard of stripe S - 1
        g.replay()
        torch.cuda.synchronize()
        assert culprit.cpu().tolist() == [-1] * (2 * S - 2) + [n - 1, -1] + [-77] * 4
