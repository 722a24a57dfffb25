"""locateCorrupt2BlockedBatch (ecx_rs_locate_corrupt2_blocked_batch) over blocked_pack, against the
oracle's brute force on the natural shards (tests/locate2_cases.py).  The suspects of caller stripe s
are cleared by the `full` block rows of the body pass that belong to it and by its tail, so the pair
flips sit where a wrong unit -> stripe quotient would charge a neighbouring stripe: the first unit of
a stripe, its last body unit, the tail, and split between a body unit and the tail.  It ends with a
heal through decodeMissingBlockedBatchMixed with doubleLossPatternSet()."""
import functools

import numpy as np
import pytest

from locate2_cases import expectations2, run_locate2
from locate_cases import valid_stripes

pytestmark = pytest.mark.gpu

S = 9
# (k, m, L, block): 3 blocks of 4 KiB + a 208-B tail (ROWS = 4); 15 blocks of 64 B + an odd 41-B tail
# (ROWS = 8, byte-safe passes)
SHAPES = [(2, 4, 3 * 4096 + 208, 4096), (3, 5, 1001, 64)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def flips_for(k, m, L, b):
    """(stripe, shard, byte): stripes 0 and 2 stay clean between the corrupt ones."""
    n = k + m
    full = L // b
    return [(1, 0, 0), (1, k, 1),                              # a pair in the first unit of stripe 1
            (3, 1, full * b - 1), (3, n - 1, full * b - 2),    # in the last body unit of stripe 3
            (4, k - 1, full * b), (4, k, L - 1),               # in the tail
            (5, 0, b + 2), (5, n - 1, L - 1),                  # split between a body unit and the tail
            (6, n - 1, L - 1),                                 # one shard, the last byte of the batch's tails
            (7, 1, 3), (7, 1, (full - 1) * b + 1),             # one shard in two blocks
            (8, 0, 5), (8, k, b + 6), (8, n - 1, L - 2)]       # three shards: nobody


@functools.lru_cache(maxsize=None)
def case(k, m, L, b):
    """Valid natural stripes, the same with the flips, and the oracle's expectations over [0, L) of
    the natural shards.  Shared: do not write."""
    nat = valid_stripes(k, m, S, L, 9600 + 13 * k + L)
    bad = nat.copy()
    for s, i, byte in flips_for(k, m, L, b):
        bad[s, i, byte] ^= 0x81
    want = expectations2(k, m, bad, 0, L)
    for a in (nat, bad) + want:
        a.setflags(write=False)
    return nat, bad, want


@pytest.mark.parametrize("k,m,L,block", SHAPES)
def test_blocked_locate2_vs_oracle_and_heal(ecx, torch_dev, k, m, L, block):
    """suspect, culprit and healId equal the oracle's on the natural shards and locateCorrupt2Batch's
    on the unpacked buffer; the outputs' guard bytes and the packed buffer are untouched; the heal
    restores the stripes with one or two culprits and leaves the others bit-identical."""
    torch = torch_dev
    n = k + m
    width = n + n * (n - 1) // 2
    assert L % block and L // block >= 2  # a tail pass, and body units that differ
    nat, bad, (want_s, want_c, want_h) = case(k, m, L, block)
    assert want_c.tolist() == [[-1, -1], [0, k], [-1, -1], [1, n - 1], [k - 1, k], [0, n - 1], [n - 1, -1], [1, -1],
                               [-2, -2]]
    rs = ecx.ReedSolomon.create(k, m)
    flat = ecx.blocked_pack(torch.from_numpy(np.array(bad)).cuda(), block)
    before = flat.clone()
    got_s, got_c, got_h, heal_dev = run_locate2(
        torch, lambda su, cu, he: rs.locateCorrupt2BlockedBatch(flat, S, L, su, cu, he, block), S, width)
    print(f"RS({k},{m}) L={L} block={block} culprit={got_c.tolist()} want={want_c.tolist()}")
    assert got_c.tolist() == want_c.tolist()
    assert (got_s == want_s).all(), (got_s.tolist(), want_s.tolist())
    assert got_h.tolist() == want_h.tolist()
    assert torch.equal(flat, before)  # read-only
    s2, c2, h2, _ = run_locate2(
        torch, lambda su, cu, he: rs.locateCorrupt2BlockedBatch(flat, S, L, su, cu, he, block), S, width, heal=False)
    assert h2 is None and c2.tolist() == want_c.tolist() and (s2 == want_s).all()
    natural = torch.from_numpy(np.array(bad)).cuda()
    s3, c3, h3, _ = run_locate2(
        torch, lambda su, cu, he: rs.locateCorrupt2Batch(natural, n * L, L, S, 0, L, su, cu, he), S, width)
    assert c3.tolist() == got_c.tolist() and (s3 == got_s).all() and h3.tolist() == got_h.tolist()

    with rs.doubleLossPatternSet() as ps:
        rs.decodeMissingBlockedBatchMixed(flat, ps, heal_dev[:S], S, L, block)
        torch.cuda.synchronize()
    healed = ecx.blocked_unpack(flat, S, n, L, block).cpu().numpy()
    for s in range(S):
        assert (healed[s] == (nat[s] if want_c[s, 0] >= 0 else bad[s])).all(), s
