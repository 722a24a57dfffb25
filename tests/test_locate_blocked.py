"""locateCorruptBlockedBatch (ecx_rs_locate_corrupt_blocked_batch) over blocked_pack, against the
oracle's brute force on the natural shards (tests/locate_cases.py).  The suspects of caller stripe s
are cleared by the `full` block rows of the body pass that belong to it and by its tail, so the
flips sit where a wrong unit -> stripe quotient would charge a neighbouring stripe: the first unit
of a stripe, its last body unit, and the tail.  It ends with a heal through
decodeMissingBlockedBatchMixed."""
import functools

import numpy as np
import pytest

from locate_cases import expectations, run_locate, valid_stripes

pytestmark = pytest.mark.gpu

S = 7
# (k, m, L, block): 6 blocks of 32 KiB + a 3,392-B tail; 25 blocks + an odd 2,049-B tail; 8 syndrome
# rows with byte-safe passes; full == 0 (tail only)
SHAPES = [(17, 3, 200000, 0), (4, 2, 104449, 4096), (5, 5, 1001, 64), (4, 2, 100, 4096)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def flips_for(k, m, L, b):
    """(stripe, shard, byte): stripes 0 and 2 stay clean between the corrupt ones."""
    n = k + m
    full, tail = divmod(L, b)
    flips = [(1, 0, 0)]                                       # the first unit of stripe 1
    if full:
        flips.append((3, n - 1, full * b - 1))                # the last body unit of stripe 3
    if tail:
        flips.append((4, k - 1, full * b))                    # byte 0 of a data shard's tail
        flips.append((6, n - 1, L - 1))                       # the last byte of the batch
    if full >= 2:
        flips += [(5, k, 3), (5, k, (full - 1) * b + 1)]      # one shard in two blocks: stays the culprit
        flips.append((6, 1, b + 2))                           # with the tail flip: two shards, nobody
    elif tail > 8:
        flips += [(5, k, 3), (5, k, L - 2)]
        flips.append((6, 1, 5))
    return flips


@functools.lru_cache(maxsize=None)
def case(k, m, L, block):
    """Valid natural stripes, the same with the flips, the oracle's expectations over [0, L) of the
    natural shards, and the resolved block.  Shared: do not write."""
    import rpamd
    b = block or rpamd.load(shape_knobs=True).ReedSolomon.create(k, m).blockedLayout(L)[0]
    nat = valid_stripes(k, m, S, L, 9500 + 13 * k + L)
    bad = nat.copy()
    for s, i, byte in flips_for(k, m, L, b):
        bad[s, i, byte] ^= 0x81
    want = expectations(k, m, bad, 0, L)
    for a in (nat, bad) + want:
        a.setflags(write=False)
    return nat, bad, want, b


@pytest.mark.parametrize("k,m,L,block", SHAPES)
def test_blocked_locate_vs_oracle_and_heal(ecx, torch_dev, k, m, L, block):
    """suspect, culprit and healId equal the oracle's on the natural shards and locateCorruptBatch's
    on the unpacked buffer; the outputs' guard bytes and the packed buffer are untouched; the heal
    restores the stripes with a culprit and leaves the others bit-identical."""
    torch = torch_dev
    n = k + m
    nat, bad, (want_s, want_c, want_h), b = case(k, m, L, block)
    assert want_c[0] == -1 and want_c[2] == -1 and want_c[1] == 0
    rs = ecx.ReedSolomon.create(k, m)
    flat = ecx.blocked_pack(torch.from_numpy(np.array(bad)).cuda(), b)
    before = flat.clone()
    got_s, got_c, got_h, heal_dev = run_locate(
        torch, lambda su, cu, he: rs.locateCorruptBlockedBatch(flat, S, L, su, cu, he, block), S, n)
    print(f"RS({k},{m}) L={L} block={b} culprit={got_c.tolist()} want={want_c.tolist()}")
    assert got_c.tolist() == want_c.tolist()
    assert (got_s == want_s).all(), (got_s.tolist(), want_s.tolist())
    assert got_h.tolist() == want_h.tolist()
    assert torch.equal(flat, before)  # read-only
    s2, c2, h2, _ = run_locate(
        torch, lambda su, cu, he: rs.locateCorruptBlockedBatch(flat, S, L, su, cu, he, block), S, n, heal=False)
    assert h2 is None and c2.tolist() == want_c.tolist() and (s2 == want_s).all()
    natural = torch.from_numpy(np.array(bad)).cuda()
    s3, c3, h3, _ = run_locate(
        torch, lambda su, cu, he: rs.locateCorruptBatch(natural, n * L, L, S, 0, L, su, cu, he), S, n)
    assert c3.tolist() == got_c.tolist() and (s3 == got_s).all() and h3.tolist() == got_h.tolist()

    with rs.singleLossPatternSet() as ps:
        rs.decodeMissingBlockedBatchMixed(flat, ps, heal_dev[:S], S, L, block)
        torch.cuda.synchronize()
    healed = ecx.blocked_unpack(flat, S, n, L, b).cpu().numpy()
    for s in range(S):
        assert (healed[s] == (nat[s] if want_c[s] >= 0 else bad[s])).all(), s
