"""Shared cases of the blocked and the host-memory mixed decode tests (tests/test_mixed_blocked.py,
tests/test_mixed_blocked_capture.py, tests/test_mixed_host.py): the pattern set, the stripes' ids,
and per shape the input stripes and the oracle's result, computed once and never written.

The stripes are fill_random bytes, not codewords (as tests/test_mixed_decode.py), so a rebuilt
shard equals the oracle's only if exactly the shards the reference reads were read."""
import functools

import numpy as np

import oracle as O

S = 9
# pattern id of each stripe: unsorted, neighbours always differ (a wrong unit -> stripe mapping
# decodes with the wrong pattern); 255 names no pattern
IDS = [3, 255, 5, 0, 6, 1, 4, 2, 0]
# (k, m, byte_count, block_bytes); 0 = the recommended block
SHAPES = [
    (17, 3, 200000, 0),            # 6 x 32 KiB plus a 3,392-B tail
    (12, 4, 3 * 65536 + 4096, 0),  # full blocks plus a 4 KiB tail
    (12, 4, 3 * 65536, 0),         # no tail
    (4, 2, 104449, 4096),          # 25 blocks plus an odd 2,049-B tail
    (5, 5, 1001, 64),              # 8-row instances, byte-safe body
    (3, 1, 34, 0),                 # one block, divisor 1
    (4, 2, 100, 4096),             # full == 0, tail only
]


def patterns_of(k, m):
    """nothing missing; one data shard; one parity shard; two shards where m >= 2 (else another
    data shard), twice; m missing (data and parity); the first two-shard pattern a second time.
    No pattern misses more than m."""
    n = k + m

    def missing(*idx):
        p = np.ones(n, np.uint8)
        p[list(idx)] = 0
        return p

    m_missing = list(range(1, 1 + (m + 1) // 2)) + list(range(n - m // 2, n))
    assert len(m_missing) == m
    two = missing(0, k - 1) if m >= 2 else missing(0)
    mixed_two = missing(2, n - 1) if m >= 2 else missing(2 % k)
    pats = np.stack([missing(), missing(1), missing(k), two, mixed_two, missing(*m_missing), two])
    assert ((pats == 0).sum(axis=1) <= m).all()
    return pats


def block_of(ecx, k, m, L, block):
    return block if block else ecx.ReedSolomon.create(k, m).blockedLayout(L)[0]


def decode_by_oracle(k, m, before, pats, ids, off, cnt):
    """The oracle's decodeMissing per stripe of the natural [S][n][pitch] array `before`."""
    want = before.copy()
    orc = O.ReedSolomon(k, m)
    n = k + m
    for s, pid in enumerate(ids):
        if pid >= len(pats):
            continue
        shards = [want[s, i].copy() for i in range(n)]
        orc.decode_missing(shards, [bool(f) for f in pats[pid]], off, cnt)
        for i in range(n):
            want[s, i] = shards[i]
    return want


@functools.lru_cache(maxsize=None)
def oracle_case(k, m, L):
    """(input stripes, expected stripes), natural [S][n][L] host arrays, for IDS over patterns_of."""
    import torch
    import rpamd
    ecx = rpamd.load(shape_knobs=True)
    pool = torch.empty((S, k + m, L), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 8100 + 31 * k + L)
    torch.cuda.synchronize()
    before = pool.cpu().numpy()
    want = decode_by_oracle(k, m, before, patterns_of(k, m), IDS, 0, L)
    before.setflags(write=False)
    want.setflags(write=False)
    return before, want


def pack(ecx, natural, block):
    """blocked_pack of a natural host array, as a flat numpy array."""
    import torch
    return ecx.blocked_pack(torch.from_numpy(natural.copy()), block).numpy()
