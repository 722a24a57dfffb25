"""Shared cases of the two-shard locate tests (tests/test_locate2*.py).  Every expected value is the
oracle's brute force, an extension of locate_cases.oracle_locate, and nothing is computed by the code
under test: shard j is a single suspect as there; the pair {i, j} is a suspect of a stripe when the
stripe with both shards zeroed and rebuilt by the oracle's decodeMissing (both absent) passes the
oracle's isParityCorrect over the window."""
import functools
import itertools

import numpy as np

import oracle as O
from locate_cases import CHUNK, GUARD, PAIR_VALUES, oracle_locate, valid_stripes

SPAN = 1024  # one wave: 64 lanes x 16 B

# (k, m, L, first byte, byte count, shard pitch) of tests/test_locate2.py.  The pitch is L + 16 (room
# for the flip just past the window) except RS(3,5)'s, L + 28, a multiple of 16: the unaligned-start
# split is only taken over 16-B strides.  RS(4,4)'s L + 16 is no multiple of 16: byte-safe throughout.
SHAPES = [(2, 4, 2 * 4096 + 208, 0, 2 * 4096 + 208, 2 * 4096 + 208 + 16),
          (2, 4, 208, 0, 208, 208 + 16),
          (12, 4, 4096 + 48, 0, 4096 + 48, 4096 + 48 + 16),
          (3, 5, 2 * 4096 + 100, 3, 2 * 4096 + 100 - 3, 2 * 4096 + 100 + 28),
          (2, 8, 4096 + 16, 0, 4096 + 16, 4096 + 16 + 16),
          (4, 4, 4096 + 1000, 0, 4096 + 1000, 4096 + 1000 + 16)]
S = 14


def pairs_of(n):
    """The C(n,2) pairs in lexicographic order: pair p of the suspect row and of doubleLossPatternSet."""
    return list(itertools.combinations(range(n), 2))


def oracle_locate2(rs, stripe, first, count):
    """(suspects [n + C(n,2)], (culprit0, culprit1), heal id) of one stripe over [first, first + count)."""
    n = stripe.shape[0]
    singles, _, _ = oracle_locate(rs, stripe, first, count)
    pairs = []
    for i, j in pairs_of(n):
        shards = [stripe[x].copy() for x in range(n)]
        shards[i][:] = 0
        shards[j][:] = 0
        rs.decode_missing(shards, [x not in (i, j) for x in range(n)], first, count)
        pairs.append(int(rs.is_parity_correct(shards, first, count)))
    if sum(singles) == n:
        culprit, heal = (-1, -1), 255
    elif sum(singles) == 1:
        culprit, heal = (singles.index(1), -1), singles.index(1)
    elif sum(singles) == 0 and sum(pairs) == 1:
        culprit, heal = pairs_of(n)[pairs.index(1)], n + pairs.index(1)
    else:
        culprit, heal = (-2, -2), 255
    return singles + pairs, culprit, heal


def expectations2(k, m, bad, first, count):
    """The oracle's (suspect [S][n + C(n,2)], culprit [S][2], heal id [S]) for bad[S][n][bytes]."""
    rs = O.ReedSolomon(k, m)
    got = [oracle_locate2(rs, bad[s], first, count) for s in range(bad.shape[0])]
    return (np.array([g[0] for g in got], np.uint8), np.array([g[1] for g in got], np.int32),
            np.array([g[2] for g in got], np.int64))


def fourteen_flips(k, m, first, count):
    """(stripe, shard, byte) of the flips of the fourteen-stripe case over [first, first + count) of
    shards with at least one more byte past the window.  Stripes 0 (clean) and 13 (random) have none."""
    n = k + m
    last = first + count - 1
    chunks = count > CHUNK + 64
    other_wave = first + SPAN + 10 if count > SPAN + 64 else last - 9
    other_chunk = first + CHUNK + 20 if chunks else last - 3
    partial = first + (count // CHUNK) * CHUNK + 1 if chunks and count % CHUNK else last - 1
    return [(1, 0, first),                                     # one flip at the window's first byte
            (2, n - 1, last),                                  # and at its last: the shortcut path
            (3, 0, first + 5), (3, 1, first + 5),              # data-data at one byte: the pair tiles
            (4, k - 1, first + 77), (4, k, first + 77),        # data-parity
            (5, k, last - 40), (5, n - 1, last - 40),          # parity-parity
            (6, 1, first + 100), (6, k + 1, first + 200),      # different bytes of one 1 KiB wave span
            (7, 0, first + 10), (7, n - 2, other_wave),        # different waves of one chunk
            (8, 1, first + 20), (8, k + 2, other_chunk),       # different chunks: two shortcut waves
            (9, 0, first + 30), (9, k, first + 31),            # the same two shards in two chunks
            (9, 0, other_chunk), (9, k, other_chunk + 1),
            (10, 0, first + 30), (10, n - 2, partial),         # one flip in the partial last chunk
            (11, 0, first + 40), (11, k, first + 41), (11, n - 1, first + 42),  # three shards
            (12, 2 % n, first + count)] + ([(12, k, first - 1)] if first > 0 else [])  # outside the window


@functools.lru_cache(maxsize=None)
def fourteen_stripes(k, m, L, first, count, P):
    """The fourteen stripes of tests/test_locate2.py as [14][n][P] arrays: the valid stripes, the same
    with the flips applied and stripe 13 random, the oracle's expectations over the window, and the
    flips.  Shared: do not write."""
    n = k + m
    nat = valid_stripes(k, m, S, P, 9200 + 37 * k + L)
    bad = nat.copy()
    flips = fourteen_flips(k, m, first, count)
    for s, i, byte in flips:
        bad[s, i, byte] ^= 0x81
    bad[13] = np.random.default_rng(9250 + k).integers(0, 256, (n, P), dtype=np.uint8)
    want = expectations2(k, m, bad, first, count)
    for a in (nat, bad) + want:
        a.setflags(write=False)
    return nat, bad, want, flips


def kinds(want_c):
    """(stripes whose culprit is a single shard, a pair, nobody) of a culprit array [S][2]."""
    single = int(((want_c[:, 0] >= 0) & (want_c[:, 1] == -1)).sum())
    pair = int(((want_c[:, 0] >= 0) & (want_c[:, 1] >= 0)).sum())
    return single, pair, int((want_c[:, 0] == -2).sum())


@functools.lru_cache(maxsize=None)
def every_pair(k, m, L):
    """One stripe per (pair of shards, PAIR_VALUES entry), both shards corrupt at one byte: 45 stripes
    for RS(2,4) (15 pairs x 3 pairs of error values)."""
    n = k + m
    cases = [(i, j, v) for i, j in pairs_of(n) for v in PAIR_VALUES]
    nat = valid_stripes(k, m, len(cases), L, 9400 + k)
    bad = nat.copy()
    for s, (i, j, (vi, vj)) in enumerate(cases):
        byte = (97 * s) % L
        bad[s, i, byte] ^= vi
        bad[s, j, byte] ^= vj
    want = expectations2(k, m, bad, 0, L)
    for a in (nat, bad) + want:
        a.setflags(write=False)
    return nat, bad, want, cases


TRIPLE_VALUES = (0x01, 0x81, 0x3C)


@functools.lru_cache(maxsize=None)
def every_triple(k, m, L):
    """One stripe per triple of shards (20 for RS(2,4)), all three corrupt at one byte by
    TRIPLE_VALUES.  The expectations are the oracle's, whatever they are: a triple may name a pair of
    other shards."""
    n = k + m
    cases = list(itertools.combinations(range(n), 3))
    nat = valid_stripes(k, m, len(cases), L, 9450 + k)
    bad = nat.copy()
    for s, tri in enumerate(cases):
        for x, v in zip(tri, TRIPLE_VALUES):
            bad[s, x, (53 * s) % L] ^= v
    want = expectations2(k, m, bad, 0, L)
    for a in (nat, bad) + want:
        a.setflags(write=False)
    return nat, bad, want, cases


def run_locate2(torch, call, nstripes, width, heal=True):
    """call(suspect, culprit, heal or None) on guarded device outputs; (suspect [S][width], culprit
    [S][2], heal ids or None, the device heal ids) after asserting that the bytes after each are kept."""
    suspect = torch.full((nstripes * width + 16,), GUARD, dtype=torch.uint8, device="cuda")
    culprit = torch.full((2 * nstripes + 4,), -77, dtype=torch.int32, device="cuda")
    heal_id = torch.full((nstripes + 16,), GUARD, dtype=torch.uint8, device="cuda") if heal else None
    call(suspect, culprit, heal_id)
    torch.cuda.synchronize()
    su, cu = suspect.cpu().numpy(), culprit.cpu().numpy()
    assert (su[nstripes * width:] == GUARD).all() and (cu[2 * nstripes:] == -77).all()
    he = None
    if heal:
        he = heal_id.cpu().numpy()
        assert (he[nstripes:] == GUARD).all()
        he = he[:nstripes]
    return su[:nstripes * width].reshape(nstripes, width), cu[:2 * nstripes].reshape(nstripes, 2), he, heal_id
