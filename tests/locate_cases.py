"""Shared cases of the corrupt-shard locate tests (tests/test_locate*.py).  Every expected value is
the oracle's brute force and nothing is computed by the code under test: shard j is a suspect of a
stripe when the stripe with shard j zeroed and rebuilt by the oracle's decodeMissing (j absent)
passes the oracle's isParityCorrect over the window."""
import functools

import numpy as np

import oracle as O

GUARD = 0xA5
CHUNK = 4096


def oracle_locate(rs, stripe, first, count):
    """(suspects, culprit, heal id) of one stripe ([n][bytes] array) over [first, first + count)."""
    n = stripe.shape[0]
    suspects = []
    for j in range(n):
        shards = [stripe[i].copy() for i in range(n)]
        shards[j][:] = 0
        rs.decode_missing(shards, [i != j for i in range(n)], first, count)
        suspects.append(int(rs.is_parity_correct(shards, first, count)))
    c = sum(suspects)
    culprit = -1 if c == n else (suspects.index(1) if c == 1 else -2)
    return suspects, culprit, culprit if culprit >= 0 else 255


def expectations(k, m, bad, first, count):
    """The oracle's (suspect [S][n], culprit [S], heal id [S]) for the stripes bad[S][n][bytes]."""
    rs = O.ReedSolomon(k, m)
    got = [oracle_locate(rs, bad[s], first, count) for s in range(bad.shape[0])]
    return (np.array([g[0] for g in got], np.uint8), np.array([g[1] for g in got], np.int32),
            np.array([g[2] for g in got], np.uint8))


def valid_stripes(k, m, nstripes, nbytes, seed):
    """nstripes codewords [nstripes][n][nbytes] by the oracle's encodeParity."""
    n = k + m
    rng = np.random.default_rng(seed)
    nat = np.zeros((nstripes, n, nbytes), np.uint8)
    nat[:, :k] = rng.integers(0, 256, (nstripes, k, nbytes), dtype=np.uint8)
    rs = O.ReedSolomon(k, m)
    for s in range(nstripes):
        rs.encode_parity([nat[s, i] for i in range(n)], 0, nbytes)
    return nat


def nine_flips(k, m, first, count):
    """(stripe, shard, byte) of the flips of the nine-stripe case over the window [first, first +
    count) of shards that have at least one more byte on each side the window leaves out."""
    n = k + m
    last = first + count - 1
    flips = [(1, 0, first),            # byte 0 of data shard 0
             (2, n - 1, last)]         # the last byte of the last parity shard: the last of the batch
    if count % CHUNK and count > CHUNK:
        flips.append((3, k - 1, first + (count // CHUNK) * CHUNK))  # byte 0 of the partial last chunk
    far = first + CHUNK + 7 if count > CHUNK + 7 else last - 1
    flips += [(5, k, first + 5), (5, k, far)]                       # one shard, two chunks
    flips += [(6, 1, first + 9), (6, n - 2, far)]                   # two shards, two chunks
    flips.append((7, 2, first + count))                             # just past the window
    if first > 0:
        flips.append((7, k, first - 1))                             # and just before it
    return flips


@functools.lru_cache(maxsize=None)
def nine_stripes(k, m, L, first, count):
    """The nine stripes of tests/test_locate.py as [9][n][L + 16] arrays (the 16 bytes after a
    shard's L belong to no window: room for the flip just outside it): the valid stripes, the same
    with the flips applied and stripe 8 random, the oracle's expectations over [first, first + count),
    and the flips.  Shared: do not write."""
    n, P = k + m, L + 16
    nat = valid_stripes(k, m, 9, P, 9000 + 37 * k + L)
    bad = nat.copy()
    flips = nine_flips(k, m, first, count)
    for s, i, byte in flips:
        bad[s, i, byte] ^= 0x81
    bad[8] = np.random.default_rng(9100 + k).integers(0, 256, (n, P), dtype=np.uint8)
    want = expectations(k, m, bad, first, count)
    for a in (nat, bad) + want:
        a.setflags(write=False)
    return nat, bad, want, flips


# the error values of the same-byte double corruptions: three pairs per pair of shards
PAIR_VALUES = ((0x01, 0x01), (0x81, 0x3C), (0xFF, 0x02))


@functools.lru_cache(maxsize=None)
def same_byte_pairs(k, m, L):
    """One stripe per (pair of shards, pair of error values): both shards corrupt at the SAME byte
    (45 stripes for RS(4,2), 30 for RS(3,2)).  With m = 2 such a stripe may name a third shard; the
    expectations are the oracle's, whatever they are."""
    n = k + m
    pairs = [(i, j, v) for i in range(n) for j in range(i + 1, n) for v in PAIR_VALUES]
    nat = valid_stripes(k, m, len(pairs), L, 9300 + k)
    bad = nat.copy()
    for s, (i, j, (vi, vj)) in enumerate(pairs):
        byte = (7 * s) % L
        bad[s, i, byte] ^= vi
        bad[s, j, byte] ^= vj
    want = expectations(k, m, bad, 0, L)
    for a in (nat, bad) + want:
        a.setflags(write=False)
    return nat, bad, want


def run_locate(torch, call, nstripes, n, heal=True):
    """call(suspect, culprit, heal or None) on guarded device outputs; the three results as numpy
    arrays (heal None when not asked for) after asserting that the 16 bytes after each are kept."""
    suspect = torch.full((nstripes * n + 16,), GUARD, dtype=torch.uint8, device="cuda")
    culprit = torch.full((nstripes + 4,), -77, dtype=torch.int32, device="cuda")
    heal_id = torch.full((nstripes + 16,), GUARD, dtype=torch.uint8, device="cuda") if heal else None
    call(suspect, culprit, heal_id)
    torch.cuda.synchronize()
    su, cu = suspect.cpu().numpy(), culprit.cpu().numpy()
    assert (su[nstripes * n:] == GUARD).all() and (cu[nstripes:] == -77).all()
    he = None
    if heal:
        he = heal_id.cpu().numpy()
        assert (he[nstripes:] == GUARD).all()
        he = he[:nstripes]
    return su[:nstripes * n].reshape(nstripes, n), cu[:nstripes], he, heal_id
