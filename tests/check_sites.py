"""Flip sites for the parity checks (tests/test_check_sites_cpu.py, tests/test_check_coverage.py):
where a single flipped bit must be seen by isParityCorrect and its batch, blocked, host-memory and
per-call forms, so that no byte, lane, wave, row, tile, chunk or unit of the reduction can drop a
mismatch unnoticed.

A site is (shard, byte, bit): `shards[shard][byte] ^= 1 << bit`, the byte counted from the start of
the shard's pitch (so the window [off, off + L) holds bytes off .. off + L - 1).  A site pool has one
stripe per site, stripe by stripe exactly that one flip, and a clean stripe after every 7 site
stripes; the expected verdict of a stripe is 0 exactly when its site lies inside the window.  The
unit rounds flip one bit per stripe and round so that over the rounds every (stripe, chunk unit,
tile) of a launch is the only unit that can see a flip exactly once.

Everything here is host-side numpy and the oracle; pools are built once per shape and never written."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O

CHUNK = 4096      # bytes of one shard a check workgroup covers (csrc/apply.hpp kChunkBytes)
TILE_ROWS = 8     # check rows per tile, one workgroup each (csrc/engine.hpp kTileRows)
BASES = 8         # distinct valid stripes a pool is tiled from
GROUP = 7         # site stripes between two clean stripes


# ---------------------------------------------------------------- sites
def outside_sites(n, off, L, pitch, shards=None):
    """Per shard one site just before and one just behind the window, where the pitch has them."""
    out = []
    for i in (range(n) if shards is None else shards):
        if off >= 1:
            out.append((i, off - 1, i % 8))
        if off + L < pitch:
            out.append((i, off + L, (i + 3) % 8))
    return out


def byte_sweep(n, off, L, pitch):
    """Every byte b of the window once, in shard b % n, with bit (b + b // 16) % 8: the sixteen bytes
    of a lane meet every bit, every lane, wave and chunk position is hit, the shards rotate.  Then
    the outside sites of every shard."""
    b = np.arange(L)
    sites = list(zip((b % n).tolist(), (off + b).tolist(), ((b + b // 16) % 8).tolist()))
    return sites + outside_sites(n, off, L, pitch)


def edge_positions(L):
    """Byte positions (window-relative) at the dword, lane, wave and chunk edges of a check launch
    over L bytes, and at the edges of the shifted window that covers a partial last chunk (8 and 11:
    with 0..4 and 15, every component of a lane's four dwords)."""
    F = L // CHUNK
    want = [0, 1, 3, 4, 8, 11, 15, 16, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, F * CHUNK - 1, F * CHUNK,
            L - CHUNK - 1, L - CHUNK, L - 17, L - 16, L - 1]
    return sorted({p for p in want if 0 <= p < L})


def edge_sweep(n, k, off, L, pitch, positions=None, shards=None):
    """Every shard (or those of `shards`) crossed with edge_positions(L) (or `positions`, clipped to
    the window); the bit rotates with the site index.  Then the outside sites of those shards."""
    pos = edge_positions(L) if positions is None else sorted({p for p in positions if 0 <= p < L})
    shards = list(range(n) if shards is None else shards)
    assert all(0 <= i < n for i in shards) and k < n
    sites = [(i, off + p) for i in shards for p in pos]
    return [(i, b, j % 8) for j, (i, b) in enumerate(sites)] + outside_sites(n, off, L, pitch, shards)


def inside(site, off, L):
    return off <= site[1] < off + L


# ---------------------------------------------------------------- pools
def stripe_of_site(j):
    """Pool stripe of site j: stripes 7, 15, 23, ... are the clean ones."""
    return j + j // GROUP


def pool_stripes(nsites):
    return nsites + -(-nsites // GROUP)


def valid_bases(k, m, off, L, pitch, seed, count=BASES):
    """`count` stripes [n][pitch] of random bytes -- pad bytes outside the window included -- whose
    parity over [off, off + L) is the oracle's encode_parity."""
    n = k + m
    rng = np.random.default_rng(seed)
    bases = rng.integers(0, 256, (count, n, pitch), dtype=np.uint8)
    rs = O.ReedSolomon(k, m)
    for b in range(count):
        rs.encode_parity([bases[b, i] for i in range(n)], off, L)
    return bases


def oracle_verdicts(k, m, pool, off, L):
    """The oracle's is_parity_correct(off, L) of every stripe of a [S][n][pitch] array (the C
    restatement releases the interpreter lock, so the stripes are spread over a few threads)."""
    S, n, _ = pool.shape
    rs = O.ReedSolomon(k, m)
    assert rs.is_parity_correct([np.zeros(1, np.uint8)] * n, 0, 1)  # the tables are built before the threads start

    def run(lo):
        return [int(rs.is_parity_correct([pool[s, i] for i in range(n)], off, L)) for s in range(lo, min(S, lo + 64))]

    with ThreadPoolExecutor(max_workers=8) as ex:
        parts = list(ex.map(run, range(0, S, 64)))
    return np.array([v for p in parts for v in p], np.uint8)


def site_pool(k, m, off, L, pitch, sites, seed):
    """(pool [S][n][pitch], expected verdicts [S], the oracle's verdicts [S]) of a site list."""
    n = k + m
    assert pitch >= off + L and all(0 <= i < n and 0 <= b < pitch and 0 <= bit < 8 for i, b, bit in sites)
    S = pool_stripes(len(sites))
    bases = valid_bases(k, m, off, L, pitch, seed)
    pool = bases[np.arange(S) % BASES]
    st = np.array([stripe_of_site(j) for j in range(len(sites))], np.int64)
    sh, by, bit = (np.array(x, np.int64) for x in zip(*sites))
    pool[st, sh, by] ^= (1 << bit).astype(np.uint8)
    want = np.ones(S, np.uint8)
    want[st[(by >= off) & (by < off + L)]] = 0
    got = oracle_verdicts(k, m, pool, off, L)
    for a in (pool, want, got):
        a.setflags(write=False)
    return pool, want, got


# ---------------------------------------------------------------- the shapes of the sweeps
# name -> (k, m, off, L, pitch, kind).  The byte sweeps are RS(4,2): a fused 16-B-multiple tail, a
# byte-safe tail, a firstByte off the 16-B grid on 16-B strides (byte-safe head, vector rest), odd
# strides (byte-safe only), and the first shape again without pad (the natural form of its blocked
# layout).  The edge sweeps: the 8-row instance; two tiles; a fused tail with 3 rows in the 4-row
# instance; RS(64,64)'s eight tiles in four pools of 32 shards each.
L_FUSED, L_RAGGED = CHUNK + 1040, CHUNK + 1001
POS_64 = (0, 1024, 4095, 4096, CHUNK + 16 - 1)
SWEEPS = {
    "byte_fused": (4, 2, 0, L_FUSED, L_FUSED + 16, "byte"),
    "byte_ragged": (4, 2, 0, L_RAGGED, -(-(L_RAGGED + 16) // 16) * 16, "byte"),
    "byte_head": (4, 2, 5, L_FUSED, -(-(5 + L_FUSED + 16) // 16) * 16, "byte"),
    "byte_odd": (4, 2, 3, 1001, 3 + 1001 + 7, "byte"),
    "byte_packed": (4, 2, 0, L_FUSED, L_FUSED, "byte"),
    "edge_5_5": (5, 5, 16, 2 * CHUNK + 48, 16 + 2 * CHUNK + 48 + 16, "edge"),
    "edge_10_10": (10, 10, 16, 2 * CHUNK + 48, 16 + 2 * CHUNK + 48 + 16, "edge"),
    "edge_17_3": (17, 3, 16, 2 * CHUNK + 3392, 16 + 2 * CHUNK + 3392 + 16, "edge"),
    "edge_packed_10_10": (10, 10, 0, 2 * CHUNK + 48, 2 * CHUNK + 48, "edge"),
    "edge_64_64_a": (64, 64, 0, CHUNK + 16, CHUNK + 32, "edge64:0"),
    "edge_64_64_b": (64, 64, 0, CHUNK + 16, CHUNK + 32, "edge64:32"),
    "edge_64_64_c": (64, 64, 0, CHUNK + 16, CHUNK + 32, "edge64:64"),
    "edge_64_64_d": (64, 64, 0, CHUNK + 16, CHUNK + 32, "edge64:96"),
}


def sweep_sites(name):
    k, m, off, L, pitch, kind = SWEEPS[name]
    n = k + m
    if kind == "byte":
        return byte_sweep(n, off, L, pitch)
    if kind == "edge":
        return edge_sweep(n, k, off, L, pitch)
    first = int(kind.split(":")[1])
    return edge_sweep(n, k, off, L, pitch, POS_64, range(first, first + 32))


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """(k, m, off, L, pitch, sites, pool, expected, oracle's) of a named sweep.  Shared: read-only."""
    k, m, off, L, pitch, _ = SWEEPS[name]
    sites = sweep_sites(name)
    pool, want, orc = site_pool(k, m, off, L, pitch, sites, 9100 + 97 * k + L + off)
    return k, m, off, L, pitch, sites, pool, want, orc


COUNT_WRAP = 4096 * 256  # threads of k_count_mismatch's grid (csrc/kernels.hip): its stride over the m * L syndrome bytes


def percall_sites(n, k, off, L):
    """Sites for the per-call checks (one call per site): an eighth of the edge sweep -- every shard
    and every position still appear, at most 64 sites --, then bytes 255 and 256 of two parity
    shards, the bytes around COUNT_WRAP of the concatenated check rows where m * L reaches it, and
    the two outside-window sites of data shard 0 and of the last parity shard."""
    pos = edge_positions(L)
    picked = [(i, off + p) for i in range(n) for q, p in enumerate(pos) if (i + q) % 8 == 0]
    assert len(picked) <= 64 and {i for i, _ in picked} == set(range(n)) and {b - off for _, b in picked} == set(pos)
    extra = [(k, off + 255), (k + 1, off + 256)]
    row, col = divmod(COUNT_WRAP, L)
    if row < n - k:
        extra += [(k + row, off + col + d) for d in (-1, 0, 1)]
    extra += [(0, off - 1), (0, off + L), (n - 1, off - 1), (n - 1, off + L)]
    return [(i, b, j % 8) for j, (i, b) in enumerate(picked + extra)]


def site_arrays(sites):
    """(pool stripe, shard, byte, xor mask) of every site, as arrays."""
    st = np.array([stripe_of_site(j) for j in range(len(sites))], np.int64)
    sh, by, bit = (np.array(x, np.int64) for x in zip(*sites))
    return st, sh, by, (1 << bit).astype(np.uint8)


def without_flips(pool, sites):
    """A writable copy of a site pool with every flip taken back: the valid stripes."""
    st, sh, by, mask = site_arrays(sites)
    clean = pool.copy()
    clean[st, sh, by] ^= mask
    return clean


# ---------------------------------------------------------------- the blocked layout
def packed_offsets(n, nstripes, L, block, stripe, shard, byte):
    """Where the blocked layout (include/ecx.h: body [stripe][block row][shard][block], then tails
    [stripe][shard][L % block]) keeps byte `byte` of shard `shard` of stripe `stripe` (arrays)."""
    stripe, shard, byte = (np.asarray(x, np.int64) for x in (stripe, shard, byte))
    full, tail = divmod(L, block)
    body = full * n * block
    in_body = byte < full * block
    a = stripe * body + (byte // block) * n * block + shard * block + byte % block
    b = nstripes * body + stripe * n * tail + shard * tail + (byte - full * block)
    return np.where(in_body, a, b)


def pack_natural(nat, block):
    """The blocked layout of a natural [S][n][L] array, restated with numpy (no library call)."""
    S, n, L = nat.shape
    full, tail = divmod(L, block)
    body = nat[:, :, :full * block].reshape(S, n, full, block).transpose(0, 2, 1, 3).reshape(-1)
    return np.concatenate([body, nat[:, :, full * block:].reshape(-1)])


# ---------------------------------------------------------------- tiles
def greedy_row_order(matrix):
    """The planner's grouping of a map's rows into tiles of eight (csrc/engine.cpp group_rows),
    restated: seed a tile with the lowest unassigned row, then keep adding the row that maximises
    shared - new inputs, the first such row on ties."""
    a = np.asarray(matrix) != 0
    n_out = a.shape[0]
    if n_out <= TILE_ROWS:
        return list(range(n_out))
    used, order = [False] * n_out, []
    for seed in range(n_out):
        if used[seed]:
            continue
        tile, in_tile = [seed], a[seed].copy()
        used[seed] = True
        while len(tile) < TILE_ROWS:
            best, score = -1, 0
            for r in range(n_out):
                if used[r]:
                    continue
                shared = int((a[r] & in_tile).sum())
                sc = shared - (int(a[r].sum()) - shared)
                if best < 0 or sc > score:
                    best, score = r, sc
            if best < 0:
                break
            used[best] = True
            tile.append(best)
            in_tile |= a[best]
        order += tile
    return order


def check_matrix(k, m):
    """The check map of RS(k, m): row p = [parity row p | unit vector p] over (data, parity)."""
    return np.concatenate([O.ReedSolomon(k, m).parity_rows, np.eye(m, dtype=np.uint8)], axis=1)


def tile_of_parity_row(k, m):
    """tile[p] of parity row p under the planner's grouping of the check map."""
    order = greedy_row_order(check_matrix(k, m))
    tile = [0] * m
    for pos, row in enumerate(order):
        tile[row] = pos // TILE_ROWS
    return tile


# ---------------------------------------------------------------- unit probes
def unit_counts(m, L):
    """(C chunk units per stripe -- full chunks plus the tail unit --, T tiles)."""
    return L // CHUNK + (1 if L % CHUNK else 0), -(-m // TILE_ROWS)


def unit_rounds(k, m, off, L, S):
    """C * T + 1 rounds over S stripes: rounds[r][s] is the site (shard, byte, bit) of stripe s in
    round r, or None for a stripe that stays clean in that round, and units[r][s] the unit (c, t) it
    probes.  In round r stripe s probes the unit with c * T + t == (r + s) % (C * T + 1); the value
    C * T is the clean one.  A probe of (c, t) lies in a parity shard whose check row belongs to tile
    t, at a byte of chunk c that no other chunk unit reads: below L - 4096 in the last full chunk
    (the shifted window of a fused tail starts there), at or behind F * 4096 in the tail unit.  The
    lane and the byte in the lane rotate with s, the row in the tile and the bit with r + s."""
    F, tail = divmod(L, CHUNK)
    C, T = unit_counts(m, L)
    tile = tile_of_parity_row(k, m)
    assert tile == [p // TILE_ROWS for p in range(m)], "rows 8t .. 8t+7 of the check map form tile t"
    P = C * T + 1
    rounds, units = [], []
    seen = {}
    for r in range(P):
        row_sites, row_units = [], []
        for s in range(S):
            v = (r + s) % P
            if v == C * T:
                row_sites.append(None)
                row_units.append(None)
                continue
            c, t = divmod(v, T)
            rows = [p for p in range(m) if tile[p] == t]
            p = rows[(r + s) % len(rows)]
            limit = tail if (tail and c >= F - 1) else CHUNK
            rel = (16 * ((37 * s) % 256) + s % 16) % limit
            byte = c * CHUNK + rel
            assert 0 <= byte < L and byte // CHUNK == c
            if tail and c == F - 1:
                assert byte < L - CHUNK
            if c == F:
                assert byte >= F * CHUNK
            row_sites.append((k + p, off + byte, (r + s) % 8))
            row_units.append((c, t))
            seen[(s, c, t)] = seen.get((s, c, t), 0) + 1
        rounds.append(row_sites)
        units.append(row_units)
    assert seen == {(s, c, t): 1 for s in range(S) for c in range(C) for t in range(T)}, "every unit probed once"
    return rounds, units


def boundary_round(k, m, off, L, S, block):
    """One more round for the blocked layout: stripe s with s % 3 == 0 carries a flip in the last
    byte of its last block row, the next stripe one in byte 0 of its first block row, the third
    stays clean -- neighbours in the body pass, where a unit charged to the wrong stripe shows."""
    full = L // block
    assert full >= 1
    n = k + m
    return [(n - 1, off + full * block - 1, s % 8) if s % 3 == 0 else ((k, off, s % 8) if s % 3 == 1 else None)
            for s in range(S)]


@functools.lru_cache(maxsize=None)
def unit_case(k, m, off, L, pitch, S, block=0):
    """(clean stripes [S][n][pitch], rounds, units, expected [R][S], the oracle's [R][S]) of the unit
    probes of a shape; with `block` the blocked layout's boundary round is appended.  Read-only."""
    n = k + m
    clean = valid_bases(k, m, off, L, pitch, 9900 + 97 * k + L + pitch, count=S)
    rounds, units = unit_rounds(k, m, off, L, S)
    if block:
        rounds = rounds + [boundary_round(k, m, off, L, S, block)]
        units = units + [[None] * S]
    want = np.array([[0 if site is not None else 1 for site in rnd] for rnd in rounds], np.uint8)
    orc = []
    for rnd in rounds:
        flipped = apply_round(clean.copy(), rnd)
        orc.append(oracle_verdicts(k, m, flipped, off, L))
    orc = np.stack(orc)
    assert oracle_verdicts(k, m, clean, off, L).all()
    for a in (clean, want, orc):
        a.setflags(write=False)
    return clean, rounds, units, want, orc


def round_indices(rnd, n, pitch):
    """(flat byte offsets into a [S][n][pitch] array, xor masks) of a round's flips."""
    idx = [(s * n + site[0]) * pitch + site[1] for s, site in enumerate(rnd) if site is not None]
    val = [1 << site[2] for site in rnd if site is not None]
    return np.array(idx, np.int64), np.array(val, np.uint8)


def apply_round(pool, rnd):
    S, n, pitch = pool.shape
    idx, val = round_indices(rnd, n, pitch)
    pool.reshape(-1)[idx] ^= val
    return pool
