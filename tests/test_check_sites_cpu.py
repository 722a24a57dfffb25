"""tests/check_sites.py against the oracle, without a GPU: for every shape tests/test_check_coverage.py
runs, the expected verdicts of the site pools equal the oracle's is_parity_correct stripe by stripe,
the unit rounds probe every (stripe, chunk unit, tile) exactly once, and the packed offsets of the
blocked form put each flip where blocked_unpack finds it."""
import numpy as np
import pytest

import check_sites as CS
import oracle as O
from test_blocked_check import packed_offset

# (k, m, off, L, pitch, S, block) of the unit probes (test_check_coverage.py UNIT_SHAPES)
UNIT_SHAPES = [(10, 10, 0, 2 * 4096 + 48, 2 * 4096 + 48 + 16, 23, 0),
               (4, 2, 0, 5 * 4096 + 1040, 5 * 4096 + 1040 + 16, 37, 0),
               (4, 2, 0, 5 * 4096 + 1040, 169 * 128, 37, 0),
               (4, 2, 0, 5 * 4096 + 1040, 5 * 4096 + 1040, 37, 4096)]


@pytest.mark.parametrize("name", sorted(CS.SWEEPS))
def test_site_pool_expectation_is_the_oracles(name):
    """Stripe by stripe the expected verdict (0 exactly when the stripe's site lies inside the
    window) is the oracle's; the clean stripes and the outside-window sites pass; each site stripe
    differs from its valid base in exactly one bit, the clean stripes in none."""
    k, m, off, L, pitch, sites, pool, want, orc = CS.sweep_case(name)
    n = k + m
    S = pool.shape[0]
    assert S == CS.pool_stripes(len(sites)) and pool.shape == (S, n, pitch)
    assert (want == orc).all(), np.nonzero(want != orc)[0][:10]
    st = np.array([CS.stripe_of_site(j) for j in range(len(sites))])
    ins = np.array([CS.inside(x, off, L) for x in sites])
    assert (want[st[ins]] == 0).all() and (want[st[~ins]] == 1).all()
    clean = np.setdiff1d(np.arange(S), st)
    assert len(clean) == S - len(sites) and (clean % 8 == 7).sum() >= len(clean) - 1 and (want[clean] == 1).all()
    assert int((want == 0).sum()) == int(ins.sum())
    kind = CS.SWEEPS[name][5]
    if kind == "byte":  # every byte of the window once, every bit in every lane's 16 bytes
        inside = [x for x in sites if CS.inside(x, off, L)]
        assert sorted(b for _, b, _ in inside) == list(range(off, off + L))
        assert {(b - off) % n for _, b, _ in inside} == {i for i, _, _ in inside}
        if L >= 256:
            bits = {((b - off) % 16, bit) for _, b, bit in inside if (b - off) < 256}
            assert bits == {(j, bit) for j in range(16) for bit in range(8)}
    else:           # every shard of the pool's range at every position
        shards = {i for i, _, _ in sites}
        pos = {b - off for _, b, _ in sites if CS.inside((0, b, 0), off, L)}
        assert {(i, b - off) for i, b, _ in sites if CS.inside((0, b, 0), off, L)} == {(i, p) for i in shards for p in pos}
        assert len({bit for _, _, bit in sites}) == 8
    # one bit per site stripe against the bases the pool is tiled from
    bases = CS.valid_bases(k, m, off, L, pitch, 9100 + 97 * k + L + off)
    diff = pool ^ bases[np.arange(S) % CS.BASES]
    changed = np.count_nonzero(diff.reshape(S, -1), axis=1)   # bytes that differ, and the one that does
    mask = diff.reshape(S, -1).max(axis=1)
    assert (changed[st] == 1).all() and (changed[clean] == 0).all()
    assert np.isin(mask[st], [1, 2, 4, 8, 16, 32, 64, 128]).all()
    for j in (0, len(sites) // 2, len(sites) - 1):
        i, b, bit = sites[j]
        assert diff[CS.stripe_of_site(j), i, b] == 1 << bit


def test_the_64_64_pools_cover_every_shard():
    shards = set()
    for name in ("edge_64_64_a", "edge_64_64_b", "edge_64_64_c", "edge_64_64_d"):
        shards |= {i for i, _, _ in CS.sweep_sites(name)}
    assert shards == set(range(128))


def test_edge_positions():
    L = 2 * 4096 + 48
    assert CS.edge_positions(L) == [0, 1, 3, 4, 8, 11, 15, 16, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, 4143, 4144,
                                    8191, 8192, L - 17, L - 16, L - 1]
    assert CS.edge_positions(100) == [0, 1, 3, 4, 8, 11, 15, 16, 83, 84, 99]
    assert {p % 16 // 4 for p in CS.edge_positions(L)} == {0, 1, 2, 3}


@pytest.mark.parametrize("k,m", [(4, 2), (5, 5), (10, 10), (17, 3), (64, 64)])
def test_check_rows_tile_in_order(ecx, k, m):
    """Rows 8t .. 8t+7 of the RS check map form tile t under the planner's grouping (restated in
    check_sites.greedy_row_order), and the library's plan of the code's m-row encode map has that
    many tiles."""
    assert CS.tile_of_parity_row(k, m) == [p // 8 for p in range(m)]
    assert (CS.check_matrix(k, m)[:, :k] == ecx.ReedSolomon.create(k, m).parityRows).all()
    stats = ecx.ReedSolomon.create(k, m).encode_map().plan_stats()
    assert stats["tiles"] == -(-m // 8), stats
    # a map whose rows do not share inputs in index order is regrouped: the restatement is not the identity
    scattered = np.zeros((16, 16), np.uint8)
    for r in range(16):
        scattered[r, (r % 2) * 8:(r % 2) * 8 + 8] = 1
    order = CS.greedy_row_order(scattered)
    assert sorted(order) == list(range(16)) and order[:8] == list(range(0, 16, 2))


@pytest.mark.parametrize("k,m,off,L,pitch,S,block", UNIT_SHAPES)
def test_unit_rounds_probe_every_unit_once(k, m, off, L, pitch, S, block):
    """C * T + 1 rounds; over them every (stripe, chunk unit, tile) carries exactly one flip, in a
    parity shard of that tile, at a byte only that chunk unit reads; each round's expectation is the
    oracle's; a stripe is clean exactly once."""
    clean, rounds, units, want, orc = CS.unit_case(k, m, off, L, pitch, S, block)
    C, T = CS.unit_counts(m, L)
    F = L // 4096
    assert len(rounds) == C * T + 1 + (1 if block else 0)
    assert (want == orc).all()
    seen = {}
    for r in range(C * T + 1):
        for s in range(S):
            site, unit = rounds[r][s], units[r][s]
            assert (site is None) == (unit is None) == ((r + s) % (C * T + 1) == C * T)
            if site is None:
                continue
            c, t = unit
            assert c * T + t == (r + s) % (C * T + 1)
            shard, byte, bit = site
            assert k <= shard < k + m and (shard - k) // 8 == t
            rel = byte - off
            assert rel // 4096 == c
            if L % 4096 and c == F - 1:
                assert rel < L - 4096
            if c == F:
                assert rel >= F * 4096
            seen[(s, c, t)] = seen.get((s, c, t), 0) + 1
    assert seen == {(s, c, t): 1 for s in range(S) for c in range(C) for t in range(T)}
    assert ((want[:C * T + 1] == 1).sum(axis=0) == 1).all()
    assert len({(site[1] - off) % 4096 // 16 for site in rounds[0] if site}) > min(S, 12) // 2  # the lanes rotate
    if block:
        last = rounds[-1]
        assert last[0] == (k + m - 1, off + (L // block) * block - 1, 0) and last[1] == (k, off, 1) and last[2] is None
        assert want[-1].tolist() == [0 if s % 3 != 2 else 1 for s in range(S)]


def test_packed_offsets_match_blocked_unpack(ecx):
    """The RS(4,2) byte sweep and the RS(10,10) edge sweep at block 4096, and the blocked unit
    rounds: a valid pool packed, each flip applied at packed_offsets -- which agrees with
    tests/test_blocked_check.py packed_offset --, unpacks (blocked_unpack) to the natural pool with
    the same flips; pack_natural is blocked_pack."""
    import torch
    block = 4096
    for name in ("byte_packed", "edge_packed_10_10"):
        k, m, off, L, pitch, sites, pool, want, orc = CS.sweep_case(name)
        n = k + m
        S = pool.shape[0]
        assert off == 0 and pitch == L
        bases = CS.valid_bases(k, m, off, L, pitch, 9100 + 97 * k + L + off)
        packed = CS.pack_natural(bases[np.arange(S) % CS.BASES], block)
        assert (packed == ecx.blocked_pack(torch.from_numpy(bases[np.arange(S) % CS.BASES]), block).numpy()).all()
        st = np.array([CS.stripe_of_site(j) for j in range(len(sites))])
        sh, by, bit = (np.array(x) for x in zip(*sites))
        at = CS.packed_offsets(n, S, L, block, st, sh, by)
        assert len(set(at.tolist())) == len(at)
        for j in range(0, len(sites), max(1, len(sites) // 97)):
            assert at[j] == packed_offset(n, S, L, block, int(st[j]), int(sh[j]), int(by[j]))
        packed[at] ^= (1 << bit).astype(np.uint8)
        nat = ecx.blocked_unpack(torch.from_numpy(packed), S, n, L, block).numpy()
        assert (nat == pool).all()
    k, m, off, L, pitch, S, _ = UNIT_SHAPES[3]
    clean, rounds, units, want, orc = CS.unit_case(k, m, off, L, pitch, S, block)
    n = k + m
    for rnd in rounds:
        packed = CS.pack_natural(clean, block)
        stripes = [s for s, site in enumerate(rnd) if site is not None]
        at = CS.packed_offsets(n, S, L, block, stripes, [rnd[s][0] for s in stripes], [rnd[s][1] for s in stripes])
        packed[at] ^= np.array([1 << rnd[s][2] for s in stripes], np.uint8)
        nat = ecx.blocked_unpack(torch.from_numpy(packed), S, n, L, block).numpy()
        assert (nat == CS.apply_round(clean.copy(), rnd)).all()
    # in the boundary round the two flips of stripes 0 and 1 are neighbours' units: the last block
    # row of stripe 0 is directly followed by the first block row of stripe 1
    full = L // block
    a = CS.packed_offsets(n, S, L, block, [0, 1], [n - 1, 0], [full * block - 1, 0])
    assert a[0] + 1 == a[1] == full * n * block


@pytest.mark.parametrize("L", [400000, 70000])
def test_percall_sites(L):
    """At most 64 edge sites over every shard and position, bytes 255 and 256, four outside-window
    sites; at L = 400,000 the three bytes around syndrome byte 1,048,576 (row 2, byte 248,576)."""
    k, m, off = 17, 3, 5
    sites = CS.percall_sites(k + m, k, off, L)
    assert len({(i, b) for i, b, _ in sites}) == len(sites)
    assert sum(not CS.inside(x, off, L) for x in sites) == 4
    assert {(k, off + 255), (k + 1, off + 256)} <= {(i, b) for i, b, _ in sites}
    wrap = {(k + 2, off + 248576 + d) for d in (-1, 0, 1)}
    assert (wrap <= {(i, b) for i, b, _ in sites}) == (L == 400000)
    assert 2 * 400000 + 248576 == CS.COUNT_WRAP
    assert len(sites) <= 64 + 2 + 3 + 4 and len({bit for _, _, bit in sites}) == 8
    # site by site the oracle fails exactly the flips inside the window
    rng = np.random.default_rng(L)
    shards = [rng.integers(0, 256, off + L + 3, dtype=np.uint8) for _ in range(k + m)]
    orc = O.ReedSolomon(k, m)
    orc.encode_parity(shards, off, L)
    assert orc.is_parity_correct(shards, off, L)
    for i, b, bit in sites:
        shards[i][b] ^= 1 << bit
        assert orc.is_parity_correct(shards, off, L) == (not CS.inside((i, b, bit), off, L)), (i, b, bit)
        shards[i][b] ^= 1 << bit


def test_issue_sized_pool_builds_quickly():
    """RS(4,2), off 16, L 5136: 5,148 sites (12 of them outside the window, which pass)."""
    k, m, off, L = 4, 2, 16, 5136
    pitch = off + L + 16
    sites = CS.byte_sweep(k + m, off, L, pitch)
    assert len(sites) == 5148 and sum(not CS.inside(x, off, L) for x in sites) == 12
    pool, want, orc = CS.site_pool(k, m, off, L, pitch, sites, 1)
    assert (want == orc).all() and int((want == 0).sum()) == 5136
    rs = O.ReedSolomon(k, m)
    assert not rs.is_parity_correct([pool[0, i].copy() for i in range(k + m)], off, L)
    assert rs.is_parity_correct([pool[7, i].copy() for i in range(k + m)], off, L)
