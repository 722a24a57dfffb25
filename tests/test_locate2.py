"""locateCorrupt2Batch (ecx_rs_locate_corrupt2_batch) against the oracle's
brute force (tests/locate2_cases.py): for each candidate shard and each candidate pair the oracle
zeroes it, rebuilds it with decodeMissing and runs isParityCorrect.  Fourteen stripes per shape put
the corruption where the kernel's paths differ -- one flip at the first and at the last byte of the
window (the wave shortcut), two shards at one byte for each kind of pair (the pair tiles), two shards
in one wave span, in two waves of a chunk, in two chunks (two shortcut waves combine through their
stores), the same two shards in two chunks, a flip in the partial last chunk, three shards, flips
just outside the window, a random stripe -- and the heal ids then drive decodeMissingBatchMixed with
doubleLossPatternSet().  Two exhaustive sets follow: every pair and every triple of RS(2,4)'s shards."""
import numpy as np
import pytest

from locate2_cases import S, SHAPES, every_pair, every_triple, fourteen_stripes, kinds, pairs_of, run_locate2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.mark.parametrize("k,m,L,first,count,P", SHAPES)
def test_locate2_vs_oracle_and_heal(ecx, torch_dev, k, m, L, first, count, P):
    """suspect, culprit and healId equal the oracle's for every stripe; the bytes after each output
    and the shards are untouched; healId=None is accepted; then the heal restores every stripe with
    one or two culprits to the original and leaves the others bit-identical."""
    torch = torch_dev
    n = k + m
    width = n + n * (n - 1) // 2
    nat, bad, (want_s, want_c, want_h), flips = fourteen_stripes(k, m, L, first, count, P)
    assert kinds(want_c)[0] >= 2 and kinds(want_c)[1] >= 5 and kinds(want_c)[2] >= 1
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.from_numpy(np.array(bad)).cuda()
    before = pool.clone()

    def call(su, cu, he):
        rs.locateCorrupt2Batch(pool, n * P, P, S, first, count, su, cu, he)

    got_s, got_c, got_h, heal_dev = run_locate2(torch, call, S, width)
    print(f"RS({k},{m}) L={L} window=[{first},{first + count}) culprit={got_c.tolist()} want={want_c.tolist()}")
    assert got_c.tolist() == want_c.tolist()
    assert (got_s == want_s).all(), (got_s.tolist(), want_s.tolist())
    assert got_h.tolist() == want_h.tolist()
    assert torch.equal(pool, before)  # read-only
    s2, c2, h2, _ = run_locate2(torch, call, S, width, heal=False)
    assert h2 is None and c2.tolist() == want_c.tolist() and (s2 == want_s).all()

    with rs.doubleLossPatternSet() as ps:
        assert ps.info() == (width, n, 2)
        rs.decodeMissingBatchMixed(pool, ps, heal_dev[:S], n * P, P, S, first, count)
        torch.cuda.synchronize()
    healed = pool.cpu().numpy()
    outside = np.ones(P, bool)
    outside[first:first + count] = False
    for s in range(S):
        inside = all(first <= byte < first + count for st, _, byte in flips if st == s)
        if want_c[s, 0] >= 0 and inside:
            assert (healed[s, :, first:first + count] == nat[s, :, first:first + count]).all(), s
            assert (healed[s][:, outside] == bad[s][:, outside]).all(), s
        else:
            assert want_c[s, 0] < 0  # every stripe with a culprit has its flips inside the window
            assert (healed[s] == bad[s]).all(), s


def test_locate2_every_pair(ecx, torch_dev):
    """RS(2,4), L = 4096, every pair of shards with the three PAIR_VALUES at one byte (45 stripes, one
    launch): the oracle names exactly that pair in all 45 -- asserted of the oracle first -- and so
    does the device."""
    torch = torch_dev
    k, m, L = 2, 4, 4096
    n, width = 6, 21
    nat, bad, (want_s, want_c, want_h), cases = every_pair(k, m, L)
    nst = len(cases)
    assert nst == 45
    assert want_c.tolist() == [[i, j] for i, j, _ in cases]
    assert want_h.tolist() == [n + pairs_of(n).index((i, j)) for i, j, _ in cases]
    assert (want_s.sum(axis=1) == 1).all()
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.from_numpy(np.array(bad)).cuda()
    got_s, got_c, got_h, _ = run_locate2(
        torch, lambda su, cu, he: rs.locateCorrupt2Batch(pool, n * L, L, nst, 0, L, su, cu, he), nst, width)
    assert got_c.tolist() == want_c.tolist()
    assert (got_s == want_s).all() and got_h.tolist() == want_h.tolist()


def test_locate2_every_triple(ecx, torch_dev):
    """RS(2,4), every triple of shards corrupt at one byte with one value triple (20 stripes, one
    launch): three errors can imitate a pair of other shards (3 + 2 >= 5), and the outputs equal the
    oracle's brute force whatever it says."""
    torch = torch_dev
    k, m, L = 2, 4, 4096
    n, width = 6, 21
    nat, bad, (want_s, want_c, want_h), cases = every_triple(k, m, L)
    nst = len(cases)
    assert nst == 20
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.from_numpy(np.array(bad)).cuda()
    got_s, got_c, got_h, _ = run_locate2(
        torch, lambda su, cu, he: rs.locateCorrupt2Batch(pool, n * L, L, nst, 0, L, su, cu, he), nst, width)
    wrong = int((want_c[:, 0] >= 0).sum())
    print(f"RS(2,4): {wrong} of {nst} triples name a single shard or a pair of other shards; culprit={got_c.tolist()}")
    assert got_c.tolist() == want_c.tolist()
    assert (got_s == want_s).all() and got_h.tolist() == want_h.tolist()


def test_locate2_edge_arguments(ecx, torch_dev):
    """nstripes == 0 touches nothing; byteCount == 0 makes every stripe clean; a short output is
    ECX_E_INDEX before any device work; m = 3 is ECX_E_ILLEGAL_ARGUMENT."""
    torch = torch_dev
    k, m, L, nst = 2, 4, 1000, 3
    n, width = 6, 21
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.zeros(nst * n * L, dtype=torch.uint8, device="cuda")
    pool[5] = 1  # stripe 0 is corrupt, were any byte looked at
    su = torch.full((nst * width + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    cu = torch.full((2 * nst + 4,), -77, dtype=torch.int32, device="cuda")
    he = torch.full((nst + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    rs.locateCorrupt2Batch(pool, n * L, L, 0, 0, L, su, cu, he)
    torch.cuda.synchronize()
    assert (su.cpu().numpy() == 0xA5).all() and (cu.cpu().numpy() == -77).all() and (he.cpu().numpy() == 0xA5).all()
    rs.locateCorrupt2Batch(pool, n * L, L, nst, 0, 0, su, cu, he)
    torch.cuda.synchronize()
    assert su.cpu().tolist() == [1] * (nst * width) + [0xA5] * 16
    assert cu.cpu().tolist() == [-1] * (2 * nst) + [-77] * 4 and he.cpu().tolist() == [255] * nst + [0xA5] * 16
    for a, b, c in ((su[17:], cu, he), (su, cu[-5:], he), (su, cu, he[-2:])):
        with pytest.raises(ecx.EcxError) as e:
            rs.locateCorrupt2Batch(pool, n * L, L, nst, 0, L, a, b, c)
        assert e.value.code == -5
    r = ecx.ReedSolomon.create(3, 3)
    for f in (lambda: r.locateCorrupt2Batch(pool, n * L, L, nst, 0, L, su, cu, he),
              lambda: r.locateCorrupt2BlockedBatch(pool, nst, L, su, cu, he)):
        with pytest.raises(ecx.EcxError) as e:
            f()
        assert e.value.code == -1
