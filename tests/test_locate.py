"""locateCorruptBatch (ecx_rs_locate_corrupt_batch) against the oracle's
brute force (tests/locate_cases.py): for each candidate shard the oracle zeroes it, rebuilds it with
decodeMissing and runs isParityCorrect.  Nine stripes per shape put the corruption where the
kernel's paths differ -- the first and the last byte of the window, the partial last chunk, one
shard in two chunks (workgroups must agree), two shards in two chunks (no workgroup sees both: the
clears combine across workgroups), a byte just outside the window, a random stripe -- and the heal
ids then drive decodeMissingBatchMixed with singleLossPatternSet()."""
import numpy as np
import pytest

from locate_cases import nine_stripes, run_locate, same_byte_pairs

pytestmark = pytest.mark.gpu

S = 9
# (k, m, L, first byte, byte count): the shifted last window (48 chunks + 3,392 B); byte-safe (odd
# strides); 8 syndrome rows, byte-safe; one chunk + 48 B; the smallest code; m = 8, 16 stage-two
# tiles; the unaligned-start split
SHAPES = [(17, 3, 200000, 0, 200000), (4, 2, 104449, 0, 104449), (5, 5, 1001, 0, 1001), (12, 4, 4096 + 48, 0, 4096 + 48),
          (3, 2, 34, 0, 34), (10, 8, 2 * 4096 + 48, 0, 2 * 4096 + 48), (12, 4, 8192, 3, 8000)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.mark.parametrize("k,m,L,first,count", SHAPES)
def test_locate_vs_oracle_and_heal(ecx, torch_dev, k, m, L, first, count):
    """suspect, culprit and healId equal the oracle's for every stripe; the 16 bytes after each
    output and the shards are untouched; healId=None is accepted; then the heal restores every
    stripe with a culprit to the original and leaves the -1 and -2 stripes bit-identical."""
    torch = torch_dev
    n, P = k + m, L + 16
    nat, bad, (want_s, want_c, want_h), flips = nine_stripes(k, m, L, first, count)
    # what the table of the case promises, as the oracle sees it
    assert want_c[0] == -1 and want_c[4] == -1 and want_c[7] == -1
    assert want_c[1] == 0 and want_c[2] == n - 1 and want_c[5] == k and want_c[6] == -2 and want_c[8] == -2
    assert want_c[3] == (k - 1 if any(f[0] == 3 for f in flips) else -1)
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.from_numpy(np.array(bad)).cuda()
    before = pool.clone()

    def call(su, cu, he):
        rs.locateCorruptBatch(pool, n * P, P, S, first, count, su, cu, he)

    got_s, got_c, got_h, heal_dev = run_locate(torch, call, S, n)
    print(f"RS({k},{m}) L={L} window=[{first},{first + count}) culprit={got_c.tolist()} want={want_c.tolist()}")
    assert got_c.tolist() == want_c.tolist()
    assert (got_s == want_s).all(), (got_s.tolist(), want_s.tolist())
    assert got_h.tolist() == want_h.tolist()
    assert torch.equal(pool, before)  # read-only
    s2, c2, h2, _ = run_locate(torch, call, S, n, heal=False)
    assert h2 is None and c2.tolist() == want_c.tolist() and (s2 == want_s).all()

    with rs.singleLossPatternSet() as ps:
        assert ps.info()[:2] == (n, n)
        rs.decodeMissingBatchMixed(pool, ps, heal_dev[:S], n * P, P, S, first, count)
        torch.cuda.synchronize()
    healed = pool.cpu().numpy()
    for s in range(S):
        if want_c[s] >= 0:
            assert (healed[s, :, first:first + count] == nat[s, :, first:first + count]).all(), s
            outside = np.ones(P, bool)
            outside[first:first + count] = False
            assert (healed[s][:, outside] == bad[s][:, outside]).all(), s
        else:
            assert (healed[s] == bad[s]).all(), s


@pytest.mark.parametrize("k,m,L", [(4, 2, 100), (3, 2, 34)])
def test_locate_same_byte_pairs(ecx, torch_dev, k, m, L):
    """Two shards corrupt at the same byte, every pair of shards with three pairs of error values
    (45 stripes of RS(4,2), 30 of RS(3,2)): with m = 2 such a stripe can name a third shard, and
    the outputs equal the oracle's brute force whatever it says."""
    torch = torch_dev
    n = k + m
    nat, bad, (want_s, want_c, want_h) = same_byte_pairs(k, m, L)
    nst = bad.shape[0]
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.from_numpy(np.array(bad)).cuda()
    got_s, got_c, got_h, _ = run_locate(
        torch, lambda su, cu, he: rs.locateCorruptBatch(pool, n * L, L, nst, 0, L, su, cu, he), nst, n)
    imitated = int((want_c >= 0).sum())
    print(f"RS({k},{m}): {imitated} of {nst} same-byte pairs name a third shard; culprit={got_c.tolist()}")
    assert got_c.tolist() == want_c.tolist()
    assert (got_s == want_s).all() and got_h.tolist() == want_h.tolist()


def test_locate_edge_arguments(ecx, torch_dev):
    """nstripes == 0 touches nothing; byteCount == 0 makes every stripe clean; a short output is
    ECX_E_INDEX before any device work; m = 1 and m = 9 are ECX_E_ILLEGAL_ARGUMENT."""
    torch = torch_dev
    k, m, L, nst = 4, 2, 1000, 3
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.zeros(nst * n * L, dtype=torch.uint8, device="cuda")
    pool[5] = 1  # stripe 0 is corrupt, were any byte looked at
    su = torch.full((nst * n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    cu = torch.full((nst + 4,), -77, dtype=torch.int32, device="cuda")
    he = torch.full((nst + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    rs.locateCorruptBatch(pool, n * L, L, 0, 0, L, su, cu, he)
    torch.cuda.synchronize()
    assert (su.cpu().numpy() == 0xA5).all() and (cu.cpu().numpy() == -77).all() and (he.cpu().numpy() == 0xA5).all()
    rs.locateCorruptBatch(pool, n * L, L, nst, 0, 0, su, cu, he)
    torch.cuda.synchronize()
    assert su.cpu().tolist() == [1] * (nst * n) + [0xA5] * 16
    assert cu.cpu().tolist() == [-1] * nst + [-77] * 4 and he.cpu().tolist() == [255] * nst + [0xA5] * 16
    for a, b, c in ((su[17:], cu, he), (su, cu[-2:], he), (su, cu, he[-2:])):
        with pytest.raises(ecx.EcxError) as e:
            rs.locateCorruptBatch(pool, n * L, L, nst, 0, L, a, b, c)
        assert e.value.code == -5
    for kk, mm in ((4, 1), (4, 9)):
        r = ecx.ReedSolomon.create(kk, mm)
        big = torch.zeros(nst * (kk + mm) * L, dtype=torch.uint8, device="cuda")
        for f in (lambda: r.locateCorruptBatch(big, (kk + mm) * L, L, nst, 0, L, su.new_zeros(nst * (kk + mm)), cu, he),
                  lambda: r.locateCorruptBlockedBatch(big, nst, L, su.new_zeros(nst * (kk + mm)), cu, he)):
            with pytest.raises(ecx.EcxError) as e:
                f()
            assert e.value.code == -1
