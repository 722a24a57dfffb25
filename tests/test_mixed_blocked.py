"""decodeMissingBlockedBatchMixed on the GPU (k_gf_apply_mixed_blocked, csrc/apply_mixed.hip): a
batch in the blocked layout whose stripes miss different shards, decoded in place in one call,
bit-exact against the oracle's decodeMissing run per stripe on the natural shards
(ReedSolomon.java:189-286).

Nine stripes whose neighbours always name different patterns, so a block row mapped to the wrong
stripe is decoded with the wrong pattern.  The whole packed buffer is compared with blocked_pack
of the oracle's result -- rebuilt shards, present shards, the stripes of id 255 and of the
nothing-missing pattern -- and 64 guard bytes behind it must stay what they were."""
import numpy as np
import pytest

from mixed_cases import IDS, S, SHAPES, block_of, oracle_case, pack, patterns_of

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _run_blocked(ecx, torch, k, m, L, block_arg):
    """The packed input with guard bytes through the blocked mixed call -> (host bytes, shape)."""
    before, _ = oracle_case(k, m, L)
    packed = pack(ecx, before, block_of(ecx, k, m, L, block_arg))
    buf = torch.from_numpy(np.concatenate([packed, np.full(GUARD, 0xA5, np.uint8)])).cuda()
    dev_ids = torch.tensor(IDS, dtype=torch.uint8, device="cuda")
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(patterns_of(k, m)) as ps:
        rs.decodeMissingBlockedBatchMixed(buf, ps, dev_ids, S, L, block_arg)
        torch.cuda.synchronize()
        shape = ecx.last_launch_shape()
    return buf.cpu().numpy(), shape


@pytest.mark.parametrize("k,m,L,block_arg", SHAPES)
def test_blocked_mixed_decode_matches_the_oracle_per_stripe(ecx, torch_dev, k, m, L, block_arg):
    torch = torch_dev
    n = k + m
    block = block_of(ecx, k, m, L, block_arg)
    before, want = oracle_case(k, m, L)
    got, shape = _run_blocked(ecx, torch, k, m, L, block_arg)
    assert (got[S * n * L:] == 0xA5).all(), "guard bytes behind the batch changed"
    want_packed = pack(ecx, want, block)
    if not (got[:S * n * L] == want_packed).all():
        # name the first stripe and shard that differ, on the natural shards
        nat = ecx.blocked_unpack(torch.from_numpy(got[:S * n * L].copy()), S, n, L, block).numpy()
        bad = np.argwhere((nat != want).any(axis=2))
        s, i = bad[0]
        pytest.fail(f"stripe {s} (pattern id {IDS[s]}) shard {i} differs from the oracle; {len(bad)} shards differ")
    # untouched stripes, stated on their own: id 255 (stripe 1) and the nothing-missing pattern (3, 8)
    before_packed = pack(ecx, before, block)
    nat_got = ecx.blocked_unpack(torch.from_numpy(got[:S * n * L].copy()), S, n, L, block).numpy()
    for s in (1, 3, 8):
        assert (nat_got[s] == before[s]).all(), s
    assert not (want_packed == before_packed).all()  # the case does rebuild something
    # the launch of record: the body pass's kernel where a stripe has several block rows and the
    # blocks are whole 16-B aligned chunks; the set's depth (8 when every pattern has >= 12
    # entries) and 4 rows (no pattern here misses more than 4)
    full = L // block
    if full >= 2 and block % 4096 == 0:
        assert shape == "k_gf_apply_mixed_blocked<false, %d, 4>" % (4 if k < 12 else 8), shape


@pytest.mark.parametrize("k,m,L,block_arg", SHAPES)
def test_blocked_mixed_equals_unpack_natural_mixed_pack(ecx, torch_dev, k, m, L, block_arg):
    """blocked_unpack -> decodeMissingBatchMixed on the natural shards -> blocked_pack gives the
    blocked call's bytes: what a caller that keeps its stripes blocked had to do before."""
    torch = torch_dev
    n = k + m
    block = block_of(ecx, k, m, L, block_arg)
    before, _ = oracle_case(k, m, L)
    got, _ = _run_blocked(ecx, torch, k, m, L, block_arg)
    packed = torch.from_numpy(pack(ecx, before, block)).cuda()
    natural = ecx.blocked_unpack(packed, S, n, L, block).contiguous()
    dev_ids = torch.tensor(IDS, dtype=torch.uint8, device="cuda")
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(patterns_of(k, m)) as ps:
        rs.decodeMissingBatchMixed(natural, ps, dev_ids, n * L, L, S, 0, L)
        torch.cuda.synchronize()
    repacked = ecx.blocked_pack(natural, block)
    assert (repacked.cpu().numpy() == got[:S * n * L]).all()


def test_blocked_mixed_eight_row_instance_is_the_launch_of_record(ecx, torch_dev):
    """RS(5,5) misses up to 5 shards: the 8-row instance of the blocked kernel, on 4 KiB blocks
    (3 per stripe) so that the body runs full chunks; bit-exact against the oracle."""
    torch = torch_dev
    from mixed_cases import decode_by_oracle
    k, m, L, block = 5, 5, 3 * 4096 + 40, 4096
    n = k + m
    pats = patterns_of(k, m)
    pool = torch.empty((S, n, L), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 8300)
    before = pool.cpu().numpy()
    want = decode_by_oracle(k, m, before, pats, IDS, 0, L)
    buf = ecx.blocked_pack(pool, block)
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(pats) as ps:
        assert ps.info() == (len(pats), n, 5)
        rs.decodeMissingBlockedBatchMixed(buf, ps, torch.tensor(IDS, dtype=torch.uint8, device="cuda"), S, L, block)
        torch.cuda.synchronize()
        assert ecx.last_launch_shape() == "k_gf_apply_mixed_blocked<false, 4, 8>"
    assert (buf.cpu().numpy() == pack(ecx, want, block)).all()
