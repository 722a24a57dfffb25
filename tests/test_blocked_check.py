"""isParityCorrect over blocked RS stripes (ecx_rs_is_parity_correct_blocked_batch and its host
forms): the verdict of caller stripe s comes from the `full` block rows
of the body pass that belong to it and from its tail, so every flip below sits where a wrong
unit -> stripe mapping would charge it to a neighbouring stripe."""
import functools

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

S = 7
GUARD = 0xA5
ECX_E_ILLEGAL_ARGUMENT, ECX_E_INDEX = -1, -5

# (k, m, L, block): 6 full 32 KiB blocks + a 3,392-B tail; full blocks + a 4 KiB tail; no tail;
# 25 blocks + an odd 2,049-B tail (byte-safe tail); the 8-row instantiation with byte-safe passes;
# one block, no tail; full == 0 (tail only); two tiles
SHAPES = [(17, 3, 200000, 0), (12, 4, 3 * 65536 + 4096, 0), (12, 4, 3 * 65536, 0), (4, 2, 104449, 4096),
          (5, 5, 1001, 64), (3, 1, 34, 0), (4, 2, 100, 4096), (10, 10, 2 * 4096 + 48, 4096)]
HOST_SHAPES = [(17, 3, 200000, 0), (4, 2, 104449, 4096), (5, 5, 1001, 64), (3, 1, 34, 0)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def packed_offset(n, nstripes, L, b, s, i, byte):
    """Where the blocked layout (include/ecx.h) keeps byte `byte` of shard i of stripe s."""
    full, tail = divmod(L, b)
    body = full * n * b
    if byte < full * b:
        return s * body + (byte // b) * n * b + i * b + byte % b
    return nstripes * body + s * n * tail + i * tail + (byte - full * b)


def flips_for(k, m, L, b, nstripes):
    """(stripe, shard, byte) of the flipped bytes the shape and stripe count have room for."""
    n = k + m
    full, tail = divmod(L, b)
    want = [(1, 0, 0)]                                   # the first unit of stripe 1
    if full:
        want.append((3, n - 1, full * b - 1))            # the last body unit of stripe 3
    if tail:
        want.append((5, k - 1, full * b))                # byte 0 of the tail of a data shard
        want.append((6, n - 1, L - 1))                   # the last byte of the batch
    return [f for f in want if f[0] < nstripes]


@functools.lru_cache(maxsize=None)
def case(k, m, L, block, nstripes=S, flips=None):
    """Valid natural stripes (the oracle's encode_parity), the same with the flips applied, the
    oracle's isParityCorrect per flipped stripe, and the resolved block.  Shared: do not write."""
    n = k + m
    rng = np.random.default_rng(7000 + 31 * k + L)
    nat = np.zeros((nstripes, n, L), np.uint8)
    nat[:, :k] = rng.integers(0, 256, (nstripes, k, L), dtype=np.uint8)
    rs = O.ReedSolomon(k, m)
    for s in range(nstripes):
        rs.encode_parity([nat[s, i] for i in range(n)], 0, L)
    import rpamd
    b = block or rpamd.load(shape_knobs=True).ReedSolomon.create(k, m).blockedLayout(L)[0]
    flips = flips_for(k, m, L, b, nstripes) if flips is None else list(flips)
    bad = nat.copy()
    for s, i, byte in flips:
        bad[s, i, byte] ^= 0x81
    want = [int(rs.is_parity_correct([bad[s, i].copy() for i in range(n)], 0, L)) for s in range(nstripes)]
    for a in (nat, bad):
        a.setflags(write=False)
    return nat, bad, want, b, flips


def pack_with_flips(ecx, torch, nat, flips, b):
    """blocked_pack of the valid stripes, then each flip applied at its packed offset."""
    nstripes, n, L = nat.shape
    packed = ecx.blocked_pack(torch.from_numpy(np.array(nat)), b).numpy()
    for s, i, byte in flips:
        packed[packed_offset(n, nstripes, L, b, s, i, byte)] ^= 0x81
    return packed


@pytest.mark.parametrize("k,m,L,block", SHAPES)
def test_blocked_check_vs_oracle(ecx, torch_dev, k, m, L, block):
    """Seven stripes made valid by the oracle, packed, one byte flipped in stripes 1 (byte 0 of data
    shard 0: its first unit), 3 (the last byte of the last full block of the last parity shard:
    its last body unit, so an off-by-one divisor fails stripe 4), 5 (byte 0 of a data shard's
    tail) and 6 (the last byte of the last parity shard's tail, the last byte of the batch),
    where the shape has them.  The verdicts equal the oracle's isParityCorrect on the flipped
    natural shards and isParityCorrectBatch on the unpacked buffer; stripes 0, 2, 4 pass; the 16
    bytes after verdict[S] and the packed buffer are untouched; random stripes all fail."""
    torch = torch_dev
    n = k + m
    nat, bad, want, b, flips = case(k, m, L, block)
    rs = ecx.ReedSolomon.create(k, m)
    assert want == [0 if s in {f[0] for f in flips} else 1 for s in range(S)]
    assert [want[s] for s in (0, 2, 4)] == [1, 1, 1]

    def check(flat):
        v = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")
        rs.isParityCorrectBlockedBatch(flat, S, L, v, block)
        torch.cuda.synchronize()
        v = v.cpu().numpy()
        assert (v[S:] == GUARD).all(), v.tolist()
        return v[:S].tolist()

    valid = ecx.blocked_pack(torch.from_numpy(np.array(nat)).cuda(), b)
    assert check(valid) == [1] * S
    packed = pack_with_flips(ecx, torch, nat, flips, b)
    flat = torch.from_numpy(packed).cuda()
    # the flips landed where the layout keeps those bytes
    assert (ecx.blocked_unpack(flat, S, n, L, b).cpu().numpy() == bad).all()
    before = flat.clone()
    got = check(flat)
    print(f"RS({k},{m}) L={L} block={b} flips={flips} verdicts={got} want={want}")
    assert got == want
    assert [got[s] for s in (0, 2, 4)] == [1, 1, 1]
    assert torch.equal(flat, before)  # read-only
    natural = ecx.blocked_unpack(flat, S, n, L, b).contiguous()
    nv = torch.full((S,), GUARD, dtype=torch.uint8, device="cuda")
    rs.isParityCorrectBatch(natural, n * L, L, S, 0, L, nv)
    torch.cuda.synchronize()
    assert got == nv.cpu().tolist()
    noise = torch.empty(S * n * L, dtype=torch.uint8, device="cuda")
    ecx.fill_random(noise, noise.numel(), 7100 + k + L)
    assert check(noise) == [0] * S


def test_blocked_check_edge_arguments(ecx, torch_dev):
    """nstripes == 0 writes nothing; byteCount == 0 makes every verdict 1; a short base or verdict
    is ECX_E_INDEX before any device work (the verdicts keep their bytes); a negative block is
    ECX_E_ILLEGAL_ARGUMENT."""
    torch = torch_dev
    k, m, L, nst = 4, 2, 104449, 3
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    flat = torch.zeros(nst * n * L, dtype=torch.uint8, device="cuda")  # zeros: valid codewords
    v = torch.full((nst + 16,), GUARD, dtype=torch.uint8, device="cuda")
    rs.isParityCorrectBlockedBatch(flat, 0, L, v, 4096)
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == GUARD).all()
    rs.isParityCorrectBlockedBatch(flat, nst, 0, v, 4096)
    torch.cuda.synchronize()
    assert v.cpu().tolist() == [1] * nst + [GUARD] * 16
    v.fill_(GUARD)
    for base, verdict in ((flat[1:], v), (flat, v[-(nst - 1):])):
        with pytest.raises(ecx.EcxError) as e:
            rs.isParityCorrectBlockedBatch(base, nst, L, verdict, 4096)
        assert e.value.code == ECX_E_INDEX
    with pytest.raises(ecx.EcxError) as e:
        rs.isParityCorrectBlockedBatch(flat, nst, L, v, -4096)
    assert e.value.code == ECX_E_ILLEGAL_ARGUMENT
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == GUARD).all()
    # the host forms refuse the same way
    hflat, hv = np.zeros(nst * n * L, np.uint8), np.full(nst + 16, GUARD, np.uint8)
    for call in (lambda bb, vv, blk: rs.isParityCorrectBlockedBatchHost(bb, nst, L, vv, blk),
                 lambda bb, vv, blk: rs.isParityCorrectBlockedBatchHostDevices(bb, nst, L, vv, [0, 0], blk)):
        for bb, vv, blk, code in ((hflat[1:], hv, 4096, ECX_E_INDEX), (hflat, hv[-(nst - 1):], 4096, ECX_E_INDEX),
                                  (hflat, hv, -1, ECX_E_ILLEGAL_ARGUMENT)):
            with pytest.raises(ecx.EcxError) as e:
                call(bb, vv, blk)
            assert e.value.code == code
    assert (hv == GUARD).all()
    rs.isParityCorrectBlockedBatchHost(hflat, 0, L, hv, 4096)
    assert (hv == GUARD).all()
    rs.isParityCorrectBlockedBatchHost(hflat, nst, 0, hv, 4096)
    assert hv.tolist() == [1] * nst + [GUARD] * 16
    for bad in ([ecx.device_count()], []):  # the device list is validated even for an empty batch
        with pytest.raises(ecx.EcxError) as e:
            rs.isParityCorrectBlockedBatchHostDevices(hflat, 0, L, hv, bad, 4096)
        assert e.value.code == ECX_E_ILLEGAL_ARGUMENT, bad


def host_check(ecx, rs, packed, nstripes, L, block, pinned, devs):
    """One host check of `packed` (a copy in pageable or pinned memory, guard bytes after it and
    after the verdicts); returns the verdicts after asserting that nothing else changed."""
    total = packed.size
    if pinned:
        hb = ecx.HostBuffer(total + 64)
        buf = hb.array
    else:
        buf = np.empty(total + 64, np.uint8)
    buf[:total] = packed
    buf[total:] = 0xE7
    hv = np.full(nstripes + 16, GUARD, np.uint8)
    if devs is None:
        rs.isParityCorrectBlockedBatchHost(buf, nstripes, L, hv, block)
    else:
        rs.isParityCorrectBlockedBatchHostDevices(buf, nstripes, L, hv, devs, block)
    assert (buf[:total] == packed).all() and (buf[total:] == 0xE7).all()
    assert (hv[nstripes:] == GUARD).all(), hv.tolist()
    return hv[:nstripes].tolist()


@pytest.mark.parametrize("k,m,L,block", HOST_SHAPES)
def test_blocked_check_host(ecx, torch_dev, k, m, L, block):
    """The host forms over the device test's stripes, flips and expectations: pageable and pinned
    memory, default chunks and 16 KiB chunks (ring reuse), one device and the lists [0, 0] and
    [0, 0, 0].  The host buffer and the bytes after the verdicts stay as they were."""
    torch = torch_dev
    nat, bad, want, b, flips = case(k, m, L, block)
    rs = ecx.ReedSolomon.create(k, m)
    packed = pack_with_flips(ecx, torch, nat, flips, b)
    valid = ecx.blocked_pack(torch.from_numpy(np.array(nat)), b).numpy()
    try:
        for small in (False, True):
            ecx.tune("host_chunk_kib", 16 if small else 65536)
            for pinned in (False, True):
                for devs in (None, [0, 0], [0, 0, 0]):
                    got = host_check(ecx, rs, packed, S, L, block, pinned, devs)
                    assert got == want, (small, pinned, devs, got)
            assert host_check(ecx, rs, valid, S, L, block, True, [0, 0]) == [1] * S
    finally:
        ecx.tune("host_chunk_kib", 65536)


def test_blocked_check_host_column_split(ecx, torch_dev):
    """Two stripes over three device entries, RS(4,2), L = 16,384 + 9,000 in 16 KiB blocks: both
    passes have fewer units than entries and slots of at least 8 KiB, so each is split by byte
    ranges of every slot (the existing column split) and a stripe passes when it passes in every
    range.  A flip in the last byte of stripe 0's block of the last parity shard, then one in the
    last byte of the batch instead: exactly that stripe fails each time."""
    torch = torch_dev
    k, m, L, block, nst = 4, 2, 16384 + 9000, 16384, 2
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    for flips in (((0, n - 1, block - 1),), ((1, n - 1, L - 1),), ((0, 0, block + 4096), (1, 2, 5000))):
        nat, bad, want, b, fl = case(k, m, L, block, nst, flips)
        assert b == block and want == [0 if s in {f[0] for f in fl} else 1 for s in range(nst)]
        packed = pack_with_flips(ecx, torch, nat, fl, b)
        for pinned in (False, True):
            assert host_check(ecx, rs, packed, nst, L, block, pinned, [0, 0, 0]) == want, flips
        assert host_check(ecx, rs, packed, nst, L, block, False, None) == want, flips
