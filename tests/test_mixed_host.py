"""The mixed decode from HOST memory, in both layouts (ecx_rs_decode_missing_mixed_batch_host,
ecx_rs_decode_missing_blocked_mixed_batch_host; host_pipe.cpp run_host_mixed_batch): every host
byte after the call equals the oracle's decodeMissing run per stripe on the natural shards
(ReedSolomon.java:189-286) -- rebuilt shards, present shards, untouched stripes, the bytes outside
the window and the padding of the pitch.

Each case runs with ecx_tune "host_chunk_kib" at 16 and at its default: at 16 a chunk is a stripe
or a single block row, so the chunks of a blocked body begin mid-stripe (the launcher is handed
first_unit % divisor != 0) and the ring of buffer sets is reused."""
import functools

import numpy as np
import pytest

from mixed_cases import IDS, S, SHAPES, block_of, decode_by_oracle, oracle_case, pack, patterns_of

pytestmark = pytest.mark.gpu

# natural layout: (k, m, byte_count, offset, pitch)
NATURAL = [(4, 2, 2983, 16, 3072 + 16),       # byte-safe, behind an offset on a padded pitch
           (12, 4, 8192 + 48, 0, 8192 + 64)]  # full chunks plus a 16-multiple rest
BLOCKED = [SHAPES[0], SHAPES[3], SHAPES[5]]
CHUNKS = [16, None]  # host_chunk_kib; None = the default


@pytest.fixture(autouse=True)
def _device():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


class chunk_kib:
    """ecx_tune host_chunk_kib for the length of a with block."""

    def __init__(self, ecx, kib):
        self.ecx, self.kib = ecx, kib

    def __enter__(self):
        self.was = self.ecx.tune_value("host_chunk_kib")
        if self.kib is not None:
            self.ecx.tune("host_chunk_kib", self.kib)

    def __exit__(self, *exc):
        self.ecx.tune("host_chunk_kib", self.was)


@functools.lru_cache(maxsize=None)
def _natural_case(k, m, cnt, off, pitch):
    rng = np.random.default_rng(9100 + k + cnt)
    before = rng.integers(0, 256, (S, k + m, pitch), dtype=np.uint8)
    want = decode_by_oracle(k, m, before, patterns_of(k, m), IDS, off, cnt)
    before.setflags(write=False)
    want.setflags(write=False)
    return before, want


def _assert_natural(got, before, want, pats, ids):
    for s, pid in enumerate(ids):
        present = pats[pid] if pid < len(pats) else np.ones(got.shape[1], np.uint8)
        for i in range(got.shape[1]):
            if present[i]:
                assert (got[s, i] == before[s, i]).all(), f"stripe {s} (pattern {pid}): present shard {i} changed"
            else:
                assert (got[s, i] == want[s, i]).all(), f"stripe {s} (pattern {pid}): rebuilt shard {i} differs"
    assert (got == want).all()


@pytest.mark.parametrize("kib", CHUNKS)
@pytest.mark.parametrize("k,m,cnt,off,pitch", NATURAL)
def test_host_mixed_decode_natural_layout(ecx, k, m, cnt, off, pitch, kib):
    n = k + m
    pats = patterns_of(k, m)
    before, want = _natural_case(k, m, cnt, off, pitch)
    host = before.copy()  # pageable
    ids = np.array(IDS, np.uint8)
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(pats) as ps, chunk_kib(ecx, kib):
        rs.decodeMissingBatchMixedHost(host, ps, ids, n * pitch, pitch, S, off, cnt)
    assert (host[:, :, :off] == before[:, :, :off]).all(), "bytes before the window changed"
    assert (host[:, :, off + cnt:] == before[:, :, off + cnt:]).all(), "bytes after the window changed"
    _assert_natural(host, before, want, pats, IDS)
    assert list(ids) == IDS


@pytest.mark.parametrize("kib", CHUNKS)
@pytest.mark.parametrize("k,m,L,block_arg", BLOCKED)
def test_host_mixed_decode_blocked_layout(ecx, k, m, L, block_arg, kib):
    import torch
    n = k + m
    block = block_of(ecx, k, m, L, block_arg)
    before, want = oracle_case(k, m, L)
    guard = np.full(64, 0xA5, np.uint8)
    host = np.concatenate([pack(ecx, before, block), guard])
    ids = np.array(IDS, np.uint8)
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(patterns_of(k, m)) as ps, chunk_kib(ecx, kib):
        rs.decodeMissingBlockedBatchMixedHost(host, ps, ids, S, L, block_arg)
    assert (host[S * n * L:] == 0xA5).all(), "guard bytes behind the batch changed"
    nat = ecx.blocked_unpack(torch.from_numpy(host[:S * n * L].copy()), S, n, L, block).numpy()
    _assert_natural(nat, before, want, patterns_of(k, m), IDS)
    assert (host[:S * n * L] == pack(ecx, want, block)).all()


def _trap_case():
    """RS(4,2): pattern 0 misses shard 5, pattern 1 misses shard 0, pattern 2 nothing; id 255 has
    no pattern.  Shard 5 is read by neither decode (a missing data shard is rebuilt from the first
    k present shards, 1..4) but it comes back from the device for every stripe, as pattern 0's
    output: uploading inputs only would overwrite the valid shard 5 of the pattern-1 stripes."""
    k, m, L = 4, 2, 4096 + 200
    pats = np.ones((3, 6), np.uint8)
    pats[0, 5] = 0
    pats[1, 0] = 0
    ids = [1, 0, 255, 1, 2, 0, 1]
    rng = np.random.default_rng(9300)
    before = rng.integers(0, 256, (len(ids), 6, L), dtype=np.uint8)
    want = decode_by_oracle(k, m, before, pats, ids, 0, L)
    return k, m, L, pats, ids, before, want


def _assert_trap(got, before, want, ids):
    assert (got == want).all()
    for s, pid in enumerate(ids):
        if pid == 1:
            assert (got[s, 5] == before[s, 5]).all(), f"valid shard 5 of stripe {s} (misses shard 0) was overwritten"
            assert not (got[s, 0] == before[s, 0]).all()
        if pid in (255, 2):
            assert (got[s] == before[s]).all(), f"stripe {s} (id {pid}) changed"


@pytest.mark.parametrize("kib", CHUNKS)
def test_union_of_output_shards_is_uploaded_natural(ecx, kib):
    k, m, L, pats, ids, before, want = _trap_case()
    host = before.copy()
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(pats) as ps, chunk_kib(ecx, kib):
        rs.decodeMissingBatchMixedHost(host, ps, np.array(ids, np.uint8), 6 * L, L, len(ids), 0, L)
    _assert_trap(host, before, want, ids)


def test_host_mixed_decode_wraps_a_ring_of_two_sets(ecx):
    """RS(4,2), 4 KiB shards, 16 KiB chunks over host_buffers 2: all six shards go up (24 KiB a
    stripe), so each of the 7 stripes is a chunk and the ring of two sets wraps three times, a set
    loaded again while its earlier stripe may still be on its way back.  Seven different one- and
    two-shard patterns; shards 0, 1, 2, 4, 5 come back for every stripe and shard 3 for none:
    every byte equals the oracle's."""
    k, m, L = 4, 2, 4096
    pats = np.ones((7, 6), np.uint8)
    for p, missing in enumerate([(0,), (1,), (5,), (0, 2), (2, 5), (4, 5), (1, 4)]):
        pats[p, list(missing)] = 0
    ids = [4, 0, 6, 2, 5, 1, 3]
    before = np.random.default_rng(9400).integers(0, 256, (len(ids), 6, L), dtype=np.uint8)
    want = decode_by_oracle(k, m, before, pats, ids, 0, L)
    host = before.copy()
    rs = ecx.ReedSolomon.create(k, m)
    buffers = ecx.tune_value("host_buffers")
    ecx.tune("host_buffers", 2)
    try:
        with rs.patternSet(pats) as ps, chunk_kib(ecx, 16):
            rs.decodeMissingBatchMixedHost(host, ps, np.array(ids, np.uint8), 6 * L, L, len(ids), 0, L)
    finally:
        ecx.tune("host_buffers", buffers)
    _assert_natural(host, before, want, pats, ids)


@pytest.mark.parametrize("kib", CHUNKS)
def test_union_of_output_shards_is_uploaded_blocked(ecx, kib):
    """The same in the blocked layout, from pinned memory (HostBuffer): 2 KiB blocks, two per
    stripe and a 200-B tail."""
    import torch
    k, m, L, pats, ids, before, want = _trap_case()
    block, ns = 2048, len(ids)
    pinned = ecx.HostBuffer(ns * 6 * L)
    pinned.array[:] = pack(ecx, before, block)
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(pats) as ps, chunk_kib(ecx, kib):
        rs.decodeMissingBlockedBatchMixedHost(pinned.array, ps, np.array(ids, np.uint8), ns, L, block)
    got = ecx.blocked_unpack(torch.from_numpy(pinned.array.copy()), ns, 6, L, block).numpy()
    _assert_trap(got, before, want, ids)
