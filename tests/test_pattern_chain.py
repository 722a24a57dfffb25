"""PatternChain (repair-pipelining_amd/chain.py): the pipelined partial-sum chain for RS stripes
under rotated placement -- node j holds shard (j + s) mod n of stripe s, and the stripes miss
different shards, so both the pattern and every helper's shard index change per stripe.

The CPU test rehearses the orchestration with gloo, world 3, RS(4,2): two nodes per rank with the
destination last on the chain, then the six nodes on two ranks with the destination off the chain;
seven stripes in slices of three (a ragged last slice).  The hop is a test-only numpy stand-in for
decodePartialBatchMixed built on the oracle's multiplication table and the codec's decode matrices.
The GPU test runs the first chain with the HIP kernel: three processes on one GPU, gloo transport.
The destination's rows must equal the oracle's decodeMissing per stripe (ReedSolomon.java:189-286),
with zeros where nothing was to be rebuilt.  The stripes are random bytes, not codewords, and the
nodes holding a stripe's missing shards hold garbage."""
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from mixed_cases import patterns_of
from test_chain import ROOT, _setup, _spawn

K, M, N = 4, 2, 6
IDS = [3, 255, 5, 0, 6, 1, 4]  # per stripe; 255 names no pattern, 0 misses nothing, 6 repeats 3
S = len(IDS)


class NumpyPartial:
    """Test-only stand-in for the library's hop (CPU tensors); `pats` are the plain flags."""

    def __init__(self, rs, pats):
        import oracle as O
        self.mt = O.mul_table()
        self.n = rs.getTotalShardCount()
        self.cols = []  # per pattern: shard index -> the coefficients of its column, one per missing shard
        for p in pats:
            missing = [i for i, f in enumerate(p) if not f]
            cols = {}
            if missing:
                mat, ins, outs = rs.decode_map(p).matrix()
                assert list(outs) == missing
                cols = {int(slot): np.asarray(mat)[:, j] for j, slot in enumerate(ins)}
            self.cols.append((len(missing), cols))
        self.max_missing = max(r for r, _ in self.cols)

    def __call__(self, ids, shard_of, inp, in_stripe_stride, acc, acc_stripe_stride, acc_row_stride, nstripes,
                 byte_count, is_first):
        x, B = inp.numpy(), byte_count
        a = acc.numpy().reshape(nstripes, -1, B)
        assert acc_row_stride == B and acc_stripe_stride == a.shape[1] * B
        for s in range(nstripes):
            p, i = int(ids[s]), int(shard_of[s])
            if p >= len(self.cols) or i >= self.n:
                continue
            rows, cols = self.cols[p]
            xin = x[s * in_stripe_stride:s * in_stripe_stride + B]
            for o in range(rows):
                c = int(cols[i][o]) if i in cols else 0
                v = self.mt[c][xin] if c else np.zeros(B, np.uint8)
                a[s, o] = v if is_first else a[s, o] ^ v


def _case(ecx, rank, node_rank, order, dest, B, slice_stripes, nbuf, device, on_gpu):
    from repair_pipelining_amd.chain import PatternChain
    import oracle as O
    pats = patterns_of(K, M)
    rs = ecx.ReedSolomon.create(K, M)
    rng = np.random.default_rng(17)
    stripes = rng.integers(0, 256, (S, N, B), dtype=np.uint8)  # every rank the same
    mine = [j for j, r in enumerate(node_rank) if r == rank]
    local = shard_of = ids = None
    if mine:
        shard_of_host = np.array([[(j + s) % N for s in range(S)] for j in mine], np.uint8)
        loc = np.zeros((S, len(mine), B), np.uint8)
        for slot in range(len(mine)):
            for s in range(S):
                loc[s, slot] = stripes[s, shard_of_host[slot, s]]
        local = torch.from_numpy(loc).to(device)
        shard_of = torch.from_numpy(shard_of_host).to(device)
        ids = torch.tensor(IDS, dtype=torch.uint8, device=device)
    ps = rs.patternSet(pats) if on_gpu else pats
    try:
        chain = PatternChain(rs, ps, order, rank, dest=dest, partial_factory=None if on_gpu else NumpyPartial)
        rows = chain.n_out_slots
        assert rows == M
        out = torch.full((S, rows, B), 0x5A, dtype=torch.uint8, device=device) if rank == dest else None
        chain.run(local, shard_of, ids, S, B, out=out, slice_stripes=slice_stripes, n_buffers=nbuf, device=device)
        if on_gpu:
            torch.cuda.synchronize()
    finally:
        if on_gpu:
            ps.close()
    if rank != dest:
        return True
    got = out.cpu().numpy()
    want = np.zeros_like(got)
    orc = O.ReedSolomon(K, M)
    for s, pid in enumerate(IDS):
        if pid >= len(pats):
            continue
        shards = [stripes[s, i].copy() for i in range(N)]
        orc.decode_missing(shards, [bool(f) for f in pats[pid]], 0, B)
        for o, i in enumerate(i for i in range(N) if not pats[pid][i]):
            want[s, o] = shards[i]
    assert want.any()
    return bool((got == want).all())


def _cpu_worker(rank, world, port, q):
    ecx = _setup(rank, world, port)
    try:
        # two nodes per rank, the destination last on the chain
        ok = _case(ecx, rank, [0, 0, 1, 1, 2, 2], [0, 1, 2], 2, 96, 3, 2, "cpu", False)
        # the six nodes on ranks 1 and 0 (in that order), the destination off the chain
        ok &= _case(ecx, rank, [0, 1, 0, 1, 0, 1], [1, 0], 2, 33, 3, 3, "cpu", False)
        dist.barrier()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_pattern_chain_orchestration_gloo():
    assert _spawn(_cpu_worker, 3) == {0: True, 1: True, 2: True}


def test_pattern_chain_rejects_a_destination_inside_the_chain():
    sys.path[:0] = [str(ROOT), str(ROOT / "oracle")]
    import rpamd
    ecx = rpamd.load()
    from repair_pipelining_amd.chain import PatternChain
    rs = ecx.ReedSolomon.create(K, M)
    with pytest.raises(ValueError):
        PatternChain(rs, patterns_of(K, M), [0, 1, 2], 0, dest=1, partial_factory=NumpyPartial)


def _gpu_worker(rank, world, port, q):
    ecx = _setup(rank, world, port)
    try:
        torch.cuda.set_device(0)
        ecx.set_device(0)
        ok = _case(ecx, rank, [0, 0, 1, 1, 2, 2], [0, 1, 2], 2, 4096 + 48, 3, 2, "cuda", True)
        torch.cuda.synchronize()
        dist.barrier()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_pattern_chain_hip_kernel_three_ranks():
    """3 ranks on one GPU (gloo transport staged through the host), k_gf_partial_mixed hops."""
    assert _spawn(_gpu_worker, 3) == {0: True, 1: True, 2: True}
