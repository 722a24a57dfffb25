"""ClayPatternChain (repair-pipelining_amd/chain.py): the pipelined partial-sum chain
(ClayCoordinator.kt:265-319, ClayCodeNode.kt:165-233) for Clay stripes under rotated placement --
helper j holds node (j + s) mod n of stripe s, and the stripes lost different nodes, so both the
erased-node list and every helper's node change per stripe.

The CPU test rehearses the orchestration with gloo, world 3, Clay(4,2): two nodes per rank with the
destination last on the chain, then the six nodes on two ranks with the destination off the chain;
seven stripes in slices of three (a ragged last slice).  The hop is a test-only numpy stand-in for
ClayPatternSet.partialBatchMixed built on the oracle's multiplication table and the columns of each
list's repair map.  The GPU test runs the first chain with the HIP kernel over 12 stripes: three
processes on one GPU, gloo transport.  The destination's rows must equal the oracle's performCoding
per stripe (ClayCodeErasureDecodingStep.java:53-107), with zeros where no list writes.  The stripes
are random bytes, not codewords, and the helpers holding a stripe's erased nodes hold garbage."""
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_chain import ROOT, _setup, _spawn

K, M, N, ALPHA = 4, 2, 6, 8
LISTS = [[1], [4], [0, 3], [], [5], [2, 4]]
IDS_CPU = [2, 255, 0, 3, 5, 1, 4]  # per stripe; 255 names no list, 3 is the empty list
IDS_GPU = [2, 255, 0, 3, 5, 1, 4, 0, 5, 2, 1, 4]


class NumpyClayPartial:
    """Test-only stand-in for the library's hop (CPU tensors)."""

    def __init__(self, lists):
        import oracle as O
        import rpamd
        ecx = rpamd.load()
        self.mt = O.mul_table()
        self.alpha = ALPHA
        self.max_erased = max(len(e) for e in lists)
        self.maps = []  # per list: (rows, {node: [(plane, column of coefficients)]})
        for e in lists:
            cols = {}
            if e:
                mat, ins, outs = ecx.ClayCodeErasureDecodingStep(e, K, M).map().matrix()
                assert list(outs) == list(range(len(e) * ALPHA))
                for j, slot in enumerate(ins):
                    cols.setdefault(int(slot) % N, []).append((int(slot) // N, np.asarray(mat)[:, j]))
            self.maps.append((len(e) * ALPHA, cols))

    def __call__(self, ids, node_of, inp, in_stripe_stride, in_sub_stride, acc, acc_stripe_stride, acc_sub_stride,
                 nstripes, buf_size, is_first):
        x, B = inp.numpy(), buf_size
        a = acc.numpy().reshape(nstripes, -1, B)
        assert acc_sub_stride == B and acc_stripe_stride == a.shape[1] * B and in_sub_stride == B
        for s in range(nstripes):
            p, i = int(ids[s]), int(node_of[s])
            if p >= len(self.maps) or i >= N:
                continue
            rows, cols = self.maps[p]
            for r in range(rows):
                v = np.zeros(B, np.uint8)
                for z, col in cols.get(i, []):
                    if col[r]:
                        v ^= self.mt[int(col[r])][x[s * in_stripe_stride + z * B:s * in_stripe_stride + (z + 1) * B]]
                a[s, r] = v if is_first else a[s, r] ^ v


def _case(ecx, rank, ids_host, node_rank, order, dest, B, slice_stripes, nbuf, device, on_gpu):
    from repair_pipelining_amd.chain import ClayPatternChain
    import oracle as O
    S = len(ids_host)
    rng = np.random.default_rng(23)
    stripes = rng.integers(0, 256, (S, N, ALPHA, B), dtype=np.uint8)  # node-major, every rank the same
    mine = [j for j, r in enumerate(node_rank) if r == rank]
    local = node_of = ids = None
    if mine:
        node_of_host = np.array([[(j + s) % N for s in range(S)] for j in mine], np.uint8)
        loc = np.zeros((S, len(mine), ALPHA, B), np.uint8)
        for slot in range(len(mine)):
            for s in range(S):
                loc[s, slot] = stripes[s, node_of_host[slot, s]]
        local = torch.from_numpy(loc).to(device)
        node_of = torch.from_numpy(node_of_host).to(device)
        ids = torch.tensor(ids_host, dtype=torch.uint8, device=device)
    ps = ecx.ClayPatternSet(LISTS, K, M) if on_gpu else LISTS
    try:
        chain = ClayPatternChain(ps, order, rank, dest=dest, partial_factory=None if on_gpu else NumpyClayPartial)
        rows = chain.n_out_slots
        assert rows == 2 * ALPHA
        out = torch.full((S, rows, B), 0x5A, dtype=torch.uint8, device=device) if rank == dest else None
        chain.run(local, node_of, ids, S, B, out=out, slice_stripes=slice_stripes, n_buffers=nbuf, device=device)
        if on_gpu:
            torch.cuda.synchronize()
    finally:
        if on_gpu:
            ps.close()
    if rank != dest:
        return True
    got = out.cpu().numpy()
    want = np.zeros_like(got)  # zeros fill the rows no list writes
    for s, pid in enumerate(ids_host):
        erased = LISTS[pid] if pid < len(LISTS) else []
        if not erased:
            continue
        inputs = [None if (i % N) in erased else stripes[s, i % N, i // N].copy() for i in range(N * ALPHA)]
        ref = [np.zeros(B, np.uint8) for _ in range(len(erased) * ALPHA)]
        O.Clay(K, M, list(erased)).perform_coding(inputs, ref, B)
        for r, sub in enumerate(ref):
            want[s, r] = sub
    # (stripe 1 has no list; stripe 2 lost one node: rows alpha.. stay zero)
    assert want[2, :ALPHA].any() and not want[1].any() and not want[2, ALPHA:].any()
    return bool((got == want).all())


def _cpu_worker(rank, world, port, q):
    ecx = _setup(rank, world, port)
    try:
        # two nodes per rank, the destination last on the chain
        ok = _case(ecx, rank, IDS_CPU, [0, 0, 1, 1, 2, 2], [0, 1, 2], 2, 96, 3, 2, "cpu", False)
        # the six nodes on ranks 1 and 0 (in that order), the destination off the chain
        ok &= _case(ecx, rank, IDS_CPU, [0, 1, 0, 1, 0, 1], [1, 0], 2, 33, 3, 3, "cpu", False)
        dist.barrier()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_clay_pattern_chain_orchestration_gloo():
    assert _spawn(_cpu_worker, 3) == {0: True, 1: True, 2: True}


def test_clay_pattern_chain_rejects_a_destination_inside_the_chain():
    sys.path[:0] = [str(ROOT), str(ROOT / "oracle")]
    import rpamd
    rpamd.load()
    from repair_pipelining_amd.chain import ClayPatternChain
    with pytest.raises(ValueError):
        ClayPatternChain(LISTS, [0, 1, 2], 0, dest=1, partial_factory=NumpyClayPartial)


def _gpu_worker(rank, world, port, q):
    ecx = _setup(rank, world, port)
    try:
        torch.cuda.set_device(0)
        ecx.set_device(0)
        ok = _case(ecx, rank, IDS_GPU, [0, 0, 1, 1, 2, 2], [0, 1, 2], 2, 4096 + 48, 5, 2, "cuda", True)
        torch.cuda.synchronize()
        dist.barrier()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_clay_pattern_chain_hip_kernel_three_ranks():
    """3 ranks on one GPU (gloo transport staged through the host), k_gf_map_partial_mixed hops."""
    assert _spawn(_gpu_worker, 3) == {0: True, 1: True, 2: True}
