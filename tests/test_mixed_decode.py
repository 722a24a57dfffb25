"""decodeMissingBatchMixed on the GPU (k_gf_apply_mixed, csrc/apply_mixed.hip): a batch whose
stripes miss different shards, decoded in one call, bit-exact against the oracle's decodeMissing
run per stripe (ReedSolomon.java:189-286).

The stripes are fill_random bytes, not codewords, so a rebuilt shard can only equal the oracle's
if it was computed from exactly the shards the reference reads.  Every byte of every shard is
compared: present shards unchanged, rebuilt shards the oracle's, and the bytes outside
[offset, offset + byteCount) unchanged.  RS(4,2), RS(12,4) and RS(17,3) have patterns of 4, 12 and
17 entries: ring depth 4 without padding, depth 8 with 12 padded to 16 and 17 to 24."""
import contextlib
import ctypes
import functools
import gc
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

KERNEL = 0  # hipGraphNodeType (hip_runtime_api.h)
ECX_E_DEVICE = -10
S = 9
# pattern id of each stripe: unsorted, neighbours always differ; 255 names no pattern
IDS = [3, 255, 5, 0, 6, 1, 4, 2, 0]
CODES = [(4, 2), (12, 4), (17, 3)]
# byte_count -> (offset, pitch): one full chunk; full chunks plus a 16-multiple rest; the
# byte-safe path on a padded pitch behind an offset; the published RS(17,3) shard
SIZES = {4096: (0, 4096 + 64), 8192 + 48: (0, 8192 + 48 + 16), 2983: (16, 3072 + 16), 200000: (0, 200000)}


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def patterns_of(k, m):
    """nothing missing; one data shard; one parity shard; two data shards; data plus parity;
    m missing (data and parity); the two-data pattern listed a second time."""
    n = k + m

    def missing(*idx):
        p = np.ones(n, np.uint8)
        p[list(idx)] = 0
        return p

    m_missing = list(range(1, 1 + (m + 1) // 2)) + list(range(n - m // 2, n))
    assert len(m_missing) == m
    return np.stack([missing(), missing(1), missing(k), missing(0, k - 1), missing(2, n - 1), missing(*m_missing),
                     missing(0, k - 1)])


@functools.lru_cache(maxsize=None)
def _oracle_case(k, m, cnt):
    """(input stripes, expected stripes) on the host for one code and size: the oracle's
    decodeMissing per stripe with that stripe's pattern; computed once, shared, never written."""
    import torch
    import rpamd
    ecx = rpamd.load(shape_knobs=True)
    off, pitch = SIZES[cnt]
    n = k + m
    pool = torch.empty((S, n, pitch), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 7100 + 31 * k + cnt)
    torch.cuda.synchronize()
    before = pool.cpu().numpy()
    want = before.copy()
    pats = patterns_of(k, m)
    orc = O.ReedSolomon(k, m)
    for s, pid in enumerate(IDS):
        if pid >= len(pats):
            continue
        shards = [want[s, i].copy() for i in range(n)]
        orc.decode_missing(shards, [bool(f) for f in pats[pid]], off, cnt)
        for i in range(n):
            want[s, i] = shards[i]
    before.setflags(write=False)
    want.setflags(write=False)
    return before, want


def _run(ecx, torch, k, m, cnt, pats, ids, stream=None):
    off, pitch = SIZES[cnt]
    n = k + m
    before, _ = _oracle_case(k, m, cnt)
    pool = torch.from_numpy(before.copy()).cuda()
    dev_ids = torch.tensor(ids, dtype=torch.uint8, device="cuda")
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(pats) as ps:
        rs.decodeMissingBatchMixed(pool, ps, dev_ids, n * pitch, pitch, S, off, cnt, stream)
        torch.cuda.synchronize()
        shape = ecx.last_launch_shape()
    return pool.cpu().numpy(), shape


def _assert_stripes(got, before, want, k, m, cnt, pats, ids):
    off, _ = SIZES[cnt]
    assert (got[:, :, :off] == before[:, :, :off]).all(), "bytes before the window changed"
    assert (got[:, :, off + cnt:] == before[:, :, off + cnt:]).all(), "bytes after the window changed"
    for s, pid in enumerate(ids):
        present = pats[pid] if pid < len(pats) else np.ones(k + m, np.uint8)
        for i in range(k + m):
            if present[i]:
                assert (got[s, i] == before[s, i]).all(), f"stripe {s} (pattern {pid}): present shard {i} changed"
            else:
                assert (got[s, i] == want[s, i]).all(), f"stripe {s} (pattern {pid}): rebuilt shard {i} differs"
    assert (got == want).all()


# every code at the three small sizes; the published 200,000-B shard for RS(17,3) only
CASES = [(k, m, cnt) for (k, m) in CODES for cnt in (4096, 8192 + 48, 2983)] + [(17, 3, 200000)]


@pytest.mark.parametrize("k,m,cnt", CASES)
def test_mixed_decode_matches_the_oracle_per_stripe(ecx, torch_dev, k, m, cnt):
    pats = patterns_of(k, m)
    before, want = _oracle_case(k, m, cnt)
    got, shape = _run(ecx, torch_dev, k, m, cnt, pats, IDS)
    _assert_stripes(got, before, want, k, m, cnt, pats, IDS)
    # the instance of record: the set's depth (8 only when every pattern has >= 12 entries) and
    # 4 accumulator rows (no pattern here misses more than 4); byte-safe launches are not noted
    if cnt >= 4096:
        assert shape == "k_gf_apply_mixed<false, %d, 4>" % (4 if k < 12 else 8), shape


def test_mixed_decode_equals_one_uniform_batch_per_stripe(ecx, torch_dev):
    """RS(12,4), 4096 B: the mixed call's bytes equal decodeMissingBatch called once per stripe
    with that stripe's shardPresent -- all a caller could do before."""
    torch = torch_dev
    k, m, cnt = 12, 4, 4096
    off, pitch = SIZES[cnt]
    n = k + m
    pats = patterns_of(k, m)
    before, _ = _oracle_case(k, m, cnt)
    mixed, _ = _run(ecx, torch, k, m, cnt, pats, IDS)
    pool = torch.from_numpy(before.copy()).cuda()
    rs = ecx.ReedSolomon.create(k, m)
    for s, pid in enumerate(IDS):
        if pid < len(pats):
            rs.decodeMissingBatch(pool[s:], [bool(f) for f in pats[pid]], n * pitch, pitch, 1, off, cnt)
    torch.cuda.synchronize()
    assert (pool.cpu().numpy() == mixed).all()


def test_sets_of_different_row_counts_agree_on_shared_stripes(ecx, torch_dev):
    """A set whose patterns all miss at most 2 shards and a set that also holds the 4-erasure
    pattern give the same bytes on the stripes that use the shared patterns; the stripe of the
    4-erasure pattern is untouched by the first set (its id names no pattern there)."""
    k, m, cnt = 12, 4, 4096
    pats = patterns_of(k, m)
    before, _ = _oracle_case(k, m, cnt)
    narrow = np.stack([pats[0], pats[1], pats[2], pats[3], pats[4]])       # ids 0..4, at most 2 missing
    wide = np.stack([pats[0], pats[1], pats[2], pats[3], pats[4], pats[5]])  # id 5: 4 missing
    ids = [3, 5, 1, 0, 4, 2, 5, 3, 0]
    got_n, _ = _run(ecx, torch_dev, k, m, cnt, narrow, ids)
    got_w, _ = _run(ecx, torch_dev, k, m, cnt, wide, ids)
    with ecx.ReedSolomon.create(k, m).patternSet(narrow) as a, ecx.ReedSolomon.create(k, m).patternSet(wide) as b:
        assert a.info()[2] == 2 and b.info()[2] == 4
    shared = [s for s, pid in enumerate(ids) if pid != 5]
    assert (got_n[shared] == got_w[shared]).all()
    for s in (1, 6):
        assert (got_n[s] == before[s]).all()
    orc = O.ReedSolomon(k, m)
    off, _ = SIZES[cnt]
    for s, pid in enumerate(ids):
        shards = [before[s, i].copy() for i in range(k + m)]
        orc.decode_missing(shards, [bool(f) for f in wide[pid]], off, cnt)
        assert all((got_w[s, i] == shards[i]).all() for i in range(k + m)), s


@pytest.mark.parametrize("k,m,depth", [(10, 6, 4), (12, 6, 8)])
def test_patterns_of_more_than_four_rows(ecx, torch_dev, k, m, depth):
    """The 8-row instances (a pattern that misses more than 4 shards), at both ring depths:
    RS(10,6) has 10 entries per pattern (depth 4, padded to 12), RS(12,6) 12 (depth 8, padded to
    16).  Three stripes -- 6 missing, one missing, nothing missing -- over full chunks plus a rest."""
    torch = torch_dev
    n, cnt, pitch = k + m, 8192 + 48, 8192 + 64
    six = np.ones(n, np.uint8)
    six[[0, 3, k - 1, k, k + 2, n - 1]] = 0
    one = np.ones(n, np.uint8)
    one[2] = 0
    pats = np.stack([six, one, np.ones(n, np.uint8)])
    ids = [1, 0, 2]
    pool = torch.empty((3, n, pitch), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 7300 + k)
    before = pool.cpu().numpy()
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(pats) as ps:
        assert ps.info() == (3, n, 6)
        rs.decodeMissingBatchMixed(pool, ps, torch.tensor(ids, dtype=torch.uint8, device="cuda"), n * pitch, pitch, 3,
                                   0, cnt)
        torch.cuda.synchronize()
        assert ecx.last_launch_shape() == "k_gf_apply_mixed<false, %d, 8>" % depth
    got = pool.cpu().numpy()
    orc = O.ReedSolomon(k, m)
    for s, pid in enumerate(ids):
        shards = [before[s, i].copy() for i in range(n)]
        orc.decode_missing(shards, [bool(f) for f in pats[pid]], 0, cnt)
        assert all((got[s, i] == shards[i]).all() for i in range(n)), s
    assert (got[:, :, cnt:] == before[:, :, cnt:]).all()


# ---------------------------------------------------------------- stream capture
# (graph inspection as tests/test_gpu_capture.py does it)
_hip = None


def _hip_runtime():
    """The HIP runtime object this process has already mapped, opened by the path it was mapped
    from (torch's own copy and the system's differ: a second one is never loaded)."""
    global _hip
    if _hip is None:
        paths = set()
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split(None, 5)
                if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith("libamdhip64.so"):
                    paths.add(os.path.realpath(parts[5].strip()))
        assert len(paths) == 1, f"expected exactly one mapped HIP runtime, found {sorted(paths)}"
        hip = ctypes.CDLL(paths.pop())
        hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                         ctypes.POINTER(ctypes.c_size_t)]
        hip.hipGraphGetNodes.restype = ctypes.c_int
        hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        hip.hipGraphNodeGetType.restype = ctypes.c_int
        _hip = hip
    return _hip


def node_types(g):
    hip = _hip_runtime()
    graph = ctypes.c_void_p(int(g.raw_cuda_graph()))
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    if n.value == 0:
        return []
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    types = []
    for i in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) == 0
        types.append(t.value)
    return sorted(types)


@contextlib.contextmanager
def capturing(torch, g):
    """torch.cuda.graph(g) with Python's cyclic collector off: torch destroys a CUDAGraph with HIP
    calls the runtime refuses on a capturing thread (tests/test_gpu_capture.py)."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            yield
    finally:
        if was_enabled:
            gc.enable()


def test_mixed_decode_under_stream_capture(ecx, torch_dev):
    """A fresh set's first call on a capturing stream is refused (its plan upload allocates and
    copies) and leaves the graph empty.  After one call outside capture the same call captures as
    kernel nodes only -- the full chunks and the byte-safe rest -- and two replays over
    re-scribbled pools equal the eager result and the oracle."""
    torch = torch_dev
    k, m, cnt = 12, 4, 8192 + 48
    off, pitch = SIZES[cnt]
    n = k + m
    pats = patterns_of(k, m)
    before, want = _oracle_case(k, m, cnt)
    pool = torch.from_numpy(before.copy()).cuda()
    dev_ids = torch.tensor(IDS, dtype=torch.uint8, device="cuda")
    rs = ecx.ReedSolomon.create(k, m)
    with rs.patternSet(pats) as ps:
        def call(p):
            rs.decodeMissingBatchMixed(p, ps, dev_ids, n * pitch, pitch, S, off, cnt)

        g0 = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g0):
            with pytest.raises(ecx.EcxError) as err:
                call(pool)
        assert err.value.code == ECX_E_DEVICE and "once outside the capture" in str(err.value), str(err.value)
        assert node_types(g0) == []
        assert (pool.cpu().numpy() == before).all()

        call(pool)  # outside capture: the plan becomes resident
        torch.cuda.synchronize()
        _assert_stripes(pool.cpu().numpy(), before, want, k, m, cnt, pats, IDS)

        g = torch.cuda.CUDAGraph(keep_graph=True)
        with capturing(torch, g):
            call(pool)
        types = node_types(g)
        assert len(types) == 2 and set(types) == {KERNEL}, types
        for seed in (7201, 7202):
            ecx.fill_random(pool, pool.numel(), seed)  # whatever the last run left is gone
            eager = pool.clone()
            g.replay()
            torch.cuda.synchronize()
            call(eager)
            torch.cuda.synchronize()
            assert torch.equal(pool, eager), seed
        # and on the case's own input the replay gives the oracle's bytes
        pool.copy_(torch.from_numpy(before.copy()))
        g.replay()
        torch.cuda.synchronize()
        _assert_stripes(pool.cpu().numpy(), before, want, k, m, cnt, pats, IDS)
        del g, g0
