"""Stream capture: every device batch entry point takes a caller stream, and a caller who
replays a fixed repair pipeline captures it into a HIP graph (INTEGRATION.md
"Stream capture").  These tests capture each entry point on a single stream (torch.cuda.graph,
the library picking torch's current stream), list the captured graph's node types through the
HIP runtime the process has already mapped, and check that a replay reads the buffers' current
contents and writes the bytes an eager call and the oracle write -- for every kernel family of
the product library, with the launch shape frozen at capture time.  They also pin that the
library leaves no event of its own in a caller's graph, that layout selection stays out of
captures, and that a first use inside a capture is refused before any HIP allocation or copy.

Every capture is a linear chain on one stream, and every call is run once eagerly with the same
arguments before it is captured (the first-use test excepted)."""
import contextlib
import ctypes
import gc
import importlib.util
import os
from pathlib import Path

import numpy as np
import pytest

import oracle as O
from conftest import gf_apply_numpy, shortened_clay_oracle

pytestmark = pytest.mark.gpu

# hipGraphNodeType (hip_runtime_api.h)
KERNEL, MEMCPY, MEMSET, HOST, WAIT_EVENT, EVENT_RECORD = 0, 1, 2, 3, 6, 7
ECX_E_DEVICE = -10
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# ---------------------------------------------------------------- graph inspection
_hip = None


def _hip_runtime():
    """The HIP runtime object this process has already mapped (torch's own copy and the system's
    differ, so a second one is never loaded): found among the loaded objects, opened by the
    path it was mapped from, which hands back the same handle."""
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
    """The node types of a captured torch.cuda.CUDAGraph(keep_graph=True), sorted."""
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
    """torch.cuda.graph(g) with Python's cyclic collector out of the way.  torch destroys a
    CUDAGraph with HIP calls the runtime refuses on a thread that is capturing, and its destructor
    then aborts the process; an earlier test's graph that sits in a reference cycle (a frame, its
    closures, a pytest.raises record) is destroyed whenever the collector happens to run.  So the
    cycles are collected before the capture begins and the collector is off until it has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            yield
    finally:
        if was_enabled:
            gc.enable()


def capture(torch, fn):
    """fn() captured on one stream into a graph that keeps its hipGraph_t for inspection."""
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with capturing(torch, g):
        fn()
    return g


def kernels_only(types, at_least=1):
    return len(types) >= at_least and set(types) == {KERNEL}


def replay_twice(ecx, torch, call, inp, out, types_ok, verify, seeds, prepare=None, after_capture=None):
    """Warm up call(inp, out) eagerly, capture it, check the node types (types_ok), then twice:
    refill `inp` with a new seed (prepare(inp) shapes it further), fill a separate `out` with the
    sentinel, replay, and assert the replay wrote what an eager call on a clone of the same input
    writes and left the input alone; verify(input before the replay, output) -- both host arrays
    -- holds the oracle and the guard bytes.  `out` is `inp` for an in-place call."""
    in_place = out is inp
    call(inp, out)
    torch.cuda.synchronize()
    g = capture(torch, lambda: call(inp, out))
    if after_capture:
        after_capture()
    types = node_types(g)
    assert types_ok(types), types
    for seed in seeds:
        ecx.fill_random(inp, inp.numel(), seed)
        if prepare:
            prepare(inp)
        if not in_place:
            out.fill_(SENTINEL)
        before = inp.clone()
        g.replay()
        torch.cuda.synchronize()
        ein = before.clone()
        eout = ein if in_place else torch.full_like(out, SENTINEL)
        call(ein, eout)
        torch.cuda.synchronize()
        assert torch.equal(out, eout), seed
        assert in_place or torch.equal(inp, before), seed
        verify(before.cpu().numpy(), out.cpu().numpy())
    return g, types


# ---------------------------------------------------------------- 1. replay parity per kernel family
# (map, byte count, pitch kind, offset, in place, accumulate, knob) over three stripes: the cases of
# test_launch_plan_names_what_runs that reach each kernel family, and what each must run
MAP_CASES = [
    ("clay42_rep1", 65536, "r16", 0, 0, 0, "", "deep"),        # k_gf_apply on 256 threads, ring of 20
    ("rs124_dec01", 65536, "r16", 0, 1, 0, "", "wave"),        # one-wave workgroups, a 64 KiB pitch
    ("lrc_rep0", 65536, "r16", 0, 1, 0, "", "small"),          # the small-row instance
    ("clay42_enc45", 65536, "r16", 0, 0, 0, "wide_tiles=0", "tlds"),  # LDS tables: dynamic LDS
    ("rs173_enc", 8208, "r16", 0, 1, 0, "", "tail"),           # k_gf_apply_tail: one node
    ("rs124_dec01", 4000, "r16", 1, 0, 0, "", "bytesafe"),     # slots off 16 B: the byte-safe launch
    ("clay42_rep03", 65536, "r16", 0, 0, 0, "", "wide"),       # k_gf_apply_wide
    ("rs173_enc", 65536, "r16", 0, 1, 0, "skew_chunks=2", "skew"),
    ("clay42_rep03", 65536, "r16", 0, 0, 0, "map_planes=2", "planes"),  # a module launch
    ("rs173_enc", 8208, "r16", 0, 1, 1, "map_planes=2", "planes"),      # ... accumulating
    ("rs173_enc", 65536, "pad", 0, 0, 1, "", "acc"),           # accumulate_batch, one tile
    ("clay42_enc45", 8208, "pad", 0, 0, 1, "", "acc"),         # accumulate_batch, two tiles
]


def _recorder():
    """scripts/record_launch_shapes.py: the maps, layouts and knob defaults of the launch-shape grid."""
    path = Path(__file__).resolve().parents[1] / "scripts" / "record_launch_shapes.py"
    spec = importlib.util.spec_from_file_location("record_launch_shapes", path)
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


def _map_case(ecx, torch, rec, gmap, name, n, p, o, ip, acc, kind, seeds):
    """One map case through replay_twice; returns the family of the kernel of record."""
    S = 3
    io, iss, isl, oo, oss, osl, in_bytes, out_bytes = rec.layout(gmap, {"n": n, "p": p, "o": o, "ip": ip, "S": S})
    inp = torch.empty(in_bytes, dtype=torch.uint8, device="cuda")
    out = inp if ip else torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    if ip:
        oo = io
    mat, ins, outs = gmap.matrix()
    fn = "accumulate_batch" if acc else "apply_batch"

    def call(i, t):
        getattr(gmap, fn)(i[io:], iss, isl, t[oo:], oss, osl, S, n)

    shape_before = ecx.last_launch_shape()
    plan = gmap.launch_plan(inp.data_ptr() + io, iss, isl, out.data_ptr() + oo, oss, osl, S, n, bool(acc))
    seen = {}

    def after_capture():  # the shape frozen into the graph is the static rules' plan
        seen["shape"], seen["kernel"] = ecx.last_launch_shape(), ecx.last_kernel()

    written = np.zeros(out.numel(), bool)
    for s in range(S):
        for slot in outs:
            written[oo + s * oss + int(slot) * osl:][:n] = True

    def verify(before, got):
        prior = before if ip else np.full(got.shape, SENTINEL, np.uint8)
        assert (got[~written] == prior[~written]).all(), (name, "bytes outside the outputs were written")
        for s in (0, S - 1):
            ref = gf_apply_numpy(mat, [before[io + s * iss + int(j) * isl:][:n] for j in ins])
            for r, slot in zip(ref, outs):
                at = oo + s * oss + int(slot) * osl
                want = r ^ prior[at:at + n] if acc else r
                assert (got[at:at + n] == want).all(), (name, s, int(slot))

    ok = (lambda t: t == [KERNEL]) if kind == "tail" else kernels_only
    replay_twice(ecx, torch, call, inp, out, ok, verify, seeds, after_capture=after_capture)
    if kind == "bytesafe":  # no full-chunk kernel: no kernel of record, the string stays
        assert plan == "" and seen["shape"] == shape_before, (plan, seen)
        return None
    assert plan and seen["shape"] == plan, (name, plan, seen)
    params = plan.split("<")[-1].split(">")[0].split(", ")
    if kind == "deep":
        assert plan.startswith("k_gf_apply<") and params[3] == "20" and params[5] == "256", plan
    elif kind == "wave":
        assert plan.startswith("k_gf_apply<") and params[5] == "64", plan
    elif kind == "small":
        assert plan.startswith("k_gf_apply<") and params[6] == "2", plan
    elif kind == "tlds":
        assert plan.startswith("k_gf_apply<") and params[4] == "true", plan
    return seen["kernel"].split("<")[0]


def test_replay_parity_of_every_map_kernel_family(ecx, torch_dev):
    """apply_batch / accumulate_batch captured and replayed, per kernel family of the product
    library: k_gf_apply on 256 threads with its deep ring, on one wave, its small-row and
    LDS-table (dynamic LDS) instances, k_gf_apply_tail (exactly one node), the byte-safe launch of
    a layout off 16 B, k_gf_apply_wide, k_gf_apply_skew, k_map_planes (a module launch) writing
    and accumulating, and accumulate_batch on a one-tile and a two-tile map (the sentinel shows
    through as an XOR).  Each graph holds kernel nodes only, last_launch_shape() at capture is
    GfMap.launch_plan, and each of two replays on refilled buffers equals an eager call on every
    byte and gf_apply_numpy on the first and last stripe, the bytes outside the outputs untouched."""
    torch = torch_dev
    rec = _recorder()
    maps = rec.build_maps(ecx)
    families = set()
    try:
        for i, (name, n, p, o, ip, acc, k, kind) in enumerate(MAP_CASES):
            rec.set_knob(ecx, k)
            fam = _map_case(ecx, torch, rec, maps[name], name, n, p, o, ip, acc, kind, (1000 + 2 * i, 1001 + 2 * i))
            if fam:
                families.add(fam)
    finally:
        rec.set_knob(ecx, "")
    want = {"k_gf_apply", "k_gf_apply_tail", "k_gf_apply_wide", "k_gf_apply_skew", "k_map_planes"}
    assert families >= want, want - families


@pytest.mark.parametrize("group,kernel", [(1, "k_clay_repair_grp"), (0, "k_clay_repair")])
def test_replay_parity_of_generated_clay_kernels(ecx, torch_dev, group, kernel):
    """Shortened Clay(10,4) repair of node 3 (4 KiB sub-chunks, five stripes) through the
    generated plane-group and per-plane kernels (hipModuleLaunchKernel): kernel nodes only,
    last_kernel() names the generated kernel, and two replays on refilled stripes equal an eager
    call and shortened_clay_oracle on the first and last stripe."""
    torch = torch_dev
    k, m, v, e, B, S = 10, 4, 2, 3, 4096, 5
    step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
    n, a = k + m, step.subPacketSize
    pool = torch.empty((S, n * a, B), dtype=torch.uint8, device="cuda")
    out = torch.empty((S, a, B), dtype=torch.uint8, device="cuda")
    seen = {}

    def call(i, t):
        step.performCodingBatch(i, n * a * B, B, t, a * B, B, S, B)

    def verify(before, got):
        for s in (0, S - 1):
            inputs = [None if (i % n) == e else before[s, i].copy() for i in range(n * a)]
            ref = shortened_clay_oracle(k, m, v, [e], inputs, B)
            bad = [z for z in range(a) if not (got[s, z] == ref[z]).all()]
            assert not bad, (group, s, bad[:8])

    try:
        ecx.tune("rtc_group", group)
        replay_twice(ecx, torch, call, pool, out, kernels_only, verify, (2000 + group, 2010 + group),
                     after_capture=lambda: seen.update(kernel=ecx.last_kernel()))
    finally:
        ecx.tune("rtc_group", 1)
    assert seen["kernel"] == kernel, seen


@pytest.mark.parametrize("first,launches", [(0, 1), (16, 1), (5, 3)])
def test_replay_parity_of_is_parity_correct_batch(ecx, torch_dev, first, launches):
    """isParityCorrectBatch (the verdicts set to 1, then k_gf_check's launches), RS(4,2),
    L = 3 * 4096, four stripes: firstByte 0 and 16 on the aligned layout, and 5, whose head up to
    the 16-B boundary goes to the byte-safe kernel -- three check launches.  With one byte of one
    stripe corrupted between replays, the replayed verdicts equal an eager call's and the oracle's
    isParityCorrect per stripe.  The graph holds kernel nodes only: the verdicts were set by a
    hipMemsetAsync, i.e. one memset node, until this test showed that the HIP runtime replays a
    memset node with the value 0 from its second replay on in every graph of a process but the
    first (a graph of the memset alone does it; [0, 0, 0, 0] where [1, 1, 0, 1] was due), so the
    library sets them with a kernel, k_set_verdicts: one node more than the check's launches."""
    torch = torch_dev
    k, m, L, S = 4, 2, 3 * 4096, 4
    n, pitch = k + m, 16 + 3 * 4096 + 32
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.empty((S, n, pitch), dtype=torch.uint8, device="cuda")
    verdict = torch.empty(S + 16, dtype=torch.uint8, device="cuda")  # 16 guard bytes
    flips = iter([(1, 0, first + 7), (2, n - 1, first + L - 1)])  # (stripe, shard, byte): data, then parity

    def call(i, t):
        rs.isParityCorrectBatch(i, n * pitch, pitch, S, first, L, t)

    def prepare(p):  # codewords over the whole pitch, so every window passes; then one flipped byte
        rs.encodeParityBatch(p, n * pitch, pitch, S, 0, pitch)
        s, i, b = next(flips)
        p[s, i, b] ^= 0x81

    def verify(before, got):
        want = [int(O.ReedSolomon(k, m).is_parity_correct([before[s, i].copy() for i in range(n)], first, L))
                for s in range(S)]
        assert sorted(want) == [0, 1, 1, 1], want
        assert got[:S].tolist() == want and (got[S:] == SENTINEL).all(), (got.tolist(), want)

    seen = {}
    _, types = replay_twice(ecx, torch, call, pool, verdict, kernels_only, verify,
                            (3000 + first, 3100 + first), prepare=prepare,
                            after_capture=lambda: seen.update(kernel=ecx.last_kernel()))
    assert len(types) == 1 + launches, types  # k_set_verdicts, then the check's launches
    assert seen["kernel"].startswith("k_gf_check<"), seen


@pytest.mark.parametrize("op", ["encode", "decode"])
def test_replay_parity_of_blocked_batches(ecx, torch_dev, op):
    """encodeParityBlockedBatch / decodeMissingBlockedBatch, RS(4,2), L = 104,449 in 4 KiB blocks:
    a body pass plus a tail pass, so at least two kernel nodes and nothing else.  Two replays on
    repacked stripes equal an eager call and the oracle's encodeParity / decodeMissing (on
    non-codewords) on the first and last stripe; the bytes past the batch stay."""
    torch = torch_dev
    k, m, L, S, b = 4, 2, 104449, 3, 4096
    n, total = k + m, 3 * 6 * 104449
    rs = ecx.ReedSolomon.create(k, m)
    present = [True] * n
    if op == "decode":
        present[0] = present[n - 1] = False
    flat = torch.empty(total + 64, dtype=torch.uint8, device="cuda")

    def call(i, t):
        if op == "encode":
            rs.encodeParityBlockedBatch(i, S, L, b)
        else:
            rs.decodeMissingBlockedBatch(i, present, S, L, b)

    def verify(before, got):
        assert (got[total:] == before[total:]).all()
        nat = ecx.blocked_unpack(torch.from_numpy(before[:total]), S, n, L, b).numpy()
        res = ecx.blocked_unpack(torch.from_numpy(got[:total]), S, n, L, b).numpy()
        for s in (0, S - 1):
            ref = [nat[s, i].copy() for i in range(n)]
            if op == "encode":
                O.ReedSolomon(k, m).encode_parity(ref, 0, L)
            else:
                O.ReedSolomon(k, m).decode_missing(ref, present, 0, L)
            assert all((res[s, i] == ref[i]).all() for i in range(n)), (op, s)

    replay_twice(ecx, torch, call, flat, flat, lambda t: kernels_only(t, 2), verify, (4000, 4001))


def test_replay_parity_of_rs_batch_codec_entry_points(ecx, torch_dev):
    """encodeParityBatch and decodeMissingBatch over a byte window (offset 16, 2,983 bytes, a
    padded pitch), RS(12,4), three stripes, in place: kernel nodes only, two replays each equal
    to an eager call and to the oracle on the first and last stripe, the bytes outside the
    window untouched (they equal the input's)."""
    torch = torch_dev
    k, m, S, pitch, off, cnt = 12, 4, 3, 3072 + 16, 16, 2983
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    present = [False, True, True, False] + [True] * 12
    for op in ("encode", "decode"):
        pool = torch.empty((S, n, pitch), dtype=torch.uint8, device="cuda")

        def call(i, t, op=op):
            if op == "encode":
                rs.encodeParityBatch(i, n * pitch, pitch, S, off, cnt)
            else:
                rs.decodeMissingBatch(i, present, n * pitch, pitch, S, off, cnt)

        def verify(before, got, op=op):
            assert (got[:, :, :off] == before[:, :, :off]).all() and (got[:, :, off + cnt:] == before[:, :, off + cnt:]).all()
            for s in (0, S - 1):
                ref = [before[s, i].copy() for i in range(n)]
                if op == "encode":
                    O.ReedSolomon(k, m).encode_parity(ref, off, cnt)
                else:
                    O.ReedSolomon(k, m).decode_missing(ref, present, off, cnt)
                assert all((got[s, i] == ref[i]).all() for i in range(n)), (op, s)

        replay_twice(ecx, torch, call, pool, pool, kernels_only, verify, (5000, 5001) if op == "encode" else (5002, 5003))


def test_replay_parity_of_partial_sum_chains(ecx, torch_dev):
    """decodePartialBatch and encodePartialBatch: a chain of four links captured in ONE graph
    (isFirst on the first link), RS(4,2), three stripes.  Kernel nodes only, at least four; two
    replays equal the eager chain; the decode chain's data row equals the oracle's
    decodeMissingSingle chain and the encode chain equals the oracle's encodeParity, on the
    first and last stripe; the accumulator's guard bytes keep the sentinel."""
    torch = torch_dev
    k, m, L, S, P = 4, 2, 8192 + 32, 3, 8192 + 32 + 48
    rs = ecx.ReedSolomon.create(k, m)
    present = [True, False, True, True, True, False]  # missing data 1 and parity 5
    chain = [0, 2, 3, 4]
    pool = torch.empty((S, 6, L), dtype=torch.uint8, device="cuda")
    acc = torch.empty((S, 2, P), dtype=torch.uint8, device="cuda")

    def decode_chain(i, t):
        for c, idx in enumerate(chain):
            rs.decodePartialBatch(present, idx, i[:, idx], 6 * L, t, 2 * P, P, S, L, c == 0)

    def encode_chain(i, t):
        for c in range(k):
            rs.encodePartialBatch(c, i[:, c], 6 * L, t, 2 * P, P, S, L, c == 0)

    def verify_decode(before, got):
        assert (got[:, :, L:] == SENTINEL).all()
        for s in (0, S - 1):
            ref = [np.zeros(L, np.uint8)]
            for c, idx in enumerate(chain):
                O.ReedSolomon(k, m).decode_missing_single(before[s, idx].copy(), idx, c, present, ref, 0, L, c == 0)
            assert (got[s, 0, :L] == ref[0]).all(), s

    def verify_encode(before, got):
        assert (got[:, :, L:] == SENTINEL).all()
        for s in (0, S - 1):
            ref = [before[s, i].copy() for i in range(6)]
            O.ReedSolomon(k, m).encode_parity(ref, 0, L)
            assert (got[s, 0, :L] == ref[4]).all() and (got[s, 1, :L] == ref[5]).all(), s

    replay_twice(ecx, torch, decode_chain, pool, acc, lambda t: kernels_only(t, 4), verify_decode, (6000, 6001))
    replay_twice(ecx, torch, encode_chain, pool, acc, lambda t: kernels_only(t, 4), verify_encode, (6002, 6003))


def test_replay_parity_of_lrc_batches(ecx, torch_dev):
    """LRC encodeBatch and decodeBatch (16 KiB blocks, three stripes, in place): kernel nodes
    only; two replays equal an eager call; the parities equal the oracle's RS(3,1) encodeParity
    and the rebuilt blocks its decodeMissing per group, on the first and last stripe."""
    torch = torch_dev
    B, S, P = 16384, 3, 16384 + 64
    present = [True] * 16
    for i in (1, 7, 14):
        present[i] = False
    pool = torch.empty((S, 16, P), dtype=torch.uint8, device="cuda")

    def verify(before, got, decode):
        assert (got[:, :, B:] == before[:, :, B:]).all()
        for s in (0, S - 1):
            for g in range(4):
                blk = [before[s, 4 * g + j, :B].copy() for j in range(4)]
                if decode:
                    O.ReedSolomon(3, 1).decode_missing(blk, present[4 * g:4 * g + 4], 0, B)
                else:
                    O.ReedSolomon(3, 1).encode_parity(blk, 0, B)
                assert all((got[s, 4 * g + j, :B] == blk[j]).all() for j in range(4)), (decode, s, g)

    replay_twice(ecx, torch, lambda i, t: ecx.LRCErasureCode.encodeBatch(i, 16 * P, P, S, B), pool, pool, kernels_only,
                 lambda b, g: verify(b, g, False), (7000, 7001))
    replay_twice(ecx, torch, lambda i, t: ecx.LRCErasureCode.decodeBatch(i, 16 * P, P, present, S, B), pool, pool,
                 kernels_only, lambda b, g: verify(b, g, True), (7002, 7003))


# ---------------------------------------------------------------- 2. a pipeline in one graph
def test_pipeline_in_one_graph_keeps_its_order(ecx, torch_dev):
    """One graph: fill_random(pool) -> RS(12,4) encodeParityBatch -> a captured copy_ of two
    shards -> zero those shards -> decodeMissingBatch -> count_mismatch against the copy.  Replayed
    three times over a scribbled pool, the counter reads 0 each time and the decoded shards equal
    the oracle's decodeMissing on one stripe: launches of different entry points keep their order
    inside one capture."""
    torch = torch_dev
    k, m, L, S = 12, 4, 65536, 3
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    present = [False, False] + [True] * 14
    pool = torch.empty((S, n, L), dtype=torch.uint8, device="cuda")
    saved = torch.empty((S, 2, L), dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")

    def pipeline():
        ecx.fill_random(pool, pool.numel(), 8000)
        rs.encodeParityBatch(pool, n * L, L, S, 0, L)
        saved.copy_(pool[:, 0:2])
        pool[:, 0:2].zero_()
        count.zero_()
        rs.decodeMissingBatch(pool, present, n * L, L, S, 0, L)
        ecx.count_mismatch(pool, n * L, saved, 2 * L, S, 2 * L, count)

    pipeline()
    torch.cuda.synchronize()
    assert int(count.item()) == 0
    g = capture(torch, pipeline)
    types = node_types(g)
    assert set(types) <= {KERNEL, MEMCPY, MEMSET} and types.count(KERNEL) >= 4, types
    for r in range(3):
        ecx.fill_random(pool, pool.numel(), 8100 + r)
        saved.fill_(SENTINEL)
        count.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert int(count.item()) == 0, r
        assert torch.equal(pool[:, 0:2], saved), r
    host = pool[S - 1].cpu().numpy()
    shards = [np.zeros(L, np.uint8) if i < 2 else host[i].copy() for i in range(n)]
    O.ReedSolomon(k, m).decode_missing(shards, present, 0, L)
    assert (shards[0] == host[0]).all() and (shards[1] == host[1]).all()
    data = [host[i].copy() for i in range(n)]  # the decoded stripe is the codeword of its data
    O.ReedSolomon(k, m).encode_parity(data, 0, L)
    assert all((data[i] == host[i]).all() for i in range(k, n))


# ---------------------------------------------------------------- 3. large launches capture no event
def _no_library_event(types, allowed):
    """The first assertion of every large capture: nothing of the library's launch registry in
    the caller's graph (an event record would outlive the event, a wait has no business here).
    On the ROCm 7.0 runtime a plain hipEventRecord on a capturing stream adds no node -- it ties
    the library's event to the capture instead -- so the node list reads the same with and without
    the registry's capture check (kernels only, measured on both); the assertion pins the contract
    on a runtime that does add the node, and the replays after it pin the bytes."""
    assert WAIT_EVENT not in types and EVENT_RECORD not in types, types
    assert set(types) <= allowed and KERNEL in types, types


def _large_apply_capture(ecx, torch):
    """Clay(4,2) repair of node 1, B = 4,096, S = 1,024: the repair map reads 20 of a stripe's 48
    sub-chunks, so the launch registry counts 80 MiB of input, a large launch (512 stripes would
    count 40 MiB and never reach the event path).  Warmed up and captured; the node check comes
    before anything is replayed."""
    k, m, B, S, e = 4, 2, 4096, 1024, 1
    step = ecx.ClayCodeErasureDecodingStep([e], k, m)
    gmap = step.map()
    pool = torch.empty((S, 48, B), dtype=torch.uint8, device="cuda")
    out = torch.empty((S, 8, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 9000)
    assert S * gmap.info()["n_in"] * B >= 64 << 20

    def call(i, t):
        gmap.apply_batch(i, 48 * B, B, t, 8 * B, B, S, B)

    call(pool, out)
    torch.cuda.synchronize()
    g = capture(torch, lambda: call(pool, out))
    types = node_types(g)
    _no_library_event(types, {KERNEL})
    return g, types, step, call, pool, out


def _check_clay42_replays(ecx, torch, g, call, pool, out, seeds, e=1):
    k, m, B = 4, 2, 4096
    n, S = k + m, pool.shape[0]
    for seed in seeds:
        ecx.fill_random(pool, pool.numel(), seed)
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        eout = torch.full_like(out, SENTINEL)
        call(pool.clone(), eout)
        torch.cuda.synchronize()
        assert torch.equal(out, eout), seed
        host, got = pool[S - 1].cpu().numpy(), out[S - 1].cpu().numpy()
        inputs = [None if (i % n) == e else host[i].copy() for i in range(48)]
        ref = [np.zeros(B, np.uint8) for _ in range(8)]
        O.Clay(k, m, [e]).perform_coding(inputs, ref, B)
        assert all((got[z] == ref[z]).all() for z in range(8)), seed


def test_large_apply_batch_captures_no_event(ecx, torch_dev):
    """launch_apply with >= 64 MiB of input on a capturing stream: the graph holds kernel nodes
    and nothing else -- no event-record node of the launch registry (the registry would destroy
    that event while the instantiated graph still records it).  Only then: a replay on a
    refilled pool equals an eager call and the oracle on one stripe."""
    torch = torch_dev
    g, types, step, call, pool, out = _large_apply_capture(ecx, torch)
    print("large apply_batch capture, node types:", types)
    _check_clay42_replays(ecx, torch, g, call, pool, out, (9001,))


def test_large_check_batch_captures_no_event(ecx, torch_dev):
    """launch_check with >= 64 MiB of input (RS(17,3), L = 65,536, S = 64) on a capturing stream:
    kernel nodes only (the verdicts are set by a kernel), no event node.  Only then: the replayed
    verdicts name the one corrupted stripe."""
    torch = torch_dev
    k, m, L, S = 17, 3, 65536, 64
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    pool = torch.empty((S, n, L), dtype=torch.uint8, device="cuda")
    verdict = torch.empty(S, dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 9100)
    rs.encodeParityBatch(pool, n * L, L, S, 0, L)
    assert S * n * L >= 64 << 20
    rs.isParityCorrectBatch(pool, n * L, L, S, 0, L, verdict)
    torch.cuda.synchronize()
    g = capture(torch, lambda: rs.isParityCorrectBatch(pool, n * L, L, S, 0, L, verdict))
    types = node_types(g)
    print("large isParityCorrectBatch capture, node types:", types)
    _no_library_event(types, {KERNEL})
    assert len(types) == 2, types  # k_set_verdicts and one k_gf_check launch
    pool[37, 5, 4097] ^= 0x10
    verdict.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [0 if s == 37 else 1 for s in range(S)]
    sh = [pool[37, i].cpu().numpy() for i in range(n)]
    assert not O.ReedSolomon(k, m).is_parity_correct(sh, 0, L)
    sh = [pool[36, i].cpu().numpy() for i in range(n)]
    assert O.ReedSolomon(k, m).is_parity_correct(sh, 0, L)


def test_large_clay_batch_captures_no_event(ecx, torch_dev):
    """The generated Clay kernel's launch (ecx_clay_perform_coding_batch, shortened Clay(10,4),
    node 3) with enough stripes that the registry counts >= 64 MiB: kernel nodes only, no event
    node.  Only then: a replay equals an eager call and the shortened oracle on one stripe."""
    torch = torch_dev
    k, m, v, e, B = 10, 4, 2, 3, 4096
    step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
    n, a = k + m, step.subPacketSize
    slots = step.map().max_slots()[0] + 1  # the step's input slots: the registry counts B bytes of each
    S = -(-(64 << 20) // (B * slots)) + 1   # one stripe to spare
    pool = torch.empty((S, n * a, B), dtype=torch.uint8, device="cuda")
    out = torch.empty((S, a, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 9200)

    def call(i, t):
        step.performCodingBatch(i, n * a * B, B, t, a * B, B, S, B)

    call(pool, out)
    torch.cuda.synchronize()
    assert ecx.last_kernel() == "k_clay_repair_grp", ecx.last_kernel()
    g = capture(torch, lambda: call(pool, out))
    assert ecx.last_kernel() == "k_clay_repair_grp", ecx.last_kernel()
    types = node_types(g)
    print("large performCodingBatch capture, node types:", types, "stripes:", S)
    _no_library_event(types, {KERNEL})
    ecx.fill_random(pool, pool.numel(), 9201)
    out.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    eout = torch.full_like(out, SENTINEL)
    call(pool.clone(), eout)
    torch.cuda.synchronize()
    assert torch.equal(out, eout)
    host, got = pool[S - 1].cpu().numpy(), out[S - 1].cpu().numpy()
    ref = shortened_clay_oracle(k, m, v, [e], [None if (i % n) == e else host[i].copy() for i in range(n * a)], B)
    assert not [z for z in range(a) if not (got[z] == ref[z]).all()]


# ---------------------------------------------------------------- 4. replay after the registry forgot the stream
def test_replay_after_the_registry_forgot_the_stream(ecx, torch_dev):
    """The large apply_batch graph again (checked to hold no event node before anything else),
    then 4,096 + 512 one-stripe 4 KiB apply_batch calls on a second stream -- more than the
    registry keeps a silent stream for, plus one ageing period -- so the capture stream has left
    the registry.  The graph then replays twice on refilled pools, equal to an eager call and to
    the oracle on one stripe: nothing the graph needs belonged to the registry."""
    torch = torch_dev
    g, types, step, call, pool, out = _large_apply_capture(ecx, torch)
    gmap = step.map()
    small_in = torch.empty((48, 4096), dtype=torch.uint8, device="cuda")
    small_out = torch.empty((8, 4096), dtype=torch.uint8, device="cuda")
    ecx.fill_random(small_in, small_in.numel(), 9300)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(4096 + 512):
        gmap.apply_batch(small_in, 48 * 4096, 4096, small_out, 8 * 4096, 4096, 1, 4096, stream=side)
    torch.cuda.synchronize()
    _check_clay42_replays(ecx, torch, g, call, pool, out, (9301, 9302))


# ---------------------------------------------------------------- 5. layout selection stays out of captures
def test_layout_selection_stays_out_of_captures(ecx, torch_dev):
    """The RS(12,4) decode layout of test_layout_select_is_measured_and_exact (L = 1 MiB at a
    1 MiB + 4 KiB pitch, >= 256 MiB of input, a fresh map): warmed up with layout_select 0, then
    captured with layout_select 1 and replayed five times.  Nothing is selected or timed
    (layout_choice -1, no timings), the shape at capture is the static plan, the graph holds
    kernel nodes only, and the replayed in-place decode restores the erased shards (and equals the
    oracle on one stripe)."""
    torch = torch_dev
    L, pitch = 1 << 20, (1 << 20) + 4096
    S = -(-(256 << 20) // (12 * L))
    rs = ecx.ReedSolomon.create(12, 4)
    present = [False, False] + [True] * 14
    pool = torch.empty((S, 16, pitch), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 88)
    rs.encode_map().apply_batch(pool, 16 * pitch, pitch, pool, 16 * pitch, pitch, S, L)
    orig = pool[:, 0:2, :L].clone()
    mat, ins_, outs_ = rs.decode_map(present).matrix()
    dmap = ecx.GfMap.from_matrix(mat, in_slot=[int(i) for i in ins_], out_slot=[int(o) for o in outs_])

    def call():
        dmap.apply_batch(pool, 16 * pitch, pitch, pool, 16 * pitch, pitch, S, L)

    try:
        ecx.tune("layout_select", 0)
        call()
        torch.cuda.synchronize()
    finally:
        ecx.tune("layout_select", 1)
    assert dmap.layout_choice(pitch) == -1
    plan = dmap.launch_plan(pool.data_ptr(), 16 * pitch, pitch, pool.data_ptr(), 16 * pitch, pitch, S, L)
    g = capture(torch, call)
    assert plan and ecx.last_launch_shape() == plan, (plan, ecx.last_launch_shape())
    types = node_types(g)
    assert kernels_only(types), types
    for r in range(5):
        pool[:, 0:2, :L] = 0
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(pool[:, 0:2, :L], orig), r
    choice, ms = dmap.layout_choice(pitch, with_times=True)
    assert choice == -1 and all(t <= 0 for t in ms), (choice, ms)
    host = pool[S - 1].cpu().numpy()
    shards = [np.zeros(L, np.uint8) if i < 2 else host[i, :L].copy() for i in range(16)]
    O.ReedSolomon(12, 4).decode_missing(shards, present, 0, L)
    assert (shards[0] == host[0, :L]).all() and (shards[1] == host[1, :L]).all()


# ---------------------------------------------------------------- 6. first use inside a capture
def _refused(ecx, torch, call):
    """call() on a capturing stream raises the library's device error naming the remedy; the
    capture ends without error and holds no node."""
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with capturing(torch, g):
        with pytest.raises(ecx.EcxError) as err:
            call()
    assert err.value.code == ECX_E_DEVICE and "once outside the capture" in str(err.value), str(err.value)
    assert node_types(g) == []


def test_first_use_of_a_map_inside_a_capture_is_refused(ecx, torch_dev):
    """A fresh GfMap of random coefficients, never launched: apply_batch on a capturing stream is
    refused with ECX_E_DEVICE before the plan upload's allocation and blocking copy, the capture
    ends valid and empty; after one eager call, a new capture of the same call succeeds and
    replays to gf_apply_numpy's bytes."""
    torch = torch_dev
    rng = np.random.default_rng(61)
    mat = rng.integers(0, 256, (5, 9), dtype=np.uint8)
    gmap = ecx.GfMap.from_matrix(mat)
    S, n, P = 3, 8208, 8208 + 64
    inp = torch.empty((S, 9, P), dtype=torch.uint8, device="cuda")
    out = torch.empty((S, 5, P), dtype=torch.uint8, device="cuda")
    ecx.fill_random(inp, inp.numel(), 610)

    def call(i, t):
        gmap.apply_batch(i, 9 * P, P, t, 5 * P, P, S, n)

    _refused(ecx, torch, lambda: call(inp, out))

    def verify(before, got):
        assert (got[:, :, n:] == SENTINEL).all()
        for s in (0, S - 1):
            ref = gf_apply_numpy(mat, [before[s, j, :n] for j in range(9)])
            assert all((got[s, r, :n] == ref[r]).all() for r in range(5)), s

    replay_twice(ecx, torch, call, inp, out, kernels_only, verify, (611, 612))


def test_first_use_of_a_generated_kernel_inside_a_capture_is_refused(ecx, torch_dev):
    """A fresh shortened Clay(10,4) step: its first performCodingBatch on a capturing stream is
    refused (no compile result is loaded, no table uploaded), and the refusal is not remembered
    as a compile or load failure: the eager warm-up after it runs k_clay_repair_grp, and a new
    capture replays to the shortened oracle's bytes."""
    torch = torch_dev
    k, m, v, e, B, S = 10, 4, 2, 9, 4096, 3
    step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
    n, a = k + m, step.subPacketSize
    pool = torch.empty((S, n * a, B), dtype=torch.uint8, device="cuda")
    out = torch.empty((S, a, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 620)
    seen = {}

    def call(i, t):
        step.performCodingBatch(i, n * a * B, B, t, a * B, B, S, B)
        seen.setdefault("first_eager", ecx.last_kernel())

    _refused(ecx, torch, lambda: step.performCodingBatch(pool, n * a * B, B, out, a * B, B, S, B))

    def verify(before, got):
        s = S - 1
        ref = shortened_clay_oracle(k, m, v, [e], [None if (i % n) == e else before[s, i].copy() for i in range(n * a)], B)
        assert not [z for z in range(a) if not (got[s, z] == ref[z]).all()]

    replay_twice(ecx, torch, call, pool, out, kernels_only, verify, (621, 622))
    assert seen["first_eager"] == "k_clay_repair_grp", seen
