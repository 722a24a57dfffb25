"""Two-erasure RS decode over stripes that miss different shards, in the blocked layout, timed
against its two neighbours in one process (the protocol of
scripts/mixed_decode_ab.py):

  a  every stripe misses the same two shards: one uniform decodeMissingBlockedBatch.  The ceiling.
  b  the missing pair rotates per stripe over all pairs of the n shards: one
     decodeMissingBlockedBatchMixed over a set of all those patterns.
  c  the same rotated placement over the same stripes in the natural layout on the recommended
     pitch: one decodeMissingBatchMixed.

Shapes, each with a pool of 1 GiB of shard bytes: RS(12,4) on 4 MiB and on 64 KiB shards, RS(17,3)
on 200,000-B shards (six 32 KiB blocks and a 3,392-B tail).  Legs interleaved a b c c b a because
rates move a few percent within a process, each leg the median of --reps calls timed with HIP
events.  Before anything is timed, (b) must give the bytes of a uniform blocked decode run stripe
by stripe.  One JSON line per shape.

--host adds one end-to-end line per host form (wall clock, pinned memory, RS(12,4) 4 MiB): the
mixed host decode against the uniform host batch on the same stripes, natural and blocked.

    ECX_SHAPE_KNOBS=1 timeout 900 python scripts/mixed_blocked_ab.py --host --out profiles/mixed_blocked_ab.jsonl
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time
from pathlib import Path

os.environ.setdefault("ECX_SHAPE_KNOBS", "1")
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import rpamd  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
ORDER = "abccba"
SHAPES = [(12, 4, 4 << 20), (12, 4, 64 << 10), (17, 3, 200000)]


def timed(torch, call, reps):
    """Median HIP-event time (ms) of `reps` single calls."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def pair_patterns(np, n):
    pairs = list(itertools.combinations(range(n), 2))
    pats = np.ones((len(pairs), n), np.uint8)
    for p, (i, j) in enumerate(pairs):
        pats[p, i] = pats[p, j] = 0
    return pats


def run_shape(ecx, torch, np, k, m, L, pool_bytes, reps, warm):
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    block, full, tail = rs.blockedLayout(L)
    pitch = rs.recommendedPitch(L)
    S = max(1, pool_bytes // (n * L))
    pats = pair_patterns(np, n)
    ids_host = (np.arange(S, dtype=np.int64) % len(pats)).astype(np.uint8)
    ids = torch.from_numpy(ids_host).cuda()
    present = [[bool(f) for f in p] for p in pats]
    natural = torch.empty((S, n, pitch), dtype=torch.uint8, device="cuda")
    ecx.fill_random(natural, natural.numel(), 8400)
    pool = ecx.blocked_pack(natural[:, :, :L], block)
    ps = rs.patternSet(pats)

    def leg_a():
        rs.decodeMissingBlockedBatch(pool, present[0], S, L, block)

    def leg_b():
        rs.decodeMissingBlockedBatchMixed(pool, ps, ids, S, L, block)

    def leg_c():
        rs.decodeMissingBatchMixed(natural, ps, ids, n * pitch, pitch, S, 0, L)

    # (b) equals a uniform blocked decode run stripe by stripe, before anything is timed
    ref = pool.clone()
    leg_b()
    torch.cuda.synchronize()
    for s in range(S):
        one = ecx.blocked_pack(ecx.blocked_unpack(ref, S, n, L, block, first=s, count=1), block)
        rs.decodeMissingBlockedBatch(one, present[ids_host[s]], 1, L, block)
        got = ecx.blocked_pack(ecx.blocked_unpack(pool, S, n, L, block, first=s, count=1), block)
        assert torch.equal(one, got), "the blocked mixed call and the uniform decode of stripe %d disagree" % s
    del ref
    kernels = {}
    leg_a()
    kernels["a"] = ecx.last_launch_shape()
    leg_b()
    kernels["b"] = ecx.last_launch_shape()
    leg_c()
    kernels["c"] = ecx.last_launch_shape()
    # warm-up: (a) is large enough for the per-layout shape selection, which first runs every
    # candidate a few times on the caller's own calls
    for _ in range(warm):
        leg_a()
    for _ in range(3):
        leg_b()
        leg_c()
    torch.cuda.synchronize()
    leg_a()
    kernels["a_selected"] = ecx.last_launch_shape()

    moved = S * (k + 2) * L  # k shards read, 2 written, per stripe
    legs = []
    for leg in ORDER:
        ms = timed(torch, {"a": leg_a, "b": leg_b, "c": leg_c}[leg], reps)
        legs.append({"leg": leg, "ms": round(ms, 4), "frac": round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)})
    med = {x: statistics.median(v["ms"] for v in legs if v["leg"] == x) for x in "abc"}
    ps.close()
    return {
        "case": "rs%d%d_two_erasures_blocked" % (k, m), "k": k, "m": m, "L": L, "block": block, "full": full,
        "tail": tail, "pitch": pitch, "stripes": S, "patterns": len(pats), "reps": reps, "order": ORDER, "legs": legs,
        "kernels": kernels,
        "a_uniform_blocked_ms": round(med["a"], 4), "b_mixed_blocked_ms": round(med["b"], 4),
        "c_mixed_natural_ms": round(med["c"], 4),
        "a_frac": round(moved / med["a"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_frac": round(moved / med["b"] / 1e6 / HBM_PEAK_GBS, 4),
        "c_frac": round(moved / med["c"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_over_a_rate": round(med["a"] / med["b"], 4),
        "b_over_c_rate": round(med["c"] / med["b"], 4),
        "a_to_a_spread": round(abs(legs[0]["ms"] - legs[5]["ms"]) / med["a"], 4),
        "b_to_b_spread": round(abs(legs[1]["ms"] - legs[4]["ms"]) / med["b"], 4),
    }


def run_host(ecx, torch, np, layout, k, m, L, pool_bytes, reps):
    """End to end from pinned host memory: (a) the uniform host batch, (b) the mixed host decode,
    interleaved a b b a, the median wall-clock time of `reps` calls each."""
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    S = max(1, pool_bytes // (n * L))
    pats = pair_patterns(np, n)
    ids = (np.arange(S, dtype=np.int64) % len(pats)).astype(np.uint8)
    present = [bool(f) for f in pats[0]]
    buf = ecx.HostBuffer(S * n * L)
    buf.array[:] = np.random.default_rng(8500).integers(0, 256, S * n * L, dtype=np.uint8)
    ps = rs.patternSet(pats)
    if layout == "natural":
        dm = rs.decode_map(present)
        a = lambda: dm.apply_batch_host(buf.array, n * L, L, buf.array, n * L, L, S, L)          # noqa: E731
        b = lambda: rs.decodeMissingBatchMixedHost(buf.array, ps, ids, n * L, L, S, 0, L)        # noqa: E731
    else:
        a = lambda: rs.decodeMissingBlockedBatchHost(buf.array, present, S, L)                   # noqa: E731
        b = lambda: rs.decodeMissingBlockedBatchMixedHost(buf.array, ps, ids, S, L)              # noqa: E731

    def wall(call):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    a(), b()  # first use: buffers, plans
    legs = [{"leg": leg, "ms": round(wall({"a": a, "b": b}[leg]), 3)} for leg in "abba"]
    med = {x: statistics.median(v["ms"] for v in legs if v["leg"] == x) for x in "ab"}
    ps.close()
    shard_gib = S * n * L / 2**30
    return {
        "case": "rs%d%d_two_erasures_host_%s" % (k, m, layout), "k": k, "m": m, "L": L, "stripes": S, "memory": "pinned",
        "patterns": len(pats), "reps": reps, "order": "abba", "legs": legs,
        "a_uniform_host_ms": round(med["a"], 3), "b_mixed_host_ms": round(med["b"], 3),
        "a_shard_gib_s": round(shard_gib / med["a"] * 1e3, 2), "b_shard_gib_s": round(shard_gib / med["b"] * 1e3, 2),
        "up_slots_a": k, "up_slots_b": n, "down_slots_a": 2, "down_slots_b": n,
        "b_over_a_rate": round(med["a"] / med["b"], 4),
        "a_to_a_spread": round(abs(legs[0]["ms"] - legs[3]["ms"]) / med["a"], 4),
        "b_to_b_spread": round(abs(legs[1]["ms"] - legs[2]["ms"]) / med["b"], 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-mib", type=int, default=1024, help="shard bytes in the pool")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=48)
    ap.add_argument("--host", action="store_true", help="also the two host forms, end to end")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mixed_blocked_ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load(shape_knobs=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()

    for k, m, L in SHAPES:
        emit(run_shape(ecx, torch, np, k, m, L, args.pool_mib << 20, args.reps, args.warm))
    if args.host:
        for layout in ("natural", "blocked"):
            emit(run_host(ecx, torch, np, layout, 12, 4, 4 << 20, args.pool_mib << 20, args.host_reps))


if __name__ == "__main__":
    main()
