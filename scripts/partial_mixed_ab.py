"""One accumulating hop of the pipelined partial-sum chain over RS(12,4) stripes with two erasures,
three placements timed in one process (the protocol of section 4.7):

  a  every stripe misses the same two shards and the helper holds the same shard index
     everywhere: one decodePartialBatch.  The ceiling.
  b  the missing pair rotates per stripe over all 120 pairs of 16 shards and the helper's shard
     index rotates with the stripe ((j + s) mod 16): one decodePartialBatchMixed.
  c  the same placement as one decodePartialBatch per stripe: all a helper could do before.

Shards of 64 KiB (1,024 stripes) and 4 MiB (16 stripes) on the recommended pitch, a pool of 1 GiB
of shard bytes from which each stripe's helper shard is read, legs interleaved a b c c b a because
rates move a few percent within a process, each leg the median of --reps calls (a third of them
for c) timed with HIP events.  A hop reads one shard and reads and writes two accumulator rows:
(1 + 2 * 2) * L bytes per stripe, reported as a fraction of 8 TB/s.  Under rotation the helper's
shard is one its stripe's pattern does not read (missing, or present but not among the first k) in
4 of every 16 stripes; an accumulating hop moves nothing for those, so (b) and (c) also report the
stripes that do work and (b)'s rate over the bytes it really moves.  Before anything is timed, (b)
and (c) must give the same bytes.  One JSON line per shard size.

    timeout 900 python scripts/partial_mixed_ab.py --out profiles/partial_mixed_ab.jsonl
"""
import argparse
import itertools
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import rpamd  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
K, M = 12, 4
N = K + M
ROWS = 2
ORDER = "abccba"
NODE = 5  # the helper: node j holds shard (j + s) mod N of stripe s


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


def run_size(ecx, torch, np, L, pool_bytes, reps):
    rs = ecx.ReedSolomon.create(K, M)
    pitch = rs.recommendedPitch(L)
    S = max(1, pool_bytes // (N * L))
    pairs = list(itertools.combinations(range(N), 2))
    pats = np.ones((len(pairs), N), np.uint8)
    for p, (i, j) in enumerate(pairs):
        pats[p, i] = pats[p, j] = 0
    ids_host = np.arange(S, dtype=np.int64) % len(pairs)
    shard_host = (NODE + np.arange(S, dtype=np.int64)) % N
    ids = torch.from_numpy(ids_host.astype(np.uint8)).cuda()
    shard_of = torch.from_numpy(shard_host.astype(np.uint8)).cuda()
    pool = torch.empty((S, N, pitch), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 8600)
    flat = pool.view(-1)
    acc = torch.empty((S, ROWS, pitch), dtype=torch.uint8, device="cuda")
    ecx.fill_random(acc, acc.numel(), 8601)
    acc_flat = acc.view(-1)
    ps = rs.patternSet(pats)
    # (a): a pattern that reads the helper's shard with two general coefficients
    a_pattern, a_index = pats[pairs.index((0, 1))], NODE

    def leg_a():
        rs.decodePartialBatch(a_pattern, a_index, flat[a_index * pitch:], N * pitch, acc, ROWS * pitch, pitch, S, L,
                              False)

    def leg_b():
        rs.decodePartialBatchMixed(ps, ids, shard_of, pool, N * pitch, pitch, acc, ROWS * pitch, pitch, S, L, False)

    def leg_c():
        for s in range(S):
            rs.decodePartialBatch(pats[ids_host[s]], int(shard_host[s]),
                                  flat[(s * N + int(shard_host[s])) * pitch:], N * pitch,
                                  acc_flat[s * ROWS * pitch:], ROWS * pitch, pitch, 1, L, False)

    # (b) and (c) agree before anything is timed
    start = acc.clone()
    leg_c()
    torch.cuda.synchronize()
    by_stripe = acc.clone()
    acc.copy_(start)
    leg_b()
    torch.cuda.synchronize()
    assert torch.equal(acc, by_stripe), "the mixed call and the per-stripe calls disagree"
    assert not torch.equal(acc, start)
    del start, by_stripe
    kernels = {}
    leg_a()
    kernels["a"] = ecx.last_launch_shape()
    leg_b()
    kernels["b"] = ecx.last_launch_shape()
    leg_c()
    kernels["c"] = ecx.last_launch_shape()
    # warm-up: (a) may go through the per-layout shape selection, which first runs every candidate
    # a few times on the caller's own calls
    for _ in range(48):
        leg_a()
    for _ in range(3):
        leg_b()
        leg_c()
    torch.cuda.synchronize()
    leg_a()
    kernels["a_selected"] = ecx.last_launch_shape()

    moved = S * (1 + 2 * ROWS) * L
    # the stripes whose pattern reads the helper's shard (present and among the first k present):
    # an accumulating hop moves bytes for those only, in (b) and in (c); in (a) that is every stripe
    working = sum(1 for s in range(S)
                  if pats[ids_host[s], shard_host[s]] and pats[ids_host[s], :shard_host[s]].sum() < K)
    legs = []
    for leg in ORDER:
        ms = timed(torch, {"a": leg_a, "b": leg_b, "c": leg_c}[leg], reps if leg != "c" else max(3, reps // 3))
        legs.append({"leg": leg, "ms": round(ms, 4), "frac": round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)})
    med = {x: statistics.median(v["ms"] for v in legs if v["leg"] == x) for x in "abc"}
    ps.close()
    return {
        "case": "rs124_two_erasures_accumulating_hop", "k": K, "m": M, "L": L, "pitch": pitch, "stripes": S,
        "patterns": len(pairs), "reps": reps, "order": ORDER, "legs": legs, "kernels": kernels,
        "a_uniform_ms": round(med["a"], 4), "b_mixed_ms": round(med["b"], 4), "c_per_stripe_ms": round(med["c"], 4),
        "a_frac": round(moved / med["a"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_frac": round(moved / med["b"] / 1e6 / HBM_PEAK_GBS, 4),
        "c_frac": round(moved / med["c"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_over_a_rate": round(med["a"] / med["b"], 4),
        "b_working_stripes": working,
        "b_frac_of_bytes_moved": round(moved * working / S / med["b"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_over_a_rate_per_byte_moved": round(med["a"] / med["b"] * working / S, 4),
        "b_over_c_rate": round(med["c"] / med["b"], 4),
        "a_to_a_spread": round(abs(legs[0]["ms"] - legs[5]["ms"]) / med["a"], 4),
        "b_to_b_spread": round(abs(legs[1]["ms"] - legs[4]["ms"]) / med["b"], 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,4194304")
    ap.add_argument("--pool-mib", type=int, default=1024, help="shard bytes in the pool")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "partial_mixed_ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load()
    for L in (int(x) for x in args.sizes.split(",")):
        line = json.dumps(run_size(ecx, torch, np, L, args.pool_mib << 20, args.reps))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
