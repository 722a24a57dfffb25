"""RS(12,4) two-erasure decode over stripes that miss different shards, three placements timed in
one process:

  a  every stripe misses the same two shards: one decodeMissingBatch.  The ceiling.
  b  the missing pair rotates per stripe over all 120 pairs of 16 shards: one
     decodeMissingBatchMixed over a set of 120 patterns.
  c  the same rotated placement as one decodeMissingBatch per stripe: all a caller could do
     before the pattern set.

Shards of 64 KiB and 4 MiB on the recommended pitch, a pool of 1 GiB of shard bytes, legs
interleaved a b c c b a because rates move a few percent within a process, each leg the median of
--reps calls timed with HIP events.  (b) also runs with the ring depth forced to 4 (ecx_tune
"depth"): the set's own depth is 8, which pads 12 entries to 16.  Before anything is timed, (b)
and (c) must give the same bytes.  One JSON line per shard size.

    ECX_SHAPE_KNOBS=1 timeout 900 python scripts/mixed_decode_ab.py --out profiles/mixed_decode_ab.jsonl
"""
import argparse
import itertools
import json
import os
import statistics
import sys
from pathlib import Path

os.environ.setdefault("ECX_SHAPE_KNOBS", "1")  # the depth-4 leg forces a launch shape
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import rpamd  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
K, M = 12, 4
N = K + M
ORDER = "abccba"


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


def run_size(ecx, torch, np, L, pool_bytes, reps, warm):
    rs = ecx.ReedSolomon.create(K, M)
    pitch = rs.recommendedPitch(L)
    S = max(1, pool_bytes // (N * L))
    pairs = list(itertools.combinations(range(N), 2))
    pats = np.ones((len(pairs), N), np.uint8)
    for p, (i, j) in enumerate(pairs):
        pats[p, i] = pats[p, j] = 0
    ids_host = np.arange(S, dtype=np.int64) % len(pairs)
    ids = torch.from_numpy(ids_host.astype(np.uint8)).cuda()
    present = [[bool(f) for f in pats[p]] for p in range(len(pairs))]
    pool = torch.empty((S, N, pitch), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 8100)
    ps = rs.patternSet(pats)

    def leg_a():
        rs.decodeMissingBatch(pool, present[0], N * pitch, pitch, S, 0, L)

    def leg_b():
        rs.decodeMissingBatchMixed(pool, ps, ids, N * pitch, pitch, S, 0, L)

    def leg_c():
        for s in range(S):
            rs.decodeMissingBatch(pool[s:], present[ids_host[s]], N * pitch, pitch, 1, 0, L)

    # (b) and (c) agree before anything is timed
    ref = pool.clone()
    leg_c()
    torch.cuda.synchronize()
    by_stripe = pool.clone()
    pool.copy_(ref)
    leg_b()
    torch.cuda.synchronize()
    assert torch.equal(pool, by_stripe), "the mixed call and the per-stripe calls disagree"
    del ref, by_stripe
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

    moved = S * (K + 2) * L  # 12 shards read, 2 written, per stripe
    legs = []
    for leg in ORDER:
        ms = timed(torch, {"a": leg_a, "b": leg_b, "c": leg_c}[leg], reps if leg != "c" else max(3, reps // 3))
        legs.append({"leg": leg, "ms": round(ms, 4), "frac": round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)})
    med = {x: statistics.median(v["ms"] for v in legs if v["leg"] == x) for x in "abc"}
    ecx.tune("depth", 4)
    try:
        leg_b()
        kernels["b_depth4"] = ecx.last_launch_shape()
        for _ in range(3):
            leg_b()
        torch.cuda.synchronize()
        b4 = statistics.median(timed(torch, leg_b, reps) for _ in range(2))
    finally:
        ecx.tune("depth", 0)
    ps.close()
    return {
        "case": "rs124_two_erasures", "k": K, "m": M, "L": L, "pitch": pitch, "stripes": S, "patterns": len(pairs),
        "reps": reps, "order": ORDER, "legs": legs, "kernels": kernels,
        "a_uniform_ms": round(med["a"], 4), "b_mixed_ms": round(med["b"], 4), "c_per_stripe_ms": round(med["c"], 4),
        "b_mixed_depth4_ms": round(b4, 4),
        "a_frac": round(moved / med["a"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_frac": round(moved / med["b"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_depth4_frac": round(moved / b4 / 1e6 / HBM_PEAK_GBS, 4),
        "c_frac": round(moved / med["c"] / 1e6 / HBM_PEAK_GBS, 4),
        "b_over_a_rate": round(med["a"] / med["b"], 4),
        "b_depth4_over_a_rate": round(med["a"] / b4, 4),
        "b_over_c_rate": round(med["c"] / med["b"], 4),
        "a_to_a_spread": round(abs(legs[0]["ms"] - legs[5]["ms"]) / med["a"], 4),
        "b_to_b_spread": round(abs(legs[1]["ms"] - legs[4]["ms"]) / med["b"], 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,4194304")
    ap.add_argument("--pool-mib", type=int, default=1024, help="shard bytes in the pool")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=48)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mixed_decode_ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load(shape_knobs=True)
    for L in (int(x) for x in args.sizes.split(",")):
        line = json.dumps(run_size(ecx, torch, np, L, args.pool_mib << 20, args.reps, args.warm))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
