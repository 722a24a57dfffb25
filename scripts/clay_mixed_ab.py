"""Clay(4,2) repair over stripes that lost different nodes, timed in one process (DESIGN.md
section 4.7.3), by the protocol of scripts/mixed_decode_ab.py:

  a    every stripe lost node 1: one uniform performCodingBatch.  The ceiling (the headline).
  b    stripe s lost node s mod 6: one performCodingBatchMixed over a set of the six single-node
       lists, at the set's own ring depth.
  b4, b8   the same call with the ring depth forced (ecx_tune "depth").  (The first two lines of
       profiles/clay_mixed_ab.jsonl also have b20: a depth-20 instance, measured and removed.)
  b21  all 21 one- and two-node lists rotating: two tiles per pattern.
  c    the placement of (b) as one performCodingBatch per stripe: all a caller could do before
       the pattern set.

32 KiB sub-chunks, a pool of 1 GiB of input, legs interleaved a b c c b a because rates move a few
percent within a process, each leg the median of --reps calls (a third of them for c) timed with
HIP events; then b4 b8 b21 b21 b8 b4.  Before anything is timed, (b) and (c) must give the
same bytes.  Fractions of 8 TB/s are over the bytes a stripe's own list moves: 20 sub-chunks read
and 8 written for one node, 32 and 16 for two.  One JSON line.

    ECX_SHAPE_KNOBS=1 timeout 900 python scripts/clay_mixed_ab.py --out profiles/clay_mixed_ab.jsonl
"""
import argparse
import itertools
import json
import os
import statistics
import sys
from pathlib import Path

os.environ.setdefault("ECX_SHAPE_KNOBS", "1")  # the forced-depth legs force a launch shape
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import rpamd  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
K, M, N, ALPHA = 4, 2, 6, 8
ORDER = "abccba"
DEPTH_ORDER = ["b4", "b8", "b21", "b21", "b8", "b4"]


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


def run(ecx, torch, np, B, pool_bytes, reps, warm):
    n_in = N * ALPHA
    S = max(6, pool_bytes // (n_in * B))
    singles = [[i] for i in range(N)]
    all21 = singles + [list(c) for c in itertools.combinations(range(N), 2)]
    ids6_host = (np.arange(S) % 6).astype(np.uint8)
    ids6 = torch.from_numpy(ids6_host).cuda()
    ids21_host = (np.arange(S) % 21).astype(np.uint8)
    ids21 = torch.from_numpy(ids21_host).cuda()
    pool = torch.empty((S, n_in, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 8300)
    out = torch.zeros((S, 2 * ALPHA, B), dtype=torch.uint8, device="cuda")
    steps = [ecx.ClayCodeErasureDecodingStep(e, K, M) for e in singles]
    ps6 = ecx.ClayPatternSet(singles, K, M)
    ps21 = ecx.ClayPatternSet(all21, K, M)
    iss, oss = n_in * B, 2 * ALPHA * B

    def leg_a():
        steps[1].performCodingBatch(pool, iss, B, out, oss, B, S, B)

    def leg_b():
        ps6.performCodingBatchMixed(pool, iss, B, out, oss, B, ids6, S, B)

    def leg_b21():
        ps21.performCodingBatchMixed(pool, iss, B, out, oss, B, ids21, S, B)

    def leg_c():
        for s in range(S):
            steps[ids6_host[s]].performCodingBatch(pool[s:], iss, B, out[s:], oss, B, 1, B)

    # (b) and (c) agree before anything is timed
    leg_c()
    torch.cuda.synchronize()
    by_stripe = out.clone()
    out.zero_()
    leg_b()
    torch.cuda.synchronize()
    assert torch.equal(out, by_stripe), "the mixed call and the per-stripe calls disagree"
    del by_stripe
    kernels = {}
    for name, leg in (("a", leg_a), ("b", leg_b), ("b21", leg_b21), ("c", leg_c)):
        leg()
        kernels[name] = ecx.last_launch_shape()
    # warm-up: (a) is large enough for the per-layout shape selection, which first runs every
    # candidate a few times on the caller's own calls
    for _ in range(warm):
        leg_a()
    for _ in range(3):
        leg_b()
        leg_b21()
        leg_c()
    torch.cuda.synchronize()
    leg_a()
    kernels["a_selected"] = ecx.last_launch_shape()

    moved1 = S * (20 + 8) * B  # one node: 20 sub-chunks read, 8 written
    per21 = [(20 + 8) if len(e) == 1 else (32 + 16) for e in all21]
    moved21 = sum(per21[i] for i in ids21_host) * B

    def frac(moved, ms):
        return round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)

    legs = []
    for leg in ORDER:
        ms = timed(torch, {"a": leg_a, "b": leg_b, "c": leg_c}[leg], reps if leg != "c" else max(3, reps // 3))
        legs.append({"leg": leg, "ms": round(ms, 4), "frac": frac(moved1, ms)})
    med = {x: statistics.median(v["ms"] for v in legs if v["leg"] == x) for x in "abc"}

    depth_legs = []
    try:
        for name in ("b4", "b8"):
            ecx.tune("depth", int(name[1:]))
            leg_b()
            kernels[name] = ecx.last_launch_shape()
            for _ in range(3):
                leg_b()
        torch.cuda.synchronize()
        for name in DEPTH_ORDER:
            ecx.tune("depth", 0 if name == "b21" else int(name[1:]))
            ms = timed(torch, leg_b21 if name == "b21" else leg_b, reps)
            depth_legs.append({"leg": name, "ms": round(ms, 4),
                               "frac": frac(moved21 if name == "b21" else moved1, ms)})
    finally:
        ecx.tune("depth", 0)
    dmed = {x: statistics.median(v["ms"] for v in depth_legs if v["leg"] == x) for x in ("b4", "b8", "b21")}

    def spread(ls, name, m):
        v = [x["ms"] for x in ls if x["leg"] == name]
        return round(abs(v[0] - v[-1]) / m, 4)

    ps6.close()
    ps21.close()
    return {
        "case": "clay42_mixed_repair", "k": K, "m": M, "B": B, "stripes": S, "reps": reps, "order": ORDER,
        "depth_order": DEPTH_ORDER, "legs": legs, "depth_legs": depth_legs, "kernels": kernels,
        "a_uniform_ms": round(med["a"], 4), "b_mixed_ms": round(med["b"], 4), "c_per_stripe_ms": round(med["c"], 4),
        "b4_ms": round(dmed["b4"], 4), "b8_ms": round(dmed["b8"], 4),
        "b21_ms": round(dmed["b21"], 4),
        "a_frac": frac(moved1, med["a"]), "b_frac": frac(moved1, med["b"]), "c_frac": frac(moved1, med["c"]),
        "b4_frac": frac(moved1, dmed["b4"]), "b8_frac": frac(moved1, dmed["b8"]),
        "b21_frac": frac(moved21, dmed["b21"]),
        "b_over_a_rate": round(med["a"] / med["b"], 4), "b_over_c_rate": round(med["c"] / med["b"], 4),
        "a_to_a_spread": spread(legs, "a", med["a"]), "b_to_b_spread": spread(legs, "b", med["b"]),
        "b4_to_b4_spread": spread(depth_legs, "b4", dmed["b4"]), "b8_to_b8_spread": spread(depth_legs, "b8", dmed["b8"]),
        "b21_to_b21_spread": spread(depth_legs, "b21", dmed["b21"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sub-chunk", type=int, default=32768)
    ap.add_argument("--pool-mib", type=int, default=1024, help="input bytes in the pool")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=48)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clay_mixed_ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load(shape_knobs=True)
    line = json.dumps(run(ecx, torch, np, args.sub_chunk, args.pool_mib << 20, args.reps, args.warm))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
