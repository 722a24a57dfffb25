"""Clay(10,4) (shortened from Clay(12,4), v = 2) repair over stripes that lost different nodes, on the
generated set kernel k_clay_repair_set, timed in one process by the
protocol of scripts/clay_mixed_ab.py:

  a    every stripe lost node 1: one uniform performCodingBatch (k_clay_repair_grp).  The ceiling.
  b    stripe s lost node s mod 14: one performCodingBatchMixed over the set of the 14 single-node
       lists -- fourteen straight-line bodies in flight side by side.
  b1   the same set and kernel, every id equal to node 1's: the switch alone, one body in flight.
  c    the placement of (b) as one uniform performCodingBatch per stripe.

4 KiB sub-chunks, 512 stripes (7 GiB of input), legs interleaved a b b1 c c b1 b a, each leg the
median of --reps calls (a third of them for c) timed with HIP events.  Before anything is timed,
(b) and (c) must give the same bytes.  Fractions of 8 TB/s are over the bytes a stripe's repair
moves: 64 helper planes of 13 nodes read, 256 sub-chunks written.  Also recorded: the hiprtc compile
time of a 4-list set's kernel and of the 14-list set's (a compile for gfx950 in this process, no
load), and the loaded 14-list kernel's registers, LDS, scratch and code size.  One JSON line.

    ECX_SHAPE_KNOBS=1 timeout 900 python scripts/clay_set_rtc_ab.py --out profiles/clay_set_rtc_ab.jsonl
"""
import argparse
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
K, M, V, N, ALPHA = 10, 4, 2, 14, 256
ORDER = ["a", "b", "b1", "c", "c", "b1", "b", "a"]


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


def compile_seconds(ecx, lists):
    with ecx.ClayPatternSet(lists, K, M, V) as ps:
        t = time.perf_counter()
        size = ps.rtcCompileCheck()
        return round(time.perf_counter() - t, 3), size


def run(ecx, torch, np, B, S, reps, warm):
    n_in = N * ALPHA
    singles = [[e] for e in range(N)]
    compile4, code4 = compile_seconds(ecx, [[2], [5], [8], [13]])
    compile14, code14 = compile_seconds(ecx, singles)
    ids_host = (np.arange(S) % N).astype(np.uint8)
    ids = torch.from_numpy(ids_host).cuda()
    ids1 = torch.full((S,), 1, dtype=torch.uint8, device="cuda")
    pool = torch.empty((S, n_in, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 8700)
    out = torch.zeros((S, ALPHA, B), dtype=torch.uint8, device="cuda")
    steps = [ecx.ClayCodeErasureDecodingStep(e, K, M, virtualUnits=V) for e in singles]
    ps = ecx.ClayPatternSet(singles, K, M, V)
    iss, oss = n_in * B, ALPHA * B

    def leg_a():
        steps[1].performCodingBatch(pool, iss, B, out, oss, B, S, B)

    def leg_b():
        ps.performCodingBatchMixed(pool, iss, B, out, oss, B, ids, S, B)

    def leg_b1():
        ps.performCodingBatchMixed(pool, iss, B, out, oss, B, ids1, S, B)

    def leg_c():
        for s in range(S):
            steps[ids_host[s]].performCodingBatch(pool[s:], iss, B, out[s:], oss, B, 1, B)

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
    for name, leg in (("a", leg_a), ("b", leg_b), ("b1", leg_b1), ("c", leg_c)):
        leg()
        kernels[name] = ecx.last_kernel()
    resources = ps.rtcResources()
    for _ in range(warm):
        leg_a()
        leg_b()
        leg_b1()
    leg_c()
    torch.cuda.synchronize()

    moved = S * (13 * 64 + ALPHA) * B

    def frac(ms):
        return round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)

    calls = {"a": leg_a, "b": leg_b, "b1": leg_b1, "c": leg_c}
    legs = []
    for leg in ORDER:
        ms = timed(torch, calls[leg], reps if leg != "c" else max(3, reps // 3))
        legs.append({"leg": leg, "ms": round(ms, 4), "frac": frac(ms)})
    med = {x: statistics.median(v["ms"] for v in legs if v["leg"] == x) for x in calls}

    def spread(name):
        v = [x["ms"] for x in legs if x["leg"] == name]
        return round(abs(v[0] - v[-1]) / med[name], 4)

    ps.close()
    return {
        "case": "clay104_set_rtc", "k": K, "m": M, "v": V, "B": B, "stripes": S, "reps": reps, "order": ORDER,
        "legs": legs, "kernels": kernels, "resources_14_lists": resources,
        "compile_s_4_lists": compile4, "code_bytes_4_lists": code4,
        "compile_s_14_lists": compile14, "code_bytes_14_lists": code14,
        "a_uniform_ms": round(med["a"], 4), "b_mixed_ms": round(med["b"], 4), "b1_one_body_ms": round(med["b1"], 4),
        "c_per_stripe_ms": round(med["c"], 4),
        "a_frac": frac(med["a"]), "b_frac": frac(med["b"]), "b1_frac": frac(med["b1"]), "c_frac": frac(med["c"]),
        "b_over_a_rate": round(med["a"] / med["b"], 4), "b1_over_a_rate": round(med["a"] / med["b1"], 4),
        "b_over_c_rate": round(med["c"] / med["b"], 4),
        "a_to_a_spread": spread("a"), "b_to_b_spread": spread("b"), "b1_to_b1_spread": spread("b1"),
        "c_to_c_spread": spread("c"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sub-chunk", type=int, default=4096)
    ap.add_argument("--stripes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clay_set_rtc_ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load(shape_knobs=True)
    line = json.dumps(run(ecx, torch, np, args.sub_chunk, args.stripes, args.reps, args.warm))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
