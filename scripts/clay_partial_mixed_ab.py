"""One accumulating hop of the pipelined Clay repair chain over Clay(4,2) stripes that lost one node
each, three placements timed in one process (the protocol of section 4.7.2):

  a  every stripe lost node 1 and the helper holds node 0 everywhere: one uniform
     GfMap.accumulate_batch of that (list, node) column map.  The ceiling.
  b  the erased node changes per stripe over the six single-node lists and the helper's node
     rotates with the stripe ((j + s) mod 6): one ClayPatternSet.partialBatchMixed.
  c  the same placement as one uniform accumulate_batch per stripe: all a helper could do before.

Sub-chunks of 32 KiB, 682 stripes, the node-major input of one helper ([stripe][plane][bytes]),
legs interleaved a b c c b a because rates move a few percent within a process, each leg the
median of --reps calls (a third of them for c) timed with HIP events.  A stripe's hop reads the
planes of its node that its list's map reads, and reads and writes the list's 8 rows: rates are
over those bytes, as a fraction of 8 TB/s.  Under rotation the helper's node is the stripe's erased
node in some stripes; an accumulating hop moves nothing for those, in (b) and in (c).  Before
anything is timed, (b) and (c) must give the same bytes.  One JSON line.

    timeout 900 python scripts/clay_partial_mixed_ab.py --out profiles/clay_partial_mixed_ab.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import rpamd  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
K, M = 4, 2
N, ALPHA = K + M, 8
ORDER = "abccba"
HELPER = 2  # helper j holds node (j + s) mod N of stripe s


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


def run(ecx, torch, np, B, S, reps):
    lists = [[e] for e in range(N)]
    # the column map of every (list, node): input slot = plane; None where the list does not read the node
    maps, planes = {}, {}
    for e in range(N):
        mat, ins, outs = ecx.ClayCodeErasureDecodingStep([e], K, M).map().matrix()
        mat = np.asarray(mat)
        for node in range(N):
            cols = [j for j, slot in enumerate(ins) if int(slot) % N == node and mat[:, j].any()]
            planes[e, node] = len(cols)
            maps[e, node] = ecx.GfMap.from_matrix(np.ascontiguousarray(mat[:, cols]),
                                                  in_slot=[int(ins[j]) // N for j in cols],
                                                  out_slot=[int(o) for o in outs]) if cols else None
    ids_host = (np.arange(S, dtype=np.int64) // 7) % N
    node_host = (HELPER + np.arange(S, dtype=np.int64)) % N
    ids = torch.from_numpy(ids_host.astype(np.uint8)).cuda()
    node_of = torch.from_numpy(node_host.astype(np.uint8)).cuda()
    inp = torch.empty((S, ALPHA, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(inp, inp.numel(), 9600)
    acc = torch.empty((S, ALPHA, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(acc, acc.numel(), 9601)
    in_flat, acc_flat = inp.view(-1), acc.view(-1)
    ps = ecx.ClayPatternSet(lists, K, M)
    a_map = maps[1, 0]

    def leg_a():
        a_map.accumulate_batch(inp, ALPHA * B, B, acc, ALPHA * B, B, S, B)

    def leg_b():
        ps.partialBatchMixed(ids, node_of, inp, ALPHA * B, 0, B, acc, ALPHA * B, B, S, B, False)

    def leg_c():
        for s in range(S):
            gm = maps[int(ids_host[s]), int(node_host[s])]
            if gm is not None:
                gm.accumulate_batch(in_flat[s * ALPHA * B:], ALPHA * B, B, acc_flat[s * ALPHA * B:], ALPHA * B, B, 1, B)

    # (b) and (c) agree before anything is timed
    start = acc.clone()
    leg_c()
    torch.cuda.synchronize()
    by_stripe = acc.clone()
    acc.copy_(start)
    leg_b()
    torch.cuda.synchronize()
    assert torch.equal(acc, by_stripe), "the mixed hop and the per-stripe calls disagree"
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

    # bytes a stripe's hop moves: the planes read, plus the rows read and written
    moved_a = S * (planes[1, 0] + 2 * ALPHA) * B
    working = [s for s in range(S) if planes[int(ids_host[s]), int(node_host[s])] > 0]
    moved_b = sum((planes[int(ids_host[s]), int(node_host[s])] + 2 * ALPHA) * B for s in working)
    moved = {"a": moved_a, "b": moved_b, "c": moved_b}
    legs = []
    for leg in ORDER:
        ms = timed(torch, {"a": leg_a, "b": leg_b, "c": leg_c}[leg], reps if leg != "c" else max(3, reps // 3))
        legs.append({"leg": leg, "ms": round(ms, 4), "frac": round(moved[leg] / ms / 1e6 / HBM_PEAK_GBS, 4)})
    med = {x: statistics.median(v["ms"] for v in legs if v["leg"] == x) for x in "abc"}
    frac = {x: moved[x] / med[x] / 1e6 / HBM_PEAK_GBS for x in "abc"}
    ps.close()
    return {
        "case": "clay42_single_node_accumulating_hop", "k": K, "m": M, "B": B, "stripes": S, "lists": len(lists),
        "helper": HELPER, "reps": reps, "order": ORDER, "legs": legs, "kernels": kernels,
        "planes_read_a": planes[1, 0], "planes_read_b": sorted({planes[int(i), int(n)] for i, n in zip(ids_host, node_host)}),
        "bytes_moved_a": moved_a, "bytes_moved_b": moved_b, "b_working_stripes": len(working),
        "a_uniform_ms": round(med["a"], 4), "b_mixed_ms": round(med["b"], 4), "c_per_stripe_ms": round(med["c"], 4),
        "a_frac": round(frac["a"], 4), "b_frac": round(frac["b"], 4), "c_frac": round(frac["c"], 4),
        "b_over_a_rate_per_byte_moved": round(frac["b"] / frac["a"], 4),
        "b_over_c_rate": round(med["c"] / med["b"], 4),
        "a_to_a_spread": round(abs(legs[0]["ms"] - legs[5]["ms"]) / med["a"], 4),
        "b_to_b_spread": round(abs(legs[1]["ms"] - legs[4]["ms"]) / med["b"], 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sub-bytes", type=int, default=32768)
    ap.add_argument("--stripes", type=int, default=682)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clay_partial_mixed_ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load()
    line = json.dumps(run(ecx, torch, np, args.sub_bytes, args.stripes, args.reps))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
