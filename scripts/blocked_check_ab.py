"""isParityCorrect over the natural and the blocked RS layout, A/B in one process (DESIGN.md
section 4.6): the natural isParityCorrectBatch ([S][n][L], A) against isParityCorrectBlockedBatch
on the same stripes packed block-major (B), interleaved A B B A A B because rates move 4-5 %
between processes (section 4.5), each leg the median of --reps launches timed with HIP events.
Then the blocked check's two passes on their own, interleaved: the body pass as a blocked check of
the first full * block bytes of every shard, the tail pass as a natural check of the tail region
(the launches launch_check_blocked makes; each timed call also sets the verdicts, one launch of
S bytes).

  rs173  RS(17,3), 200,000-B shards, 4,096 stripes: 6 blocks of 32 KiB + a 3,392-B tail
  rs124  RS(12,4), 4 MiB shards, 128 stripes: 64 blocks of 64 KiB, no tail

One JSON line per case: the legs, blocked / natural, the A-to-A spread, the per-pass times and the
tail pass's share.  Both layouts are checked first (all valid, then one flipped byte in the last
stripe) and must agree.

    timeout 600 python scripts/blocked_check_ab.py --case rs173 --out profiles/blocked_check_ab.jsonl
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
CASES = {"rs173": (17, 3, 200000, 4096), "rs124": (12, 4, 4 << 20, 128)}
ORDER = "ABBAAB"


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


def run_case(ecx, torch, name, reps, stripes):
    k, m, L, S = CASES[name]
    S = stripes or S
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    b, full, tail = (int(x) for x in rs.blockedLayout(L))
    nat = torch.empty((S, n, L), dtype=torch.uint8, device="cuda")
    ecx.fill_random(nat, nat.numel(), 4600 + k)
    rs.encodeParityBatch(nat, n * L, L, S, 0, L)
    flat = ecx.blocked_pack(nat, b)
    vn = torch.zeros(S, dtype=torch.uint8, device="cuda")
    vb = torch.zeros(S, dtype=torch.uint8, device="cuda")
    body = S * full * n * b

    def natural():
        rs.isParityCorrectBatch(nat, n * L, L, S, 0, L, vn)

    def blocked():
        rs.isParityCorrectBlockedBatch(flat, S, L, vb)

    def body_pass():
        rs.isParityCorrectBlockedBatch(flat, S, full * b, vb, b)

    def tail_pass():
        rs.isParityCorrectBatch(flat[body:], n * tail, tail, S, 0, tail, vb)

    # both layouts agree before anything is timed: all valid, then one flipped byte
    natural()
    blocked()
    torch.cuda.synchronize()
    assert bool((vn == 1).all()) and bool((vb == 1).all()), "valid stripes must pass in both layouts"
    nat[S - 1, n - 1, L - 1] ^= 1
    flat[S * n * L - 1] ^= 1  # the same byte: the last of the batch
    natural()
    blocked()
    torch.cuda.synchronize()
    want = [1] * (S - 1) + [0]
    assert vn.cpu().tolist() == want and vb.cpu().tolist() == want, "the layouts disagree on a flipped byte"
    nat[S - 1, n - 1, L - 1] ^= 1
    flat[S * n * L - 1] ^= 1
    kernels = {}
    natural()
    kernels["natural"] = ecx.last_kernel()
    blocked()
    kernels["blocked"] = ecx.last_kernel()
    for f in (natural, blocked, body_pass) + ((tail_pass,) if tail else ()):  # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()

    data = S * n * L
    legs = []
    for leg in ORDER:
        ms = timed(torch, natural if leg == "A" else blocked, reps)
        legs.append({"leg": leg, "ms": round(ms, 4), "frac": round(data / ms / 1e6 / HBM_PEAK_GBS, 4)})
    a = [x["ms"] for x in legs if x["leg"] == "A"]
    bb = [x["ms"] for x in legs if x["leg"] == "B"]
    passes = {"body": [], "tail": []}
    for _ in range(3):
        passes["body"].append(timed(torch, body_pass, reps))
        if tail:
            passes["tail"].append(timed(torch, tail_pass, reps))
    body_ms = statistics.median(passes["body"])
    tail_ms = statistics.median(passes["tail"]) if tail else 0.0
    nat_ms, blk_ms = statistics.median(a), statistics.median(bb)
    return {
        "case": name, "k": k, "m": m, "L": L, "stripes": S, "block": b, "full": full, "tail": tail,
        "reps": reps, "order": ORDER, "legs": legs, "kernels": kernels,
        "natural_ms": round(nat_ms, 4), "blocked_ms": round(blk_ms, 4),
        "natural_frac": round(data / nat_ms / 1e6 / HBM_PEAK_GBS, 4),
        "blocked_frac": round(data / blk_ms / 1e6 / HBM_PEAK_GBS, 4),
        "blocked_over_natural_time": round(blk_ms / nat_ms, 4),
        "a_to_a_spread": round((max(a) - min(a)) / nat_ms, 4),
        "b_to_b_spread": round((max(bb) - min(bb)) / blk_ms, 4),
        "body_pass_ms": round(body_ms, 4), "tail_pass_ms": round(tail_ms, 4),
        "body_pass_frac": round(S * n * full * b / body_ms / 1e6 / HBM_PEAK_GBS, 4),
        "tail_pass_frac": round(S * n * tail / tail_ms / 1e6 / HBM_PEAK_GBS, 4) if tail else None,
        "tail_share_of_time": round(tail_ms / (body_ms + tail_ms), 4),
        "tail_share_of_bytes": round(tail / L, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="rs173,rs124")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stripes", type=int, default=0, help="override the case's stripe count (smoke runs)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "blocked_check_ab.jsonl"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load()
    for name in args.case.split(","):
        line = json.dumps(run_case(ecx, torch, name, args.reps, args.stripes))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
