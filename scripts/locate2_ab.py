"""locateCorrupt2Batch against the check and the single-shard locate it extends, and against the only
route there was before it for two corrupt shards, in one process, each leg
the median of --reps single calls timed with HIP events (the protocol of scripts/locate_ab.py; every
ratio is taken inside one process):

  check            isParityCorrectBatch, timed three times between the other legs: its run-to-run
                   spread is the yardstick
  locate_clean     locateCorruptBatch (the single-shard locate, kernel unchanged), no corrupt stripe
  locate2_clean    locateCorrupt2Batch, no corrupt stripe (every wave leaves after the ballot)
  locate2_1pct_one 1 % of the stripes (at least one) with one flipped byte
  locate2_1pct_two 1 % of the stripes with one flipped byte in each of two shards
  locate2_shortcut every byte of one shard of every stripe flipped: every wave keeps one single
                   candidate and takes the shortcut
  locate2_pairs    every byte of two shards of every stripe flipped: every wave runs the pair tiles
  candidates       the old route on the locate2_1pct_two stripes: for each of the n + C(n,2)
                   candidates, copy the stripes, decodeMissingBatch with the candidate missing on the
                   copy, then isParityCorrectBatch on it

  rs124      RS(12,4), 4 MiB shards, 16 stripes (1 GiB)
  rs124_64k  RS(12,4), 64 KiB shards, 1024 stripes (1 GiB)

One JSON line per case.  The answers are checked against the candidate route (the 1 % cases, suspect
for suspect) and against the flips (every case) before anything is timed.

    timeout 900 python scripts/locate2_ab.py --out profiles/locate2_ab.jsonl
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
CASES = {"rs124": (12, 4, 4 << 20, 16), "rs124_64k": (12, 4, 64 << 10, 1024)}


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
    pairs = list(itertools.combinations(range(n), 2))
    width = n + len(pairs)
    candidates = [(j,) for j in range(n)] + pairs
    rs = ecx.ReedSolomon.create(k, m)
    clean = torch.empty((S, n, L), dtype=torch.uint8, device="cuda")
    ecx.fill_random(clean, clean.numel(), 4900 + k)
    rs.encodeParityBatch(clean, n * L, L, S, 0, L)
    pool = clean.clone()
    verdict = torch.zeros(S, dtype=torch.uint8, device="cuda")
    suspect1 = torch.zeros(S * n, dtype=torch.uint8, device="cuda")
    culprit1 = torch.zeros(S, dtype=torch.int32, device="cuda")
    suspect = torch.zeros(S * width, dtype=torch.uint8, device="cuda")
    culprit = torch.zeros(2 * S, dtype=torch.int32, device="cuda")
    heal = torch.zeros(S, dtype=torch.uint8, device="cuda")

    def check():
        rs.isParityCorrectBatch(pool, n * L, L, S, 0, L, verdict)

    def locate():
        rs.locateCorruptBatch(pool, n * L, L, S, 0, L, suspect1, culprit1, heal)

    def locate2():
        rs.locateCorrupt2Batch(pool, n * L, L, S, 0, L, suspect, culprit, heal)

    def corrupt(which, two, whole):
        """One or two shards of each stripe in `which` flipped: one byte each (different bytes), or
        every byte.  Returns the culprits the flips promise."""
        pool.copy_(clean)
        want = [[-1, -1] for _ in range(S)]
        for s in which:
            i = (5 * s + 3) % n
            j = (i + 1 + (7 * s) % (n - 1)) % n
            for x, shard in enumerate((i, j) if two else (i,)):
                if whole:
                    pool[s, shard] ^= 0x5A
                else:
                    pool[s, shard, (977 * s + 4099 * x) % L] ^= 0x5A
            want[s] = sorted((i, j)) if two else [i, -1]
        return want

    def candidate_route(which, scratch, v):
        """The old route: suspects of the stripes `which` by one decode and one check of a copy for
        each of the n + C(n,2) candidates."""
        idx = torch.tensor(which, device="cuda")
        out = []
        for cand in candidates:
            torch.index_select(pool, 0, idx, out=scratch)
            rs.decodeMissingBatch(scratch, [i not in cand for i in range(n)], n * L, L, len(which), 0, L)
            rs.isParityCorrectBatch(scratch, n * L, L, len(which), 0, L, v)
            out.append(v.clone())
        return out

    one_pct = sorted({(s * 100 + 37) % S for s in range(max(1, S // 100))})
    everyone = list(range(S))
    sets = {"locate2_1pct_one": (one_pct, False, False), "locate2_1pct_two": (one_pct, True, False),
            "locate2_shortcut": (everyone, False, True), "locate2_pairs": (everyone, True, True)}
    # the answers, before anything is timed
    locate2()
    torch.cuda.synchronize()
    assert culprit.cpu().tolist() == [-1] * (2 * S), "a clean pool must locate nothing"
    scratch = torch.empty((len(one_pct), n, L), dtype=torch.uint8, device="cuda")
    v = torch.zeros(len(one_pct), dtype=torch.uint8, device="cuda")
    for leg, (which, two, whole) in sets.items():
        want = corrupt(which, two, whole)
        locate2()
        torch.cuda.synchronize()
        assert culprit.view(S, 2).cpu().tolist() == want, leg
        old = torch.stack(candidate_route(one_pct, scratch, v), 1).cpu()  # on the 1 % stripes of every case
        assert torch.equal(old, suspect.view(S, width)[one_pct].cpu()), leg + ": the two routes disagree"

    data = S * n * L
    frac = lambda ms: round(data / ms / 1e6 / HBM_PEAK_GBS, 4)  # noqa: E731
    kernels = {}
    pool.copy_(clean)
    for f in (check, locate, locate2):
        for _ in range(3):
            f()
    for label, f in (("check", check), ("locate", locate), ("locate2", locate2)):
        f()
        kernels[label] = ecx.last_kernel()
    torch.cuda.synchronize()
    out = {"case": name, "k": k, "m": m, "L": L, "stripes": S, "reps": reps, "kernels": kernels,
           "candidates": len(candidates), "one_pct_stripes": len(one_pct)}
    checks = [timed(torch, check, reps)]
    out["locate_clean_ms"] = timed(torch, locate, reps)
    out["locate2_clean_ms"] = timed(torch, locate2, reps)
    checks.append(timed(torch, check, reps))
    for leg, (which, two, whole) in sets.items():
        corrupt(which, two, whole)
        for _ in range(2):
            locate2()
        torch.cuda.synchronize()
        out[leg + "_ms"] = timed(torch, locate2, reps)
        if leg == "locate2_1pct_two":
            candidate_route(one_pct, scratch, v)  # warm-up: the decode maps compile and upload here
            torch.cuda.synchronize()
            out["candidates_ms"] = timed(torch, lambda: candidate_route(one_pct, scratch, v), 3)
    pool.copy_(clean)
    checks.append(timed(torch, check, reps))
    check_ms = statistics.median(checks)
    out["check_ms"] = [round(x, 4) for x in checks]
    out["check_frac"] = frac(check_ms)
    out["check_spread"] = round((max(checks) - min(checks)) / check_ms, 4)
    out["locate2_clean_over_locate_clean"] = round(out["locate2_clean_ms"] / out["locate_clean_ms"], 4)
    out["locate2_1pct_one_over_clean"] = round(out["locate2_1pct_one_ms"] / out["locate2_clean_ms"], 4)
    out["locate2_1pct_two_over_clean"] = round(out["locate2_1pct_two_ms"] / out["locate2_clean_ms"], 4)
    out["candidates_over_locate2"] = round(out["candidates_ms"] / out["locate2_1pct_two_ms"], 1)
    for leg in ["locate_clean", "locate2_clean"] + list(sets):
        out[leg + "_frac"] = frac(out[leg + "_ms"])
        out[leg + "_over_check_time"] = round(out[leg + "_ms"] / check_ms, 4)
        out[leg + "_ms"] = round(out[leg + "_ms"], 4)
    out["candidates_ms"] = round(out["candidates_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="rs124,rs124_64k")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stripes", type=int, default=0, help="override the case's stripe count (smoke runs)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "locate2_ab.jsonl"))
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
