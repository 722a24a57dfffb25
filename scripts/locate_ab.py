"""locateCorruptBatch against the check it extends and against the only route there was before it,
in one process, each leg the median of --reps calls timed with HIP events
(the protocol of scripts/blocked_check_ab.py; rates move 4-5 % between processes, section 4.5, so
every ratio here is taken inside one process):

  check         isParityCorrectBatch, timed three times between the other legs: its run-to-run
                spread is the yardstick for the clean locate
  locate_clean  locateCorruptBatch with no corrupt stripe (every wave leaves after the ballot)
  locate_1pct   locateCorruptBatch with 1 % of the stripes corrupt (at least one), one byte each
  locate_all    locateCorruptBatch with every stripe corrupt, one byte in every 4 KiB chunk of one
                shard (every workgroup runs stage two)
  n_decode      the old route over the corrupt stripes alone: for each of the n candidate shards,
                copy the stripes, decodeMissingBatch with that shard missing on the copy, then
                isParityCorrectBatch on it -- against locate_1pct and locate_all

  rs173  RS(17,3), 200,000-B shards, 268 stripes (1 GiB)
  rs124  RS(12,4), 4 MiB shards, 16 stripes (1 GiB)

One JSON line per case.  The locate's answers are checked against the n-decode route before
anything is timed.

    timeout 600 python scripts/locate_ab.py --out profiles/locate_ab.jsonl
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
CASES = {"rs173": (17, 3, 200000, 268), "rs124": (12, 4, 4 << 20, 16)}
CHUNK = 4096


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
    clean = torch.empty((S, n, L), dtype=torch.uint8, device="cuda")
    ecx.fill_random(clean, clean.numel(), 4800 + k)
    rs.encodeParityBatch(clean, n * L, L, S, 0, L)
    pool = clean.clone()
    verdict = torch.zeros(S, dtype=torch.uint8, device="cuda")
    suspect = torch.zeros(S * n, dtype=torch.uint8, device="cuda")
    culprit = torch.zeros(S, dtype=torch.int32, device="cuda")
    heal = torch.zeros(S, dtype=torch.uint8, device="cuda")

    def check():
        rs.isParityCorrectBatch(pool, n * L, L, S, 0, L, verdict)

    def locate():
        rs.locateCorruptBatch(pool, n * L, L, S, 0, L, suspect, culprit, heal)

    def corrupt(which, every_chunk):
        """One shard of each stripe in `which` flipped: one byte, or one in every 4 KiB chunk."""
        pool.copy_(clean)
        want = [-1] * S
        for s in which:
            j = (5 * s + 3) % n
            if every_chunk:
                pool[s, j, 7::CHUNK] ^= 0x5A
            else:
                pool[s, j, (977 * s) % L] ^= 0x5A
            want[s] = j
        return want

    def n_decode(which, scratch, v):
        """The old route: suspects of the stripes `which` by n decodes and n checks of a copy."""
        idx = torch.tensor(which, device="cuda")
        out = []
        for j in range(n):
            torch.index_select(pool, 0, idx, out=scratch)
            rs.decodeMissingBatch(scratch, [i != j for i in range(n)], n * L, L, len(which), 0, L)
            rs.isParityCorrectBatch(scratch, n * L, L, len(which), 0, L, v)
            out.append(v.clone())
        return out

    one_pct = sorted({(s * 100 + 37) % S for s in range(max(1, S // 100))})
    sets = {"locate_1pct": (one_pct, False), "locate_all": (list(range(S)), True)}
    # the answers, before anything is timed: clean, and each corrupt set against the old route
    locate()
    torch.cuda.synchronize()
    assert culprit.cpu().tolist() == [-1] * S, "a clean pool must locate nothing"
    for leg, (which, every) in sets.items():
        want = corrupt(which, every)
        locate()
        torch.cuda.synchronize()
        assert culprit.cpu().tolist() == want, leg
        scratch = torch.empty((len(which), n, L), dtype=torch.uint8, device="cuda")
        v = torch.zeros(len(which), dtype=torch.uint8, device="cuda")
        old = torch.stack(n_decode(which, scratch, v), 1).cpu()
        assert torch.equal(old, suspect.view(S, n)[which].cpu()), leg + ": the two routes disagree"
        del scratch

    data = S * n * L
    frac = lambda ms: round(data / ms / 1e6 / HBM_PEAK_GBS, 4)  # noqa: E731
    kernels = {}
    pool.copy_(clean)
    for f in (check, locate):
        for _ in range(3):
            f()
    check()
    kernels["check"] = ecx.last_kernel()
    locate()
    kernels["locate"] = ecx.last_kernel()
    torch.cuda.synchronize()
    out = {"case": name, "k": k, "m": m, "L": L, "stripes": S, "reps": reps, "kernels": kernels}
    checks = [timed(torch, check, reps)]
    out["locate_clean_ms"] = timed(torch, locate, reps)
    checks.append(timed(torch, check, reps))
    for leg, (which, every) in sets.items():
        corrupt(which, every)
        for _ in range(2):
            locate()
        torch.cuda.synchronize()
        out[leg + "_ms"] = timed(torch, locate, reps)
        scratch = torch.empty((len(which), n, L), dtype=torch.uint8, device="cuda")
        v = torch.zeros(len(which), dtype=torch.uint8, device="cuda")
        n_decode(which, scratch, v)  # warm-up: the n decode maps compile and upload here
        torch.cuda.synchronize()
        out[leg + "_n_decode_ms"] = timed(torch, lambda: n_decode(which, scratch, v), max(3, reps // 3))
        out[leg + "_corrupt_stripes"] = len(which)
        out[leg + "_n_decode_over_locate"] = round(out[leg + "_n_decode_ms"] / out[leg + "_ms"], 2)
        del scratch
    pool.copy_(clean)
    checks.append(timed(torch, check, reps))
    check_ms = statistics.median(checks)
    out["check_ms"] = [round(x, 4) for x in checks]
    out["check_frac"] = frac(check_ms)
    out["check_spread"] = round((max(checks) - min(checks)) / check_ms, 4)
    for leg in ("locate_clean", "locate_1pct", "locate_all"):
        out[leg + "_frac"] = frac(out[leg + "_ms"])
        out[leg + "_over_check_time"] = round(out[leg + "_ms"] / check_ms, 4)
        out[leg + "_ms"] = round(out[leg + "_ms"], 4)
    for leg in sets:
        out[leg + "_n_decode_ms"] = round(out[leg + "_n_decode_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="rs173,rs124")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stripes", type=int, default=0, help="override the case's stripe count (smoke runs)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "locate_ab.jsonl"))
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
