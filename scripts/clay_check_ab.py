"""The Clay codeword check against the routes that existed before it, A/B in one process
(DESIGN.md section 4.9).  Arms, interleaved a b c c b a per round because rates move 4-5 % between
processes (section 4.5), each leg the median of --reps launches timed with HIP events:

  a  ClayParityCheck.isParityCorrectBatch (k_clay_check), one read-only launch
  b  the two-step route: performCodingBatch with the parity nodes erased into a scratch pool, then
     count_mismatch of the scratch against the stored parity; the pair timed together
  c  Clay(4,2) only, diagnostic library only (make DIAG=1, ECX_LIB_PATH=.../libecx_diag.so): the
     existing k_gf_check over the program's dense syndrome map (16 rows, two tiles), forced
  p  with c: k_clay_check forced.  Arm a itself takes route c for geometries of at most 16
     syndrome rows, Clay(4,2) among them, because c measured faster there

  clay42   Clay(4,2), 32 KiB sub-chunks, 683 stripes (1.0 GiB)
  clay104  Clay(10,4) shortened from (12,4), 4 KiB sub-chunks, 73 stripes (1.0 GiB)

Then arm a's own sweep, each variant interleaved with the default (d v v d): ring depth 4 / 8
against 2, and the block order -- dispatch order, and runs of 2 and 8 (stripe, chunk) units per XCD,
against the alpha planes of one unit per XCD.  The bare read rate of the same pool in the same
process (the read-only probe kernel) is the ceiling arm a is judged against.

One JSON line per shape.  All arms are checked first (clean pool, then one flipped byte) and must
agree.

    ECX_SHAPE_KNOBS=1 timeout 600 python scripts/clay_check_ab.py --out profiles/clay_check_ab.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("ECX_SHAPE_KNOBS", "1")
import rpamd  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
CASES = {"clay42": (4, 2, 0, 32 << 10, 683), "clay104": (10, 4, 2, 4 << 10, 73)}
DEFAULTS = {"depth": 0, "rtc_xcd": 2, "xcd_group": 0, "xcd_run": 8}  # csrc/tuning.hpp
VARIANTS = {
    "depth4": {"depth": 4}, "depth8": {"depth": 8}, "dispatch_order": {"rtc_xcd": 0},
    "run2": {"xcd_group": 3, "xcd_run": 2}, "run8": {"xcd_group": 3, "xcd_run": 8},
}


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


def spread(legs, med):
    return round((max(legs) - min(legs)) / med, 4)


def run_case(ecx, torch, name, reps, stripes, rounds):
    k, m, v, B, S = CASES[name]
    S = stripes or S
    chk = ecx.ClayParityCheck(k, m, v)
    q, t, alpha, nr = chk.geometry()
    slots = alpha * nr
    pool = torch.empty((S, slots, B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(pool, pool.numel(), 4900 + k)
    enc = ecx.ClayCodeErasureDecodingStep(list(range(k, k + m)), k, m, v)
    scratch = torch.empty((S, alpha * m, B), dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    verdict = torch.zeros(S, dtype=torch.uint8, device="cuda")
    vdense = torch.zeros(S, dtype=torch.uint8, device="cuda")
    stored = pool.view(-1)[k * B:]  # parity nodes k .. k+m-1 of a plane are m * B consecutive bytes

    def encode_into(dst):
        enc.performCodingBatch(pool, slots * B, B, dst, alpha * m * B, B, S, B)

    # the pool's parity is the engine's own encode (tests/test_clay_check.py holds it to the oracle)
    encode_into(scratch)
    pool.view(S, alpha, nr, B)[:, :, k:, :] = scratch.view(S, alpha, m, B)

    def arm_a():
        chk.isParityCorrectBatch(pool, slots * B, B, S, B, verdict)

    def arm_b():
        encode_into(scratch)
        ecx.count_mismatch(scratch, m * B, stored, nr * B, S * alpha, m * B, count)

    dense = planes = None
    if name == "clay42" and ecx.is_diag():
        route_fn = ecx.lib().ecx_diag_clay_check_route_batch
        I, P, I64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
        route_fn.argtypes, route_fn.restype = [I, I, I, I, P, I64, I64, I64, I64, P, P], I
        stream = int(torch.cuda.current_stream().cuda_stream)

        def dense():
            assert route_fn(1, k, m, v, pool.data_ptr(), slots * B, B, S, B, vdense.data_ptr(), stream) == 0

        def planes():
            assert route_fn(0, k, m, v, pool.data_ptr(), slots * B, B, S, B, verdict.data_ptr(), stream) == 0

    arms = {"a": arm_a, "b": arm_b}
    if dense:
        arms["c"] = dense
        arms["p"] = planes

    # every arm agrees before anything is timed: a clean pool, then one flipped byte
    def verdicts_of_b():
        per_stripe = []
        for s in (0, S - 1):
            count.zero_()
            ecx.count_mismatch(scratch[s], m * B, pool[s].view(-1)[k * B:], nr * B, alpha, m * B, count)
            per_stripe.append(int(count.item()) == 0)
        return per_stripe

    for flipped in (False, True):
        if flipped:
            pool[S - 1, slots - 1, B - 1] ^= 1
        arm_a()
        encode_into(scratch)
        if dense:
            dense()
        torch.cuda.synchronize()
        want = [1] * (S - 1) + [0 if flipped else 1]
        assert verdict.cpu().tolist() == want, "k_clay_check disagrees"
        assert verdicts_of_b() == [True, not flipped], "the two-step route disagrees"
        assert not dense or vdense.cpu().tolist() == want, "the dense check map disagrees"
        if flipped:
            pool[S - 1, slots - 1, B - 1] ^= 1
    arm_a()
    kernel = ecx.last_launch_shape()
    for f in arms.values():  # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()

    data = S * slots * B
    frac = lambda ms: round(data / ms / 1e6 / HBM_PEAK_GBS, 4)  # noqa: E731
    order = "".join(arms) + "".join(reversed(arms))
    legs = {a: [] for a in arms}
    for _ in range(rounds):
        for a in order:
            legs[a].append(timed(torch, arms[a], reps))
    med = {a: statistics.median(x) for a, x in legs.items()}
    out = {"case": name, "k": k, "m": m, "v": v, "alpha": alpha, "buf_size": B, "stripes": S, "bytes_read": data,
           "reps": reps, "order": order, "rounds": rounds, "kernel": kernel,
           "ms": {a: round(x, 4) for a, x in med.items()},
           "legs_ms": {a: [round(y, 4) for y in x] for a, x in legs.items()},
           "spread": {a: spread(legs[a], med[a]) for a in arms},
           "frac_of_hbm": {a: frac(x) for a, x in med.items()},
           "b_over_a_time": round(med["b"] / med["a"], 4)}
    if dense:
        out["c_over_p_time"] = round(med["c"] / med["p"], 4)

    # the ceiling: the bare read of the same pool, interleaved with arm a
    nprobe = data // (16 << 10) * (16 << 10)

    def bare():
        ecx.probe_bandwidth(0, pool, pool, nprobe, False)

    for _ in range(3):
        bare()
    rl, al = [], []
    for _ in range(rounds):
        al.append(timed(torch, arm_a, reps))
        rl.append(timed(torch, bare, reps))
        rl.append(timed(torch, bare, reps))
        al.append(timed(torch, arm_a, reps))
    rmed = statistics.median(rl)
    out["bare_read"] = {"ms": round(rmed, 4), "frac_of_hbm": round(nprobe / rmed / 1e6 / HBM_PEAK_GBS, 4),
                        "spread": spread(rl, rmed), "a_ms": round(statistics.median(al), 4),
                        "a_over_read_rate": round(rmed / statistics.median(al) * data / nprobe, 4)}

    # arm a's sweep: default, variant, variant, default
    sweep = {}
    swept = planes or arm_a
    for vname, knobs in (VARIANTS if planes or m * alpha > 16 else {}).items():  # (k_clay_check's knobs)
        d, x = [], []
        for leg in "dvvd" * rounds:
            for key, val in (knobs if leg == "v" else {}).items():
                ecx.tune(key, val)
            swept()  # (a forced depth uploads its plan on its first use)
            (x if leg == "v" else d).append(timed(torch, swept, reps))
            for key, val in DEFAULTS.items():
                ecx.tune(key, val)
        dm, xm = statistics.median(d), statistics.median(x)
        sweep[vname] = {"default_ms": round(dm, 4), "ms": round(xm, 4), "over_default_time": round(xm / dm, 4),
                        "spread": max(spread(d, dm), spread(x, xm))}
    out["sweep"] = sweep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="clay42,clay104")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stripes", type=int, default=0, help="override the case's stripe count (smoke runs)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clay_check_ab.jsonl"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    ecx = rpamd.load(shape_knobs=True)
    for name in args.case.split(","):
        res = run_case(ecx, torch, name, args.reps, args.stripes, args.rounds)
        res["library"] = "diag" if ecx.is_diag() else "product"
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
