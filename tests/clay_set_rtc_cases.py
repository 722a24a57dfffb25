"""Shared cases of the generated Clay set kernel's GPU tests (tests/test_clay_set_rtc.py,
test_clay_set_rtc_capture.py, test_clay_set_rtc_host.py): the lists and ids the issue of the feature
names, the batch layouts, the device input and the expected OUTPUT BUFFER.

As in tests/clay_rtc_sweep_cases.py the inputs are random bytes, the erased nodes' slots hold garbage,
and the expected buffer is built whole from the oracle alone (ClayCodeErasureDecodingStep.java:53-107;
a shortened code is the reference Clay(k+v, m) with the virtual data nodes zero-filled): the guard
bytes, the gaps between padded slots, the stripes whose id has no list or the empty list, and every
sub-chunk of every repaired stripe -- one comparison of every byte covers the repair and everything
that must stay as it was."""
import functools

import numpy as np

from clay_rtc_sweep_cases import GUARD, SENTINEL, Layout, alpha_of

S = 9  # 9 * 8 slices * 4 plane groups: one full period of the rtc_xcd block maps plus a remainder
B = 4096

# Clay(10,4) shortened from Clay(12,4): one node per erased row, the empty list and a duplicate
LISTS104 = ((2,), (5,), (8,), (13,), (), (2,))
# neighbours differ; id 255 (no list) and the empty list (4) fall in the full period of 8 stripes,
# and a repaired stripe (the last) in the remainder
IDS104 = (2, 0, 3, 255, 1, 5, 4, 3, 1)
LISTS124 = ((3,), (6,), (9,), (12,))
IDS124 = (2, 0, 3, 255, 1, 3, 0, 2, 1)
# the layout and knob cases: a data node and a parity node
LISTS_LAYOUT = ((6,), (11,))
IDS_LAYOUT = (0, 1, 1, 0, 255, 1, 0, 1, 0)


def layout(k, m, v, B=B, in_pad=0, out_pad=0, in_off=0, out_off=0, out_slots=None):
    a = alpha_of(k, m, v)
    n_in, n_out = (k + m) * a, a if out_slots is None else out_slots
    return Layout(B, n_in * (B + in_pad), B + in_pad, n_out * (B + out_pad), B + out_pad, in_off, out_off)


def in_bytes(k, m, v, lay, S=S):
    return (S - 1) * lay.in_stripe + ((k + m) * alpha_of(k, m, v) - 1) * lay.in_sub + lay.B


def out_bytes(lay, S=S):
    """Bytes from the output base to the end of the last slot the layout's stripe stride holds."""
    return (S - 1) * lay.out_stripe + (lay.out_stripe // lay.out_sub - 1) * lay.out_sub + lay.B


def device_input(ecx, torch, k, m, v, lay, seed, S=S):
    """The input allocation (GUARD + in_off bytes, then the batch) filled by seed."""
    buf = torch.empty(GUARD + lay.in_off + in_bytes(k, m, v, lay, S), dtype=torch.uint8, device="cuda")
    ecx.fill_random(buf, buf.numel(), seed)
    return buf


def oracle_stripe(k, m, v, e, inputs, nbytes):
    """The oracle's alpha sub-chunks of one stripe repaired for node e (inputs: n*alpha arrays)."""
    import oracle as O
    from conftest import shortened_clay_oracle
    n, a = k + m, alpha_of(k, m, v)
    inputs = [None if (i % n) == e else x for i, x in enumerate(inputs)]
    if v == 0:
        ref = [np.zeros(nbytes, np.uint8) for _ in range(a)]
        O.Clay(k, m, [e]).perform_coding(inputs, ref, nbytes)
        return ref
    return shortened_clay_oracle(k, m, v, [e], inputs, nbytes)


@functools.lru_cache(maxsize=6)
def expected_output(k, m, v, lists, ids, lay, seed, unwritten=None):
    """The whole output allocation after the mixed call over device_input(seed): GUARD + out_off
    sentinel bytes, len(ids) stripes in the layout's strides, GUARD sentinel bytes.  Stripe s holds
    the oracle's sub-chunks of list ids[s] in slots 0..alpha-1; a stripe without a list keeps the
    sentinel -- or, with `unwritten` (the host form's zero rule), zeros in bytes [0, B) of slots
    0..alpha-1."""
    import torch
    import rpamd
    ecx = rpamd.load(shape_knobs=True)
    n, a, nst = k + m, alpha_of(k, m, v), len(ids)
    dev = device_input(ecx, torch, k, m, v, lay, seed, nst)
    torch.cuda.synchronize()
    flat = dev.cpu().numpy()[GUARD + lay.in_off:]
    del dev
    want = np.full(GUARD + lay.out_off + out_bytes(lay, nst) + GUARD, SENTINEL, np.uint8)
    for s, pid in enumerate(ids):
        base = GUARD + lay.out_off + s * lay.out_stripe
        erased = lists[pid] if pid < len(lists) else ()
        if unwritten is not None:
            for z in range(a):
                want[base + z * lay.out_sub:base + z * lay.out_sub + lay.B] = unwritten
        if not erased:
            continue
        at = lambda i: s * lay.in_stripe + i * lay.in_sub  # noqa: E731
        ref = oracle_stripe(k, m, v, erased[0], [flat[at(i):at(i) + lay.B].copy() for i in range(n * a)], lay.B)
        for z in range(a):
            want[base + z * lay.out_sub:base + z * lay.out_sub + lay.B] = ref[z]
    want.setflags(write=False)
    return want


def run_mixed(ecx, torch, ps, k, m, v, ids, lay, seed, stream=None):
    """One performCodingBatchMixed over device_input(seed) -> (whole output allocation, kernel)."""
    nst = len(ids)
    inp = device_input(ecx, torch, k, m, v, lay, seed, nst)
    out = torch.full((GUARD + lay.out_off + out_bytes(lay, nst) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    dev_ids = torch.tensor(list(ids), dtype=torch.uint8, device="cuda")
    ps.performCodingBatchMixed(inp[GUARD + lay.in_off:], lay.in_stripe, lay.in_sub,
                               out[GUARD + lay.out_off:len(out) - GUARD], lay.out_stripe, lay.out_sub, dev_ids, nst,
                               lay.B, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ecx.last_kernel()


def assert_same(got, want, lay, what):
    """got == want; the message names the first differing bytes as (stripe, sub-chunk, byte)."""
    if np.array_equal(got, want):
        return
    bad = np.nonzero(got != want)[0]
    where = []
    for off in bad[:6]:
        rel = int(off) - GUARD - lay.out_off
        s, r = divmod(rel, lay.out_stripe) if rel >= 0 else (-1, rel)
        where.append((s, r // lay.out_sub, r % lay.out_sub))
    stripes = sorted({(int(o) - GUARD - lay.out_off) // lay.out_stripe for o in bad})
    raise AssertionError(f"{what}: {len(bad)} bytes differ from the oracle; first (stripe, sub-chunk, byte) {where}; "
                         f"stripes touched {stripes}")
