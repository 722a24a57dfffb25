"""Shared cases of the generated Clay repair kernel sweep (tests/test_clay_rtc_sweep.py on the GPU,
tests/test_clay_rtc_sweep_cpu.py without one): the codes, every real node of each, the nodes picked
for the knob and layout parts, the arrangement a generated source declares in its first line, the
batch layouts, and the expected OUTPUT BUFFER.

clay_rtc.cpp writes different source for every erased node (ex, ey) and every placement of virtual
nodes: which row is exchanged in lane rows (ya), which through LDS (yb), which is read from memory
(yc), the plane weights in z, the zero-fill of virtual own loads, the zero-page partner loads and the
mate stores all depend on them.  The host pins the repair PROGRAM against the composed map; the step
from program to source is pinned only by running it, so the sweep runs every node of every code.

The inputs are random bytes, not codewords, and the erased node's input slots hold garbage like every
other slot.  The expected buffer is built whole -- guard bytes, the gaps between padded slots -- from
the oracle alone (ClayCodeErasureDecodingStep.java:53-107; a shortened code is the reference
Clay(k+v, m) with the virtual data nodes zero-filled), for every stripe and every sub-chunk, so one
comparison of every byte covers the repair and everything that must stay as it was."""
import contextlib
import functools
import re
from collections import namedtuple

import numpy as np

SENTINEL = 0x5A
GUARD = 64  # a multiple of 16: the guard alone leaves the bases 16-byte aligned
S = 9       # 9 * 8 * G slice units: one full period of the rtc_xcd block maps plus a remainder
B = 4096

# (k, m, v): Clay(k, m) shortened from Clay(k + v, m); the virtual nodes are k .. k+v-1 of that code
GRP_CODES = [(12, 4, 0), (11, 4, 1), (10, 4, 2), (9, 4, 3),  # t = 4: one row from memory, 4 plane groups
             (8, 4, 0), (7, 4, 1), (6, 4, 2), (5, 4, 3),     # t = 3: no row from memory; shortened: ya > yb
             (6, 4, 6), (3, 4, 9)]                           # whole rows virtual, virtual nodes in ya / yb / yc
PLANE_CODES = [(4, 2, 0), (3, 2, 1), (2, 2, 0), (6, 3, 0), (5, 3, 1), (3, 3, 0), (1, 4, 3)]
CODES = GRP_CODES + PLANE_CODES
# part a: every real node of every code
NODE_CASES = [(k, m, v, e) for k, m, v in CODES for e in range(k + m)]

# part b: one node per distinct arrangement (ya, yb, rows from memory, erased row) of four codes --
# test_clay_rtc_sweep_cpu.py checks that the picks cover every arrangement those codes have
KNOB_NODES = [(10, 4, 2, 2), (10, 4, 2, 5), (10, 4, 2, 8), (10, 4, 2, 13),
              (6, 4, 2, 3), (6, 4, 2, 5), (6, 4, 2, 8),
              (6, 4, 6, 1), (6, 4, 6, 4), (6, 4, 6, 9),
              (12, 4, 0, 3), (12, 4, 0, 6), (12, 4, 0, 9), (12, 4, 0, 12)]
# the knob families: each a list of settings run one after the other on one input
KNOB_FAMILIES = {
    "sched": [{"rtc_sched": s} for s in (0, 1, 2)],
    "lookahead": [{"rtc_sched": 0, "rtc_lookahead": la} for la in (0, 1, 3, 5, 6, 12)],
    "xcd": [{"rtc_xcd": x} for x in (0, 1, 2, 3, 4)],
    "waves": [{"rtc_waves": w} for w in (2, 4)],
    "nt": [{"rtc_nt": nt} for nt in (0, 15)],
    "group0": [{"rtc_group": 0}],
    "wide": [{"rtc_wide": 1}],
}
# the two-slice units and the persistent grid exist in the diagnostic library only
DIAG_SETTINGS = [{"rtc_units": 2, "rtc_sched": 0}, {"rtc_persist": 2}]
KNOB_CASES = [(code_e, fam) for code_e in KNOB_NODES for fam in KNOB_FAMILIES]

# part c: a data node and a parity node of a t = 4 and of a t = 3 shortened code
LAYOUT_NODES = [(10, 4, 2, 6), (10, 4, 2, 11), (6, 4, 2, 4), (6, 4, 2, 7)]


def is_grp(k, m, v):
    """clay_grp_supported (clay_rtc.cpp): q = 4 and at least two free plane digits."""
    return m == 4 and (k + v + m) // m >= 3


def alpha_of(k, m, v):
    return m ** ((k + v + m) // m)


Arrangement = namedtuple("Arrangement", "ya yb mem_rows groups ex ey")
_HEADER = re.compile(r"rows ya=(\d+) \(lane rows\), yb=(\d+) \(waves\), (\d+) row\(s\) from memory, "
                     r"(\d+) plane groups, erased \((\d+), (\d+)\)")


def arrangement(src):
    """What the plane-group kernel's source says of itself in its first line."""
    m = _HEADER.search(src.split("\n", 1)[0])
    assert m, src[:200]
    return Arrangement(*map(int, m.groups()))


def memory_row_has_virtual(k, m, v, arr):
    """True when the one row whose partners come from memory holds a virtual node: then
    rtc_lookahead bit 2 asks for a second body, which rtc_sched 1 does not have (refused)."""
    if arr.mem_rows != 1:
        return False
    (yc,) = set(range((k + v + m) // m)) - {arr.ya, arr.yb, arr.ey}
    return any(k <= x + m * yc < k + v for x in range(m))


# A batch layout: buf_size, the four strides and the bases' offsets past the leading guard
Layout = namedtuple("Layout", "B in_stripe in_sub out_stripe out_sub in_off out_off")


def layout(k, m, v, B=B, in_pad=0, out_pad=0, in_off=0, out_off=0):
    n_in, a = (k + m) * alpha_of(k, m, v), alpha_of(k, m, v)
    return Layout(B, n_in * (B + in_pad), B + in_pad, a * (B + out_pad), B + out_pad, in_off, out_off)


def in_bytes(k, m, v, lay):
    return (S - 1) * lay.in_stripe + ((k + m) * alpha_of(k, m, v) - 1) * lay.in_sub + lay.B


def out_bytes(k, m, v, lay):
    return (S - 1) * lay.out_stripe + (alpha_of(k, m, v) - 1) * lay.out_sub + lay.B


def seed_of(k, m, v, e):
    return 7000 + 1000 * k + 100 * v + 10 * m + e


def device_input(ecx, torch, k, m, v, e, lay):
    """The input allocation (GUARD + in_off bytes, then the batch) filled by seed: the same bytes
    on every call, so the expected buffer is computed once per case."""
    buf = torch.empty(GUARD + lay.in_off + in_bytes(k, m, v, lay), dtype=torch.uint8, device="cuda")
    ecx.fill_random(buf, buf.numel(), seed_of(k, m, v, e))
    return buf


@functools.lru_cache(maxsize=4)
def expected_output(k, m, v, e, lay):
    """The whole output allocation after the repair of node e: GUARD + out_off sentinel bytes,
    S stripes of alpha slots in the layout's strides, GUARD sentinel bytes; every slot of every
    stripe holds the oracle's sub-chunk, every other byte the sentinel."""
    import torch
    import oracle as O
    import rpamd
    from conftest import shortened_clay_oracle
    ecx = rpamd.load(shape_knobs=True)
    n, a = k + m, alpha_of(k, m, v)
    dev = device_input(ecx, torch, k, m, v, e, lay)
    torch.cuda.synchronize()
    flat = dev.cpu().numpy()[GUARD + lay.in_off:]
    del dev
    want = np.full(GUARD + lay.out_off + out_bytes(k, m, v, lay) + GUARD, SENTINEL, np.uint8)
    for s in range(S):
        at = lambda i: s * lay.in_stripe + i * lay.in_sub  # noqa: E731
        inputs = [None if (i % n) == e else flat[at(i):at(i) + lay.B].copy() for i in range(n * a)]
        if v == 0:
            ref = [np.zeros(lay.B, np.uint8) for _ in range(a)]
            O.Clay(k, m, [e]).perform_coding(inputs, ref, lay.B)
        else:
            ref = shortened_clay_oracle(k, m, v, [e], inputs, lay.B)
        base = GUARD + lay.out_off + s * lay.out_stripe
        for z in range(a):
            want[base + z * lay.out_sub:base + z * lay.out_sub + lay.B] = ref[z]
    want.setflags(write=False)
    return want


# the library's defaults of the shape knobs the sweep sets (tuning.hpp); ecx_tune_value reads
# deployment knobs only, so the with block below puts these back
DEFAULTS = {"clay_rtc": 1, "rtc_group": 1, "rtc_sched": 2, "rtc_lookahead": 1, "rtc_xcd": 2, "rtc_waves": 3,
            "rtc_nt": 5, "rtc_wide": 0, "rtc_units": 1, "rtc_persist": 0}


@contextlib.contextmanager
def knobs(ecx, **settings):
    """ecx_tune settings for the length of a with block; the defaults come back after it."""
    try:
        for key, val in settings.items():
            ecx.tune(key, val)
        yield
    finally:
        for key in settings:
            ecx.tune(key, DEFAULTS[key])
