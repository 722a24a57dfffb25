"""Shared cases of the Clay pattern-set tests (tests/test_clay_mixed.py, test_clay_mixed_capture.py,
test_clay_mixed_host.py): the erased-node lists, the stripes' ids, the buffer layouts and the
expected output buffer, which is the oracle's performCoding (ClayCodeErasureDecodingStep.java:53-107)
run per stripe with that stripe's own list.

The inputs are random bytes, not codewords, and the erased nodes' input slots hold garbage like
every other slot, so a repaired sub-chunk can only equal the oracle's if it was computed from
exactly the sub-chunks the reference reads.  The expected OUTPUT BUFFER is built whole -- guard
bytes, the gaps between slots, the slots a stripe's list does not write -- so one comparison of
every byte covers the repaired slots and everything that must stay as it was."""
import functools
import itertools
from collections import namedtuple

import numpy as np

import oracle as O

SENTINEL = 0x5A
GUARD = 64

# Clay(4,2): all 6 single nodes (ids 0-5), all 15 pairs (ids 6-20) and the empty list (id 21)
LISTS42 = [[i] for i in range(6)] + [list(c) for c in itertools.combinations(range(6), 2)] + [[]]
# 24 stripes: every list once, id 255 (no list), one repeat (7); unsorted, neighbours differ
IDS42 = [7, 0, 20, 3, 255, 12, 5, 21, 9, 1, 16, 6, 4, 13, 2, 18, 8, 10, 19, 11, 14, 17, 15, 7]
assert sorted(set(IDS42)) == list(range(22)) + [255] and len(IDS42) == 24
assert all(a != b for a, b in zip(IDS42, IDS42[1:]))

# A batch layout: buf_size and the four strides; the output has `out_slots` slots per stripe
Layout = namedtuple("Layout", "B in_stripe in_sub out_stripe out_sub")


def layout(B, n_in, out_slots, in_pitch=None, out_pitch=None, in_extra=0, out_extra=0):
    in_pitch = B if in_pitch is None else in_pitch
    out_pitch = B if out_pitch is None else out_pitch
    return Layout(B, n_in * in_pitch + in_extra, in_pitch, out_slots * out_pitch + out_extra, out_pitch)


def alpha_of(k, m, v=0):
    return m ** ((k + v + m) // m)


@functools.lru_cache(maxsize=None)
def _oracle_stripe(k, m, erased, B, in_sub, raw):
    """The oracle's |E|*alpha output sub-chunks of one stripe (raw: its input bytes)."""
    n, a = k + m, alpha_of(k, m)
    host = np.frombuffer(raw, np.uint8)
    inputs = [None if (i % n) in erased else host[i * in_sub:i * in_sub + B].copy() for i in range(n * a)]
    ref = [np.zeros(B, np.uint8) for _ in range(len(erased) * a)]
    O.Clay(k, m, list(erased)).perform_coding(inputs, ref, B)
    return tuple(r.tobytes() for r in ref)


@functools.lru_cache(maxsize=None)
def make_input(k, m, S, lay, seed):
    """S stripes of n*alpha slots of fill_random bytes, flat, in the layout's strides: the host
    copy (read-only, shared by the tests that use the case)."""
    import torch
    import rpamd
    ecx = rpamd.load(shape_knobs=True)
    n_in = (k + m) * alpha_of(k, m)
    size = (S - 1) * lay.in_stripe + (n_in - 1) * lay.in_sub + lay.B
    dev = torch.empty(size, dtype=torch.uint8, device="cuda")
    ecx.fill_random(dev, size, seed)
    torch.cuda.synchronize()
    flat = dev.cpu().numpy()
    flat.setflags(write=False)
    return flat


def expected_output(k, m, lists, ids, lay, out_slots, flat_in, fill=SENTINEL, unwritten=None):
    """The whole output buffer after the call: GUARD bytes, S stripes of out_slots slots in the
    layout's strides, GUARD bytes, prefilled with `fill`; stripe s holds the oracle's sub-chunks
    of list ids[s] in slots 0 .. |E|*alpha - 1.  `unwritten` (the host form's zero rule): the
    value of bytes [0, B) of the other slots below `unwritten[1]` -- (value, slot count)."""
    S, a = len(ids), alpha_of(k, m)
    n_in = (k + m) * a
    size = 2 * GUARD + (S - 1) * lay.out_stripe + (out_slots - 1) * lay.out_sub + lay.B
    want = np.full(size, fill, np.uint8)
    for s, pid in enumerate(ids):
        erased = tuple(lists[pid]) if pid < len(lists) else ()
        base = GUARD + s * lay.out_stripe
        if unwritten is not None:
            for slot in range(unwritten[1]):
                want[base + slot * lay.out_sub:base + slot * lay.out_sub + lay.B] = unwritten[0]
        if not erased:
            continue
        raw = flat_in[s * lay.in_stripe:s * lay.in_stripe + (n_in - 1) * lay.in_sub + lay.B].tobytes()
        for slot, sub in enumerate(_oracle_stripe(k, m, erased, lay.B, lay.in_sub, raw)):
            want[base + slot * lay.out_sub:base + slot * lay.out_sub + lay.B] = np.frombuffer(sub, np.uint8)
    return want
