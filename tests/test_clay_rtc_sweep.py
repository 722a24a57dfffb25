"""The generated Clay single-node repair kernels (clay_rtc.cpp: k_clay_repair_grp, the plane-group
kernel of q = 4 codes, and k_clay_repair, one helper plane per workgroup) swept over every real
node of every code in tests/clay_rtc_sweep_cases.py, over the launch-shape knobs on one node per
arrangement, and over the layout edges.  Every comparison is of the whole output allocation, byte
for byte, with a buffer built from the oracle alone: all 9 stripes, every sub-chunk, and the
sentinel in the guard bytes and between padded slots (clay_rtc_sweep_cases.expected_output)."""
import numpy as np
import pytest

import clay_rtc_sweep_cases as C
from conftest import diag_build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def repair(ecx, torch, k, m, v, e, lay):
    """One performCodingBatch of node e's repair in the layout -> (whole output allocation, kernel)."""
    step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
    assert step.subPacketSize == C.alpha_of(k, m, v)
    inp = C.device_input(ecx, torch, k, m, v, e, lay)
    out = torch.full((C.GUARD + lay.out_off + C.out_bytes(k, m, v, lay) + C.GUARD,), C.SENTINEL,
                     dtype=torch.uint8, device="cuda")
    step.performCodingBatch(inp[C.GUARD + lay.in_off:], lay.in_stripe, lay.in_sub,
                            out[C.GUARD + lay.out_off:len(out) - C.GUARD], lay.out_stripe, lay.out_sub, C.S, lay.B)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ecx.last_kernel()


def assert_same(got, want, k, m, v, lay, what):
    """got == want; the message names the first bytes that differ as (stripe, sub-chunk, byte), a
    sub-chunk index >= alpha or a byte >= B meaning a guard or gap byte."""
    if np.array_equal(got, want):
        return
    bad = np.nonzero(got != want)[0]
    where = []
    for off in bad[:6]:
        rel = int(off) - C.GUARD - lay.out_off
        s, r = divmod(rel, lay.out_stripe) if rel >= 0 else (-1, rel)
        where.append((s, r // lay.out_sub, r % lay.out_sub))
    slots = sorted({(int(o) - C.GUARD - lay.out_off) % lay.out_stripe // lay.out_sub for o in bad})
    raise AssertionError(f"{what}: {len(bad)} bytes differ from the oracle; first (stripe, sub-chunk, byte) "
                         f"{where}; {len(slots)} sub-chunk indexes touched, first {slots[:16]}")


# ---------------------------------------------------------------- a. every node, default shape
@pytest.mark.parametrize("k,m,v,e", C.NODE_CASES)
def test_every_node_default_shape_vs_oracle(ecx, torch_dev, k, m, v, e):
    """Every real node of every code, at the launch shape a caller gets: the plane-group codes on
    auto (clay_rtc 1 picks the generated kernel for alpha > 8), the others with clay_rtc forced to 2.
    The kernel that ran is the one clay_grp_supported implies."""
    lay = C.layout(k, m, v)
    want = C.expected_output(k, m, v, e, lay)
    grp = C.is_grp(k, m, v)
    with C.knobs(ecx, clay_rtc=1 if grp else 2):
        got, kern = repair(ecx, torch_dev, k, m, v, e, lay)
    assert kern == ("k_clay_repair_grp" if grp else "k_clay_repair"), kern
    assert_same(got, want, k, m, v, lay, (k, m, v, e))


# ---------------------------------------------------------------- b. knob classes
@pytest.mark.parametrize("code_e,family", C.KNOB_CASES,
                         ids=lambda p: "-".join(map(str, p)) if isinstance(p, tuple) else p)
def test_knob_families_vs_oracle(ecx, torch_dev, code_e, family):
    """One node per arrangement of Clay(10,4) v=2, Clay(6,4) v=2, Clay(6,4) v=6 and Clay(12,4), at
    every value of each launch-shape knob: the same bytes as the oracle at every setting.  A setting
    the generator refuses must be one it refuses by design (rtc_sched 1 has no second body), and the
    refusal an EcxError that leaves no kernel launched, never another kernel run in silence."""
    k, m, v, e = code_e
    lay = C.layout(k, m, v)
    want = C.expected_output(k, m, v, e, lay)
    step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
    arr = C.arrangement(step.rtcSource())
    settings = list(C.KNOB_FAMILIES[family])
    if family == "xcd" and diag_build():
        settings += C.DIAG_SETTINGS
    for kn in settings:
        refused = (kn.get("rtc_sched") == 1 and kn.get("rtc_lookahead", 1) & 4
                   and C.memory_row_has_virtual(k, m, v, arr))
        with C.knobs(ecx, clay_rtc=2, **kn):
            if refused:
                with pytest.raises(ecx.EcxError):
                    repair(ecx, torch_dev, k, m, v, e, lay)
                continue
            got, kern = repair(ecx, torch_dev, k, m, v, e, lay)
        assert kern == ("k_clay_repair" if kn.get("rtc_group") == 0 else "k_clay_repair_grp"), (kn, kern)
        assert_same(got, want, k, m, v, lay, (code_e, kn))


@pytest.mark.parametrize("k,m,v,e", [(10, 4, 2, 5), (6, 4, 6, 1)])
def test_lean_schedule_refuses_second_body(ecx, torch_dev, k, m, v, e):
    """rtc_sched 1 with rtc_lookahead bit 2 on a repair whose memory row holds virtual nodes: the
    generator has no such kernel.  Forced or on auto, the call fails with an EcxError and writes
    nothing; it does not run another kernel in its place."""
    lay = C.layout(k, m, v)
    for mode in (2, 1):
        with C.knobs(ecx, clay_rtc=mode, rtc_sched=1, rtc_lookahead=5):
            step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
            inp = C.device_input(ecx, torch_dev, k, m, v, e, lay)
            out = torch_dev.full((C.GUARD + C.out_bytes(k, m, v, lay) + C.GUARD,), C.SENTINEL,
                                 dtype=torch_dev.uint8, device="cuda")
            with pytest.raises(ecx.EcxError):
                step.performCodingBatch(inp[C.GUARD:], lay.in_stripe, lay.in_sub, out[C.GUARD:len(out) - C.GUARD],
                                        lay.out_stripe, lay.out_sub, C.S, lay.B)
            torch_dev.cuda.synchronize()
            assert bool((out == C.SENTINEL).all()), mode


# ---------------------------------------------------------------- c. layout edges
LAYOUTS = {
    # input slot pitch B + 16, output slot pitch B + 4096
    "padded": dict(in_pad=16, out_pad=4096),
    # both bases 16 bytes into their allocations
    "offset16": dict(in_off=16, out_off=16),
    # two whole 4 KiB chunks on the generated kernel, 48 bytes on the composed-map kernel
    "tail": dict(B=2 * 4096 + 48),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("k,m,v,e", C.LAYOUT_NODES)
def test_layout_edges_vs_oracle(ecx, torch_dev, k, m, v, e, name):
    """Padded slot pitches, bases offset by 16 bytes and a ragged byte count, on the default launch:
    the generated kernel runs and the whole allocation equals the oracle's, the bytes between padded
    output slots and around the batch keeping the sentinel."""
    lay = C.layout(k, m, v, **LAYOUTS[name])
    want = C.expected_output(k, m, v, e, lay)
    got, kern = repair(ecx, torch_dev, k, m, v, e, lay)
    assert kern == "k_clay_repair_grp", kern
    assert_same(got, want, k, m, v, lay, (k, m, v, e, name))


@pytest.mark.parametrize("which", ["in", "out"])
@pytest.mark.parametrize("k,m,v,e", C.LAYOUT_NODES)
def test_unaligned_base_runs_no_generated_kernel(ecx, torch_dev, k, m, v, e, which):
    """A base one byte off 16-byte alignment (the input's or the output's) cannot use the generated
    kernels' 16-byte loads and stores: the composed-map kernel's byte-safe form runs instead, and
    the whole allocation still equals the oracle's.  A byte-safe launch leaves ecx_last_kernel as it
    was (launch_rules.hpp), and every generated-kernel launch sets it, so the name is first set by
    an aligned RS encode: afterwards it is still no generated kernel's."""
    torch = torch_dev
    shards = torch.zeros((1, 6, 4096), dtype=torch.uint8, device="cuda")
    ecx.ReedSolomon.create(4, 2).encode_map().apply_batch(shards, 6 * 4096, 4096, shards, 6 * 4096, 4096, 1, 4096)
    torch.cuda.synchronize()
    before = ecx.last_kernel()
    assert before and not before.startswith("k_clay_repair"), before
    lay = C.layout(k, m, v, **{which + "_off": 1})
    want = C.expected_output(k, m, v, e, lay)
    got, kern = repair(ecx, torch, k, m, v, e, lay)
    assert kern and not kern.startswith("k_clay_repair"), (kern, before)
    assert_same(got, want, k, m, v, lay, (k, m, v, e, which))
