"""ecx_clay_is_parity_correct_batch under stream capture, by the protocol of
tests/test_gpu_capture.py (its helpers are imported, the file is not edited): after a warm-up call
outside capture the call is captured on one stream, the graph holds kernel nodes only
(k_clay_set_verdicts, the vector body, the byte-safe tail -- a memset node replays with the value
0 from its second replay on), and the replays follow a pool whose flips
move between them.  The ClayParityCheck object holds the codec, and with it the device records the
graph's nodes point to, for as long as the graph lives."""
import numpy as np
import pytest

import clay_check_cases as C
from test_gpu_capture import _refused, capture, kernels_only, node_types

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_replays_follow_the_pool(ecx, torch_dev):
    """Clay(6,3), 10 clean stripes of 4096 + 32 bytes per sub-chunk.  Four replays: clean -> all 1;
    flips in stripes 2 and 7 -> those 0; the flips moved to stripes 0 and 9 (one in the byte-safe
    tail) -> those 0 and 2 and 7 pass again; all taken back -> all 1."""
    torch = torch_dev
    S, B = 10, C.CHUNK + 32
    case = C.build(6, 3, 0, B, B, S, [], 8800)
    flat, view, stride = C.device_pool(case, torch)
    verdict = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")
    chk = ecx.ClayParityCheck(6, 3)

    def call():
        chk.isParityCorrectBatch(view, stride, B, S, B, verdict)

    call()  # once outside the capture
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [1] * S + [GUARD] * 16
    g = capture(torch, call)
    types = node_types(g)
    assert kernels_only(types, 3) and len(types) == 3, types  # k_clay_set_verdicts, body, tail
    rounds = [[], [(2, 5, 1, 100, 3), (7, 0, 4, 4095, 0)], [(0, 26, 8, B - 1, 7), (9, 3, 0, 0, 1)], []]
    for sites in rounds:
        C.flip_sites(case, torch, view, sites)
        verdict.fill_(GUARD)
        before = flat.clone()
        g.replay()
        torch.cuda.synchronize()
        want = np.ones(S, np.uint8)
        want[[s for s, *_ in sites]] = 0
        assert verdict.cpu().tolist() == want.tolist() + [GUARD] * 16, (sites, verdict.cpu().tolist())
        assert torch.equal(flat, before)
        C.flip_sites(case, torch, view, sites)


def test_first_check_of_a_geometry_inside_a_capture_is_refused(ecx, torch_dev):
    """A geometry whose node records were never uploaded to this device: its first check on a
    capturing stream is refused with ECX_E_DEVICE before anything is enqueued, and after one eager
    call the same call captures as kernel nodes."""
    torch = torch_dev
    k, m, S, B = 4, 4, 3, 64  # Clay(4,4): q = 4, t = 2, alpha = 16, used by no other test
    case = C.build(k, m, 0, B, B, S, [(1, 11, 5, 63, 6)], 8801, count=2)
    flat, view, stride = C.device_pool(case, torch)
    verdict = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")
    chk = ecx.ClayParityCheck(k, m)

    def call():
        chk.isParityCorrectBatch(view, stride, B, S, B, verdict)

    _refused(ecx, torch, call)
    torch.cuda.synchronize()
    assert (verdict.cpu().numpy() == GUARD).all()
    call()
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [1, 0, 1] + [GUARD] * 16
    g = capture(torch, call)
    assert kernels_only(node_types(g), 2)
    verdict.fill_(GUARD)
    g.replay()
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [1, 0, 1] + [GUARD] * 16
