"""ecx_clay_is_parity_correct_batch on the GPU (k_clay_check, csrc/apply_clay_check.hip): whole
verdict vectors against the expected ones of tests/clay_check_cases.py, which
tests/test_clay_check_cpu.py ties to the oracle.  Four groups: every (plane, node) sub-chunk is seen,
every byte and lane position is seen, every (stripe, chunk, plane) workgroup is visited, and
Clay(12,4) unshortened.  Geometries of at most 16 syndrome rows, Clay(2,2) and Clay(4,2), run their
dense syndrome map on k_gf_check, so the byte and unit groups also run on
Clay(3,3), which k_clay_check takes.  The verdict array carries guard bytes behind it, and the pool
is compared with a clone of itself after the call (the check is read-only)."""
import numpy as np
import pytest

import clay_check_cases as C

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def run(ecx, torch, case, base_offset=0, stripe_pad=0, view=None, flat=None, stride=None):
    """The verdicts of a case's pool (built on the device unless given), read-only on the pool."""
    if view is None:
        flat, view, stride = C.device_pool(case, torch, base_offset=base_offset, stripe_pad=stripe_pad)
    S = case.nstripes
    verdict = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")
    chk = ecx.ClayParityCheck(case.k, case.m, case.v)
    before = flat.clone()
    chk.isParityCorrectBatch(view, stride, case.pitch, S, case.B, verdict)
    torch.cuda.synchronize()
    got = verdict.cpu().numpy()
    assert (got[S:] == GUARD).all(), "bytes behind the verdicts were written"
    assert torch.equal(flat, before), "the check wrote to the stripes"
    del before
    return got[:S]


def assert_verdicts(got, want, case):
    wrong = np.nonzero(got != want)[0]
    site_of = {s: site for site in case.sites for s in [site[0]]}
    assert wrong.size == 0, "%d stripes differ; first: %s" % (
        wrong.size, [(int(s), int(got[s]), int(want[s]), site_of.get(int(s))) for s in wrong[:8]])


# ---------------------------------------------------------------- every sub-chunk is seen
@pytest.mark.parametrize("k,m,v,B,cover,kernel", [
    (4, 2, 0, 4096, False, "k_gf_check<false, 4, 8>"),      # 48 sites, the vector path (16 dense rows: k_gf_check)
    (4, 2, 0, 48, False, None),                             # 48 sites, the byte-safe path
    (6, 3, 0, 4096, False, "k_clay_check<false, 2, 4>"),    # 243 sites, q = 3
    (10, 4, 2, 16, False, None),                            # all 3,584 sites, byte-safe, virtual partners
    (10, 4, 2, 4096, True, "k_clay_check<false, 2, 4>"),    # every node x the covering planes, vector
])
def test_a_flip_in_every_subchunk_is_seen(ecx, torch_dev, k, m, v, B, cover, kernel):
    case = C.subchunk_case(k, m, v, B, B, cover)
    _, _, alpha, nr = C.geometry(k, m, v)
    if not cover:
        assert {(z, n) for _, z, n, _, _ in case.sites} == {(z, n) for z in range(alpha) for n in range(nr)}
    if v:
        assert any(not C.is_dot(k, m, v, z, n) and C.partner(k, m, v, z, n)[1] is None for _, z, n, _, _ in case.sites)
    got = run(ecx, torch_dev, case)
    assert_verdicts(got, case.want, case)
    assert 0 < int(case.want.sum()) < case.nstripes
    if kernel:
        assert ecx.last_kernel() == kernel


# ---------------------------------------------------------------- every byte and lane position is seen
@pytest.mark.parametrize("k,m", [(4, 2), (3, 3)])  # the dense route (k_gf_check) and k_clay_check
@pytest.mark.parametrize("B,pitch,base_offset,stripe_pad", [
    (4096, 4096, 0, 0),            # one full chunk: byte 0, byte B - 1, the dword, lane and wave edges, every bit
    (4096 + 16, 4096 + 16, 0, 0),  # a vector body with a byte-safe tail of one lane
    (8192 + 5, 8192 + 16, 0, 0),   # two chunks and a 5-byte tail; 11 pad bytes whose flips pass
    (4096 + 16, 4096 + 32, 1, 0),  # the base off by one byte: byte-safe throughout
    (1001, 1011, 0, 7),            # odd sub-chunk pitch and odd stripe stride
    (1000, 1024, 0, 0),            # a padded layout: flips just past buf_size pass
])
def test_every_byte_and_lane_position_is_seen(ecx, torch_dev, k, m, B, pitch, base_offset, stripe_pad):
    case = C.byte_case(k, m, 0, B, pitch)
    bytes_hit = {byte for *_, byte, _ in case.sites}
    assert {0, B - 1} <= bytes_hit and {bit for *_, bit in case.sites} == set(range(8))
    if pitch > B:
        assert B in bytes_hit and int(case.want.sum()) > case.nstripes - len(case.sites)
    got = run(ecx, torch_dev, case, base_offset=base_offset, stripe_pad=stripe_pad)
    assert_verdicts(got, case.want, case)


# ---------------------------------------------------------------- every unit is visited
@pytest.mark.parametrize("k,m", [(2, 2), (3, 3)])
@pytest.mark.parametrize("S", [9, 17, 65])
def test_every_stripe_chunk_and_plane_is_visited(ecx, torch_dev, k, m, S):
    """Clay(2,2) at two chunks: 8 workgroups per stripe, so 9, 17 and 65 stripes leave the block
    order's last run of 8 x 4 incomplete in different ways (its 8 dense rows run on k_gf_check, one
    tile per stripe and chunk); Clay(3,3), 18 workgroups per stripe, is the same for k_clay_check.
    In every round a stripe carries one flip in a dot node of one plane at a byte of one chunk: only
    that workgroup can clear its verdict."""
    torch = torch_dev
    case, rounds = C.unit_case(k, m, 0, 2 * C.CHUNK, S)
    flat, view, stride = C.device_pool(case, torch)
    assert run(ecx, torch, case, view=view, flat=flat, stride=stride).tolist() == [1] * S
    for sites in rounds:
        C.flip_sites(case, torch, view, sites)
        want = np.ones(S, np.uint8)
        want[[s for s, *_ in sites]] = 0
        got = run(ecx, torch, case, view=view, flat=flat, stride=stride)
        assert got.tolist() == want.tolist(), [site for site in sites if got[site[0]] != 0][:4]
        C.flip_sites(case, torch, view, sites)


@pytest.mark.parametrize("knob,value", [("rtc_xcd", 0), ("xcd_group", 3), ("depth", 4), ("depth", 8)])
def test_block_orders_and_ring_depths_give_the_same_verdicts(ecx, torch_dev, knob, value):
    """The orders and depths the A/B script sweeps (scripts/clay_check_ab.py), on Clay(3,3)."""
    case = C.subchunk_case(3, 3, 0, 4096)
    defaults = {"rtc_xcd": 2, "xcd_group": 0, "xcd_run": 8, "depth": 0}  # csrc/tuning.hpp
    try:
        ecx.tune(knob, value)
        if knob == "xcd_group":
            ecx.tune("xcd_run", 3)
        assert_verdicts(run(ecx, torch_dev, case), case.want, case)
        if knob == "depth":
            assert ecx.last_kernel() == "k_clay_check<false, %d, 4>" % value
        else:
            assert ecx.last_kernel() == "k_clay_check<false, 2, 4>"
    finally:
        for key, val in defaults.items():
            ecx.tune(key, val)


# ---------------------------------------------------------------- Clay(12,4)
def test_clay_12_4_unshortened(ecx, torch_dev):
    case = C.clay124_case()
    got = run(ecx, torch_dev, case)
    assert got.tolist() == case.want.tolist() == [0, 0, 0, 1]


# ---------------------------------------------------------------- the rules that need a device
def test_buf_size_zero_passes_every_stripe_and_refused_geometries_touch_nothing(ecx, torch_dev):
    torch = torch_dev
    pool = torch.zeros(48 * 64, dtype=torch.uint8, device="cuda")
    verdict = torch.full((3 + 16,), GUARD, dtype=torch.uint8, device="cuda")
    ecx.ClayParityCheck(4, 2).isParityCorrectBatch(pool, 0, 0, 3, 0, verdict)
    torch.cuda.synchronize()
    assert verdict.cpu().tolist() == [1] * 3 + [GUARD] * 16
    verdict.fill_(GUARD)
    with pytest.raises(ecx.EcxError) as e:
        ecx.ClayParityCheck(9, 9).isParityCorrectBatch(pool, 0, 0, 3, 0, verdict)
    assert e.value.code == -1 and "parity_units" in str(e.value)
    torch.cuda.synchronize()
    assert (verdict.cpu().numpy() == GUARD).all()
