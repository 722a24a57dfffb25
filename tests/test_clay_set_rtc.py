"""The generated set kernel k_clay_repair_set (clay_rtc.cpp clay_set_source) on the GPU: one
performCodingBatchMixed over a batch of Clay(10,4) (v = 2) or Clay(12,4) stripes that lost different
nodes.  9 stripes of 4 KiB sub-chunks are one full period of the rtc_xcd block maps plus a
remainder.  Every comparison is of the whole output allocation, byte for byte, with a buffer built
from the oracle alone (clay_set_rtc_cases.expected_output): the repaired stripes, the stripes whose
id has no list or the empty list, the guard bytes and the gaps between padded slots."""
import numpy as np
import pytest

import clay_rtc_sweep_cases as C
import clay_set_rtc_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# one set per geometry for the module: its kernel is compiled once per source
@pytest.fixture(scope="module")
def set104(ecx):
    with ecx.ClayPatternSet([list(x) for x in T.LISTS104], 10, 4, 2) as ps:
        yield ps


@pytest.fixture(scope="module")
def set124(ecx):
    with ecx.ClayPatternSet([list(x) for x in T.LISTS124], 12, 4) as ps:
        yield ps


@pytest.fixture(scope="module")
def set_layout(ecx):
    with ecx.ClayPatternSet([list(x) for x in T.LISTS_LAYOUT], 10, 4, 2) as ps:
        yield ps


def _uniform_stripes(ecx, torch, k, m, v, lists, ids, lay, seed):
    """{stripe: alpha x B array}: every repaired stripe through a uniform performCodingBatch of its node."""
    a = C.alpha_of(k, m, v)
    inp = T.device_input(ecx, torch, k, m, v, lay, seed, len(ids))
    got = {}
    for e in sorted({lists[i][0] for i in ids if i < len(lists) and lists[i]}):
        out = torch.zeros((len(ids), a, lay.B), dtype=torch.uint8, device="cuda")
        ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v).performCodingBatch(
            inp[C.GUARD + lay.in_off:], lay.in_stripe, lay.in_sub, out, a * lay.B, lay.B, len(ids), lay.B)
        torch.cuda.synchronize()
        assert ecx.last_kernel() == "k_clay_repair_grp"
        host = out.cpu().numpy()
        for s, i in enumerate(ids):
            if i < len(lists) and lists[i] == (e,):
                got[s] = host[s]
    return got


def _against_oracle_and_uniform(ecx, torch, ps, k, m, v, lists, ids, seed):
    assert ps.generated
    lay = T.layout(k, m, v)
    want = T.expected_output(k, m, v, lists, ids, lay, seed)
    got, kern = T.run_mixed(ecx, torch, ps, k, m, v, ids, lay, seed)
    assert kern == "k_clay_repair_set", kern
    T.assert_same(got, want, lay, (k, m, v, ids))
    a = C.alpha_of(k, m, v)
    uniform = _uniform_stripes(ecx, torch, k, m, v, lists, ids, lay, seed)
    assert sorted(uniform) == [s for s, i in enumerate(ids) if i < len(lists) and lists[i]]
    for s, sub in uniform.items():
        mine = got[C.GUARD + s * lay.out_stripe:C.GUARD + (s + 1) * lay.out_stripe].reshape(a, lay.B)
        assert np.array_equal(mine, sub), f"stripe {s} differs from the uniform repair of its node"


def test_clay_10_4_mixed_vs_oracle_and_uniform(ecx, torch_dev, set104):
    """One node per erased row, the empty list and a duplicate; neighbouring stripes differ, id 255
    and the empty list fall inside the full period of the block map, a repaired stripe in the
    remainder."""
    _against_oracle_and_uniform(ecx, torch_dev, set104, 10, 4, 2, T.LISTS104, T.IDS104, 8100)


def test_clay_12_4_mixed_vs_oracle_and_uniform(ecx, torch_dev, set124):
    _against_oracle_and_uniform(ecx, torch_dev, set124, 12, 4, 0, T.LISTS124, T.IDS124, 8200)


LAYOUTS = {
    "padded": (dict(in_pad=64, out_pad=64), {}),       # both slot pitches B + 64
    "offset16": (dict(in_off=16, out_off=16), {}),     # both bases 16 bytes into their allocations
    "two_chunks": (dict(B=8192), {}),
    "xcd0": ({}, {"rtc_xcd": 0}),
    "xcd3": ({}, {"rtc_xcd": 3}),
    "sched0": ({}, {"rtc_sched": 0}),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts_and_shapes_vs_oracle(ecx, torch_dev, set_layout, name):
    lay_kw, kn = LAYOUTS[name]
    lay = T.layout(10, 4, 2, **lay_kw)
    want = T.expected_output(10, 4, 2, T.LISTS_LAYOUT, T.IDS_LAYOUT, lay, 8300)
    with C.knobs(ecx, **kn):
        got, kern = T.run_mixed(ecx, torch_dev, set_layout, 10, 4, 2, T.IDS_LAYOUT, lay, 8300)
    assert kern == "k_clay_repair_set", kern
    T.assert_same(got, want, lay, name)


def test_wide_form_for_slot_offsets_past_31_bits(ecx, torch_dev, set_layout):
    """in_sub_stride 1 MiB (Clay(10,4)'s other sub-chunk size) with buf_size 4096: the last slots of
    a stripe lie 3.5 GiB past its base, beyond a buffer resource's 31-bit offsets, so the launch
    takes the 64-bit-address form (the 32-bit form would read such slots as zeros).  Two stripes,
    two lists; only the bytes the batch reads are filled."""
    torch = torch_dev
    k, m, v, a = 10, 4, 2, 256
    n_in, sub, nst = 14 * a, 1 << 20, 2
    with C.knobs(ecx, rtc_wide=1):
        assert "const long long vz" in set_layout.rtcSource()  # the source such a launch uses
    assert "const long long vz" not in set_layout.rtcSource()
    src = torch.empty((nst, n_in, T.B), dtype=torch.uint8, device="cuda")
    ecx.fill_random(src, src.numel(), 8400)
    inp = torch.empty(nst * n_in * sub, dtype=torch.uint8, device="cuda")
    inp.view(nst, n_in, sub)[:, :, :T.B] = src
    lay = T.layout(k, m, v)
    out = torch.full((C.GUARD + T.out_bytes(lay, nst) + C.GUARD,), C.SENTINEL, dtype=torch.uint8, device="cuda")
    ids = (1, 0)
    set_layout.performCodingBatchMixed(inp, n_in * sub, sub, out[C.GUARD:len(out) - C.GUARD], lay.out_stripe, lay.out_sub,
                                       torch.tensor(ids, dtype=torch.uint8, device="cuda"), nst, T.B)
    torch.cuda.synchronize()
    assert ecx.last_kernel() == "k_clay_repair_set"
    del inp
    host, got = src.cpu().numpy(), out.cpu().numpy()
    want = np.full(got.size, C.SENTINEL, np.uint8)
    for s, i in enumerate(ids):
        ref = T.oracle_stripe(k, m, v, T.LISTS_LAYOUT[i][0], [host[s, j].copy() for j in range(n_in)], T.B)
        for z in range(a):
            at = C.GUARD + s * lay.out_stripe + z * lay.out_sub
            want[at:at + T.B] = ref[z]
    T.assert_same(got, want, lay, "wide")


def test_resources_fit_three_waves_per_simd_without_scratch(ecx, torch_dev, set104):
    """The bodies are inlined into the switch: the kernel needs no scratch, at most the registers
    that rtc_waves 3 leaves a wave (512 per SIMD lane / 3, in granules of 8), and the one 32 KiB
    exchange buffer."""
    res = set104.rtcResources()
    assert res["scratch_bytes"] == 0, res
    assert 0 < res["vgprs"] <= 512 // 3 // 8 * 8, res
    assert res["lds_bytes"] == 4 * 4 * 2 * 64 * 16, res
    assert res["code_bytes"] > 0, res
