"""The unit orders of the kernels that write: logical_block and unit_of (csrc/apply.hpp) decide
which (stripe, chunk, tile) a workgroup of k_gf_apply computes, and a mapping that is no bijection
leaves stale bytes in the output.  tests/native/unit_order_check.cpp walks the arithmetic on the
CPU; here k_gf_apply itself runs under every order knob -- xcd_group 1 and 2 (multi-tile maps),
xcd_group 3 with runs of 1, 3 and 8, chunk_major, the staggers, and xcd_group 3 with a stagger --
over one, two and three tiles, overwriting and accumulating, on grids that take the remainder
branches of both functions, and every byte of the output buffer is compared with
conftest.gf_apply_numpy over every stripe.  (k_gf_apply_wide and k_gf_apply_skew never call
logical_block, whatever xcd_group their launch shape reports -- DESIGN.md section 4 -- so they are
kept out: wide_tiles, skew_chunks and map_planes are 0 throughout.)"""
import pytest

import instance_cases as IC

pytestmark = pytest.mark.gpu

S = 13
CHUNK = 4096
L = 5 * CHUNK + 1040            # five full chunks and a 16-B-multiple tail
PITCHES = (169 * 128, L + 16)   # a multiple of 128 B, and one that is none
BASE = "wide_tiles=0,skew_chunks=0,map_planes=0"
# (map, tiles, in place)
MAPS = (("rs173_enc", 1, 1), ("rs1010_enc", 2, 0), ("rand24x12", 3, 0))
ORDERS = ({"xcd_group": 1}, {"xcd_group": 2},
          {"xcd_group": 3, "xcd_run": 1}, {"xcd_group": 3, "xcd_run": 3}, {"xcd_group": 3, "xcd_run": 8},
          {"chunk_major": 1}, {"stagger": 3}, {"stagger": 8}, {"xcd_group": 3, "stagger": 3})
CASES = [(name, T, ip, order) for name, T, ip in MAPS for order in ORDERS
         if T > 1 or order.get("xcd_group", 0) not in (1, 2)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def wants():
    """The expectation of a (map, pitch, mode): computed by the first order that needs it."""
    return {}


def order_id(order):
    return "-".join("%s%d" % (k, v) for k, v in order.items())


@pytest.mark.parametrize("acc", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("name,T,ip,order", CASES, ids=["%s-%s" % (c[0], order_id(c[3])) for c in CASES])
def test_order_against_reference(ecx, torch_dev, wants, name, T, ip, order, pitch, acc):
    gmap = IC.maps(ecx)[name]
    assert T == -(-gmap.info()["n_out"] // 8)
    tu = dict({"xcd_group": 0, "xcd_run": 8, "stagger": 0, "chunk_major": 0}, **order)
    # the order the rules pass to the kernel (csrc/launch_rules.cpp): single-tile maps run 0 or 3,
    # and 3 on their own when a slot pitch is no multiple of 128 B
    xcd = tu["xcd_group"] if T > 1 or tu["xcd_group"] == 3 else (3 if pitch % 128 else 0)
    want_order = "stagger=%d xcd_group=%d xcd_run=%d" % (tu["stagger"], xcd, tu["xcd_run"] if xcd == 3 else 0)
    IC.set_knobs(ecx, BASE + "".join(",%s=%d" % kv for kv in order.items()))
    try:
        plan = IC.plan_of(gmap, L, pitch, ip, acc, S)
        # the grid of the launch of record: the five full chunks, and the tail where it is fused
        family = plan.split("<")[0]
        assert family in ("k_gf_apply", "k_gf_apply_tail"), plan
        assert plan.endswith(want_order), (plan, want_order)
        grid = S * (L // CHUNK + (family == "k_gf_apply_tail")) * T
        if xcd == 1:
            assert grid % 8, grid                       # XCDs with q + 1 and with q blocks
        if xcd in (2, 3):
            R = T * (tu["xcd_run"] if xcd == 3 else 1)
            assert grid > 8 * R and grid % (8 * R), (grid, R)  # full > 0, and the identity remainder behind it
        if tu["stagger"] > 1:
            assert S > tu["stagger"] and S % tu["stagger"], (S, tu["stagger"])  # whole groups, and stripes past them
        got_plan, got, want = IC.run_case(ecx, torch_dev, gmap, L, pitch, ip, acc, S, 1300 + T, wants)
        shape = ecx.last_launch_shape()
    finally:
        IC.set_knobs(ecx, "")
    assert shape == got_plan == plan, (shape, got_plan, plan)
    assert not IC.first_difference(got, want), (name, order, pitch, acc, shape, IC.first_difference(got, want))
