"""Every reachable instance of the composed-map kernels -- k_gf_apply, k_gf_apply_tail,
k_gf_apply_wide, k_gf_apply_skew, k_map_planes -- executed on the device and held against a
reference.  include/ecx_tune.h promises that results are bit-identical for every knob setting; the
cover of tests/instance_cases.py (one case per instance the launch rules can ask for, checked to be
a cover by tests/test_instance_cover_cpu.py) runs each instance once, under the knobs that reach
it, over three stripes, and compares every byte of the output buffer -- rows, gaps between rows,
unused slots and the guards around it -- with conftest.gf_apply_numpy over the library's dense
matrix (tied to the oracle in tests/test_planner.py)."""
import pytest

import instance_cases as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_cover_is_not_empty():
    assert len(IC.COVER) >= IC.N_REACHABLE


@pytest.mark.parametrize("inst,name,n,p,ip,acc,k", IC.COVER, ids=[c[0].replace(" ", "") for c in IC.COVER])
def test_instance_against_reference(ecx, torch_dev, inst, name, n, p, ip, acc, k):
    gmap = IC.maps(ecx)[name]
    IC.set_knobs(ecx, k)
    try:
        plan, got, want = IC.run_case(ecx, torch_dev, gmap, n, p, ip, acc, IC.S_COVER, 4200 + n)
        shape = ecx.last_launch_shape()
    finally:
        IC.set_knobs(ecx, "")
    assert shape == plan, (shape, plan)  # the rules asked without a device name what ran
    assert shape == inst or shape.startswith(inst + " "), (shape, inst)
    assert not IC.first_difference(got, want), (inst, name, n, p, ip, acc, k, IC.first_difference(got, want))
