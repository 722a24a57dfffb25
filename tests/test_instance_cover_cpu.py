"""The instance cover of tests/test_instance_cover.py, checked without a device: the enumeration of
tests/instance_cases.py (GfMap.launch_plan over maps x layouts x modes x knob settings) finds every
kernel instance ever recorded on a device and no fewer than it did when the cover was written, and
the literal cover reaches each of them."""
import pytest

import instance_cases as IC

GOLDEN = IC.ROOT / "tests" / "golden" / "launch_shapes.jsonl.gz"


@pytest.fixture(scope="module")
def found(ecx):
    return IC.reachable(ecx)


def test_enumeration_holds_every_recorded_instance(ecx, found):
    """Every product-library instance of tests/golden/launch_shapes.jsonl.gz (recorded on an MI355X,
    one knob at a time) is reachable: nothing recorded on a device is lost from the enumeration."""
    lines = IC.recorder().read_lines(GOLDEN)
    golden = {IC.instance_of(r["shape"]) for r in lines if r["diag"] == 0 and r["shape"]}
    assert len(golden) == 46
    assert not golden - set(found), sorted(golden - set(found))


def test_enumeration_finds_no_fewer_instances(ecx, found):
    """62 instances when the cover was written: a rule change that makes one unreachable fails here,
    one that makes a new one reachable fails test_cover_reaches_every_instance until the cover has it."""
    assert IC.N_REACHABLE == 62
    print("reachable instances: %d over %d knob settings" % (len(found), len(IC.knob_settings())))
    assert len(found) >= IC.N_REACHABLE, sorted(found)


def test_cover_reaches_every_instance(ecx, found):
    """The literal list is a cover of reachable(), sorted by instance name with one case each, every
    case one of the grid's (so it can run: a defined in-place, at most 256 MiB), and it is what
    cover() chooses."""
    names = [c[0] for c in IC.COVER]
    assert names == sorted(set(names))
    assert not set(found) - set(names), sorted(set(found) - set(names))
    for c in IC.COVER:
        assert c[1:] in set(found[c[0]]), c
    assert IC.COVER == IC.cover(ecx, found)


def test_cover_entries_plan_their_instance(ecx):
    """Each entry's launch_plan string, asked under its knobs alone, names its instance; no case
    allocates more than 256 MiB and only the instances that need one run at a 4 MiB pitch."""
    mp = IC.maps(ecx)
    try:
        for inst, name, n, p, ip, acc, k in IC.COVER:
            IC.set_knobs(ecx, k)
            plan = IC.plan_of(mp[name], n, p, ip, acc)
            assert plan.startswith(inst + " ") or plan == inst, (inst, plan)
            assert IC.case_bytes(mp[name], n, p, ip) <= IC.MAX_CASE_BYTES
    finally:
        IC.set_knobs(ecx, "")
    assert not [c for c in IC.COVER if c[3] == "4m"]
