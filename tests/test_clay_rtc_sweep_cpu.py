"""The case table of the generated Clay repair kernel sweep (tests/clay_rtc_sweep_cases.py), checked
without a device: every (code, node) source compiles with hiprtc for gfx950, and the table still
holds the arrangements the sweep exists for."""
import pytest

import clay_rtc_sweep_cases as C


def source_of(ecx, k, m, v, e):
    return ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v).rtcSource()


@pytest.mark.parametrize("k,m,v", C.CODES)
def test_every_node_source_compiles(ecx, k, m, v):
    """Part a's table: the kernel generated for every real node of the code is the one
    clay_grp_supported implies and compiles."""
    name = "k_clay_repair_grp(" if C.is_grp(k, m, v) else "k_clay_repair("
    for e in range(k + m):
        step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
        assert step.subPacketSize == C.alpha_of(k, m, v)
        assert name in step.rtcSource(), (k, m, v, e)
        assert step.rtcCompileCheck() > 0, (k, m, v, e)


def test_table_lists_every_real_node_once():
    assert len(C.NODE_CASES) == len(set(C.NODE_CASES)) == sum(k + m for k, m, _ in C.CODES)
    assert len(C.CODES) == len(set(C.CODES)) == 17
    for k, m, v, e in C.KNOB_NODES + C.LAYOUT_NODES:
        assert (k, m, v, e) in C.NODE_CASES and C.is_grp(k, m, v)


def test_table_keeps_the_new_arrangements(ecx):
    """The arrangements no earlier test ran stay in the table: lane rows above the LDS row
    (ya > yb), no row from memory, every erased row of Clay(10,4) v=2 (row 1: ya=0, yb=3; row 2:
    node 8, whose row mates are virtual), a virtual node in an on-chip exchange row."""
    seen = {}
    for k, m, v, e in C.NODE_CASES:
        if C.is_grp(k, m, v):
            seen[(k, m, v, e)] = C.arrangement(source_of(ecx, k, m, v, e))
    arrs = set(seen.values())
    assert any(a.ya > a.yb for a in arrs)
    assert any(a.mem_rows == 0 for a in arrs) and any(a.mem_rows == 1 for a in arrs)
    assert any(a.ya > a.yb and a.mem_rows == 0 for a in arrs)  # t = 3, shortened
    assert any(a.ya > a.yb and a.mem_rows == 1 for a in arrs)  # t = 4, deep shortening
    assert {a.ey for c, a in seen.items() if c[:3] == (10, 4, 2)} == {0, 1, 2, 3}
    assert seen[(10, 4, 2, 5)][:2] == (0, 3)
    assert seen[(10, 4, 2, 8)].ex == 0 and seen[(10, 4, 2, 8)].ey == 2
    # t = 4 codes run 4 plane groups per slice, t = 3 codes one: with 9 stripes both sides of
    # the block maps' 8 * 8 * G period
    assert {a.groups for a in arrs} == {1, 4}

    def virtual_rows(k, m, v):
        return {u // m for u in range(k, k + v)}
    on_chip_virtual = [c for c, a in seen.items() if {a.ya, a.yb} & virtual_rows(*c[:3])]
    assert {c[:3] for c in on_chip_virtual} >= {(7, 4, 1), (6, 4, 2), (5, 4, 3), (6, 4, 6), (3, 4, 9)}
    # Clay(3,4) v=9, parity row erased: virtual nodes in ya, yb and the memory row at once
    a = seen[(3, 4, 9, 5)]
    assert virtual_rows(3, 4, 9) >= {a.ya, a.yb} and C.memory_row_has_virtual(3, 4, 9, a)


def test_knob_nodes_cover_every_arrangement_of_their_codes(ecx):
    """Part b runs one node per distinct (ya, yb, rows from memory, erased row) of its four codes,
    a row-1 node and node 8 of Clay(10,4) v=2 among them."""
    codes = sorted({c[:3] for c in C.KNOB_NODES})
    assert codes == [(6, 4, 2), (6, 4, 6), (10, 4, 2), (12, 4, 0)]
    cls = lambda a: (a.ya, a.yb, a.mem_rows, a.ey)  # noqa: E731
    for k, m, v in codes:
        every = {cls(C.arrangement(source_of(ecx, k, m, v, e))) for e in range(k + m)}
        picked = [cls(C.arrangement(source_of(ecx, *c))) for c in C.KNOB_NODES if c[:3] == (k, m, v)]
        assert set(picked) == every and len(picked) == len(every), (k, m, v)
    assert (10, 4, 2, 8) in C.KNOB_NODES and (10, 4, 2, 5) in C.KNOB_NODES
    # part c: a data node and a parity node of each of its codes
    for code in {c[:3] for c in C.LAYOUT_NODES}:
        assert sorted(c[3] < code[0] for c in C.LAYOUT_NODES if c[:3] == code) == [False, True]


@pytest.mark.parametrize("k,m,v,e", [(10, 4, 2, 5), (6, 4, 6, 1)])
def test_lean_schedule_refusal_is_an_error(ecx, k, m, v, e):
    """rtc_sched 1 has no second body (rtc_lookahead bit 2) where the memory row holds virtual
    nodes: refused as an EcxError, and only there -- a code with no memory row generates."""
    step = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
    default = step.rtcSource()
    assert C.memory_row_has_virtual(k, m, v, C.arrangement(default))
    with C.knobs(ecx, rtc_sched=1, rtc_lookahead=5):
        with pytest.raises(ecx.EcxError):
            step.rtcSource()
        other = ecx.ClayCodeErasureDecodingStep([3], 6, 4, virtualUnits=2)
        assert not C.memory_row_has_virtual(6, 4, 2, C.arrangement(other.rtcSource()))
    assert step.rtcSource() == default  # the knobs are back at their defaults
