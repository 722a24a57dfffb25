"""Generated Clay pattern sets on the host: sets whose lists are single nodes of a geometry with
more than 64 rows per node (Clay(12,4), the shortened Clay(10,4)) and run on the generated kernel
k_clay_repair_set (clay_rtc.cpp).  Everything decided before the first HIP call runs without a
device: what the create accepts and still refuses, info(), the generated source and its hiprtc
compile for gfx950, the status codes of the batch calls and their order, the refusal of the
partial-sum hop, the plan of the host form and the JNI forwarders.  The repair itself is
tests/test_clay_set_rtc.py.

The uniform kernels' sources are pinned by hash: the set kernel was cut out of clay_grp_source, and
the single-program output of that generator must stay byte for byte what it was.  The constants
were taken from a library built from the parent commit's tree (an export of it built on its own,
next to the working tree): sha256 of ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v)
.rtcSource() at the default knobs."""
import ctypes
import hashlib
import re

import numpy as np
import pytest

OK, ILL, NULL = 0, -1, -6
B = 4096
LISTS104 = [[e] for e in range(14)] + [[]]
LISTS124 = [[e] for e in range(16)]
FOUR = [[2], [5], [8], [13], [], [2]]  # one node per erased row, the empty list and a duplicate

UNIFORM_SOURCE_SHA256 = {
    (10, 4, 2, 2): "923f212e7cf6e72fb97f2f2d5319ea8fba5365c519e6818fafce7d780225bec7",
    (10, 4, 2, 5): "7aad079307f83009519f53f1ed4a9c101e8d2f1cd7d34858358962ed07694f3c",
    (10, 4, 2, 8): "475ac579d4fb33cbcf2d0db6d1ab82644878d44667bfdc058d3c168536c51980",
    (10, 4, 2, 13): "c0e905a08555221f9df2a6bfc213b4f0ea9413a28221f150cc76692aebc94ecd",
    (12, 4, 0, 3): "482718928afebe493330d30cd1083b3f2a3348203519353de1c597dfaeda5ecd",
    (6, 4, 2, 5): "f3e0fd9e5b1a2c383ce4339ac5870d898c41e905ca8adc112f627e9b666b3926",
    (4, 2, 0, 1): "d904d73ce36c6afea73e89574000389cb617d1dab9388eaa42f614219e1d879a",
}


def _create(lib, k, m, v, lists):
    flat = np.ascontiguousarray([e for lst in lists for e in lst] + [0], np.int32)
    counts = np.ascontiguousarray([len(lst) for lst in lists] + [0], np.int32)
    h = ctypes.c_void_p()
    st = lib.ecx_clay_pattern_set_create(k, m, v, flat.ctypes.data, counts.ctypes.data, len(lists), ctypes.byref(h))
    return st, h


def _clay_live(lib):
    v = [ctypes.c_int() for _ in range(4)]
    assert lib.ecx_codec_stats(*[ctypes.byref(x) for x in v]) == OK
    return v[2].value


@pytest.fixture(scope="module")
def full104(ecx):
    with ecx.ClayPatternSet(LISTS104, 10, 4, 2) as ps:
        yield ps


def test_create_accepts_every_single_node_list(ecx, full104):
    """All 14 single-node lists of Clay(10,4) (v = 2) plus the empty list, and all 16 of Clay(12,4):
    each has a 256-row map, which the composed plan refuses."""
    assert full104.info() == (15, 14, 256, 1) and full104.generated
    assert (full104.numTotalUnits, full104.subPacketSize, full104.maxErased) == (14, 256, 1)
    with ecx.ClayPatternSet(LISTS124, 12, 4) as ps:
        assert ps.info() == (16, 16, 256, 1) and ps.generated
    # a set of short maps is what it was: composed, and without a generated source
    with ecx.ClayPatternSet([[1], [0, 3], []], 4, 2) as ps:
        assert not ps.generated and ps.info() == (3, 6, 8, 2)
        with pytest.raises(ecx.EcxError) as err:
            ps.rtcSource()
        assert err.value.code == ILL
    # nothing but empty lists: no kernel to generate, a composed set that does nothing
    with ecx.ClayPatternSet([[], []], 10, 4, 2) as ps:
        assert not ps.generated and ps.info() == (2, 14, 256, 0)


def test_set_holds_one_codec_reference_per_distinct_list(ecx):
    lib = ecx.lib()
    before = _clay_live(lib)
    # (virtualUnits 1 of Clay(11,4): a geometry no other test's sets hold)
    with ecx.ClayPatternSet([[0], [7], [0], [], [14]], 11, 4, 1) as ps:
        assert _clay_live(lib) == before + 4  # {0}, {7}, {}, {14}
        assert ps.info() == (5, 15, 256, 1) and ps.generated
    assert _clay_live(lib) == before


def test_create_still_refuses_and_drops_its_references(ecx):
    lib = ecx.lib()
    before = _clay_live(lib)
    # two nodes of Clay(10,4): 512 rows, no generated body for it
    st, h = _create(lib, 10, 4, 2, [[3], [0, 1]])
    msg = lib.ecx_last_error().decode()
    assert st == ILL and not h.value
    assert "list 1" in msg and "{0,1}" in msg and "512 rows" in msg and "ecx_clay_perform_coding_batch" in msg, msg
    assert _clay_live(lib) == before
    # a single node of Clay(9,3): 81 rows, and q = 3 has no plane-group kernel
    st, h = _create(lib, 9, 3, 0, [[4]])
    msg = lib.ecx_last_error().decode()
    assert st == ILL and not h.value
    assert "list 0" in msg and "{4}" in msg and "81 rows" in msg and "q = 4" in msg, msg
    assert "ecx_clay_perform_coding_batch" in msg, msg
    assert _clay_live(lib) == before
    # an out-of-range node among generated lists: the step's own refusal, references dropped
    st, h = _create(lib, 10, 4, 2, [[3], [14]])
    assert st < 0 and not h.value and _clay_live(lib) == before


def test_set_source_and_compile(ecx):
    """The 4-list set's source: its lists in the first line, the one kernel, the one LDS buffer, a
    body per distinct list with the ids of duplicates sharing one, and no case for the empty list;
    it compiles for gfx950 through hiprtc."""
    with ecx.ClayPatternSet(FOUR, 10, 4, 2) as ps:
        src = ps.rtcSource()
        first = src.split("\n", 1)[0]
        assert first.startswith("// k_clay_repair_set:") and "4 bodies" in first, first
        assert re.findall(r"\{(\d+)\}", first) == ["2", "5", "8", "13"], first
        assert src.count("k_clay_repair_set(") == 1 and "k_clay_repair_grp(" not in src
        assert src.count("__shared__") == 1
        assert len(re.findall(r"^    \{  // body \d+: list", src, flags=re.M)) == 4
        cases = [int(c) for c in re.findall(r"^    case (\d+):$", src, flags=re.M)]
        assert sorted(cases) == [0, 1, 2, 3, 5], cases       # id 4 is the empty list: the default
        assert src.index("case 0:") < src.index("case 5:") < src.index("// body 0:") < src.index("case 1:")
        # the id is read wave-uniform, and nothing is loaded from `in` or stored before the switch
        head = src[src.index("k_clay_repair_set("):src.index("switch (id)")]
        assert "__builtin_amdgcn_readfirstlane((int)ids[s])" in head
        assert not re.search(r"\b(ldv0|ldv2|st)\(", head.replace("auto st = [&](", "")), head[-400:]
        assert "const long long vz" not in src   # 4 KiB sub-chunks: buffer loads, not the 64-bit form
        size = ps.rtcCompileCheck()
        assert size > 0
    # the shape knobs of the diagnostic library are refused by name
    with ecx.ClayPatternSet([[2], [5]], 10, 4, 2) as ps:
        for key, val in (("rtc_units", 2), ("rtc_persist", 2)):
            try:
                ecx.tune(key, val)
            except ecx.EcxError:
                continue  # the product library does not know the knob at all
            try:
                with pytest.raises(ecx.EcxError) as err:
                    ps.rtcSource()
                assert err.value.code == ILL and key in str(err.value)
            finally:
                ecx.tune(key, 1 if key == "rtc_units" else 0)


@pytest.mark.parametrize("k,m,v,e", list(UNIFORM_SOURCE_SHA256))
def test_uniform_source_unchanged(ecx, k, m, v, e):
    src = ecx.ClayCodeErasureDecodingStep([e], k, m, virtualUnits=v).rtcSource()
    assert hashlib.sha256(src.encode()).hexdigest() == UNIFORM_SOURCE_SHA256[(k, m, v, e)]


@pytest.mark.parametrize("fn", ["ecx_clay_perform_coding_batch_mixed", "ecx_clay_perform_coding_mixed_batch_host"])
def test_batch_status_codes_and_their_order(ecx, full104, fn):
    """The order of tests/test_clay_mixed_cpu.py first, then the layout rule of a generated set --
    whole 4 KiB chunks, and on the device 16-byte-aligned bases and strides -- each refusal naming
    the offending value, all before any device work (no call here gets past its checks)."""
    lib = ecx.lib()
    f = getattr(lib, fn)
    host = fn.endswith("_host")
    mem = np.zeros(256, np.uint8)
    p = (mem.ctypes.data + 15) // 16 * 16
    n_in, n_out = 14 * 256, 256

    def call(h, ids=p, inp=p, iss=n_in * B, isl=B, out=p, oss=n_out * B, osl=B, S=1, buf=B):
        args = [h, ids, inp, iss, isl, out, oss, osl, S, buf]
        return f(*args) if host else f(*(args + [None]))

    h = full104._h
    assert call(None, S=-1, ids=None) == NULL
    assert call(h, S=-1, ids=None) == ILL and call(h, buf=-1, inp=None) == ILL
    # nstripes == 0 needs no buffers, and no layout either
    assert call(h, S=0, ids=None, inp=None, out=None, iss=-1, buf=4097) == OK
    assert call(h, buf=0, ids=None, inp=None, out=None, osl=-1) == OK
    assert call(h, ids=None, iss=-1, buf=4097) == NULL and call(h, inp=None, buf=2048) == NULL
    assert call(h, out=None, oss=-1) == NULL
    for kw in ({"iss": -1}, {"isl": -1}, {"oss": -1}, {"osl": -1}):
        assert call(h, buf=4097, **kw) == ILL and "negative stride" in lib.ecx_last_error().decode(), kw
    assert call(h, S=4, iss=1 << 62, buf=4097) == ILL and "overflows" in lib.ecx_last_error().decode()
    # the layout rule, after all of the above
    for bad in (4097, 2048):
        assert call(h, buf=bad) == ILL
        msg = lib.ecx_last_error().decode()
        assert "4096" in msg and str(bad) in msg, msg
    if not host:  # the host form stages every slot in its own aligned buffers
        for kw in ({"isl": 4104}, {"iss": n_in * 4104 + 8}, {"osl": 4104}, {"oss": n_out * B + 8}):
            assert call(h, **kw) == ILL, kw
            msg = lib.ecx_last_error().decode()
            name = {"isl": "in_sub_stride", "iss": "in_stripe_stride", "osl": "out_sub_stride",
                    "oss": "out_stripe_stride"}[next(iter(kw))]
            assert "16" in msg and name in msg and str(next(iter(kw.values()))) in msg, msg
        for kw in ({"inp": p + 1}, {"out": p + 8}):
            assert call(h, **kw) == ILL, kw
            msg = lib.ecx_last_error().decode()
            assert "16" in msg and str(next(iter(kw.values()))) in msg, msg
    assert (mem == 0).all()


def test_partial_hop_and_chain_refuse_a_generated_set_by_name(ecx, full104):
    lib = ecx.lib()
    st = lib.ecx_clay_partial_batch_mixed(full104._h, None, None, None, 0, 0, 0, None, 0, 0, 5, B, 1, None)
    msg = lib.ecx_last_error().decode()
    assert st == ILL and "generated pattern set" in msg and "k_clay_repair_set" in msg, msg
    with pytest.raises(ecx.EcxError) as err:
        full104.partialBatchMixed(None, None, None, 0, 0, 0, None, 0, 0, 0, 0, True)
    assert err.value.code == ILL and "generated pattern set" in str(err.value)
    from repair_pipelining_amd.chain import ClayPatternChain
    with pytest.raises(ecx.EcxError) as err2:
        ClayPatternChain(full104, order=[0], rank=0)
    assert str(err2.value) == str(err.value)


def test_host_plan_of_the_full_clay_10_4_set(ecx, full104):
    """The 14 single-node lists together read every sub-chunk of a stripe: 3,584 slots go up, and
    slots 0..255 come back."""
    plan = full104.host_plan(14 * 256 * B, B, 256 * B, B, 6, B)
    assert (plan["slots_up"], plan["slots_down"]) == (3584, 256), plan
    assert plan["chunk"] * plan["chunks"] >= 6 and plan["buffers"] >= 1
    # one list reads its 64 helper planes of the 13 other nodes
    with ecx.ClayPatternSet([[5]], 10, 4, 2) as ps:
        plan = ps.host_plan(14 * 256 * B, B, 256 * B, B, 6, B)
        assert (plan["slots_up"], plan["slots_down"]) == (13 * 64, 256), plan
        assert plan["slots_up"] == ecx.ClayCodeErasureDecodingStep([5], 10, 4, virtualUnits=2).map().info()["n_in"]
    zero = dict.fromkeys(("slots_up", "slots_down", "chunk", "chunks", "buffers", "h2d_copies", "d2h_copies"), 0)
    assert full104.host_plan(14 * 256 * B, B, 256 * B, B, 0, B) == zero


def test_jni_forwarders_over_a_generated_set():
    """The generated forwarders (jni/ecx_jni.c) over the fake JNIEnv: the create reads its two int[]
    without pinning them, info and the host plan report n * alpha = 3,584 input slots and 256 output
    slots, and the batch forwarders' own refusals and the export's layout rule come through."""
    from jni_harness import Jni
    J = Jni()
    try:
        J.reset()
        flat = np.array([e for lst in LISTS104 for e in lst], np.int32)
        cnt = np.array([len(lst) for lst in LISTS104], np.int32)
        hh = np.zeros(1, np.int64)
        assert J.call("clayPatternSetCreate", 10, 4, 2, J.array(flat), J.array(cnt), len(LISTS104), J.array(hh)) == OK
        h = int(hh[0])
        assert h != 0 and J.counters()["pins"] == 0
        n, nodes, alpha, erased = (np.zeros(1, np.int32) for _ in range(4))
        assert J.call("clayPatternSetInfo", h, J.array(n), J.array(nodes), J.array(alpha), J.array(erased)) == OK
        assert (n[0], nodes[0], alpha[0], erased[0]) == (15, 14, 256, 1)
        plan = np.zeros(7, np.int64)
        assert J.call("clayPatternSetHostPlan", h, 3584 * B, B, 256 * B, B, 5, B, J.array(plan)) == OK
        assert (plan[0], plan[1]) == (int(nodes[0]) * int(alpha[0]), 256) and plan[0] == 3584
        assert J.call("clayPatternSetHostPlan", h, 3584 * B, B, 256 * B, B, 5, B, J.array(plan[:6].copy())) == -5
        args = (16, 4096, 3584 * B, B, 8192, 256 * B, B)
        assert J.call("clayPerformCodingBatchMixed", 0, *args, 1, B, 0) == NULL
        assert J.call("clayPerformCodingBatchMixed", h, *args, -1, B, 0) == ILL
        assert J.call("clayPerformCodingBatchMixed", h, 0, *args[1:], 1, B, 0) == NULL
        assert J.call("clayPerformCodingBatchMixed", h, *args, 0, B, 0) == OK          # empty batch
        assert J.call("clayPerformCodingBatchMixed", h, *args, 1, 4097, 0) == ILL      # no kernel takes a tail
        assert J.call("clayPerformCodingBatchMixed", h, *args[:3], 4104, *args[4:], 1, B, 0) == ILL
        assert J.call("clayPerformCodingMixedBatchHost", h, *args, 1, 2048) == ILL
        assert J.call("clayPerformCodingMixedBatchHost", h, *args, 0, B) == OK
        # two nodes of this geometry are refused through the forwarder as through the export
        two = np.zeros(1, np.int64)
        assert J.call("clayPatternSetCreate", 10, 4, 2, J.array(np.array([0, 1], np.int32)),
                      J.array(np.array([2], np.int32)), 1, J.array(two)) == ILL and two[0] == 0
        J.call("clayPatternSetDestroy", h)
        c = J.counters()
        assert c["pins_now"] == 0 and c["violations"] == 0 and c["calls_while_pinned"] == 0, c
    finally:
        J.free_all()
