"""Every byte, row and unit the parity checks reduce over ("What the check
tests guarantee").  k_gf_check and k_gf_check_blocked reduce (k + m) * L bytes per stripe to one
verdict byte, so a lane, dword component, row, tile, chunk or unit the reduction drops fails
silently: a corrupt stripe reported clean.  The pools of tests/check_sites.py carry one single-bit
flip per stripe -- every byte of a window, every edge position of every shard, every
(stripe, chunk unit, tile) under every ordering knob -- and the verdict vector must equal the
expected one exactly, which tests/test_check_sites_cpu.py ties to the oracle's isParityCorrect
stripe by stripe (asserted again here before anything runs on the device).  The shards are never
written and the bytes behind the verdicts keep their guard value."""
import numpy as np
import pytest

import check_sites as CS
import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 0xA5
BLOCK = 4096
# (k, m, off, L, pitch, S, block): two tiles; six chunk units on a 16-B pitch that is no 128-B
# multiple (the default runs-per-XCD order) and on a 128-B pitch (the identity order); the blocked form
UNIT_SHAPES = [(10, 10, 0, 2 * 4096 + 48, 2 * 4096 + 48 + 16, 23, 0),
               (4, 2, 0, 5 * 4096 + 1040, 5 * 4096 + 1040 + 16, 37, 0),
               (4, 2, 0, 5 * 4096 + 1040, 169 * 128, 37, 0)]
BLOCKED_UNIT_SHAPE = (4, 2, 0, 5 * 4096 + 1040, 5 * 4096 + 1040, 37, BLOCK)
KNOBS = {"default": {}, "xcd3_run1": {"xcd_group": 3, "xcd_run": 1}, "xcd3_run3": {"xcd_group": 3, "xcd_run": 3},
         "xcd3_run8": {"xcd_group": 3, "xcd_run": 8}, "stagger3": {"stagger": 3}, "stagger8": {"stagger": 8}}
KNOB_DEFAULTS = {"xcd_group": 0, "xcd_run": 8, "stagger": 0, "depth": 0}


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def same(got, want, sites=None):
    """got == want, stripe by stripe; the message names the first stripes that differ and their sites."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero(got != want)[0]
    if len(bad) == 0:
        return True
    by_stripe = {} if sites is None else {CS.stripe_of_site(j): x for j, x in enumerate(sites)}
    raise AssertionError("%d verdicts differ; first: %s" % (
        len(bad), [(int(s), int(got[s]), int(want[s]), by_stripe.get(int(s))) for s in bad[:8]]))


def report(what, k, m, off, L, pitch, nsites, want, got):
    print(f"{what}: RS({k},{m}) L={L} off={off} pitch={pitch} sites={nsites} stripes={len(want)} "
          f"failing wanted={int((np.asarray(want) == 0).sum())} got={int((np.asarray(got) == 0).sum())}")


def batch_verdicts(torch, rs, dpool, n, pitch, S, off, L):
    v = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")
    rs.isParityCorrectBatch(dpool, n * pitch, pitch, S, off, L, v)
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    assert (v[S:] == GUARD).all(), v[S:].tolist()
    return v[:S]


def blocked_verdicts(torch, rs, flat, S, L, block):
    v = torch.full((S + 16,), GUARD, dtype=torch.uint8, device="cuda")
    rs.isParityCorrectBlockedBatch(flat, S, L, v, block)
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    assert (v[S:] == GUARD).all(), v[S:].tolist()
    return v[:S]


def sweep_on_device(ecx, torch, name, what, kernel=None):
    k, m, off, L, pitch, sites, pool, want, orc = CS.sweep_case(name)
    assert (want == orc).all()  # the expectation is the oracle's, before anything runs on the device
    n, S = k + m, pool.shape[0]
    rs = ecx.ReedSolomon.create(k, m)
    dpool = torch.from_numpy(pool.copy()).cuda()
    before = dpool.clone()
    got = batch_verdicts(torch, rs, dpool, n, pitch, S, off, L)
    report(what, k, m, off, L, pitch, len(sites), want, got)
    if kernel:
        assert ecx.last_kernel() == kernel, ecx.last_kernel()
    assert same(got, want, sites)
    assert torch.equal(dpool, before)  # read-only


# ---------------------------------------------------------------- a. byte sweeps, natural layout
@pytest.mark.parametrize("name,kernel", [("byte_fused", "k_gf_check<false, 4, 4>"), ("byte_ragged", "k_gf_check<false, 4, 4>"),
                                         ("byte_head", "k_gf_check<false, 4, 4>"), ("byte_odd", None)])
def test_byte_sweep(ecx, torch_dev, name, kernel):
    """RS(4,2), every byte of the window flipped once, one bit each, plus the bytes just outside it:
    a fused 16-B-multiple tail (the shifted 4 KiB window), a byte-safe tail, a firstByte of 5 on 16-B
    strides (byte-safe head, vector rest) and odd strides (byte-safe only)."""
    sweep_on_device(ecx, torch_dev, name, "byte sweep " + name, kernel)


@pytest.mark.parametrize("depth", [8, 20])
def test_byte_sweep_at_forced_depth(ecx, torch_dev, depth):
    """The fused-tail byte sweep on the 8- and 20-deep load rings (ecx_tune "depth")."""
    ecx.tune("depth", depth)
    try:
        sweep_on_device(ecx, torch_dev, "byte_fused", "byte sweep depth %d" % depth, "k_gf_check<false, %d, 4>" % depth)
    finally:
        ecx.tune("depth", KNOB_DEFAULTS["depth"])


# ---------------------------------------------------------------- b. edge sweeps, natural layout
@pytest.mark.parametrize("name,kernel", [("edge_5_5", "k_gf_check<false, 4, 8>"), ("edge_10_10", "k_gf_check<false, 4, 8>"),
                                         ("edge_17_3", "k_gf_check<false, 4, 4>"), ("edge_64_64_a", "k_gf_check<false, 4, 8>"),
                                         ("edge_64_64_b", "k_gf_check<false, 4, 8>"), ("edge_64_64_c", "k_gf_check<false, 4, 8>"),
                                         ("edge_64_64_d", "k_gf_check<false, 4, 8>")])
def test_edge_sweep(ecx, torch_dev, name, kernel):
    """Every shard crossed with the dword, lane, wave, chunk and shifted-window edges: RS(5,5) (five
    rows in the 8-row instance), RS(10,10) (two tiles, each of the ten parity rows), RS(17,3) (three
    rows in the 4-row instance, fused tail), RS(64,64) (eight tiles; its 128 shards in four pools of
    32, at positions 0, 1024, 4095, 4096 and L - 1)."""
    sweep_on_device(ecx, torch_dev, name, "edge sweep " + name, kernel)


# ---------------------------------------------------------------- c. unit probes, natural layout
def set_knobs(ecx, knobs):
    for key, value in {**KNOB_DEFAULTS, **knobs}.items():
        ecx.tune(key, value)


def device_round(torch, flat, idx, val):
    """XOR a round's flips into (or, a second time, out of) the flat device buffer."""
    if len(idx):
        i = torch.from_numpy(idx).cuda()
        flat[i] = flat[i] ^ torch.from_numpy(val).cuda()


@pytest.mark.parametrize("knobs", sorted(KNOBS))
@pytest.mark.parametrize("k,m,off,L,pitch,S,block", UNIT_SHAPES)
def test_unit_probes(ecx, torch_dev, k, m, off, L, pitch, S, block, knobs):
    """C * T + 1 rounds over S stripes; in each, every stripe but the clean ones carries one flipped
    bit that exactly one (chunk unit, tile) workgroup can see, and over the rounds every unit of
    every stripe is that workgroup once -- so a unit that logical_block or unit_of never visits, or
    visits for the wrong stripe, shows as a wrong verdict.  The grid is no multiple of
    8 * xcd_run * T and S none of the stagger, so the remainder branches of both run too."""
    torch = torch_dev
    n = k + m
    clean, rounds, units, want, orc = CS.unit_case(k, m, off, L, pitch, S, block)
    assert (want == orc).all()
    C, T = CS.unit_counts(m, L)
    assert L % 4096 % 16 == 0  # a fused tail: one launch of S * C * T workgroups
    for run in (1, 3, 8):
        assert (S * C * T) % (8 * run * T) != 0
    assert S % 3 and S % 8
    rs = ecx.ReedSolomon.create(k, m)
    dpool = torch.from_numpy(clean.copy()).cuda()
    before = dpool.clone()
    flat = dpool.view(-1)
    set_knobs(ecx, KNOBS[knobs])
    try:
        got = batch_verdicts(torch, rs, dpool, n, pitch, S, off, L)
        assert got.tolist() == [1] * S  # the round without flips
        tu = {**KNOB_DEFAULTS, **KNOBS[knobs]}
        xcd = 3 if tu["xcd_group"] == 3 or pitch % 128 else 0
        order = "stagger=%d xcd_group=%d xcd_run=%d" % (tu["stagger"], xcd, tu["xcd_run"] if xcd == 3 else 0)
        assert ecx.last_launch_shape().endswith(order), (ecx.last_launch_shape(), order)
        failing = 0
        for r, rnd in enumerate(rounds):
            idx, val = CS.round_indices(rnd, n, pitch)
            device_round(torch, flat, idx, val)
            got = batch_verdicts(torch, rs, dpool, n, pitch, S, off, L)
            device_round(torch, flat, idx, val)
            failing += int((got == 0).sum())
            assert got.tolist() == want[r].tolist(), (r, [u for u in units[r]], got.tolist(), want[r].tolist())
        print(f"unit probes {knobs} ({order}): RS({k},{m}) L={L} pitch={pitch} stripes={S} units={C}x{T} "
              f"rounds={len(rounds)} sites={int((want == 0).sum())} failing wanted={int((want == 0).sum())} got={failing}")
        assert torch.equal(dpool, before)
    finally:
        set_knobs(ecx, {})


# ---------------------------------------------------------------- d. blocked layout
def packed_sweep(ecx, torch, name):
    """(k, m, L, S, sites, packed flat host array with each flip applied at its packed offset, want, pool)."""
    k, m, off, L, pitch, sites, pool, want, orc = CS.sweep_case(name)
    assert off == 0 and pitch == L and (want == orc).all()
    n, S = k + m, pool.shape[0]
    packed = CS.pack_natural(CS.without_flips(pool, sites), BLOCK)
    st, sh, by, mask = CS.site_arrays(sites)
    packed[CS.packed_offsets(n, S, L, BLOCK, st, sh, by)] ^= mask
    return k, m, L, S, sites, packed, want, pool


@pytest.mark.parametrize("name,kernel", [("byte_packed", "k_gf_check<false, 4, 4>"),
                                         ("edge_packed_10_10", "k_gf_check_blocked<false, 4, 8>")])
def test_blocked_sweep(ecx, torch_dev, name, kernel):
    """The RS(4,2) byte sweep and the RS(10,10) edge sweep over the blocked layout at block 4096
    (one block row per unit, verdict[unit / full]; the tail pass byte-safe), each flip applied at its
    packed offset; the verdicts also equal isParityCorrectBatch on the unpacked buffer.  The byte
    sweep's stripes have one block row each (divisor 1: the body pass is a k_gf_check launch over the
    block-major slots), the edge sweep's two (k_gf_check_blocked; the unit probes below have five)."""
    torch = torch_dev
    k, m, L, S, sites, packed, want, pool = packed_sweep(ecx, torch, name)
    n = k + m
    rs = ecx.ReedSolomon.create(k, m)
    flat = torch.from_numpy(packed).cuda()
    natural = ecx.blocked_unpack(flat, S, n, L, BLOCK).contiguous()
    assert torch.equal(natural, torch.from_numpy(pool.copy()).cuda())  # the flips landed where the layout keeps those bytes
    before = flat.clone()
    got = blocked_verdicts(torch, rs, flat, S, L, BLOCK)
    report("blocked sweep " + name, k, m, 0, L, L, len(sites), want, got)
    assert ecx.last_kernel() == kernel, ecx.last_kernel()
    assert same(got, want, sites)
    assert torch.equal(flat, before)
    assert same(batch_verdicts(torch, rs, natural, n, L, S, 0, L), got, sites)


@pytest.mark.parametrize("knobs", sorted(KNOBS))
def test_blocked_unit_probes(ecx, torch_dev, knobs):
    """The unit rounds over the blocked layout, RS(4,2), L = 5 * 4096 + 1040, block 4096, 37 stripes:
    the units are the five block rows and the tail of every stripe; one more round puts a flip in
    the last byte of a stripe's last block row and one in byte 0 of the next stripe's first block
    row, neighbours in the body pass."""
    torch = torch_dev
    k, m, off, L, pitch, S, block = BLOCKED_UNIT_SHAPE
    n = k + m
    clean, rounds, units, want, orc = CS.unit_case(k, m, off, L, pitch, S, block)
    assert (want == orc).all() and len(rounds) == 6 + 1 + 1
    rs = ecx.ReedSolomon.create(k, m)
    flat = torch.from_numpy(CS.pack_natural(clean, block)).cuda()
    before = flat.clone()
    dnat = torch.from_numpy(clean.copy()).cuda()
    set_knobs(ecx, KNOBS[knobs])
    try:
        assert blocked_verdicts(torch, rs, flat, S, L, block).tolist() == [1] * S
        failing = 0
        for r, rnd in enumerate(rounds):
            stripes = [s for s, site in enumerate(rnd) if site is not None]
            idx = CS.packed_offsets(n, S, L, block, stripes, [rnd[s][0] for s in stripes], [rnd[s][1] for s in stripes])
            val = np.array([1 << rnd[s][2] for s in stripes], np.uint8)
            device_round(torch, flat, idx, val)
            got = blocked_verdicts(torch, rs, flat, S, L, block)
            if r in (0, len(rounds) - 1):  # the flips sit where the layout keeps those bytes
                nidx, nval = CS.round_indices(rnd, n, pitch)
                device_round(torch, dnat.view(-1), nidx, nval)
                assert torch.equal(ecx.blocked_unpack(flat, S, n, L, block), dnat)
                assert batch_verdicts(torch, rs, dnat, n, L, S, 0, L).tolist() == got.tolist()
                device_round(torch, dnat.view(-1), nidx, nval)
            device_round(torch, flat, idx, val)
            failing += int((got == 0).sum())
            assert got.tolist() == want[r].tolist(), (r, units[r], got.tolist(), want[r].tolist())
        print(f"blocked unit probes {knobs}: RS({k},{m}) L={L} block={block} stripes={S} rounds={len(rounds)} "
              f"sites={int((want == 0).sum())} failing wanted={int((want == 0).sum())} got={failing}")
        assert torch.equal(flat, before)
    finally:
        set_knobs(ecx, {})


# ---------------------------------------------------------------- e. host memory
def host_copy(ecx, data, pinned):
    """`data` in pageable or pinned host memory with 64 guard bytes behind it; (keep-alive, array)."""
    total = data.size
    hb = ecx.HostBuffer(total + 64) if pinned else None
    buf = hb.array if pinned else np.empty(total + 64, np.uint8)
    buf[:total] = data.reshape(-1)
    buf[total:] = 0xE7
    return hb, buf


@pytest.mark.parametrize("name", ["byte_fused", "byte_ragged"])
def test_byte_sweep_from_host_memory(ecx, torch_dev, name):
    """The byte-sweep pools through isParityCorrectBatchHost and isParityCorrectBatchHostDevices
    ([0, 0, 0]) in 16 KiB chunks, from pageable and from pinned memory: every chunk, slice and device
    entry's verdicts land on their own stripes."""
    k, m, off, L, pitch, sites, pool, want, orc = CS.sweep_case(name)
    assert (want == orc).all()
    n, S = k + m, pool.shape[0]
    rs = ecx.ReedSolomon.create(k, m)
    ecx.tune("host_chunk_kib", 16)
    try:
        for pinned in (False, True):
            keep, buf = host_copy(ecx, pool, pinned)
            for devs in (None, [0, 0, 0]):
                hv = np.full(S + 16, GUARD, np.uint8)
                if devs is None:
                    rs.isParityCorrectBatchHost(buf, n * pitch, pitch, S, off, L, hv)
                else:
                    rs.isParityCorrectBatchHostDevices(buf, n * pitch, pitch, S, off, L, hv, devs)
                report(f"host sweep {name} pinned={pinned} devices={devs}", k, m, off, L, pitch, len(sites), want, hv[:S])
                assert (hv[S:] == GUARD).all()
                assert same(hv[:S], want, sites)
            assert (buf[:pool.size] == pool.reshape(-1)).all() and (buf[pool.size:] == 0xE7).all()
            del buf, keep
    finally:
        ecx.tune("host_chunk_kib", 65536)


def test_blocked_byte_sweep_from_host_memory(ecx, torch_dev):
    """The blocked RS(4,2) byte sweep through isParityCorrectBlockedBatchHost and ...HostDevices
    ([0, 0, 0]) in 16 KiB chunks, pageable and pinned."""
    k, m, L, S, sites, packed, want, pool = packed_sweep(ecx, torch_dev, "byte_packed")
    rs = ecx.ReedSolomon.create(k, m)
    ecx.tune("host_chunk_kib", 16)
    try:
        for pinned in (False, True):
            keep, buf = host_copy(ecx, packed, pinned)
            for devs in (None, [0, 0, 0]):
                hv = np.full(S + 16, GUARD, np.uint8)
                if devs is None:
                    rs.isParityCorrectBlockedBatchHost(buf, S, L, hv, BLOCK)
                else:
                    rs.isParityCorrectBlockedBatchHostDevices(buf, S, L, hv, devs, BLOCK)
                report(f"blocked host sweep pinned={pinned} devices={devs}", k, m, 0, L, L, len(sites), want, hv[:S])
                assert (hv[S:] == GUARD).all()
                assert same(hv[:S], want, sites)
            assert (buf[:packed.size] == packed).all() and (buf[packed.size:] == 0xE7).all()
            del buf, keep
    finally:
        ecx.tune("host_chunk_kib", 65536)


# ---------------------------------------------------------------- f. per-call device paths
@pytest.mark.parametrize("L,gather_kib", [(400000, 512), (70000, 0)])
def test_per_call_sites(ecx, torch_dev, L, gather_kib):
    """rs.isParityCorrect and CodingLoop.checkSomeShards on the device (host_exec_kib 0), one call
    per site, RS(17,3): the gathered path at L = 400,000 (one k_count_mismatch over the 3 * L
    syndrome bytes, past its grid of 4,096 x 256 threads, so the bytes around 1,048,576 are counted
    on the second trip of the stride loop) and the staged path (host_gather_kib 0) at L = 70,000.
    Windows: firstByte 5, so a flip at first - 1 or first + count passes."""
    k, m, off = 17, 3, 5
    n = k + m
    assert ecx.tune_value("host_exec_kib") == 0
    assert (m * L > CS.COUNT_WRAP) == (gather_kib > 0)
    sites = CS.percall_sites(n, k, off, L)
    rng = np.random.default_rng(9300 + L)
    shards = [rng.integers(0, 256, off + L + 3, dtype=np.uint8) for _ in range(n)]
    orc = O.ReedSolomon(k, m)
    orc.encode_parity(shards, off, L)
    before = [s.copy() for s in shards]
    rs = ecx.ReedSolomon.create(k, m)
    rows = rs.parityRows
    loop = ecx.CodingLoop()
    ecx.tune("host_gather_kib", gather_kib)
    try:
        assert rs.isParityCorrect(shards, off, L) and loop.checkSomeShards(rows, shards[:k], k, shards[k:], m, off, L)
        want, got_rs, got_loop = [], [], []
        for i, b, bit in sites:
            shards[i][b] ^= 1 << bit
            expect = not CS.inside((i, b, bit), off, L)
            assert orc.is_parity_correct(shards, off, L) == expect, (i, b, bit)
            want.append(int(expect))
            got_rs.append(int(rs.isParityCorrect(shards, off, L)))
            got_loop.append(int(loop.checkSomeShards(rows, shards[:k], k, shards[k:], m, off, L)))
            shards[i][b] ^= 1 << bit
        for what, got in (("isParityCorrect", got_rs), ("checkSomeShards", got_loop)):
            print(f"per-call {what} host_gather_kib={gather_kib}: RS({k},{m}) L={L} off={off} sites={len(sites)} "
                  f"failing wanted={want.count(0)} got={got.count(0)}")
            assert got == want, [(sites[j], got[j], want[j]) for j in range(len(sites)) if got[j] != want[j]][:8]
        assert want.count(1) == 4
        assert all((a == b).all() for a, b in zip(shards, before))
    finally:
        ecx.tune("host_gather_kib", 512)
