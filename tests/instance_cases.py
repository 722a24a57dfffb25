"""Shared cases of the apply-kernel instance cover (tests/test_instance_cover*.py) and of the
unit-order test (tests/test_unit_order.py).  Host-only: which kernel instance a (map, layout, knob
setting) case launches is asked of GfMap.launch_plan (csrc/launch_rules.cpp), which touches no
device; the expected bytes of a case are conftest.gf_apply_numpy -- the oracle's multiplication
table -- over the library's own dense matrix (tied to the oracle in tests/test_planner.py).

reachable() walks maps x layouts x modes x knob settings and returns every kernel instance of record
the rules can ask for, with the cases that reach it; cover() picks one case per instance, and COVER
is that choice written out, which tests/test_instance_cover_cpu.py holds against reachable().
"""
import functools
import importlib.util
import itertools
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GUARD = 64                      # guard bytes behind every output
LEAD = 128                      # and before it: 64 guard bytes and 64 more, so that the output keeps the
                                # 128-B alignment of its allocation (the launch rules read it)
MAX_CASE_BYTES = 256 << 20      # no case allocates more (input + output)
S_COVER = 3
# (shard bytes, pitch kind of scripts/record_launch_shapes.py pitch_of): two full chunks and 16 B;
# three chunks; sixteen; a pitch longer than the rows; a 4 MiB pitch (the skew's auto rule); byte-safe
# only (no instance of record); a fused 16-B-multiple tail
LAYOUTS = ((8208, "r16"), (12288, "r16"), (65536, "r16"), (8208, "pad"), (16384, "4m"), (4000, "r16"), (8176, "r16"))
MODES = ((0, 0), (1, 0), (0, 1))  # (in place, accumulate): separate buffers, in place, accumulate
TRIPLE_A = ("depth", "nontemporal", "store_scope")
TRIPLE_B = ("lds_tables", "block_threads")
N_REACHABLE = 62  # instances reachable() finds; tests/test_instance_cover_cpu.py


@functools.lru_cache(maxsize=None)
def recorder():
    """scripts/record_launch_shapes.py as a module (its maps, knob table and set_knob)."""
    spec = importlib.util.spec_from_file_location("record_launch_shapes", ROOT / "scripts" / "record_launch_shapes.py")
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


def random_map(ecx, n_out, n_in, seed):
    """A dense n_out x n_in map without a zero; outputs behind the inputs, so in place is defined."""
    m = np.random.default_rng(seed).integers(1, 256, (n_out, n_in), dtype=np.uint8)
    return ecx.GfMap.from_matrix(m, in_slot=list(range(n_in)), out_slot=list(range(n_in, n_in + n_out)))


_MAPS = {}


def maps(ecx):
    """name -> GfMap: the recorder's ten maps, the RS(10,10) encode map (two tiles that do not pair
    without wide tiles) and two random dense maps, 24 x 12 (three tiles) and 17 x 9 (tiles of 8, 8
    and 1 rows).  Built once per process (host-only)."""
    if not _MAPS:
        rec = recorder()
        built = rec.build_maps(ecx)
        rs1010 = ecx.ReedSolomon.create(10, 10)
        built["rs1010_enc"] = rs1010.encode_map()
        built["rand24x12"] = random_map(ecx, 24, 12, 2412)
        built["rand17x9"] = random_map(ecx, 17, 9, 1709)
        built["_owners"] = built["_owners"] + (rs1010,)
        _MAPS.update(built)
    return _MAPS


def map_names(ecx):
    return [k for k in maps(ecx) if not k.startswith("_")]


def in_place_ok(gmap):
    """In place is defined when no output slot is an input slot (a tile would overwrite what
    another still reads)."""
    _, ins, outs = gmap.matrix()
    return not set(ins.tolist()) & set(outs.tolist())


def knob_settings():
    """The defaults, every single value of the recorder's KNOBS, every pair of them, and the
    triples: two or all three of depth / nontemporal / store_scope with one of lds_tables /
    block_threads, and those three together.  Each a "key=value,..." string in KNOBS order."""
    knobs = recorder().KNOBS
    values = dict(knobs)
    order = [k for k, _ in knobs]

    def settings(keys):
        keys = sorted(keys, key=order.index)
        return [",".join("%s=%d" % kv for kv in zip(keys, vs)) for vs in itertools.product(*(values[k] for k in keys))]

    out = [""]
    for r in (1, 2):
        for keys in itertools.combinations(order, r):
            out += settings(keys)
    for a in list(itertools.combinations(TRIPLE_A, 2)) + [TRIPLE_A]:
        for b in TRIPLE_B:
            out += settings(a + (b,))
    out += settings(TRIPLE_A)
    return out


def set_knobs(ecx, k):
    """Every shape knob back to its default (xcd_run too: the recorder's defaults do not list it),
    then the setting's."""
    recorder().set_knob(ecx, "")
    ecx.tune("xcd_run", 8)
    for kv in filter(None, k.split(",")):
        key, _, v = kv.partition("=")
        ecx.tune(key, int(v))


def layout(gmap, n, p, ip, S):
    """(input offset, stripe stride, slot pitch, output offset, stripe stride, slot pitch, bytes of the
    input buffer, bytes of the output buffer or 0 in place) of a case.  Every stripe has one slot
    more than the map uses; the output lies LEAD bytes into its buffer with GUARD bytes behind it,
    and in place the one buffer is the output's.  `p` is a pitch kind of the recorder's or a pitch."""
    mi, mo = gmap.max_slots()
    pitch = p if isinstance(p, int) else recorder().pitch_of(p, n)
    if ip:
        stride = (max(mi, mo) + 2) * pitch
        return LEAD, stride, pitch, LEAD, stride, pitch, LEAD + S * stride + GUARD, 0
    return 0, (mi + 2) * pitch, pitch, LEAD, (mo + 2) * pitch, pitch, S * (mi + 2) * pitch, LEAD + S * (mo + 2) * pitch + GUARD


def case_bytes(gmap, n, p, ip, S=S_COVER):
    lay = layout(gmap, n, p, ip, S)
    return lay[6] + lay[7]


def plan_of(gmap, n, p, ip, acc, S=S_COVER, in_base=1 << 40, out_base=1 << 44):
    """GfMap.launch_plan of a case under the current knobs, at made-up addresses with the alignment
    a device allocation has (or at the real ones)."""
    io, iss, isl, oo, oss, osl, _, _ = layout(gmap, n, p, ip, S)
    return gmap.launch_plan(in_base + io, iss, isl, (in_base if ip else out_base) + oo, oss, osl, S, n, bool(acc))


def instance_of(plan):
    """The kernel instance of a launch-shape string: what stands before the unit order."""
    return plan.split(" stagger=")[0]


def reachable(ecx):
    """instance -> [(map, bytes, pitch kind, in place, accumulate, knobs), ...]: every case of the
    grid that can run (a defined in-place, at most MAX_CASE_BYTES) by the instance of record
    GfMap.launch_plan names for it.  No device is touched."""
    mp = maps(ecx)
    grid = []
    for name in map_names(ecx):
        ipok = in_place_ok(mp[name])
        for n, p in LAYOUTS:
            for ip, acc in MODES:
                if (ip and not ipok) or case_bytes(mp[name], n, p, ip) > MAX_CASE_BYTES:
                    continue
                grid.append((name, n, p, ip, acc))
    found = {}
    try:
        for k in knob_settings():
            set_knobs(ecx, k)
            for name, n, p, ip, acc in grid:
                plan = plan_of(mp[name], n, p, ip, acc)
                if plan:
                    found.setdefault(instance_of(plan), []).append((name, n, p, ip, acc, k))
    finally:
        set_knobs(ecx, "")
    return found


def ring_depth(inst):
    """The load-ring depth in an instance's name (k_map_planes has no ring: a tile's rows, 8)."""
    if "<" not in inst:
        return 8
    family, args = inst[:-1].split("<")
    return int(args.split(", ")[{"k_gf_apply": 3, "k_gf_apply_tail": 2, "k_gf_apply_wide": 3, "k_gf_apply_skew": 1}[family]])


def cover(ecx, found=None):
    """One case per instance, sorted by instance name.  A 4 MiB pitch only where no other layout
    reaches the instance.  Then the map that falls least short of one input more than the instance's
    ring is deep: with fewer the ring holds the whole tile and its refill never runs (the one-input
    partial-sum map would otherwise cover half the instances).  Then the (map, layout, knobs) with the smallest buffers (as two buffers, whatever the mode), the
    fewest knobs, and the first in the order of its fields -- so a 4 MiB pitch or the 3,584-slot
    Clay(10,4) map is chosen only where nothing smaller reaches the instance.  The accumulate flag
    and the aliasing are no template parameters, so the mode goes round: instance i of the sorted
    list runs mode i mod 3 of MODES among those with which that (map, layout, knobs) reaches it."""
    found = reachable(ecx) if found is None else found
    mp = maps(ecx)
    n_in = {name: mp[name].info()["n_in"] for name in map_names(ecx)}
    out = []
    for i, inst in enumerate(sorted(found)):
        depth = ring_depth(inst)

        def cost(c):
            name, n, p, ip, acc, k = c
            return (p == "4m", max(0, depth + 1 - n_in[name]), case_bytes(mp[name], n, p, 0), len(k.split(",")) if k else 0,
                    (name, n, p, k))

        name, n, p, _, _, k = min(found[inst], key=cost)
        reach = set(found[inst])
        modes = [m for m in MODES if (name, n, p) + m + (k,) in reach]
        out.append((inst, name, n, p) + modes[i % len(modes)] + (k,))
    return out


# cover(), written out: (instance, map, shard bytes, pitch kind, in place, accumulate, knobs)
COVER = [
    ('k_gf_apply<false, false, 0, 4, false, 256, 8>', 'rs124_dec01', 8176, 'r16', 0, 0, 'depth=2,nontemporal=0'),
    ('k_gf_apply<false, false, 0, 4, true, 256, 8>', 'rs124_dec01', 8176, 'r16', 1, 0, 'depth=2,nontemporal=0,lds_tables=2'),
    ('k_gf_apply<false, false, 0, 8, false, 256, 8>', 'rs124_dec01', 8176, 'r16', 0, 1, 'nontemporal=0'),
    ('k_gf_apply<false, false, 0, 8, true, 256, 8>', 'rs124_dec01', 8176, 'r16', 0, 0, 'nontemporal=0,lds_tables=2'),
    ('k_gf_apply<false, false, 1, 2, false, 256, 8>', 'clay104_rep3', 8176, 'r16', 1, 0, 'depth=2,lds_tables=0'),
    ('k_gf_apply<false, false, 1, 2, true, 256, 8>', 'rs1010_enc', 8176, 'r16', 0, 1, 'depth=2,wide_tiles=0'),
    ('k_gf_apply<false, false, 1, 4, false, 256, 8>', 'rs1010_enc', 8176, 'r16', 0, 0, 'wide_tiles=0,lds_tables=0'),
    ('k_gf_apply<false, false, 1, 4, false, 64, 8>', 'rs1010_enc', 4000, 'r16', 1, 0, 'lds_tables=0,block_threads=64'),
    ('k_gf_apply<false, false, 1, 4, true, 256, 8>', 'rs1010_enc', 8176, 'r16', 0, 1, 'wide_tiles=0'),
    ('k_gf_apply<false, false, 1, 4, true, 64, 8>', 'rs1010_enc', 4000, 'r16', 0, 0, 'block_threads=64'),
    ('k_gf_apply<false, false, 1, 8, false, 256, 8>', 'rand24x12', 8176, 'r16', 1, 0, 'wide_tiles=0,lds_tables=0'),
    ('k_gf_apply<false, false, 1, 8, false, 64, 8>', 'rand24x12', 4000, 'r16', 0, 1, 'lds_tables=0,block_threads=64'),
    ('k_gf_apply<false, false, 1, 8, true, 256, 8>', 'rs1010_enc', 8176, 'r16', 0, 0, 'depth=10,wide_tiles=0'),
    ('k_gf_apply<false, false, 1, 8, true, 64, 8>', 'rs1010_enc', 4000, 'r16', 1, 0, 'depth=10,block_threads=64'),
    ('k_gf_apply<false, false, 2, 4, false, 256, 8>', 'clay104_rep3', 8176, 'r16', 0, 1, 'depth=2,store_scope=1,lds_tables=0'),
    ('k_gf_apply<false, false, 2, 4, true, 256, 8>', 'rs1010_enc', 8176, 'r16', 0, 0, 'store_scope=1,wide_tiles=0'),
    ('k_gf_apply<false, false, 2, 8, false, 256, 8>', 'clay104_rep3', 8176, 'r16', 1, 0, 'store_scope=1,lds_tables=0'),
    ('k_gf_apply<false, false, 2, 8, true, 256, 8>', 'rand24x12', 8176, 'r16', 0, 1, 'store_scope=1,wide_tiles=0'),
    ('k_gf_apply<false, true, 1, 10, false, 256, 8>', 'rs124_dec01', 8176, 'r16', 0, 0, 'depth=10,block_threads=256'),
    ('k_gf_apply<false, true, 1, 12, false, 256, 2>', 'rs42_enc', 8176, 'r16', 1, 0, 'depth=12'),
    ('k_gf_apply<false, true, 1, 12, false, 256, 4>', 'rs173_enc', 8176, 'r16', 0, 1, 'depth=12,small_tiles=1'),
    ('k_gf_apply<false, true, 1, 12, false, 256, 8>', 'rs173_enc', 8176, 'r16', 0, 0, 'depth=12'),
    ('k_gf_apply<false, true, 1, 16, false, 256, 8>', 'rs173_enc', 8176, 'r16', 1, 0, 'depth=16'),
    ('k_gf_apply<false, true, 1, 2, false, 256, 8>', 'lrc_rep0', 8176, 'r16', 0, 1, 'depth=2,small_tiles=0'),
    ('k_gf_apply<false, true, 1, 2, true, 256, 8>', 'lrc_enc', 8176, 'r16', 0, 0, 'depth=2,lds_tables=2'),
    ('k_gf_apply<false, true, 1, 20, false, 256, 8>', 'clay42_rep1', 8176, 'r16', 1, 0, ''),
    ('k_gf_apply<false, true, 1, 24, false, 256, 8>', 'clay42_rep1', 8176, 'r16', 0, 1, 'depth=24'),
    ('k_gf_apply<false, true, 1, 4, false, 256, 2>', 'rs42_enc', 8176, 'r16', 0, 0, ''),
    ('k_gf_apply<false, true, 1, 4, false, 256, 4>', 'lrc_enc', 8176, 'r16', 1, 0, 'depth=10,small_tiles=1'),
    ('k_gf_apply<false, true, 1, 4, false, 256, 8>', 'rs124_dec01', 12288, 'r16', 0, 1, 'depth=4,block_threads=256'),
    ('k_gf_apply<false, true, 1, 4, false, 64, 8>', 'rs124_dec01', 12288, 'r16', 0, 0, 'depth=2'),
    ('k_gf_apply<false, true, 1, 4, true, 256, 8>', 'rs1010_enc', 8176, 'r16', 1, 0, 'nontemporal=2,wide_tiles=0'),
    ('k_gf_apply<false, true, 1, 4, true, 64, 8>', 'rs124_dec01', 4000, 'r16', 0, 1, 'depth=2,lds_tables=2'),
    ('k_gf_apply<false, true, 1, 8, false, 256, 2>', 'rs124_dec01', 8176, 'r16', 0, 0, 'small_tiles=1,block_threads=256'),
    ('k_gf_apply<false, true, 1, 8, false, 256, 4>', 'lrc_enc', 8176, 'r16', 1, 0, 'small_tiles=1'),
    ('k_gf_apply<false, true, 1, 8, false, 256, 8>', 'rs124_dec01', 12288, 'r16', 0, 1, 'block_threads=256'),
    ('k_gf_apply<false, true, 1, 8, false, 64, 8>', 'rs124_dec01', 12288, 'r16', 0, 0, ''),
    ('k_gf_apply<false, true, 1, 8, true, 256, 8>', 'rs124_dec01', 8176, 'r16', 1, 0, 'lds_tables=2,block_threads=256'),
    ('k_gf_apply<false, true, 1, 8, true, 64, 8>', 'rs124_dec01', 4000, 'r16', 0, 1, 'lds_tables=2'),
    ('k_gf_apply<false, true, 2, 20, false, 256, 8>', 'clay42_rep1', 8176, 'r16', 0, 0, 'store_scope=1'),
    ('k_gf_apply<false, true, 2, 4, false, 256, 8>', 'rs124_dec01', 8176, 'r16', 1, 0, 'depth=2,store_scope=1'),
    ('k_gf_apply<false, true, 2, 4, true, 256, 8>', 'rs124_dec01', 8176, 'r16', 0, 1, 'depth=2,store_scope=1,lds_tables=2'),
    ('k_gf_apply<false, true, 2, 8, false, 256, 8>', 'rs124_dec01', 8176, 'r16', 0, 0, 'store_scope=1'),
    ('k_gf_apply<false, true, 2, 8, true, 256, 8>', 'rs124_dec01', 8176, 'r16', 1, 0, 'store_scope=1,lds_tables=2'),
    ('k_gf_apply_skew<true, 4, 2, 2, 256>', 'rs42_enc', 8208, 'r16', 0, 1, 'skew_chunks=2'),
    ('k_gf_apply_skew<true, 4, 2, 4, 256>', 'rs42_enc', 65536, 'r16', 0, 0, 'skew_chunks=4'),
    ('k_gf_apply_skew<true, 4, 4, 2, 256>', 'lrc_enc', 8208, 'r16', 1, 0, 'depth=4,skew_chunks=2'),
    ('k_gf_apply_skew<true, 4, 4, 4, 256>', 'lrc_enc', 65536, 'r16', 0, 1, 'depth=4,skew_chunks=4'),
    ('k_gf_apply_skew<true, 4, 8, 2, 256>', 'clay42_rep1', 8208, 'r16', 0, 0, 'skew_chunks=2'),
    ('k_gf_apply_skew<true, 8, 2, 2, 256>', 'rs124_dec01', 8208, 'r16', 1, 0, 'block_threads=256,skew_chunks=2'),
    ('k_gf_apply_skew<true, 8, 2, 4, 256>', 'rs124_dec01', 65536, 'r16', 0, 1, 'block_threads=256,skew_chunks=4'),
    ('k_gf_apply_skew<true, 8, 4, 2, 256>', 'lrc_enc', 8208, 'r16', 0, 0, 'skew_chunks=2'),
    ('k_gf_apply_skew<true, 8, 4, 4, 256>', 'lrc_enc', 65536, 'r16', 1, 0, 'skew_chunks=4'),
    ('k_gf_apply_tail<true, 1, 4, false, 256, 8>', 'rs124_dec01', 8176, 'r16', 0, 1, 'depth=4,block_threads=256'),
    ('k_gf_apply_tail<true, 1, 4, false, 64, 8>', 'rs124_dec01', 4000, 'r16', 0, 0, 'depth=2'),
    ('k_gf_apply_tail<true, 1, 8, false, 256, 8>', 'rs124_dec01', 8176, 'r16', 1, 0, 'block_threads=256'),
    ('k_gf_apply_tail<true, 1, 8, false, 64, 8>', 'rs124_dec01', 4000, 'r16', 0, 1, ''),
    ('k_gf_apply_wide<false, false, 1, 4>', 'rs1010_enc', 8176, 'r16', 0, 0, 'nontemporal=0'),
    ('k_gf_apply_wide<false, false, 1, 8>', 'rs1010_enc', 8176, 'r16', 1, 0, 'depth=8,nontemporal=0'),
    ('k_gf_apply_wide<false, true, 1, 4>', 'rs1010_enc', 8176, 'r16', 0, 1, ''),
    ('k_gf_apply_wide<false, true, 1, 8>', 'rs1010_enc', 8176, 'r16', 0, 0, 'depth=8'),
    ('k_map_planes', 'rs124_dec01', 8176, 'r16', 1, 0, 'block_threads=256,map_planes=2'),
]


# ---------------------------------------------------------------- running a case (GPU tests)
def run_case(ecx, torch, gmap, n, p, ip, acc, S, seed, wants=None):
    """Run one case on the device under the current knobs and return (plan, got, want): the plan
    asked for the real addresses, the whole output buffer after the launch and what it must hold.
    The input is ecx.fill_random; a separate output is prefilled with seeded random bytes (a
    constant would hide an assignment where an accumulation was due); the expectation is
    gf_apply_numpy over the host copy of the input for every stripe, XORed with the prefill when
    accumulating, and every other byte of the buffer -- guards, gaps between rows, unused slots --
    as it was before the launch.  `wants`: a dict that keeps the expectation of a (layout, mode, seed)
    for the next call with it (other knobs, the same bytes); it is never written to again."""
    from conftest import gf_apply_numpy
    io, iss, isl, oo, oss, osl, in_bytes, out_bytes = layout(gmap, n, p, ip, S)
    inp = torch.empty(in_bytes, dtype=torch.uint8, device="cuda")
    ecx.fill_random(inp, in_bytes, seed)
    if ip:
        out = inp
    else:
        out = torch.from_numpy(np.random.default_rng(seed + 1).integers(0, 256, out_bytes, dtype=np.uint8)).cuda()
    assert inp.data_ptr() % 256 == 0 and out.data_ptr() % 256 == 0  # the alignment plan_of's made-up addresses assume
    torch.cuda.synchronize()
    key = (id(gmap), n, p, ip, acc, S, seed)
    if wants is None or key not in wants:
        host_in = inp.cpu().numpy()
        want = host_in.copy() if ip else out.cpu().numpy()
    plan = plan_of(gmap, n, p, ip, acc, S, inp.data_ptr(), out.data_ptr())
    (gmap.accumulate_batch if acc else gmap.apply_batch)(inp[io:], iss, isl, out[oo:], oss, osl, S, n)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    if wants is not None and key in wants:
        return plan, got, wants[key]
    matrix, ins, outs = gmap.matrix()
    for s in range(S):
        rows = gf_apply_numpy(matrix, [host_in[io + s * iss + j * isl:][:n] for j in ins.tolist()])
        for o, row in zip(outs.tolist(), rows):
            dst = want[oo + s * oss + o * osl:][:n]
            dst[:] = dst ^ row if acc else row
    if wants is not None:
        want.setflags(write=False)
        wants[key] = want
    return plan, got, want


def first_difference(got, want):
    """"" when the buffers are equal, or where they first differ and how many bytes do."""
    bad = np.nonzero(got != want)[0]
    return "" if len(bad) == 0 else "%d bytes differ, the first at buffer offset %d" % (len(bad), int(bad[0]))
