"""Pools for the Clay codeword check (tests/test_clay_check_cpu.py, tests/test_clay_check.py and its
capture and JNI companions), in the manner of tests/check_sites.py.

A stripe of Clay(k, m) shortened by v virtual data nodes holds alpha * n_real sub-chunks, real slot
z * n_real + node, `pitch` bytes apart; the check covers bytes [0, B) of every sub-chunk.  A site is
(stripe, plane, node, byte, bit): `stripe[plane * n_real + node][byte] ^= 1 << bit`, at most one per
stripe.  The expected verdict of a stripe is 0 exactly when it has a site with byte < B (a flip in
the pad bytes of a layout with pitch > B passes).

Every stripe is a copy of one of a few base stripes whose parity nodes the oracle encoded from
random data nodes (shortened_clay_perform_coding with the parity nodes erased), so a case is kept
as (bases, base of each stripe, sites): the 3.6 GiB pools of the alpha = 256 geometries exist only
on the device (device_pool), never in host memory.  Everything here is host-side numpy and the
oracle but for device_pool; cases are built once per shape and never written."""
import functools
from dataclasses import dataclass

import numpy as np

import oracle as O

CHUNK = 4096  # bytes of one sub-chunk a check workgroup covers (csrc/launch_rules.hpp kChunkBytes)
GROUP = 7     # site stripes between two clean stripes
BASES = 4     # distinct encoded stripes a pool is tiled from


# ---------------------------------------------------------------- geometry
def geometry(k, m, v=0):
    """(q, t, alpha, n_real) of Clay(k, m) shortened by v."""
    q, t = m, (k + v + m) // m
    return q, t, q ** t, k + m


def zvec(z, q, t):
    """Digits of plane z, most significant first: digit y has weight q^(t-1-y)."""
    return [(z // q ** (t - 1 - y)) % q for y in range(t)]


def under(node, k, v):
    """Underlying node of real node `node` (the virtual nodes are underlying k .. k+v-1)."""
    return node if node < k else node + v


def real_of(u, k, v):
    """Real node of underlying node u, None for a virtual one."""
    return u if u < k else (None if u < k + v else u - v)


def is_dot(k, m, v, z, node):
    q, t, _, _ = geometry(k, m, v)
    u = under(node, k, v)
    return zvec(z, q, t)[u // q] == u % q


def dot_nodes(k, m, v, z):
    """The real dot nodes of plane z: their sub-chunks are read by plane z's workgroup alone."""
    return [r for r in range(k + m) if is_dot(k, m, v, z, r)]


def partner(k, m, v, z, node):
    """(z', real node' or None when it is virtual) of a non-dot real node of plane z."""
    q, t, _, _ = geometry(k, m, v)
    u = under(node, k, v)
    x, y = u % q, u // q
    d = zvec(z, q, t)[y]
    assert d != x
    return z + (x - d) * q ** (t - 1 - y), real_of(d + q * y, k, v)


# ---------------------------------------------------------------- pools
def stripe_of_site(j):
    """Pool stripe of site j: stripes 7, 15, 23, ... are the clean ones."""
    return j + j // GROUP


def pool_stripes(nsites):
    return nsites + -(-nsites // GROUP)


def encode_parity(k, m, v, stripe, B):
    """The oracle's parity of a [alpha * n_real][>= B] stripe's data nodes over bytes [0, B): a
    list of m * alpha arrays, [z * m + p] = parity node k + p of plane z."""
    _, _, alpha, nr = geometry(k, m, v)
    ins = [None if i % nr >= k else stripe[i, :B] for i in range(alpha * nr)]
    return O.shortened_clay_perform_coding(k, m, v, list(range(k, k + m)), ins, B)


def encoded_bases(k, m, v, B, pitch, seed, count=BASES):
    """`count` stripes [alpha * n_real][pitch] of random bytes -- pad bytes included -- whose parity
    nodes over [0, B) are the oracle's encode of their data nodes."""
    _, _, alpha, nr = geometry(k, m, v)
    rng = np.random.default_rng(seed)
    bases = rng.integers(0, 256, (count, alpha * nr, pitch), dtype=np.uint8)
    for b in range(count):
        par = encode_parity(k, m, v, bases[b], B)
        for z in range(alpha):
            for p in range(m):
                bases[b, z * nr + k + p, :B] = par[z * m + p]
    return bases


@dataclass(frozen=True, eq=False)
class Case:
    k: int
    m: int
    v: int
    B: int
    pitch: int
    bases: np.ndarray    # [count][alpha * n_real][pitch], read-only
    base_of: np.ndarray  # [S] base of each stripe
    sites: tuple         # (stripe, plane, node, byte, bit), at most one per stripe
    want: np.ndarray     # [S] expected verdicts

    @property
    def nstripes(self):
        return len(self.base_of)

    @property
    def slots(self):
        _, _, alpha, nr = geometry(self.k, self.m, self.v)
        return alpha * nr

    def flat_flips(self):
        """(flat byte offsets into the [S][slots][pitch] pool, xor masks) of the sites."""
        nr = self.k + self.m
        idx = [(s * self.slots + z * nr + node) * self.pitch + byte for s, z, node, byte, _ in self.sites]
        return np.array(idx, np.int64), np.array([1 << bit for *_, bit in self.sites], np.uint8)

    def host_pool(self):
        """The pool [S][slots][pitch] in host memory (small cases only)."""
        pool = self.bases[self.base_of]
        idx, val = self.flat_flips()
        pool.reshape(-1)[idx] ^= val
        return pool

    def stripe(self, s):
        """Stripe s [slots][pitch], flipped as the pool has it."""
        st = self.bases[self.base_of[s]].copy()
        nr = self.k + self.m
        for ss, z, node, byte, bit in self.sites:
            if ss == s:
                st[z * nr + node, byte] ^= 1 << bit
        return st


def build(k, m, v, B, pitch, nstripes, sites, seed, count=BASES):
    """The case of a site list: stripe s is base s % count, flipped at its site if it has one; the
    expected verdict of a stripe is 0 exactly when its site lies inside [0, B)."""
    _, _, alpha, nr = geometry(k, m, v)
    sites = tuple(tuple(int(x) for x in site) for site in sites)
    assert pitch >= B and len({s for s, *_ in sites}) == len(sites), "at most one site per stripe"
    assert all(0 <= s < nstripes and 0 <= z < alpha and 0 <= node < nr and 0 <= byte < pitch and 0 <= bit < 8
               for s, z, node, byte, bit in sites)
    bases = encoded_bases(k, m, v, B, pitch, seed, count)
    want = np.ones(nstripes, np.uint8)
    for s, _, _, byte, _ in sites:
        if byte < B:
            want[s] = 0
    base_of = np.arange(nstripes) % count
    for a in (bases, want, base_of):
        a.setflags(write=False)
    return Case(k, m, v, B, pitch, bases, base_of, sites, want)


def oracle_verdicts(case):
    """The oracle's verdict of every stripe: re-encode the parity nodes from the stripe's data nodes
    and compare with the stored parity.  A base is re-encoded and compared over all of [0, B); a
    stripe with a site differs from its base in one byte and the code acts on every byte position by
    itself, so it is re-encoded over the 16-byte window of [0, B) around that byte; a site in the
    pad bytes leaves [0, B) as the base has it."""
    k, m, v, B = case.k, case.m, case.v, case.B
    _, _, alpha, nr = geometry(k, m, v)

    def agrees(stripe, lo, hi):
        window = stripe[:, lo:hi]
        par = encode_parity(k, m, v, window, hi - lo)
        return all((par[z * m + p] == window[z * nr + k + p]).all() for z in range(alpha) for p in range(m))

    base_ok = [int(agrees(b, 0, B)) for b in case.bases]
    got = np.array([base_ok[b] for b in case.base_of], np.uint8)
    for s, _, _, byte, _ in case.sites:
        if byte < B:
            lo = byte // 16 * 16
            got[s] = int(agrees(case.stripe(s), lo, min(B, lo + 16)))
    return got


def device_pool(case, torch, device="cuda:0", base_offset=0, stripe_pad=0):
    """The pool on the device: (flat uint8 tensor, view of the stripes' bytes, stripe_stride).  The
    stripes start `base_offset` bytes into the tensor and lie slots * pitch + stripe_pad apart."""
    S, row = case.nstripes, case.slots * case.pitch
    stride = row + stripe_pad
    flat = torch.zeros(base_offset + S * stride + 16, dtype=torch.uint8, device=device)
    view = flat[base_offset:base_offset + S * stride].as_strided((S, row), (stride, 1))
    bases = torch.from_numpy(case.bases.copy()).to(device).reshape(len(case.bases), row)
    view.copy_(bases[torch.from_numpy(case.base_of.copy()).to(device)])
    flip_sites(case, torch, view, case.sites)
    return flat, view, stride


def flip_sites(case, torch, view, sites):
    """XOR the sites' bits into a device_pool view (again to take them back)."""
    if not sites:
        return
    nr = case.k + case.m
    rows = torch.tensor([s for s, *_ in sites], dtype=torch.int64, device=view.device)
    cols = torch.tensor([(z * nr + node) * case.pitch + byte for _, z, node, byte, _ in sites], dtype=torch.int64,
                        device=view.device)
    val = torch.tensor([1 << bit for *_, bit in sites], dtype=torch.uint8, device=view.device)
    view[rows, cols] = view[rows, cols] ^ val


# ---------------------------------------------------------------- site lists
def subchunk_sites(k, m, v, B, planes=None, nodes=None):
    """One site in every (plane, node) sub-chunk (of `planes` x `nodes`), site j in stripe
    stripe_of_site(j); the byte walks the window and the bit rotates.  Returns (sites, stripes)."""
    _, _, alpha, nr = geometry(k, m, v)
    pairs = [(z, node) for z in (range(alpha) if planes is None else planes)
             for node in (range(nr) if nodes is None else nodes)]
    sites = [(stripe_of_site(j), z, node, (37 * j + 5) % B, j % 8) for j, (z, node) in enumerate(pairs)]
    return sites, pool_stripes(len(sites))


def covering_planes(q, t):
    """Planes 0 and alpha - 1 and, for every digit position y and value x, a plane with
    zvec[y] == x: the planes x * (1 + q + ... + q^(t-1)) have every digit x; two mixed planes more."""
    alpha = q ** t
    ones = sum(q ** i for i in range(t))
    planes = {0, alpha - 1} | {x * ones for x in range(q)}
    planes |= {sum(((y + s) % q) * q ** (t - 1 - y) for y in range(t)) for s in range(q)}  # digit y = y + s
    planes |= {1, q, alpha // q, alpha - 2, alpha // 2 + 1, ones + 1, alpha - q - 1}
    planes = sorted(p for p in planes if 0 <= p < alpha)
    assert all(any(zvec(z, q, t)[y] == x for z in planes) for y in range(t) for x in range(q))
    return planes


def edge_positions(B):
    """Byte positions at the dword, lane, wave and chunk edges of a check over B bytes."""
    F = B // CHUNK
    want = [0, 1, 3, 4, 8, 11, 15, 16, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, F * CHUNK - 1, F * CHUNK,
            B - 17, B - 16, B - 1]
    return sorted({p for p in want if 0 <= p < B})


def byte_sites(k, m, v, B, pitch):
    """Edge positions of the window crossed with every bit, the (plane, node) rotating, then --
    where the pitch has them -- sites in the pad bytes just past B.  Returns (sites, stripes)."""
    _, _, alpha, nr = geometry(k, m, v)
    picks = [(p, bit) for p in edge_positions(B) for bit in range(8)]
    picks += [(B, 0), (B, 7), (pitch - 1, 3)] if pitch > B else []
    sites = [(stripe_of_site(j), (5 * j + 1) % alpha, (7 * j + 2) % nr, byte, bit) for j, (byte, bit) in enumerate(picks)]
    return sites, pool_stripes(len(sites))


def unit_rounds(k, m, v, B, S):
    """C * alpha + 1 rounds over S stripes: in round r stripe s carries one flip that only the
    workgroup of unit (chunk c, plane z) with c * alpha + z == (r + s) % (C * alpha + 1) can see --
    a dot node of plane z (no other plane reads it), at a byte of chunk c -- or none when that
    value is C * alpha.  Over the rounds every (stripe, chunk, plane) is probed exactly once."""
    _, _, alpha, _ = geometry(k, m, v)
    C = -(-B // CHUNK)
    P = C * alpha + 1
    rounds, seen = [], set()
    for r in range(P):
        sites = []
        for s in range(S):
            val = (r + s) % P
            if val == C * alpha:
                continue
            c, z = divmod(val, alpha)
            dots = dot_nodes(k, m, v, z)
            node = dots[(r + s) % len(dots)]
            byte = c * CHUNK + (16 * ((37 * s) % 256) + s % 16) % min(CHUNK, B - c * CHUNK)
            sites.append((s, z, node, byte, (r + s) % 8))
            seen.add((s, c, z))
        rounds.append(sites)
    assert len(seen) == S * C * alpha
    return rounds


# ---------------------------------------------------------------- the named cases
def _seed(k, m, v, B, pitch):
    return 7700 + 97 * k + 13 * m + v + B + pitch


@functools.lru_cache(maxsize=None)
def subchunk_case(k, m, v, B, pitch=None, cover=False):
    """Every (plane, node) sub-chunk once (cover: every node crossed with covering_planes)."""
    pitch = B if pitch is None else pitch
    q, t, _, _ = geometry(k, m, v)
    sites, S = subchunk_sites(k, m, v, B, covering_planes(q, t) if cover else None)
    return build(k, m, v, B, pitch, S, sites, _seed(k, m, v, B, pitch))


@functools.lru_cache(maxsize=None)
def byte_case(k, m, v, B, pitch):
    sites, S = byte_sites(k, m, v, B, pitch)
    return build(k, m, v, B, pitch, S, sites, _seed(k, m, v, B, pitch))


@functools.lru_cache(maxsize=None)
def unit_case(k, m, v, B, S):
    """(case without sites: S clean stripes, rounds)."""
    return build(k, m, v, B, B, S, [], _seed(k, m, v, B, S), count=min(S, BASES)), unit_rounds(k, m, v, B, S)


@functools.lru_cache(maxsize=None)
def clay124_case():
    """Clay(12,4) unshortened, 4 stripes at 4096: a flip in a data node of an inner grid row (5), in
    a parity node, which lies in the last grid row (13), and in a node of the first grid row (2);
    the last stripe is clean."""
    sites = [(0, 255, 5, 4095, 7), (1, 0, 13, 0, 0), (2, 77, 2, 1000, 3)]
    return build(12, 4, 0, CHUNK, CHUNK, 4, sites, _seed(12, 4, 0, CHUNK, CHUNK), count=2)
