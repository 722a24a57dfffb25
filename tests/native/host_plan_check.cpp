// host_plan_check.cpp -- the plans of the host-memory batches (csrc/host_plan.cpp), on the CPU:
// built from that one file with no ROCm include path (tests/test_host_plan_native.py).
//
// A plan is expanded into the rows it would move -- (host offset, device offset, length) triples:
// a 2D copy is n * rows rows at its two pitches, continuing across stripes; row r of stripe t of
// a 3D copy sits at off + r * pitch + t * stripe, and the stripe must be a multiple of the pitch
// on both sides (the pitched pointer's height is that quotient) -- and compared with the plain
// definition: for every stripe t of a chunk and every used slot with compact index c, nbytes
// bytes go from host t * stripe_stride + slot * slot_stride to device t * per + c * nbytes (the
// mixed plan: c = slot, per = n * nbytes; a slice: bytes [c0, c0 + w) of each such slot, to
// device (t * used + c) * w).  Both sides are merged where rows are adjacent on host and device,
// so an exact match means every used byte moves exactly once and nothing else moves.  On top of
// that: chunks tile the stripes, slices tile the slot in 4 KiB multiples, the ring is within its
// bounds, the chunk floor holds, stripe_range tiles in order and the column split happens exactly
// when it should.  Fixed cases repeat the ones tests/test_host_plan.py pins through the library
// (the slot lists are those its docstrings describe); seeded random cases run under all of it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>

#include "../../repair-pipelining_amd/csrc/host_plan.hpp"

using namespace ecx;

static long g_checks = 0;
#define REQUIRE(c)                                                              \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

using Row = std::tuple<int64_t, int64_t, int64_t>;  // host offset, device offset, length

// sorted by host offset, rows that continue one another on both sides joined; no host byte twice
static std::vector<Row> merged(std::vector<Row> rows) {
    std::sort(rows.begin(), rows.end());
    std::vector<Row> out;
    for (const Row &r : rows) {
        REQUIRE(std::get<2>(r) > 0);
        if (!out.empty()) {
            Row &b = out.back();
            REQUIRE(std::get<0>(b) + std::get<2>(b) <= std::get<0>(r));  // no byte twice
            if (std::get<0>(b) + std::get<2>(b) == std::get<0>(r) && std::get<1>(b) + std::get<2>(b) == std::get<1>(r)) {
                std::get<2>(b) += std::get<2>(r);
                continue;
            }
        }
        out.push_back(r);
    }
    // nor a device byte
    std::vector<std::pair<int64_t, int64_t>> dev;
    for (const Row &r : out) dev.push_back({std::get<1>(r), std::get<2>(r)});
    std::sort(dev.begin(), dev.end());
    for (size_t i = 1; i < dev.size(); ++i) REQUIRE(dev[i - 1].first + dev[i - 1].second <= dev[i].first);
    return out;
}

// what issue_copy moves for the n stripes of a chunk
static std::vector<Row> rows_of(const std::vector<Copy> &cs, int64_t host_stripe, int64_t dev_stripe, int64_t n) {
    std::vector<Row> rows;
    for (const Copy &c : cs) {
        REQUIRE(c.width > 0 && c.rows >= 1 && c.host_off >= 0 && c.dev_off >= 0);
        if (c.three_d) {
            REQUIRE(c.host_pitch > 0 && c.dev_pitch > 0);
            REQUIRE(host_stripe % c.host_pitch == 0 && dev_stripe % c.dev_pitch == 0);
            REQUIRE(c.rows <= host_stripe / c.host_pitch && c.rows <= dev_stripe / c.dev_pitch);
            for (int64_t t = 0; t < n; ++t)
                for (int64_t r = 0; r < c.rows; ++r)
                    rows.push_back({c.host_off + r * c.host_pitch + t * host_stripe,
                                    c.dev_off + r * c.dev_pitch + t * dev_stripe, c.width});
        } else {
            for (int64_t r = 0; r < n * c.rows; ++r)
                rows.push_back({c.host_off + r * c.host_pitch, c.dev_off + r * c.dev_pitch, c.width});
        }
    }
    return rows;
}

// what issue_sliced moves for bytes [c0, c0 + w) of the n stripes (host offsets include c0)
static std::vector<Row> sliced_rows_of(const std::vector<Run> &runs, const std::vector<Segment> &segs,
                                       int64_t host_stripe, int64_t slot_stride, int64_t used, int64_t n, int64_t c0,
                                       int64_t w) {
    std::vector<Row> rows;
    size_t next = 0;
    for (const Segment &g : segs) {  // the progressions partition the runs, in order
        REQUIRE(g.i == next && g.j >= g.i && g.j < runs.size());
        next = g.j + 1;
    }
    REQUIRE(next == runs.size());
    for (int64_t t = 0; t < n; ++t)
        for (const Segment &g : segs) {
            const Run &r = runs[g.i];
            const int64_t host = c0 + t * host_stripe + r.slot0 * slot_stride, dev = (t * used + r.compact0) * w;
            if (g.j > g.i) REQUIRE(g.ds >= r.len && g.dc >= r.len);  // the 3D copy's height holds its rows
            for (size_t k = g.i; k <= g.j; ++k) {
                REQUIRE(runs[k].len == r.len);
                // 3D: plane k - g.i is ds slots (host) and dc slots (device) on; the fallback
                // addresses run k by its own slots -- the two must agree
                REQUIRE(runs[k].slot0 - r.slot0 == (int64_t)(k - g.i) * g.ds);
                REQUIRE(runs[k].compact0 - r.compact0 == (int64_t)(k - g.i) * g.dc);
                for (int q = 0; q < runs[k].len; ++q)
                    rows.push_back({host + ((int64_t)(k - g.i) * g.ds + q) * slot_stride,
                                    dev + ((int64_t)(k - g.i) * g.dc + q) * w, w});
            }
        }
    return rows;
}

// the definition: bytes [c0, c0 + w) of slot i (compact index c) of each of n stripes
static std::vector<Row> defined_rows(const std::vector<int> &slots, bool compacted, int64_t stripe_stride,
                                     int64_t slot_stride, int64_t dev_stripe, int64_t dev_slot, int64_t n, int64_t c0,
                                     int64_t w) {
    std::vector<Row> rows;
    for (int64_t t = 0; t < n; ++t)
        for (size_t i = 0; i < slots.size(); ++i) {
            const int64_t c = compacted ? (int64_t)i : slots[i];
            rows.push_back({c0 + t * stripe_stride + slots[i] * slot_stride, t * dev_stripe + c * dev_slot, w});
        }
    return rows;
}

// the ring's depth over `ring_units` chunks or slices
static void check_ring(int nb, int host_buffers, int64_t ring_units) {
    REQUIRE(nb >= 1 && nb <= std::min(8, std::max(1, host_buffers)) && nb <= ring_units);
}

static void check_chunking(int64_t chunk, int64_t nchunks, int64_t up_per, size_t ncopies, int64_t units,
                           int64_t host_chunk) {
    REQUIRE(chunk >= 1 && nchunks >= 1);  // chunks of `chunk`, the last one shorter, tile [0, units)
    REQUIRE((nchunks - 1) * chunk < units && nchunks * chunk >= units);
    const int64_t base = std::max<int64_t>(1, std::min(units, host_chunk / up_per));
    REQUIRE(chunk >= base);
    if (chunk > base) {
        REQUIRE(ncopies > 8);
        REQUIRE(chunk <= std::min(units, std::min<int64_t>(160, 8 * host_chunk / up_per)));
    }
}

struct Layout {
    std::vector<int> ins, outs;
    int64_t in_ss, in_slot, out_ss, out_slot, nstripes, nbytes, host_chunk;
    int host_buffers;
};

static Plan check_uniform(const Layout &L, bool outputs) {
    const Plan pl = make_plan(L.ins, L.outs, L.in_ss, L.in_slot, L.out_ss, L.out_slot, L.nstripes, L.nbytes, outputs,
                              L.host_chunk, L.host_buffers);
    const int64_t used_in = (int64_t)L.ins.size(), used_out = outputs ? (int64_t)L.outs.size() : 0;
    REQUIRE(pl.in_per == used_in * L.nbytes && pl.out_per == used_out * L.nbytes);
    check_chunking(pl.chunk, pl.nchunks, pl.in_per, pl.cin.size(), L.nstripes, L.host_chunk);
    check_ring(pl.nb, L.host_buffers, pl.nslices > 1 ? pl.nslices : pl.nchunks);
    if (!outputs) REQUIRE(pl.cout.empty() && pl.nslices == 1);
    // every chunk length that occurs: full chunks and the last one
    const int64_t last = L.nstripes - (pl.nchunks - 1) * pl.chunk;
    for (int64_t n : {pl.chunk, last}) {
        REQUIRE(n >= 1 && n <= pl.chunk);
        REQUIRE(merged(rows_of(pl.cin, L.in_ss, pl.in_per, n)) ==
                merged(defined_rows(L.ins, true, L.in_ss, L.in_slot, pl.in_per, L.nbytes, n, 0, L.nbytes)));
        if (outputs)
            REQUIRE(merged(rows_of(pl.cout, L.out_ss, pl.out_per, n)) ==
                    merged(defined_rows(L.outs, true, L.out_ss, L.out_slot, pl.out_per, L.nbytes, n, 0, L.nbytes)));
    }
    const bool want_slices = outputs && pl.nchunks == 1 && L.nbytes >= 8192 && L.nstripes * pl.in_per >= 4 * L.host_chunk;
    REQUIRE((pl.nslices > 1) == want_slices);
    if (pl.nslices > 1) {
        REQUIRE(pl.slice > 0 && pl.slice % 4096 == 0);  // every slice but the last is `slice` bytes
        REQUIRE((pl.nslices - 1) * pl.slice < L.nbytes && pl.nslices * pl.slice >= L.nbytes);
        for (int64_t s = 0; s < pl.nslices; ++s) {
            const int64_t c0 = s * pl.slice, w = std::min(pl.slice, L.nbytes - c0);
            REQUIRE(w > 0);
            REQUIRE(merged(sliced_rows_of(pl.rin, pl.sin, L.in_ss, L.in_slot, used_in, L.nstripes, c0, w)) ==
                    merged(defined_rows(L.ins, true, L.in_ss, L.in_slot, used_in * w, w, L.nstripes, c0, w)));
            REQUIRE(merged(sliced_rows_of(pl.rout, pl.sout, L.out_ss, L.out_slot, used_out, L.nstripes, c0, w)) ==
                    merged(defined_rows(L.outs, true, L.out_ss, L.out_slot, used_out * w, w, L.nstripes, c0, w)));
        }
    }
    return pl;
}

static void check_mixed(const std::vector<int> &up, const std::vector<int> &down, int n, int64_t ss, int64_t slot,
                        int64_t units, int64_t nbytes, int64_t host_chunk, int host_buffers) {
    const HostMixedPlan mp = make_mixed_plan(up, down, ss, slot, n, units, nbytes, host_chunk, host_buffers);
    REQUIRE(mp.per == (int64_t)n * nbytes);
    check_chunking(mp.chunk, mp.nchunks, (int64_t)up.size() * nbytes, mp.cin.size(), units, host_chunk);
    check_ring(mp.nb, host_buffers, mp.nchunks);
    const int64_t last = units - (mp.nchunks - 1) * mp.chunk;
    for (int64_t cnt : {mp.chunk, last}) {
        REQUIRE(merged(rows_of(mp.cin, ss, mp.per, cnt)) ==
                merged(defined_rows(up, false, ss, slot, mp.per, nbytes, cnt, 0, nbytes)));
        REQUIRE(merged(rows_of(mp.cout, ss, mp.per, cnt)) ==
                merged(defined_rows(down, false, ss, slot, mp.per, nbytes, cnt, 0, nbytes)));
    }
}

static void check_split(int64_t nstripes, int parts) {
    int64_t at = 0, prev = -1;
    for (int j = 0; j < parts; ++j) {
        int64_t b = -1, e = -1;
        stripe_range(nstripes, parts, j, &b, &e);
        REQUIRE(b == at && e >= b);
        if (prev >= 0) REQUIRE(e - b == prev || e - b == prev - 1);  // larger ones first
        prev = e - b;
        at = e;
    }
    REQUIRE(at == nstripes);
    REQUIRE(prev >= nstripes / parts);  // sizes differ by at most 1: the smallest is the floor
}

static void check_columns(int64_t nstripes, int ndev, int64_t nbytes) {
    const int64_t units = column_units(nstripes, ndev, nbytes);
    REQUIRE((units > 0) == (0 < nstripes && nstripes < ndev && nbytes >= 8192));
    if (!units) return;
    REQUIRE((units - 1) * kColUnit < nbytes && units * kColUnit >= nbytes);  // the units tile [0, nbytes)
    int64_t at = 0;
    for (int j = 0; j < ndev; ++j) {  // as the _devices batches cut them
        int64_t u0 = 0, u1 = 0;
        stripe_range(units, ndev, j, &u0, &u1);
        if (u1 <= u0) continue;
        const int64_t c0 = u0 * kColUnit, w = std::min((u1 - u0) * kColUnit, nbytes - c0);
        REQUIRE(c0 == at && w > 0);
        at += w;
    }
    REQUIRE(at == nbytes);
}

static std::vector<int> iota(int lo, int hi) {  // lo..hi inclusive
    std::vector<int> v;
    for (int i = lo; i <= hi; ++i) v.push_back(i);
    return v;
}

static std::vector<int> random_slots(std::mt19937_64 &rng, int *total) {
    std::vector<int> v;
    const int kind = (int)(rng() % 4);
    if (kind == 0) {  // any sorted subset
        const int span = 1 + (int)(rng() % 256), want = 1 + (int)(rng() % 64);
        for (int i = 0; i < span; ++i)
            if ((int)(rng() % (uint64_t)span) < want && (int)v.size() < 64) v.push_back(i);
        if (v.empty()) v.push_back((int)(rng() % (uint64_t)span));
        *total = span;
        return v;
    }
    // runs of `len` at `step`, `reps` times; exact (folds), or with a hole, or with an extra run
    const int len = 1 + (int)(rng() % 4), step = len + (int)(rng() % 4), reps = 1 + (int)(rng() % (uint64_t)(64 / len));
    const int lead = (int)(rng() % (uint64_t)(step - len + 1));
    for (int r = 0; r < reps; ++r)
        for (int q = 0; q < len; ++q) v.push_back(lead + r * step + q);
    *total = reps * step;
    if (kind == 2 && v.size() > 1) v.erase(v.begin() + (long)(rng() % v.size()));  // a hole
    if (kind == 3 && (int)v.size() + len <= 64) {                                  // an extra run behind
        const int gap = 1 + (int)(rng() % 3);
        for (int q = 0; q < len; ++q) v.push_back(*total + gap + q);
        *total += gap + len + (int)(rng() % 3);
    }
    return v;
}

int main() {
    const int64_t MiB = 1 << 20;
    // Clay(4,2) node 1: planes 4-7 without node 1 (tests/test_host_plan.py)
    std::vector<int> node1 = {24};
    for (int lo : {26, 32, 38}) for (int i = lo; i < lo + 5; ++i) node1.push_back(i);
    for (int i = 44; i < 48; ++i) node1.push_back(i);
    REQUIRE(node1.size() == 20);
    std::vector<int> periodic;  // Clay(4,2) {0,3}: nodes 1-2 and 4-5 of all 8 planes
    for (int i = 0; i < 16; ++i) periodic.push_back(3 * i + 1), periodic.push_back(3 * i + 2);
    const std::vector<int> out8 = iota(0, 7), out16 = iota(0, 15);

    {  // the headline's e2e leg
        const int64_t B = 32768;
        const Layout L{node1, out8, 48 * B, B, 8 * B, B, 2048, B, 64 * MiB, 3};
        const Plan pl = check_uniform(L, true);
        REQUIRE(pl.cin.size() == 3 && pl.chunk == 102 && pl.nchunks == 21 && pl.nb == 3 && pl.nslices == 1);
        int n3d = 0;
        for (const Copy &c : pl.cin) {
            n3d += c.three_d;
            REQUIRE(c.rows == (c.three_d ? 3 : 1));
        }
        REQUIRE(n3d == 1 && pl.cout.size() == 1 && !pl.cout[0].three_d && pl.cout[0].rows == 1);
        const HostBatchPlan hp = host_batch_plan(L.ins, L.outs, L.in_ss, L.in_slot, L.out_ss, L.out_slot, L.nstripes,
                                                 L.nbytes, L.host_chunk, L.host_buffers);
        REQUIRE(hp.chunk == 102 && hp.nchunks == 21 && hp.buffers == 3 && hp.h2d_copies == 3 && hp.h2d_rows == 3 &&
                hp.d2h_copies == 1 && hp.d2h_rows == 1 && hp.h2d_3d == 1 && hp.d2h_3d == 0 && hp.slices == 1);
        check_uniform(L, false);  // the same slots as a check
    }
    {  // periodic runs fold into one 2D copy
        const int64_t B = 32768;
        const Plan pl = check_uniform({periodic, out16, 48 * B, B, 16 * B, B, 2048, B, 64 * MiB, 3}, true);
        REQUIRE(pl.cin.size() == 1 && pl.cin[0].rows == 16 && !pl.cin[0].three_d);
        REQUIRE(pl.chunk == 64 && pl.nchunks == 32);
    }
    {  // a padded pitch reading every slot: one run per slot folds; back to back they are one run
        const Plan p = check_uniform({iota(0, 5), {0}, 6144, 1024, 1000, 1000, 50, 1000, 64 * MiB, 3}, true);
        REQUIRE(p.cin.size() == 1 && p.cin[0].rows == 6 && p.cout.size() == 1 && p.cout[0].rows == 1);
        const Plan q = check_uniform({iota(0, 5), {0}, 6000, 1000, 1000, 1000, 50, 1000, 64 * MiB, 3}, true);
        REQUIRE(q.cin.size() == 1 && q.cin[0].rows == 1);
    }
    {  // small chunks: one stripe per chunk and a full ring
        const int64_t B = 2048;
        const Plan pl = check_uniform({node1, out8, 48 * B, B, 8 * B, B, 7, B, 16384, 3}, true);
        REQUIRE(pl.chunk == 1 && pl.nchunks == 7 && pl.nb == 3);
    }
    {  // one huge stripe: column slices
        const Layout L{node1, out8, 48 * MiB, MiB, 8 * MiB, MiB, 1, MiB, 4 * MiB, 3};
        const Plan pl = check_uniform(L, true);
        REQUIRE(pl.nchunks == 1 && pl.slice == 212992 && pl.nslices == 5 && pl.nb == 3);
        const HostBatchPlan hp = host_batch_plan(L.ins, L.outs, L.in_ss, L.in_slot, L.out_ss, L.out_slot, 1, MiB,
                                                 L.host_chunk, 3);
        REQUIRE(hp.slices == 5 && hp.buffers == 3 && hp.nchunks == 1 && hp.h2d_copies == 3 && hp.d2h_copies == 1);
        REQUIRE(check_uniform(L, false).nslices == 1);  // a check is never sliced
    }
    for (int64_t S : {0, 5})  // empty batches: all zero
        for (int64_t B : {0, 2048}) {
            if (S > 0 && B > 0) continue;
            const HostBatchPlan hp = host_batch_plan(node1, out8, 48 * B, B, 8 * B, B, S, B, 64 * MiB, 3);
            REQUIRE(hp.chunk == 0 && hp.nchunks == 0 && hp.buffers == 0 && hp.h2d_copies == 0 && hp.h2d_rows == 0 &&
                    hp.d2h_copies == 0 && hp.d2h_rows == 0 && hp.h2d_3d == 0 && hp.d2h_3d == 0 && hp.slices == 0);
        }
    // the mixed decode of RS(4,2): 7 one-stripe chunks of all six shards, three of them coming back
    check_mixed(iota(0, 5), {1, 4, 5}, 6, 6 * 4096, 4096, 7, 4096, 16384, 2);

    std::mt19937_64 rng(20261020);
    for (int r = 0; r < 2500; ++r) {
        int in_total = 0, out_total = 0;
        Layout L;
        L.ins = random_slots(rng, &in_total);
        L.outs = random_slots(rng, &out_total);
        L.nbytes = 1 + (int64_t)(rng() % (r % 8 == 0 ? 20000 : 3000));
        L.in_slot = L.nbytes + (rng() % 2 ? 0 : (int64_t)(rng() % 200));
        L.out_slot = L.nbytes + (rng() % 2 ? 0 : (int64_t)(rng() % 200));
        L.in_ss = in_total * L.in_slot + (rng() % 2 ? 0 : (int64_t)(rng() % 500));
        L.out_ss = out_total * L.out_slot + (rng() % 2 ? 0 : (int64_t)(rng() % 500));
        L.nstripes = 1 + (int64_t)(rng() % 400);
        L.host_chunk = 4096 << (rng() % 9);  // 4 KiB .. 1 MiB
        L.host_buffers = (int)(rng() % 10);
        if (r % 8 == 0) L.nstripes = 1 + (int64_t)(rng() % 3);  // few large stripes: slices
        check_uniform(L, true);
        check_uniform(L, false);
        // the same host layout decoded in place: down within up, every slot on the device
        std::vector<int> down;
        for (int s : L.ins)
            if (rng() % 3 == 0) down.push_back(s);
        if (down.empty()) down.push_back(L.ins[rng() % L.ins.size()]);
        check_mixed(L.ins, down, in_total, L.in_ss, L.in_slot, L.nstripes, L.nbytes, L.host_chunk, L.host_buffers);
    }

    for (int64_t S : {0, 1, 2, 7, 8, 9, 219, 2048, 100003})
        for (int parts : {1, 2, 3, 7, 8, 16}) check_split(S, parts);
    for (int r = 0; r < 2000; ++r) check_split((int64_t)(rng() % 5000), 1 + (int)(rng() % 40));
    for (int64_t S : {-1, 0, 1, 2, 3, 7, 8, 9})
        for (int ndev : {1, 2, 3, 8})
            for (int64_t B : {0, 1, 4096, 8191, 8192, 8193, 12288, 100000, 1 << 20}) check_columns(S, ndev, B);
    for (int r = 0; r < 2000; ++r)
        check_columns((int64_t)(rng() % 12), 1 + (int)(rng() % 16), (int64_t)(rng() % 200000));

    std::printf("host_plan_check: ok (%ld checks)\n", g_checks);
    return 0;
}
