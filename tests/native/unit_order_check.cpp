// unit_order_check.cpp -- the workgroup-to-unit arithmetic of the composed-map kernels
// (csrc/apply.hpp: logical_block, unit_of) walked on the CPU.  Both functions read blockIdx.x and
// gridDim.x themselves, so no host code can call them as they stand; tests/test_native.py cuts
// their text out of apply.hpp, unchanged, into unit_order_slice.inc, and this file compiles that
// text with __device__ / __forceinline__ defined away and blockIdx / gridDim as host variables it
// sets before every call.  What is walked is the kernels' own source, not a copy of it.
//
// A workgroup b of a launch over nst stripes x nc chunks x T tiles computes tile w % T of unit
// unit_of(w / T), w = logical_block(); a mapping that is no bijection leaves a (stripe, chunk, tile)
// unwritten -- stale bytes in the output -- and writes another twice.  For every grid size 1..4096
// the launcher can produce (grid = nst * nc * T) with T in {1, 2, 3, 5, 32}, nc in 1..9, xcd_group
// 0..3 (1 and 2: multi-tile maps only, as launch_rules.cpp passes them), xcd_run in {1, 3, 8, 4096},
// stagger in {0, 2, 3, 8, 64} and chunk_major 0 / 1:
//   1. w = logical_block() is a permutation of 0..grid-1 (it depends on grid, T, xcd_group, xcd_run);
//   2. unit_of is a bijection of 0..nst*nc-1 onto (stripe, chunk) (on nst, nc, stagger, chunk_major);
//   3. (w % T, unit_of(w / T)) hits every (tile, stripe, chunk) exactly once -- which follows from 1
//      and 2, and is walked as written over the full cross product for every grid up to 512 and for
//      the grids 4096 - 8 .. 4096.
// Built with -fsanitize=address,undefined by tests/test_native.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#define __device__
#define __forceinline__ inline
namespace ecx {
struct Dim3 {
    uint32_t x;
};
static Dim3 blockIdx, gridDim;
#include "unit_order_slice.inc"
// workgroup b of a grid of g
static uint32_t logical_block_of(uint32_t b, uint32_t g, int xcd_group, uint32_t n_tiles, uint32_t run) {
    blockIdx.x = b;
    gridDim.x = g;
    return logical_block(xcd_group, n_tiles, run);
}
}  // namespace ecx

namespace {
constexpr uint32_t kMaxGrid = 4096, kComposedMax = 512;
const uint32_t kTiles[] = {1, 2, 3, 5, 32};
const uint32_t kRuns[] = {1, 3, 8, 4096};
const uint32_t kStaggers[] = {0, 2, 3, 8, 64};

long failures = 0, walked = 0;

void fail(const char *what, uint32_t grid, uint32_t T, int xg, uint32_t run, uint32_t nc, uint32_t G, int cm, uint32_t at) {
    if (++failures <= 10)
        std::printf("FAIL %s: grid=%u T=%u xcd_group=%d xcd_run=%u nc=%u stagger=%u chunk_major=%d at %u\n", what, grid, T,
                    xg, run, nc, G, cm, at);
}

// 1: logical_block over the grid is a permutation
bool blocks_ok(uint32_t grid, uint32_t T, int xg, uint32_t run, std::vector<uint8_t> &seen) {
    seen.assign(grid, 0);
    for (uint32_t b = 0; b < grid; ++b) {
        const uint32_t w = ecx::logical_block_of(b, grid, xg, T, run);
        if (w >= grid || seen[w]++) {
            fail("logical_block", grid, T, xg, run, 0, 0, 0, b);
            return false;
        }
    }
    ++walked;
    return true;
}

// 2: unit_of over nst * nc units is a bijection onto (stripe, chunk)
bool units_ok(uint32_t nst, uint32_t nc, int cm, uint32_t G, std::vector<uint8_t> &seen) {
    const uint32_t units = nst * nc;
    seen.assign(units, 0);
    for (uint32_t u = 0; u < units; ++u) {
        int64_t s = -1, c = -1;
        ecx::unit_of(u, nc, nst, cm, G, s, c);
        if (s < 0 || s >= nst || c < 0 || c >= nc || seen[s * nc + c]++) {
            fail("unit_of", units, 1, 0, 0, nc, G, cm, u);
            return false;
        }
    }
    ++walked;
    return true;
}

// 3: the composition, as the kernels compute it (apply.hpp apply_unit)
bool composed_ok(uint32_t grid, uint32_t T, int xg, uint32_t run, uint32_t nc, int cm, uint32_t G, std::vector<uint8_t> &seen) {
    const uint32_t nst = grid / (T * nc);
    seen.assign(grid, 0);
    for (uint32_t b = 0; b < grid; ++b) {
        const uint32_t w = ecx::logical_block_of(b, grid, xg, T, run);
        const uint32_t tl = w % T, rest = w / T;
        int64_t s = -1, c = -1;
        ecx::unit_of(rest, nc, nst, cm, G, s, c);
        if (w >= grid || s < 0 || s >= nst || c < 0 || c >= nc || seen[((uint64_t)s * nc + c) * T + tl]++) {
            fail("composed", grid, T, xg, run, nc, G, cm, b);
            return false;
        }
    }
    ++walked;
    return true;
}
}  // namespace

int main() {
    std::vector<uint8_t> seen;
    for (uint32_t grid = 1; grid <= kMaxGrid; ++grid) {
        const bool composed = grid <= kComposedMax || grid + 8 >= kMaxGrid;
        for (uint32_t T : kTiles) {
            if (grid % T) continue;
            const uint32_t units = grid / T;
            for (int xg = 0; xg <= 3; ++xg) {
                if (T == 1 && (xg == 1 || xg == 2)) continue;  // single-tile maps run 0 or 3 (launch_rules.cpp)
                for (uint32_t run : kRuns) {
                    if (xg != 3 && run != kRuns[0]) continue;  // only xcd_group 3 reads the run
                    blocks_ok(grid, T, xg, run, seen);
                    if (!composed) continue;
                    for (uint32_t nc = 1; nc <= 9; ++nc) {
                        if (units % nc) continue;
                        for (uint32_t G : kStaggers)
                            for (int cm = 0; cm <= 1; ++cm) composed_ok(grid, T, xg, run, nc, cm, G, seen);
                    }
                }
            }
        }
        for (uint32_t nc = 1; nc <= 9; ++nc) {  // grid as the unit count nst * nc of a one-tile launch
            if (grid % nc) continue;
            for (uint32_t G : kStaggers)
                for (int cm = 0; cm <= 1; ++cm) units_ok(grid / nc, nc, cm, G, seen);
        }
    }
    if (failures) {
        std::printf("unit_order_check: %ld of the walked mappings are no bijection\n", failures);
        return 1;
    }
    std::printf("unit_order_check: ok (%ld mappings walked)\n", walked);
    return 0;
}
