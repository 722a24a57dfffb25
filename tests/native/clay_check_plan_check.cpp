// clay_check_plan_check.cpp -- clay_check_program (csrc/clay_check_plan.cpp) on the CPU: for
// Clay(2,2), (4,2), (6,3), (12,4) and the shortened (10,4) the program proves itself (an encoded
// stripe has zero syndromes, and the parity block of the syndrome map is invertible), its dense
// map has at most 2 * n_under - t entries per row, its node map has one column per underlying
// node; a program with pair_a and pair_b exchanged, a geometry with more parity units than one
// accumulator tile has rows, and a geometry that does not fill the grid are refused.  For the
// geometries with alpha <= 27 the dense map is also run on bytes: a stripe encoded with the
// planner's own perform_coding_map passes, and a bit flip in every (plane, node) sub-chunk fails.
// Built from this file, clay_check_plan.cpp, codes.cpp and gf.cpp alone (tests/test_clay_check_plan_native.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../repair-pipelining_amd/csrc/clay_check_plan.hpp"

using namespace ecx;

namespace {
int g_fail = 0;
void expect(bool ok, const std::string &what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what.c_str());
        ++g_fail;
    }
}

std::vector<uint8_t> run_map(const LinearMap &m, const std::vector<uint8_t> &in) {
    const Field &f = Field::get();
    std::vector<uint8_t> out(m.n_out, 0);
    for (int o = 0; o < m.n_out; ++o)
        for (int j = 0; j < m.n_in; ++j)
            if (m.at(o, j)) out[o] ^= f.mul(m.at(o, j), in[m.in_slot[j]]);
    return out;
}

void geometry(int k, int mm, int v) {
    const std::string name = "Clay(" + std::to_string(k) + "," + std::to_string(mm) + ")" + (v ? " v=" + std::to_string(v) : "");
    const ClayPlanner pl(k, mm, {}, v);
    const auto t0 = std::chrono::steady_clock::now();
    ClayCheckProgram pg;
    try {
        pg = clay_check_program(pl);
    } catch (const Error &e) {
        expect(false, name + ": check_program refused: " + e.what());
        return;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    expect(pg.pair_a == 3 && pg.pair_b == 2, name + ": (pair_a, pair_b) is (3, 2)");
    expect(pg.q == pl.q() && pg.t == pl.t() && pg.alpha == pl.alpha() && pg.n_real == pl.n_real() && pg.n_under == pl.n(),
           name + ": geometry");
    const LinearMap syn = pg.compose();
    expect(syn.n_out == pg.m * pg.alpha && syn.n_in == pg.n_real * pg.alpha, name + ": compose() shape");
    int widest = 0;
    for (int o = 0; o < syn.n_out; ++o) {
        int nz = 0;
        for (int j = 0; j < syn.n_in; ++j) nz += syn.at(o, j) != 0;
        widest = nz > widest ? nz : widest;
    }
    expect(widest <= 2 * pg.n_under - pg.t, name + ": at most 2 * n_under - t entries per row");
    const LinearMap nm = pg.node_map();
    expect(nm.n_out == pg.m && nm.n_in == pg.n_under, name + ": node map shape");
    for (int j = 0; j < nm.n_in; ++j) {
        int nz = 0;
        for (int p = 0; p < nm.n_out; ++p) nz += nm.at(p, j) != 0;
        expect(nz >= 1, name + ": every node has a coefficient");
    }
    bool swapped_refused = false;
    try {
        (void)clay_check_program(pl, true);
    } catch (const Error &e) {
        swapped_refused = e.code == ECX_E_ILLEGAL_ARGUMENT;
    }
    expect(swapped_refused, name + ": the program with pair_a and pair_b exchanged is refused");
    std::printf("%s n_real=%d alpha=%d: proved in %.0f ms, widest row %d of %d\n", name.c_str(), pg.n_real, pg.alpha, ms,
                widest, 2 * pg.n_under - pg.t);
    if (pg.alpha > 27) return;
    // bytes: encode with the planner, flip every sub-chunk
    const int nr = pg.n_real, kd = nr - pg.m, w = nr * pg.alpha;
    std::vector<int> parity;
    for (int p = 0; p < pg.m; ++p) parity.push_back(kd + p);
    const ClayPlanner enc(k, mm, parity, v);
    std::vector<bool> pres(w, true);
    for (int z = 0; z < pg.alpha; ++z)
        for (int p : parity) pres[z * nr + p] = false;
    const LinearMap E = enc.perform_coding_map(pres);
    std::vector<uint8_t> stripe(w, 0);
    uint32_t rng = 12345u + (uint32_t)k * 131u + (uint32_t)mm;
    for (int z = 0; z < pg.alpha; ++z)
        for (int d = 0; d < kd; ++d) {
            rng = rng * 1664525u + 1013904223u;
            stripe[z * nr + d] = (uint8_t)(rng >> 24);
        }
    const std::vector<uint8_t> par = run_map(E, stripe);
    for (int z = 0; z < pg.alpha; ++z)
        for (int p = 0; p < pg.m; ++p) stripe[z * nr + kd + p] = par[z * pg.m + p];
    auto clean = [&](const std::vector<uint8_t> &s) {
        for (uint8_t b : run_map(syn, s))
            if (b) return false;
        return true;
    };
    expect(clean(stripe), name + ": an encoded stripe passes");
    int missed = 0;
    for (int slot = 0; slot < w; ++slot) {
        std::vector<uint8_t> bad = stripe;
        bad[slot] ^= (uint8_t)(1u << (slot % 8));
        missed += clean(bad);
    }
    expect(missed == 0, name + ": a bit flip in every (plane, node) sub-chunk fails (" + std::to_string(missed) + " missed)");
}

void refused(int k, int mm, int v, const char *why) {
    bool ok = false;
    try {
        (void)clay_check_program(ClayPlanner(k, mm, {}, v));
    } catch (const Error &e) {
        ok = e.code == ECX_E_ILLEGAL_ARGUMENT;
    }
    expect(ok, std::string(why) + " is refused with ECX_E_ILLEGAL_ARGUMENT");
}
}  // namespace

int main() {
    geometry(2, 2, 0);
    geometry(4, 2, 0);
    geometry(6, 3, 0);
    geometry(12, 4, 0);
    geometry(10, 4, 2);
    refused(9, 9, 0, "Clay(9,9): parity_units > kClayCheckMaxParity");
    refused(5, 2, 0, "Clay(5,2): seven nodes on a 2 x 3 grid");
    if (g_fail) {
        std::printf("clay_check_plan_check: %d failure(s)\n", g_fail);
        return 1;
    }
    std::printf("clay_check_plan_check: ok\n");
    return 0;
}
