// clay_check_plan.cpp -- see clay_check_plan.hpp.
#include "clay_check_plan.hpp"

#include <algorithm>
#include <string>

namespace ecx {

LinearMap ClayCheckProgram::node_map() const {
    LinearMap mp;
    mp.n_out = m;
    mp.n_in = n_under;
    for (int j = 0; j < n_under; ++j) mp.in_slot.push_back(j);
    for (int p = 0; p < m; ++p) mp.out_slot.push_back(p);
    mp.a.assign((size_t)m * n_under, 0);
    for (int p = 0; p < m; ++p)
        for (int j = 0; j < n_under; ++j) mp.a[(size_t)p * n_under + j] = coef(p, j);
    return mp;
}

LinearMap ClayCheckProgram::compose() const {
    const Field &f = Field::get();
    const int width = n_real * alpha;
    LinearMap mp;
    mp.n_out = m * alpha;
    mp.n_in = width;
    for (int j = 0; j < width; ++j) mp.in_slot.push_back(j);
    for (int o = 0; o < mp.n_out; ++o) mp.out_slot.push_back(o);
    mp.a.assign((size_t)mp.n_out * width, 0);
    std::vector<int> weight(t);  // of digit y in z
    for (int y = t - 1, w = 1; y >= 0; --y, w *= q) weight[y] = w;
    for (int z = 0; z < alpha; ++z)
        for (int p = 0; p < m; ++p) {
            uint8_t *row = mp.a.data() + (size_t)(z * m + p) * width;
            auto add = [&](int zz, int u, uint8_t c) {
                if (real_of[u] >= 0) row[(size_t)zz * n_real + real_of[u]] ^= c;
            };
            for (int j = 0; j < n_under; ++j) {
                const uint8_t c = coef(p, j);
                if (!c) continue;
                const int x = j % q, y = j / q, d = (z / weight[y]) % q;
                if (d == x) {
                    add(z, j, c);
                } else {
                    add(z, j, f.mul(c, pair_a));
                    add(z + (x - d) * weight[y], d + q * y, f.mul(c, pair_b));
                }
            }
        }
    return mp;
}

ClayCheckProgram clay_check_program(const ClayPlanner &pl, bool swap_pair) {
    const int nn = pl.n(), nr = pl.n_real(), m_ = pl.m(), v_ = pl.virtual_units(), k_ = pl.k(), kd = k_ - v_;  // kd real data nodes
    const int q_ = pl.q(), t_ = pl.t(), alpha_ = pl.alpha();
    const RsCode pair_(2, 2), rs_(k_, m_);  // the pair transform and the plane code, as the planner builds them
    if (m_ > kClayCheckMaxParity)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "check program: parity_units " + std::to_string(m_) + " exceeds the " +
                                                std::to_string(kClayCheckMaxParity) + " rows of one accumulator tile");
    if (q_ * t_ != nn || kd <= 0)
        throw Error(ECX_E_ILLEGAL_ARGUMENT, "check program: the nodes do not fill the q x t grid");
    ClayCheckProgram pg;
    pg.q = q_;
    pg.t = t_;
    pg.alpha = alpha_;
    pg.m = m_;
    pg.n_under = nn;
    pg.n_real = nr;
    pg.virtual_units = v_;
    {
        const LinearMap dec = pair_.decode_map({true, true, false, false});  // U from (C, C')
        for (int o = 0; o < dec.n_out; ++o)
            if (dec.out_slot[o] == 2)
                for (int j = 0; j < dec.n_in; ++j) {
                    if (dec.in_slot[j] == 0) pg.pair_a = dec.at(o, j);
                    if (dec.in_slot[j] == 1) pg.pair_b = dec.at(o, j);
                }
    }
    if ((pg.pair_a ^ pg.pair_b) != 1) throw Error(ECX_E_ILLEGAL_ARGUMENT, "pair transform without the dot identity");
    if (swap_pair) std::swap(pg.pair_a, pg.pair_b);
    for (int p = 0; p < m_; ++p) pg.prow.insert(pg.prow.end(), rs_.parity_row(p), rs_.parity_row(p) + k_);
    for (int u = 0; u < nn; ++u) pg.real_of.push_back(u >= kd && u < k_ ? -1 : (u < kd ? u : u - v_));

    // Proof 1: every codeword passes.  E encodes the parity nodes from the data nodes (the
    // reference's stage sequence); the syndromes of [d; E d] must vanish for every d.
    const LinearMap syn = pg.compose();
    std::vector<int> parity;
    for (int p = 0; p < m_; ++p) parity.push_back(kd + p);
    const ClayPlanner enc(kd, m_, parity, v_);
    std::vector<bool> pres((size_t)nr * alpha_, true);
    for (int z = 0; z < alpha_; ++z)
        for (int p : parity) pres[(size_t)z * nr + p] = false;
    const LinearMap E = enc.perform_coding_map(pres);
    if (E.n_out != m_ * alpha_) throw Error(ECX_E_ILLEGAL_ARGUMENT, "check program: unexpected encode map");
    const int width = nr * alpha_, np = m_ * alpha_;
    std::vector<int> pcol(np);  // parity column c = z * m + p of the square block -> input slot
    for (int z = 0; z < alpha_; ++z)
        for (int p = 0; p < m_; ++p) pcol[z * m_ + p] = z * nr + kd + p;
    std::vector<uint8_t> acc(width);
    for (int r = 0; r < np; ++r) {
        const uint8_t *row = syn.a.data() + (size_t)r * width;
        std::copy(row, row + width, acc.begin());
        for (int c = 0; c < np; ++c) {
            const uint8_t s = row[pcol[c]];
            if (!s) continue;
            acc[pcol[c]] = 0;
            if (E.out_slot[c] != c) throw Error(ECX_E_ILLEGAL_ARGUMENT, "check program: unexpected encode order");
            const uint8_t *mul = Field::get().row(s);
            const uint8_t *erow = E.a.data() + (size_t)c * E.n_in;
            for (int j = 0; j < E.n_in; ++j) acc[E.in_slot[j]] ^= mul[erow[j]];
        }
        for (int j = 0; j < width; ++j)
            if (acc[j]) throw Error(ECX_E_ILLEGAL_ARGUMENT, "check program: an encoded stripe has a non-zero syndrome");
    }
    // Proof 2: nothing but codewords passes.  The block of compose() over the parity columns is
    // invertible, so the data nodes leave one parity that zeroes the syndromes: E's.
    std::vector<uint8_t> sq((size_t)np * np);
    for (int r = 0; r < np; ++r)
        for (int c = 0; c < np; ++c) sq[(size_t)r * np + c] = syn.a[(size_t)r * width + pcol[c]];
    const Field &f = Field::get();
    for (int c = 0; c < np; ++c) {
        int piv = c;
        while (piv < np && !sq[(size_t)piv * np + c]) ++piv;
        if (piv == np) throw Error(ECX_E_ILLEGAL_ARGUMENT, "check program: the parity block of the syndrome map is singular");
        if (piv != c) std::swap_ranges(sq.begin() + (size_t)piv * np, sq.begin() + (size_t)(piv + 1) * np, sq.begin() + (size_t)c * np);
        const uint8_t *prow = sq.data() + (size_t)c * np;
        const uint8_t inv = f.div(1, prow[c]);
        for (int r = c + 1; r < np; ++r) {
            uint8_t *rr = sq.data() + (size_t)r * np;
            if (!rr[c]) continue;
            const uint8_t *mul = f.row(f.mul(rr[c], inv));
            for (int j = c; j < np; ++j) rr[j] ^= mul[prow[j]];
        }
    }
    return pg;
}

}  // namespace ecx
