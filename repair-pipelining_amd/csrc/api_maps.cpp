// api_maps.cpp -- the maps and rules of the C ABI's entry points (api_maps.hpp).
#include "api_maps.hpp"

#include <algorithm>
#include <cstring>
#include <map>

namespace ecx {

std::vector<bool> present_vec(const uint8_t *p, int n) {
    std::vector<bool> v(n);
    for (int i = 0; i < n; ++i) v[i] = p[i] != 0;
    return v;
}

LinearMap dense_map(const uint8_t *m, int n_out, int n_in) {
    LinearMap lm;
    lm.n_out = n_out;
    lm.n_in = n_in;
    lm.a.assign(m, m + (size_t)n_out * n_in);
    for (int j = 0; j < n_in; ++j) lm.in_slot.push_back(j);
    for (int o = 0; o < n_out; ++o) lm.out_slot.push_back(o);
    return lm;
}

LinearMap check_map(const uint8_t *rows, int n_out, int n_in) {
    const int w = n_in + n_out;
    std::vector<uint8_t> a((size_t)n_out * w, 0);
    for (int o = 0; o < n_out; ++o) {
        std::memcpy(&a[(size_t)o * w], rows + (size_t)o * n_in, (size_t)n_in);
        a[(size_t)o * w + n_in + o] = 1;
    }
    return dense_map(a.data(), n_out, w).pruned();
}

// (the parity rows are the generator matrix's last m, one after the other)
LinearMap rs_check_map(const RsCode &c) { return check_map(c.parity_row(0), c.m(), c.k()); }

LinearMap single_input_map(const LinearMap &m, int column_slot) {
    int col = -1;
    for (int j = 0; j < m.n_in; ++j)
        if (m.in_slot[j] == column_slot) col = j;
    std::vector<uint8_t> a;
    for (int o = 0; o < m.n_out; ++o) a.push_back(col < 0 ? 0 : m.at(o, col));
    return dense_map(a.data(), m.n_out, 1);
}

LinearMap encode_partial_map(const RsCode &c, int input_index) {
    std::vector<uint8_t> a;
    for (int p = 0; p < c.m(); ++p) a.push_back(c.parity_row(p)[input_index]);
    return dense_map(a.data(), c.m(), 1);
}

LinearMap decode_single_map(const RsCode &c, const std::vector<bool> &present, int index, int output_count,
                            bool is_first) {
    int np = 0;
    for (bool b : present) np += b;
    // fewer than k present leaves zero rows in the sub-matrix: "Matrix is singular"
    if (np < c.k()) throw Error(ECX_E_SINGULAR, "Matrix is singular");
    const Matrix dec = c.data_decoder(present, nullptr);
    std::vector<int> missing;
    for (int i = 0; i < c.k(); ++i)
        if (!present[i]) missing.push_back(i);
    if (output_count > c.m() || (int)missing.size() > c.m()) throw Error(ECX_E_INDEX, "matrixRows index");
    if (output_count > (int)missing.size()) throw Error(ECX_E_NULL, "no decode row for this output (no missing data shard)");
    if (index < 0 || index >= c.k()) throw Error(ECX_E_INDEX, "matrix column index");
    const int w = 1 + std::max(output_count, 0);
    std::vector<uint8_t> a((size_t)(w - 1) * w, 0);
    for (int j = 0; j < w - 1; ++j) {
        a[(size_t)j * w] = dec.at(missing[j], index);
        if (!is_first) a[(size_t)j * w + 1 + j] = 1;
    }
    return dense_map(a.data(), w - 1, w).pruned();
}

LinearMap scale_map(uint8_t c, bool accumulate) {
    const uint8_t row[2] = {c, (uint8_t)(accumulate ? 1 : 0)};
    return dense_map(row, 1, 2);
}

std::string map_key(const LinearMap &m) {
    std::string key;
    key.reserve(sizeof(int) * (2 + m.in_slot.size() + m.out_slot.size()) + m.a.size());
    auto put = [&](const void *p, size_t n) { key.append(static_cast<const char *>(p), n); };
    put(&m.n_out, sizeof(int));  // the shape first: it says where the slots and the coefficients begin
    put(&m.n_in, sizeof(int));
    put(m.in_slot.data(), m.in_slot.size() * sizeof(int));
    put(m.out_slot.data(), m.out_slot.size() * sizeof(int));
    put(m.a.data(), m.a.size());
    return key;
}

int64_t recommended_pitch(int64_t byte_count) {
    constexpr int64_t kStep = 4 << 10;
    int64_t c = (byte_count + kStep - 1) / kStep;
    if (c % 2 == 0 && c > 0) ++c;
    return c * kStep;
}

bool extent_fits(std::initializer_list<std::pair<int64_t, int64_t>> dims, int64_t bytes) {
    int64_t total = bytes;
    for (const auto &d : dims) {
        int64_t span = 0;
        if (d.second < 0) return false;
        if (__builtin_mul_overflow(d.first > 0 ? d.first - 1 : 0, d.second, &span) ||
            __builtin_add_overflow(total, span, &total))
            return false;
    }
    return true;
}

int index_patterns(int shards, const uint8_t *present, int64_t nstripes, uint8_t *patterns, int cap, uint8_t *ids) {
    std::map<std::string, int> index;
    std::string row((size_t)shards, '\0');
    for (int64_t s = 0; s < nstripes; ++s) {
        for (int i = 0; i < shards; ++i) row[(size_t)i] = present[(size_t)s * shards + i] ? 1 : 0;
        auto it = index.find(row);
        if (it == index.end()) {
            if ((int)index.size() == cap)
                throw Error(ECX_E_ILLEGAL_ARGUMENT, "more than " + std::to_string(cap) + " distinct patterns");
            std::memcpy(patterns + index.size() * (size_t)shards, row.data(), (size_t)shards);
            it = index.emplace(row, (int)index.size()).first;
        }
        ids[s] = (uint8_t)it->second;
    }
    return (int)index.size();
}

void fold_unit_verdicts(const uint8_t *unit, int64_t divisor, bool first_pass, uint8_t *verdict, int64_t nstripes) {
    for (int64_t s = 0; s < nstripes; ++s) {
        uint8_t ok = first_pass ? 1 : verdict[s];
        for (int64_t j = 0; j < divisor; ++j) ok = (uint8_t)(ok && unit[(size_t)(s * divisor + j)]);
        verdict[s] = ok;
    }
}

}  // namespace ecx
