// apply_launch.inc -- launch_shape_t<T>: run-time launch shape -> template instance
// of k_gf_apply.  Included once per instantiation unit (apply_t256.hip, apply_t64.hip).
namespace ecx {

template <bool SAFE, bool NTL, int NTS, int D, bool TLDS, int T, int R = kTileRows>
void launch_k(dim3 grid, size_t lds, hipStream_t stream, const ApplyArgs &a) {
    if constexpr (!SAFE) note_kernel("k_gf_apply", SAFE, NTL, NTS, D, TLDS, T, R);
    hipLaunchKernelGGL((k_gf_apply<SAFE, NTL, NTS, D, TLDS, T, R>), grid, dim3(T), lds, stream, a);
}

// Instances: every (non-temporal policy, depth 4 / 8, LDS tables) for 8-row tiles;
// depth 2 for 256-thread workgroups with plain-nt stores; deep rings (10 / 12 / 16 /
// 20 / 24; 20 also with scoped stores) for single tiles with NT loads, SGPR tables and
// 256-thread workgroups; the small-tile variants (2 or 4 rows, NT loads and stores,
// depth 4 / 8 / 12) for 256-thread workgroups.
// The launch rules (launch_rules.cpp choose_launch) only ask for shapes that exist: they do all
// the clamping, and a shape without an instance is refused here.  `lds` is the TLDS
// table bytes plus ecx_tune "occ_lds" (0 by default) for every non-byte-safe instance.
template <int T>
void launch_shape_t(const Shape &s, dim3 grid, size_t lds, hipStream_t stream, const ApplyArgs &a) {
    const auto no_instance = [] { return Error(ECX_E_ILLEGAL_ARGUMENT, "no k_gf_apply instance for this launch shape"); };
    if (s.tail) {  // the rules ask for it only on this shape
        if (s.safe || !s.ntl || s.nts != 1 || s.tlds || s.rows != kTileRows || (s.depth != 4 && s.depth != 8))
            throw Error(ECX_E_ILLEGAL_ARGUMENT, "no k_gf_apply_tail instance for this launch shape");
        if (s.note) note_kernel("k_gf_apply_tail", true, 1, s.depth, false, T, kTileRows);
        if (s.depth == 8) hipLaunchKernelGGL((k_gf_apply_tail<true, 1, 8, false, T, kTileRows>), grid, dim3(T), 0, stream, a);
        else hipLaunchKernelGGL((k_gf_apply_tail<true, 1, 4, false, T, kTileRows>), grid, dim3(T), 0, stream, a);
        return;
    }
    if (s.safe) {  // the byte-safe kernel's ring must match the plan's padding
        if (s.depth == 2) return launch_k<true, false, 0, 2, false, T>(grid, 0, stream, a);
        if (s.depth == 4) return launch_k<true, false, 0, 4, false, T>(grid, 0, stream, a);
        throw no_instance();
    }
    if (s.ntl ? s.nts == 0 : s.nts < 0 || s.nts > 2) throw no_instance();
    if (T != kBlockThreads && s.nts != 1) throw no_instance();  // one-wave workgroups: plain-nt stores only
    if constexpr (T == kBlockThreads) {
        if (s.rows < kTileRows) {
            if (!s.ntl || s.nts != 1 || s.tlds) throw no_instance();
            auto small = [&](auto rows) {
                constexpr int R = decltype(rows)::value;
                if (s.depth == 12) launch_k<false, true, 1, 12, false, T, R>(grid, lds, stream, a);
                else if (s.depth == 8) launch_k<false, true, 1, 8, false, T, R>(grid, lds, stream, a);
                else if (s.depth == 4) launch_k<false, true, 1, 4, false, T, R>(grid, lds, stream, a);
                else throw no_instance();
            };
            if (s.rows == 2) small(std::integral_constant<int, 2>{});
            else if (s.rows == 4) small(std::integral_constant<int, 4>{});
            else throw no_instance();
            return;
        }
    }
    if (s.rows != kTileRows) throw no_instance();
    auto by_depth = [&](auto ntl, auto nts) {
        constexpr bool L = decltype(ntl)::value;
        constexpr int S = decltype(nts)::value;
        if (s.depth == 8) {
            if (s.tlds) launch_k<false, L, S, 8, true, T>(grid, lds, stream, a);
            else launch_k<false, L, S, 8, false, T>(grid, lds, stream, a);
            return;
        }
        if constexpr (S == 2 && T == kBlockThreads && L) {  // scoped NT stores, headline ring only
            if (s.depth == 20 && !s.tlds) return launch_k<false, true, 2, 20, false, T>(grid, lds, stream, a);
        }
        if constexpr (S == 1 && T == kBlockThreads && L) {
            // Deep rings for single-tile maps: every load of a short tile in flight at once
            // (one-wave workgroups measured 0.8 % slower at depth 20: profiles/r01_kbench_deep.jsonl).
            if (!s.tlds) {
                switch (s.depth) {
                case 10: return launch_k<false, true, 1, 10, false, T>(grid, lds, stream, a);
                case 12: return launch_k<false, true, 1, 12, false, T>(grid, lds, stream, a);
                case 16: return launch_k<false, true, 1, 16, false, T>(grid, lds, stream, a);
                case 20: return launch_k<false, true, 1, 20, false, T>(grid, lds, stream, a);
                case 24: return launch_k<false, true, 1, 24, false, T>(grid, lds, stream, a);
                default: break;
                }
            }
        }
        if (s.depth > 8) throw Error(ECX_E_ILLEGAL_ARGUMENT, "no deep-ring instance for this launch shape");
        if constexpr (S == 1 && T == kBlockThreads) {
            if (s.depth == 2) {
                if (s.tlds) launch_k<false, L, S, 2, true, T>(grid, lds, stream, a);
                else launch_k<false, L, S, 2, false, T>(grid, lds, stream, a);
                return;
            }
        }
        if (s.depth != 4) throw no_instance();
        if (s.tlds) launch_k<false, L, S, 4, true, T>(grid, lds, stream, a);
        else launch_k<false, L, S, 4, false, T>(grid, lds, stream, a);
    };
    using t_ = std::true_type;
    using f_ = std::false_type;
    using one = std::integral_constant<int, 1>;
    if constexpr (T == kBlockThreads) {
        if (s.ntl) {
            if (s.nts == 2) by_depth(t_{}, std::integral_constant<int, 2>{});
            else by_depth(t_{}, one{});
        } else if (s.nts == 2) by_depth(f_{}, std::integral_constant<int, 2>{});
        else if (s.nts == 1) by_depth(f_{}, one{});
        else by_depth(f_{}, std::integral_constant<int, 0>{});
    } else {  // one-wave workgroups: plain-nt stores only
        if (s.ntl) by_depth(t_{}, one{});
        else by_depth(f_{}, one{});
    }
}

}  // namespace ecx
