// hostsim_value_only.cpp — TEST HARNESS ONLY.  The playout of tafl_fast.hpp on the host under each playout policy (tafl_core.hpp: KeepState,
// ValueOnly), on run-time Consts and on the constexpr Consts of the presets - the host-sim library proper
// (tests/hostsim) runs the default policy on run-time Consts only.  tests/test_hostsim_value_only.py compares all of them with the oracle.
#include <stdint.h>
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_ops.hpp"

using namespace tafl;

namespace {
enum : int { POL_KEEP = 0, POL_VALUE_ONLY = 1 };

template <int NL, int W, class P>
void rollouts(const Consts<NL>& C, const tafl_state* st, uint32_t cnt, uint64_t seed, uint32_t sim, uint32_t max_plies, uint64_t base, tafl_rollout_result* out) {
    for (uint32_t g = 0; g < cnt; ++g) {
        DState<NL> s;
        if constexpr (NL == 6) { DState<8> t; state_from_abi<8>(st[g], t); restride<8, 15, 6, 13>(t, 13, s); }       // the dense 13-column layout
        else state_from_abi<NL>(st[g], s);
        Ops<NL, W>::rollout(s, seed, base + g, sim, max_plies, C, out[g], false, IdxComputed<NL>(), P());
    }
}
template <int NL, int W>
int by_policy(const Consts<NL>& C, int policy, const tafl_state* st, uint32_t cnt, uint64_t seed, uint32_t sim, uint32_t max_plies, uint64_t base, tafl_rollout_result* out) {
    switch (policy) {
        case POL_KEEP: rollouts<NL, W, KeepState>(C, st, cnt, seed, sim, max_plies, base, out); return 0;
        case POL_VALUE_ONLY: rollouts<NL, W, ValueOnly>(C, st, cnt, seed, sim, max_plies, base, out); return 0;
        default: return -3;
    }
}
// preset != 0: the constexpr Consts of the preset the rules and board are (an error if they are none); else Consts made at run time
template <int NL, int W, int PRESET, class F>
int with_consts(const tafl_rules* r, uint8_t n, uint32_t word_bits, int preset, F&& f) {
    if (preset) {
        if (detect_preset(*r, n, word_bits) != PRESET) return -4;
        static constexpr Consts<NL> C = preset_consts<NL, W, PRESET>();
        return f(C);
    }
    Consts<NL> C;
    if (make_consts<NL, W>(*r, n, C)) return -1;
    return f(C);
}
}  // namespace

extern "C" {
// game g plays with the key (seed, base + g, sim), as tafl_rollout.  dense13: a 13x13 position of a 256-bit batch in the layout <6, 13>.
int hsv_rollout(const tafl_rules* r, uint8_t n, uint32_t word_bits, int policy, int preset, int dense13, const tafl_state* st, uint32_t cnt, uint64_t seed,
                uint32_t sim, uint32_t max_plies, uint64_t base, tafl_rollout_result* out) {
    auto run = [&](const auto& C, auto nl, auto w) { return by_policy<decltype(nl)::value, decltype(w)::value>(C, policy, st, cnt, seed, sim, max_plies, base, out); };
    using I2 = std::integral_constant<int, 2>; using I4 = std::integral_constant<int, 4>; using I6 = std::integral_constant<int, 6>; using I8 = std::integral_constant<int, 8>;
    using I7 = std::integral_constant<int, 7>; using I11 = std::integral_constant<int, 11>; using I13 = std::integral_constant<int, 13>; using I15 = std::integral_constant<int, 15>;
    if (word_bits == 64) return with_consts<2, 7, PRESET_BRANDUBH7>(r, n, word_bits, preset, [&](const Consts<2>& C) { return run(C, I2(), I7()); });
    if (word_bits == 128) return with_consts<4, 11, PRESET_COPENHAGEN11>(r, n, word_bits, preset, [&](const Consts<4>& C) { return run(C, I4(), I11()); });
    if (word_bits == 256 && dense13) return n == 13 ? with_consts<6, 13, PRESET_COPENHAGEN13>(r, n, word_bits, preset, [&](const Consts<6>& C) { return run(C, I6(), I13()); }) : -2;
    if (word_bits == 256) return with_consts<8, 15, PRESET_COPENHAGEN13>(r, n, word_bits, preset, [&](const Consts<8>& C) { return run(C, I8(), I15()); });
    return -2;
}
// in-place playouts (always the keeping policy: Ops::random_advance has no other), preset as above
int hsv_random_advance(const tafl_rules* r, uint8_t n, uint32_t word_bits, int preset, tafl_state* st, uint32_t cnt, uint64_t seed, const uint32_t* plies, uint64_t base) {
    auto run = [&](const auto& C, auto nl, auto w) {
        constexpr int NL = decltype(nl)::value, W = decltype(w)::value;
        for (uint32_t g = 0; g < cnt; ++g) { DState<NL> s; state_from_abi<NL>(st[g], s); Ops<NL, W>::random_advance(s, seed, base + g, plies[g], C); state_to_abi<NL>(s, n, st[g]); }
        return 0;
    };
    using I2 = std::integral_constant<int, 2>; using I4 = std::integral_constant<int, 4>; using I8 = std::integral_constant<int, 8>;
    using I7 = std::integral_constant<int, 7>; using I11 = std::integral_constant<int, 11>; using I15 = std::integral_constant<int, 15>;
    if (word_bits == 64) return with_consts<2, 7, PRESET_BRANDUBH7>(r, n, word_bits, preset, [&](const Consts<2>& C) { return run(C, I2(), I7()); });
    if (word_bits == 128) return with_consts<4, 11, PRESET_COPENHAGEN11>(r, n, word_bits, preset, [&](const Consts<4>& C) { return run(C, I4(), I11()); });
    if (word_bits == 256) return with_consts<8, 15, PRESET_COPENHAGEN13>(r, n, word_bits, preset, [&](const Consts<8>& C) { return run(C, I8(), I15()); });
    return -2;
}
}
