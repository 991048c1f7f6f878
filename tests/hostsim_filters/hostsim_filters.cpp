// hostsim_filters.cpp — TEST HARNESS ONLY.  The exact pre-filters of the playout ply (tafl_fast.hpp: fort_candidate, the enclosure filter;
// tafl_core.hpp: the far-tile filter of the king capture) next to the full tests they stand in front of, position by position along
// in-place playouts on run-time Consts.  tests/test_hostsim_filters.py checks "filter false => full test false" and compares the states the
// walk leaves with the oracle's.  Built twice: plain (the product's ply), and with -DTAFL_FILTER_PROBE (tafl_bits.hpp), in which the
// king-capture block runs whatever its filter says and reports both.
#include <stdint.h>
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_ops.hpp"

using namespace tafl;

// counts[4 * rule + k], k: 0 positions tested, 1 filter true, 2 full test true, 3 filter false and full test true (must stay 0)
enum : int { RULE_KING_I = 0, RULE_KING_II = 1, RULE_FORT = 2, RULE_ENCLOSED = 3, N_RULES = 4 };
static uint64_t* g_counts = nullptr;
static void seen(int rule, bool filter, bool full) {
    if (!g_counts) return;
    uint64_t* c = g_counts + 4 * rule;
    c[0] += 1; c[1] += filter; c[2] += full; c[3] += !filter && full;
}
#ifdef TAFL_FILTER_PROBE
extern "C" void tafl_filter_probe(int rule, bool filter, bool full) { seen(rule, filter, full); }
#endif
#ifdef TAFL_STAT
// statistics builds (tools/playout_event_stats.py): event counters of the TAFL_STAT_HIT marks
extern "C" { unsigned long long tafl_stat_acc[32] = {}; }
#endif

namespace {
// the enclosure test of Engine::outcome_early, unfiltered
template <int NL, int W>
bool enclosed(const DState<NL>& st, const Consts<NL>& C) {
    using E = Engine<NL, W>;
    Bits<NL> fill;
    const Bits<NL> inside = andn(C.board, st.att);
    if (!E::flood(E::king_sq(st, C), inside, bz<NL>(), C.rules.enclosure_win == TAFL_ENCL_WITHOUT_EDGE_ACCESS, true, C, fill)) return false;
    if (popc(fill & st.def) != popc(st.def & C.board)) return false;
    return E::secure(st, fill, E::dilate(fill, C) & st.att, CLS_ATT, false, true, C);
}

// Fast::rollout's loop under the key of random_advance, one ply at a time, with the tests on every position behind a ply
template <int NL, int W>
int walk(const tafl_rules& r, uint8_t n, tafl_state* io, uint32_t cnt, uint64_t seed, const uint32_t* plies, uint64_t base) {
    using E = Engine<NL, W>; using FA = Fast<NL, W>;
    Consts<NL> C;
    if (make_consts<NL, W>(r, n, C)) return -1;
    if (!fast_ok<NL>(C)) return -5;
    const FastConsts<NL> fc = make_fast_consts<NL>(C);
    for (uint32_t g = 0; g < cnt; ++g) {
        DState<NL> st; state_from_abi<NL>(io[g], st);
        Bits<NL> attT, defT;
        FA::transpose_in(st.att & C.board, attT); FA::transpose_in(st.def & C.board, defT);
        typename FA::Gen gn;
        if (TAFL_F_STATUS(st.flags) != TAFL_STATUS_ONGOING) continue;
        FA::gen(st, attT, defT, st.flags & TAFL_F_SIDE, C, fc, gn);
        uint32_t rk = E::sim_key(E::game_key(seed, base + g), 0xFFFFFFFFu);
        for (uint32_t ply = 0; ply < plies[g] && TAFL_F_STATUS(st.flags) == TAFL_STATUS_ONGOING && gn.total != 0; ++ply) {
            const uint32_t mover = st.flags & TAFL_F_SIDE;
            if (mover == 0) FA::template ply_of<0>(st, attT, defT, gn, rk, C, fc); else FA::template ply_of<1>(st, attT, defT, gn, rk, C, fc);
            if (!any(E::king_bit(st, C))) continue;                  // the king is gone: no test below is defined
            if (mover != 0 && C.rules.exit_fort) seen(RULE_FORT, FA::fort_candidate(st, attT, defT, C), E::exit_fort(st, C));
            if (mover == 0 && C.rules.enclosure_win != TAFL_ENCL_NONE) {
                const bool skip = C.rules.enclosure_win == TAFL_ENCL_WITHOUT_EDGE_ACCESS && (gn.edge_hit || any(st.def & C.edge));      // as ply_of
                seen(RULE_ENCLOSED, !skip, enclosed<NL, W>(st, C));
            }
        }
        state_to_abi<NL>(st, n, io[g]);
    }
    return 0;
}
}  // namespace

extern "C" {
// in-place playouts of plies[g] plies under the key (seed, base + g) of tafl_random_advance; counts: 4 x N_RULES words, added to
int hsf_walk(const tafl_rules* r, uint8_t n, uint32_t word_bits, tafl_state* st, uint32_t cnt, uint64_t seed, const uint32_t* plies, uint64_t base, uint64_t* counts) {
    g_counts = counts;
    int rc = -2;
    if (word_bits == 64) rc = walk<2, 7>(*r, n, st, cnt, seed, plies, base);
    else if (word_bits == 128) rc = walk<4, 11>(*r, n, st, cnt, seed, plies, base);
    g_counts = nullptr;
    return rc;
}
int hsf_probe_build(void) {
#ifdef TAFL_FILTER_PROBE
    return 1;
#else
    return 0;
#endif
}
#ifdef TAFL_STAT
// what tools/playout_event_stats.py calls (tests/hostsim: hs_rollout), for 64- and 128-bit boards
int hs_rollout(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, uint32_t cnt, uint64_t seed, uint32_t sim, uint32_t max_plies, uint64_t base, tafl_rollout_result* out) {
    if (word_bits == 64) { Consts<2> C; if (make_consts<2, 7>(*r, n, C)) return -1; for (uint32_t g = 0; g < cnt; ++g) { DState<2> s; state_from_abi<2>(st[g], s); Ops<2, 7>::rollout(s, seed, base + g, sim, max_plies, C, out[g]); } return 0; }
    if (word_bits == 128) { Consts<4> C; if (make_consts<4, 11>(*r, n, C)) return -1; for (uint32_t g = 0; g < cnt; ++g) { DState<4> s; state_from_abi<4>(st[g], s); Ops<4, 11>::rollout(s, seed, base + g, sim, max_plies, C, out[g]); } return 0; }
    return -2;
}
#endif
}
