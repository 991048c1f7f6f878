// hostsim_examples.cpp — TEST HARNESS ONLY (see hostsim.cpp).  The recording self-play run (tafl_selfplay_record), the results kernel
// and the minibatch gather as the library's kernels drive them, on the host: the per-game functions are the product's
// (tafl_ops.hpp, tafl_examples.hpp), the loops around them restate k_mcts_tree_selfplay_rec / k_examples_finalize / k_examples_gather.
#include "hostsim_common.hpp"

// DENSE13 as in hostsim.cpp: the batch in the reference's 15-column layout, the search (and the recorded position) in the dense 13-column one
template <int NL, int W, bool DENSE13 = false>
struct HostRec {
    using O = Ops<NL, W>;
    using S = DState<NL>;
    // tafl_selfplay_record: the round driver of a self-play run, advancing with selfplay_advance_rec
    static int record(const tafl_rules* r, uint8_t n, tafl_state* st, uint32_t G, const tafl_mcts_params* p, uint64_t base, uint32_t n_moves,
                      const tafl_selfplay_opts* o, ExHost* ex, tafl_play* plays_out, tafl_mcts_stats* stats, const RunKnobs& knobs) {
        RolloutArena<NL, W, DENSE13> R;
        if (R.init(r, n, st, G, p, knobs, n_moves, plays_out)) return -1;
        const SelfPlayRec rec = make_rec(ex, o, base);
        const int rc = R.run(p, base, stats, [&](uint32_t g, uint32_t round) { return O::template selfplay_advance_rec<R.NLB, R.WB>(R.M, g, R.soa.data(), R.sp, rec, p->n_sims, round, R.C); });
        if (rc == 0) R.store_states(n, st);
        return rc;
    }
    // k_examples_finalize: one game after the other, the flags word of its current state
    static int finalize(uint8_t n, const tafl_state* st, ExHost* ex) {
        for (uint32_t g = 0; g < ex->G; ++g) {
            S s; state_from_abi<NL>(st[g], s);
            const uint32_t len = ex->len[g] < ex->max_moves ? ex->len[g] : ex->max_moves;
            for (uint32_t j = 0; j < len; ++j) {
                const size_t e = (size_t)j * ex->G + g;
                uint8_t fin; ex->z[e] = example_outcome(s.flags, (ex->info[e] >> 16) & 0xFFu, fin); ex->fin[e] = fin;
            }
        }
        return 0;
    }
};

static bool g_dense13 = false;
#define DISPATCH_REC(call)                                                        \
    if (g_dense13 && word_bits == 256 && n == 13) return HostRec<6, 13, true>::call; \
    switch (word_bits) {                                                          \
        case 64:  return HostRec<2, 7>::call;                                     \
        case 128: return HostRec<4, 11>::call;                                    \
        case 256: return HostRec<8, 15>::call;                                    \
        default:  return -2;                                                      \
    }

extern "C" {
void hsx_set_dense13(int on) { g_dense13 = on != 0; }
void* hsx_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return new ExHost(G, n, max_moves, K); }
void hsx_free(void* h) { delete (ExHost*)h; }
void hsx_clear(void* h) { ExHost* x = (ExHost*)h; x->len.assign(x->G, 0); memset(x->counters, 0, sizeof x->counters); }
void hsx_counts(void* h, uint32_t* len, uint64_t* counters) { ((ExHost*)h)->counts(len, counters); }
// example e = j * G + g as plain fields (ExHost::read) and z, final
int hsx_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits, float* z, uint8_t* fin) {
    ExHost* x = (ExHost*)h;
    if (x->read(e, out5, board, actions, visits)) return -1;
    *z = x->z[e]; *fin = x->fin[e];
    return 0;
}
// the same buffer for a guided run (tests/gselfplay_util.py)
void* hsg_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return hsx_new(G, n, max_moves, K); }
void hsg_ex_free(void* h) { hsx_free(h); }
void hsg_ex_counts(void* h, uint32_t* len, uint64_t* counters) { hsx_counts(h, len, counters); }
int hsg_ex_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits) { return ((ExHost*)h)->read(e, out5, board, actions, visits); }
int hsx_record(const tafl_rules* r, uint8_t n, uint32_t word_bits, tafl_state* st, uint32_t G, const tafl_mcts_params* p, uint64_t base, uint32_t n_moves,
               const tafl_selfplay_opts* o, void* ex, tafl_play* plays, tafl_mcts_stats* stats, uint32_t spec_k, uint32_t spec_target, uint32_t capacity) {
    RunKnobs cfg; cfg.spec_k = spec_k; cfg.spec_target = spec_target; cfg.capacity = capacity;
    ExHost* x = (ExHost*)ex;
    if (x && (x->G != G || x->n != n)) return -6;
    DISPATCH_REC(record(r, n, st, G, p, base, n_moves, o, x, plays, stats, cfg))
}
int hsx_finalize(void* ex, uint8_t n, uint32_t word_bits, const tafl_state* st) {
    ExHost* x = (ExHost*)ex;
    switch (word_bits) {
        case 64:  return HostRec<2, 7>::finalize(n, st, x);
        case 128: return HostRec<4, 11>::finalize(n, st, x);
        case 256: return HostRec<8, 15>::finalize(n, st, x);
        default:  return -2;
    }
}
// k_examples_gather, one row after the other: returns the number of indices that name no recorded example (their rows are all zero)
uint32_t hsx_gather(void* ex, const uint32_t* index, const uint8_t* sym, uint32_t count, uint8_t* boards, uint8_t* sides, float* pi, float* z, uint8_t* fin) {
    ExHost* x = (ExHost*)ex;
    const uint32_t n = x->n, nn = n * n, A = nn * 2u * (n - 1u);
    uint32_t bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t e = index[i], g = e % x->G, j = e / x->G;
        const bool ok = j < x->max_moves && j < x->len[g];
        const uint32_t s = sym ? (sym[i] & 7u) : 0u, info = ok ? x->info[e] : 0u, nc = info & 0xFFFFu;
        if (!ok) ++bad;
        if (pi) {
            float* row = pi + (size_t)i * A;
            for (uint32_t a = 0; a < A; ++a) row[a] = 0.0f;
            const double N = ok ? (double)(x->played[e] >> 16) : 0.0;
            for (uint32_t k = 0; k < nc; ++k) {
                const uint32_t w = x->pol[((size_t)j * x->K + k) * x->G + g], a = w & 0xFFFFu;
                row[s ? sym_action(s, a, n) : a] = (float)((double)(w >> 16) / N);
            }
        }
        if (boards) for (uint32_t t = 0; t < nn; ++t) {
            const uint32_t w = ok ? x->boards[((size_t)j * x->BW + (t >> 2)) * x->G + g] : 0u;
            boards[(size_t)i * nn + (s ? sym_tile(s, t, n) : t)] = (uint8_t)(w >> (8u * (t & 3u)));
        }
        if (sides) sides[i] = (uint8_t)((info >> 16) & 0xFFu);
        if (z) z[i] = ok ? x->z[e] : 0.0f;
        if (fin) fin[i] = ok ? x->fin[e] : (uint8_t)0;
    }
    return bad;
}
// Ops::selfplay_pick on a vector of visit counts
void hsx_pick_many(const uint32_t* visits, uint32_t m, const uint32_t* r, uint32_t count, uint32_t* out) {
    std::vector<Edge> eb(m ? m : 1);
    uint32_t N = 0;
    for (uint32_t j = 0; j < m; ++j) { eb[j].q = 0.0; eb[j].n = visits[j]; eb[j].child = j + 1; N += visits[j]; }
    for (uint32_t i = 0; i < count; ++i) out[i] = Ops<2, 7>::selfplay_pick(eb.data(), m, N, r[i]);
}
uint32_t hsx_pick(const uint32_t* visits, uint32_t m, uint32_t r) { uint32_t out; hsx_pick_many(visits, m, &r, 1, &out); return out; }
// Guided::selfplay_pick on a vector of visit counts (one edge per entry, zeros included): the index of the drawn edge
void hsg_pick_many(const uint32_t* visits, uint32_t m, const uint32_t* r, uint32_t count, uint32_t* out) {
    std::vector<GEdge> eb(m ? m : 1);
    uint32_t N = 0;
    for (uint32_t j = 0; j < m; ++j) { eb[j] = GEdge{}; eb[j].n = visits[j]; eb[j].action = 3u * j + 1u; N += visits[j]; }
    for (uint32_t i = 0; i < count; ++i) out[i] = Guided<2, 7>::selfplay_pick(eb.data(), m, N, r[i]);
}
uint32_t hsx_rand(uint64_t sample_seed, uint64_t game_id, uint32_t move_no) { return selfplay_rand(sample_seed, game_id, move_no); }
uint32_t hsg_rand(uint64_t sample_seed, uint64_t game_id, uint32_t move_no) { return selfplay_rand(sample_seed, game_id, move_no); }
// sym_tile for every tile, sym_action for every action of an n x n board
void hsx_sym_tables(uint32_t sym, uint32_t n, uint32_t* tiles, uint32_t* actions) {
    for (uint32_t t = 0; t < n * n; ++t) tiles[t] = sym_tile(sym, t, n);
    for (uint32_t a = 0; a < n * n * 2u * (n - 1u); ++a) actions[a] = sym_action(sym, a, n);
}
}
