// hostsim_examples.cpp — TEST HARNESS ONLY (see hostsim.cpp).  The recording self-play run (tafl_selfplay_record), the results kernel
// and the minibatch gather as the library's kernels drive them, on the host: the per-game functions are the product's
// (tafl_ops.hpp, tafl_examples.hpp), the loops around them restate k_mcts_tree_selfplay_rec / k_examples_finalize / k_examples_gather.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_ops.hpp"

using namespace tafl;

struct ExHost {
    uint32_t G, n, max_moves, K, BW;
    std::vector<uint32_t> len, boards, info, played, move_no, pol;
    std::vector<float> z; std::vector<uint8_t> fin;
    unsigned long long counters[EX_COUNTERS];
    ExamplesMem mem() {
        ExamplesMem X; X.len = len.data(); X.boards = boards.data(); X.info = info.data(); X.played = played.data(); X.move_no = move_no.data();
        X.pol = pol.data(); X.z = z.data(); X.fin = fin.data(); X.counters = counters; X.G = G; X.max_moves = max_moves; X.K = K; X.BW = BW;
        return X;
    }
};

struct RunCfg { uint32_t spec_k, spec_target, capacity; };

// DENSE13 as in hostsim.cpp: the batch in the reference's 15-column layout, the search (and the recorded position) in the dense 13-column one
template <int NL, int W, bool DENSE13 = false>
struct HostRec {
    using O = Ops<NL, W>;
    using S = DState<NL>;
    using K = Consts<NL>;
    // the round driver of tafl_selfplay_run's host loop (hostsim.cpp Host::mcts with n_moves != 0), advancing with selfplay_advance_rec
    static int record(const tafl_rules* r, uint8_t n, tafl_state* st, uint32_t G, const tafl_mcts_params* p, uint64_t base, uint32_t n_moves,
                      const tafl_selfplay_opts* o, ExHost* ex, tafl_play* plays_out, tafl_mcts_stats* stats, const RunCfg& cfg) {
        K C; if (make_consts<NL, W>(*r, n, C)) return -1;
        using IO = StateIO<NL>;
        const uint32_t spec_k = cfg.spec_k < 1 ? 1 : (cfg.spec_k > 8 ? 8 : cfg.spec_k), log_cap = 16;
        MctsMem M; M.G = G; M.node_cap = p->n_sims + 1; M.edge_cap = 4 * (p->n_sims + 1); M.spec_k = spec_k; M.flags = p->flags & TAFL_MCTS_FLAG_FPU_INF;
        std::vector<Quad> ns((size_t)M.node_cap * G * IO::QUADS), sst((size_t)M.spec_k * G * IO::QUADS);
        std::vector<NodeHdr> hdr((size_t)M.node_cap * G);
        std::vector<Edge> edges((size_t)M.edge_cap * G);
        std::vector<uint32_t> ntop(G), etop(G), leaf(G), simn(G), spend(G), splies((size_t)M.spec_k * G), smeta((size_t)M.spec_k * G), sref((size_t)M.spec_k * G), simbase(G), sbias(G);
        std::vector<uint8_t> kind(G), fault(G), skind((size_t)M.spec_k * G), sreason((size_t)M.spec_k * G), scls((size_t)M.spec_k * G);
        std::vector<int8_t> sval((size_t)M.spec_k * G);
        std::vector<uint32_t> logw((size_t)log_cap * (kUndoEWords + kUndoHWords) + 1);
        LogMem lm; lm.base = logw.data(); lm.stride = 1; lm.lane = 0; lm.cap = spec_k > 1 ? log_cap : 0;
        M.node_state = ns.data(); M.hdr = hdr.data(); M.edges = edges.data(); M.node_top = ntop.data(); M.edge_top = etop.data();
        M.leaf = leaf.data(); M.kind = kind.data(); M.fault = fault.data();
        M.sim_next = simn.data(); M.spec_state = sst.data(); M.spec_value = sval.data(); M.spec_kind = skind.data(); M.spec_reason = sreason.data(); M.spec_meta = smeta.data();
        M.spec_plies = splies.data(); M.spec_ref = sref.data(); M.spec_cls = scls.data(); M.spec_pend = spend.data();
        M.sim_base = simbase.data(); M.spec_bias = sbias.data();
        memset(stats, 0, sizeof *stats);
        for (uint32_t g = 0; g < G; ++g) {
            S s;
            if constexpr (DENSE13) { DState<8> t; state_from_abi<8>(st[g], t); restride<8, 15, NL, W>(t, 13, s); } else state_from_abi<NL>(st[g], s);
            O::mcts_init_game(M, g, s, C);
        }
        constexpr int NLB = DENSE13 ? 8 : NL, WB = DENSE13 ? 15 : W;
        std::vector<Quad> soa((size_t)StateIO<NLB>::QUADS * G);
        std::vector<uint32_t> mdone(G, 0), sround(G, 0);
        SelfPlay sp; sp.moves_done = mdone.data(); sp.start_round = sround.data(); sp.plays = plays_out; sp.n_moves = n_moves;
        SelfPlayRec rec{};
        if (ex) rec.ex = ex->mem();
        rec.sample_seed = o->sample_seed; rec.game_id_base = base; rec.temp_moves = o->temp_moves; rec.move_base = o->move_base;
        for (uint32_t g = 0; g < G; ++g) { DState<NLB> t; state_from_abi<NLB>(st[g], t); StateIO<NLB>::store_soa(soa.data(), G, g, t); }
        memset(plays_out, 0, sizeof(tafl_play) * (size_t)n_moves * G);
        uint32_t sp_done = 0;
        const uint32_t planned = cfg.spec_target ? (p->n_sims + cfg.spec_target - 1) / cfg.spec_target : 0;
        const uint64_t bound = (uint64_t)(p->n_sims + 2) * (cfg.capacity ? 1 + G / cfg.capacity : 1) * n_moves + n_moves;
        for (uint64_t i = 0; i < bound; ++i) {
            const uint32_t round_no = (uint32_t)i;
            for (uint32_t g = 0; g < G; ++g) {                 // as k_mcts_tree_selfplay_rec: advance, then the plan of the game's own search
                LaneStats ls; memset(&ls, 0, sizeof ls);
                const int rr = O::template selfplay_advance_rec<NLB, WB>(M, g, soa.data(), sp, rec, p->n_sims, round_no, C);
                if (rr == 2) ++sp_done;
                const uint32_t rel = round_no - sround[g];
                const uint32_t rounds_left = cfg.spec_target ? (rel < planned ? planned - rel : 1u) : 0u;
                if (!(simn[g] < p->n_sims || kind[g] == 1)) continue;
                O::mcts_tree_step(M, g, p->c_puct, p->n_sims, rounds_left, O::mcts_scenarios(rounds_left, planned), spec_k, C, ls, lm);
                stats->sims += ls.sims; stats->tree_depth_sum += ls.depth; stats->children_scanned += ls.scanned;
                stats->terminal_hits += ls.terminal_hits; stats->faults += ls.faults;
                stats->rollouts += ls.rollouts; stats->rollout_plies += ls.rollout_plies;
                stats->spec_issued += ls.spec_issued; stats->spec_hits += ls.spec_hits;
            }
            uint32_t work = 0;
            for (uint32_t c = 0; c < kMctsMaxSlots; ++c)
                for (uint32_t g = 0; g < G; ++g) {
                    if (!(simn[g] < p->n_sims || kind[g] == 1)) continue;
                    uint32_t found = 0, slot = 0;
                    for (uint32_t j = 0; j < M.spec_k; ++j) if (skind[(size_t)j * G + g] == 1 && scls[(size_t)j * G + g] == c) { ++found; slot = j; }
                    if (found > 1) return -5;
                    if (!found) continue;
                    if (cfg.capacity && work >= cfg.capacity) continue;
                    ++work; O::mcts_slot_rollout(M, slot, g, p->seed, base + g, p->sim_offset, p->max_rollout_plies, C);
                }
            if (work == 0 && sp_done >= G) break;
        }
        if (sp_done < G) return -3;
        for (uint32_t g = 0; g < G; ++g) { DState<NLB> t; StateIO<NLB>::load_soa(soa.data(), G, g, t); state_to_abi<NLB>(t, n, st[g]); }
        return 0;
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
void* hsx_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) {
    ExHost* x = new ExHost();
    x->G = G; x->n = n; x->max_moves = max_moves; x->K = K; x->BW = ((uint32_t)n * n + 3u) / 4u;
    const size_t E = (size_t)G * max_moves;
    x->len.assign(G, 0); x->boards.assign(E * x->BW, 0xDEADBEEFu); x->info.assign(E, 0xDEADBEEFu); x->played.assign(E, 0xDEADBEEFu); x->move_no.assign(E, 0xDEADBEEFu);
    x->pol.assign(E * K, 0xDEADBEEFu); x->z.assign(E, -7.f); x->fin.assign(E, 0xEE);
    memset(x->counters, 0, sizeof x->counters);
    return x;
}
void hsx_free(void* h) { delete (ExHost*)h; }
void hsx_clear(void* h) { ExHost* x = (ExHost*)h; x->len.assign(x->G, 0); memset(x->counters, 0, sizeof x->counters); }
void hsx_counts(void* h, uint32_t* len, uint64_t* counters) {
    ExHost* x = (ExHost*)h;
    for (uint32_t g = 0; g < x->G; ++g) len[g] = x->len[g];
    for (int i = 0; i < EX_COUNTERS; ++i) counters[i] = x->counters[i];
}
// example e = j * G + g as plain fields: out5 = n_children, side, overflow, played, move_no; board[n * n]; actions / visits [K]; z, final
int hsx_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits, float* z, uint8_t* fin) {
    ExHost* x = (ExHost*)h;
    const uint32_t g = e % x->G, j = e / x->G;
    if (j >= x->max_moves || j >= x->len[g]) return -1;
    const uint32_t info = x->info[e];
    out5[0] = info & 0xFFFFu; out5[1] = (info >> 16) & 0xFFu; out5[2] = (info & kExOverflow) ? 1u : 0u; out5[3] = x->played[e] & 0xFFFFu; out5[4] = x->move_no[e];
    for (uint32_t t = 0; t < (uint32_t)x->n * x->n; ++t) board[t] = (uint8_t)(x->boards[((size_t)j * x->BW + (t >> 2)) * x->G + g] >> (8u * (t & 3u)));
    for (uint32_t k = 0; k < out5[0] && k < x->K; ++k) { const uint32_t w = x->pol[((size_t)j * x->K + k) * x->G + g]; actions[k] = w & 0xFFFFu; visits[k] = w >> 16; }
    *z = x->z[e]; *fin = x->fin[e];
    return 0;
}
int hsx_record(const tafl_rules* r, uint8_t n, uint32_t word_bits, tafl_state* st, uint32_t G, const tafl_mcts_params* p, uint64_t base, uint32_t n_moves,
               const tafl_selfplay_opts* o, void* ex, tafl_play* plays, tafl_mcts_stats* stats, uint32_t spec_k, uint32_t spec_target, uint32_t capacity) {
    RunCfg cfg; cfg.spec_k = spec_k; cfg.spec_target = spec_target; cfg.capacity = capacity;
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
uint32_t hsx_pick(const uint32_t* visits, uint32_t m, uint32_t r) {
    std::vector<Edge> eb(m ? m : 1);
    uint32_t N = 0;
    for (uint32_t j = 0; j < m; ++j) { eb[j].q = 0.0; eb[j].n = visits[j]; eb[j].child = j + 1; N += visits[j]; }
    return Ops<2, 7>::selfplay_pick(eb.data(), m, N, r);
}
void hsx_pick_many(const uint32_t* visits, uint32_t m, const uint32_t* r, uint32_t count, uint32_t* out) {
    std::vector<Edge> eb(m ? m : 1);
    uint32_t N = 0;
    for (uint32_t j = 0; j < m; ++j) { eb[j].q = 0.0; eb[j].n = visits[j]; eb[j].child = j + 1; N += visits[j]; }
    for (uint32_t i = 0; i < count; ++i) out[i] = Ops<2, 7>::selfplay_pick(eb.data(), m, N, r[i]);
}
uint32_t hsx_rand(uint64_t sample_seed, uint64_t game_id, uint32_t move_no) { return selfplay_rand(sample_seed, game_id, move_no); }
// sym_tile for every tile, sym_action for every action of an n x n board
void hsx_sym_tables(uint32_t sym, uint32_t n, uint32_t* tiles, uint32_t* actions) {
    for (uint32_t t = 0; t < n * n; ++t) tiles[t] = sym_tile(sym, t, n);
    for (uint32_t a = 0; a < n * n * 2u * (n - 1u); ++a) actions[a] = sym_action(sym, a, n);
}
}
