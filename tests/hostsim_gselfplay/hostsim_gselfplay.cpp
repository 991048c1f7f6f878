// hostsim_gselfplay.cpp — TEST HARNESS ONLY (see hostsim.cpp).  The guided self-play run (tafl_gselfplay_*) as the library's kernels drive
// it, on the host: the per-game functions are the product's (tafl_guided.hpp), the loops around them restate k_gselfplay_init /
// k_gselfplay_step / k_gmcts_leaves, one game after the other.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_guided.hpp"

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

struct GspBase {
    virtual ~GspBase() {}
    virtual uint32_t step(const float* priors, const float* values) = 0;
    virtual void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) = 0;
    virtual void end(tafl_state* st, tafl_play* plays, uint32_t* moves, uint8_t* faults) = 0;
    uint64_t sims = 0, predicts = 0, terminal_hits = 0, faults = 0;
};
template <int NL, int W>
struct Gsp : GspBase {
    using GD = Guided<NL, W>;
    using IO = StateIO<NL>;
    Consts<NL> C; GuidedMem M; GSelfPlay sp; SelfPlayRec rec; uint32_t A, n, n_sims; double c_puct;
    std::vector<Quad> ns, soa; std::vector<GNode> hdr; std::vector<uint32_t> pedge, ntop, etop, leaf, simsd, mdone; std::vector<GEdge> edges; std::vector<uint8_t> kind, fault;
    std::vector<tafl_play> plays;
    // tafl_gselfplay_begin: the arena of tafl_gmcts_begin, k_gselfplay_init, and the first round
    int init(const tafl_rules* r, uint8_t side, const tafl_state* st, uint32_t G, uint32_t sims_, uint32_t edges_per_node, double cp, const tafl_selfplay_opts* o, uint32_t n_moves,
             uint64_t base, ExHost* ex) {
        if (make_consts<NL, W>(*r, side, C)) return -1;
        n = side; A = (uint32_t)side * side * 2u * (side - 1u); n_sims = sims_; c_puct = cp;
        M.G = G; M.node_cap = n_sims + 1; M.edge_cap = (n_sims + 1) * edges_per_node;
        ns.resize((size_t)M.node_cap * G * IO::QUADS); hdr.resize((size_t)M.node_cap * G); pedge.resize((size_t)M.node_cap * G); edges.resize((size_t)M.edge_cap * G);
        ntop.resize(G); etop.resize(G); leaf.resize(G); simsd.resize(G); kind.resize(G); fault.resize(G); mdone.resize(G); soa.resize((size_t)IO::QUADS * G);
        plays.assign((size_t)n_moves * G, tafl_play{});
        M.node_state = ns.data(); M.hdr = hdr.data(); M.pedge = pedge.data(); M.edges = edges.data(); M.node_top = ntop.data(); M.edge_top = etop.data();
        M.leaf = leaf.data(); M.kind = kind.data(); M.fault = fault.data(); M.sims_done = simsd.data();
        sp.moves_done = mdone.data(); sp.plays = plays.data(); sp.n_moves = n_moves;
        rec = SelfPlayRec{};
        if (ex) rec.ex = ex->mem();
        rec.sample_seed = o->sample_seed; rec.game_id_base = base; rec.temp_moves = o->temp_moves; rec.move_base = o->move_base;
        for (uint32_t g = 0; g < G; ++g) {
            DState<NL> s; state_from_abi<NL>(st[g], s); IO::store_soa(soa.data(), G, g, s);
            DState<NL> t; IO::load_soa(soa.data(), G, g, t); GD::selfplay_init(M, g, t, sp);
        }
        step(nullptr, nullptr);
        return 0;
    }
    uint32_t step(const float* priors, const float* values) override {
        uint32_t waiting = 0;
        for (uint32_t g = 0; g < M.G; ++g) {
            GuidedStats gs; memset(&gs, 0, sizeof gs);
            GD::selfplay_step(M, g, soa.data(), priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, rec, C, gs);
            sims += gs.sims; predicts += gs.predicts; terminal_hits += gs.terminal_hits; faults += gs.faults;
            waiting += M.kind[g] == 1;
        }
        return waiting;
    }
    void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) override {
        for (uint32_t g = 0; g < M.G; ++g) {
            const bool w = M.kind[g] == 1; const uint32_t L = w ? M.leaf[g] : 0u;
            DState<NL> s; IO::load_rec(M.node_state + ((size_t)L * M.G + g) * IO::QUADS, s);
            for (uint32_t r = 0; r < n; ++r) for (uint32_t c = 0; c < n; ++c) boards[((size_t)g * n + r) * n + c] = (uint8_t)Ops<NL, W>::board_byte(s, r, c, C);
            sides[g] = (uint8_t)((s.flags & TAFL_F_SIDE) ? TAFL_DEFENDER : TAFL_ATTACKER); waiting[g] = w ? 1 : 0;
        }
    }
    void end(tafl_state* st, tafl_play* out_plays, uint32_t* moves, uint8_t* faults) override {
        for (uint32_t g = 0; g < M.G; ++g) {
            if (st) { DState<NL> t; IO::load_soa(soa.data(), M.G, g, t); state_to_abi<NL>(t, (uint8_t)n, st[g]); }
            if (moves) moves[g] = mdone[g] & ~kGspStopped;
            if (faults) faults[g] = fault[g];
        }
        if (out_plays) memcpy(out_plays, plays.data(), sizeof(tafl_play) * plays.size());
    }
};

extern "C" {
void* hsg_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) {
    ExHost* x = new ExHost();
    x->G = G; x->n = n; x->max_moves = max_moves; x->K = K; x->BW = ((uint32_t)n * n + 3u) / 4u;
    const size_t E = (size_t)G * max_moves;
    x->len.assign(G, 0); x->boards.assign(E * x->BW, 0xDEADBEEFu); x->info.assign(E, 0xDEADBEEFu); x->played.assign(E, 0xDEADBEEFu); x->move_no.assign(E, 0xDEADBEEFu);
    x->pol.assign(E * K, 0xDEADBEEFu); x->z.assign(E, -7.f); x->fin.assign(E, 0xEE);
    memset(x->counters, 0, sizeof x->counters);
    return x;
}
void hsg_ex_free(void* h) { delete (ExHost*)h; }
void hsg_ex_counts(void* h, uint32_t* len, uint64_t* counters) {
    ExHost* x = (ExHost*)h;
    for (uint32_t g = 0; g < x->G; ++g) len[g] = x->len[g];
    for (int i = 0; i < EX_COUNTERS; ++i) counters[i] = x->counters[i];
}
// example e = j * G + g as plain fields: out5 = n_children, side, overflow, played, move_no; board[n * n]; actions / visits [K]
int hsg_ex_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits) {
    ExHost* x = (ExHost*)h;
    const uint32_t g = e % x->G, j = e / x->G;
    if (j >= x->max_moves || j >= x->len[g]) return -1;
    const uint32_t info = x->info[e];
    out5[0] = info & 0xFFFFu; out5[1] = (info >> 16) & 0xFFu; out5[2] = (info & kExOverflow) ? 1u : 0u; out5[3] = x->played[e] & 0xFFFFu; out5[4] = x->move_no[e];
    for (uint32_t t = 0; t < (uint32_t)x->n * x->n; ++t) board[t] = (uint8_t)(x->boards[((size_t)j * x->BW + (t >> 2)) * x->G + g] >> (8u * (t & 3u)));
    for (uint32_t k = 0; k < out5[0] && k < x->K; ++k) { const uint32_t w = x->pol[((size_t)j * x->K + k) * x->G + g]; actions[k] = w & 0xFFFFu; visits[k] = w >> 16; }
    return 0;
}
void* hsg_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, uint32_t G, uint32_t n_sims, uint32_t edges_per_node, double c_puct,
                const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t base, void* ex) {
    ExHost* x = (ExHost*)ex;
    if (x && (x->G != G || x->n != n)) return nullptr;
    GspBase* s = nullptr; int rc = -2;
    if (word_bits == 64) { auto* p = new Gsp<2, 7>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, o, n_moves, base, x); s = p; }
    else if (word_bits == 128) { auto* p = new Gsp<4, 11>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, o, n_moves, base, x); s = p; }
    else if (word_bits == 256) { auto* p = new Gsp<8, 15>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, o, n_moves, base, x); s = p; }
    if (rc) { delete s; return nullptr; }
    return s;
}
void hsg_free(void* h) { delete (GspBase*)h; }
// every step after hsg_begin (which ran the first round); priors == NULL only counts the waiting games, as the first tafl_gselfplay_step
uint32_t hsg_step(void* h, const float* priors, const float* values) { return ((GspBase*)h)->step(priors, values); }
void hsg_leaves(void* h, uint8_t* boards, uint8_t* sides, uint8_t* waiting) { ((GspBase*)h)->leaves(boards, sides, waiting); }
// the batch states, the plays [m * G + g], the moves made, out4 = sims, predicts, terminal hits, faults of the stats, and the games' fault flags
void hsg_end(void* h, tafl_state* st, tafl_play* plays, uint32_t* moves, uint64_t* out4, uint8_t* faults) {
    GspBase* s = (GspBase*)h; s->end(st, plays, moves, faults);
    out4[0] = s->sims; out4[1] = s->predicts; out4[2] = s->terminal_hits; out4[3] = s->faults;
}
// Guided::selfplay_pick on a vector of visit counts (one edge per entry, zeros included): the index of the drawn edge
void hsg_pick_many(const uint32_t* visits, uint32_t m, const uint32_t* r, uint32_t count, uint32_t* out) {
    std::vector<GEdge> eb(m ? m : 1);
    uint32_t N = 0;
    for (uint32_t j = 0; j < m; ++j) { eb[j] = GEdge{}; eb[j].n = visits[j]; eb[j].action = 3u * j + 1u; N += visits[j]; }
    for (uint32_t i = 0; i < count; ++i) out[i] = Guided<2, 7>::selfplay_pick(eb.data(), m, N, r[i]);
}
uint32_t hsg_rand(uint64_t sample_seed, uint64_t game_id, uint32_t move_no) { return selfplay_rand(sample_seed, game_id, move_no); }
}
