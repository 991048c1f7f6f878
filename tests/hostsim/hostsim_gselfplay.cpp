// hostsim_gselfplay.cpp — TEST HARNESS ONLY (see hostsim.cpp).  The guided self-play run (tafl_gselfplay_*) as the library's kernels drive
// it, on the host: the per-game functions are the product's (tafl_guided.hpp), the loops around them restate k_gselfplay_init /
// k_gselfplay_step / k_gmcts_leaves, one game after the other.
#include "hostsim_common.hpp"

struct GspBase : GuidedCounts {
    virtual ~GspBase() {}
    virtual uint32_t step(const float* priors, const float* values) = 0;
    virtual void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) = 0;
    virtual void end(tafl_state* st, tafl_play* plays, uint32_t* moves, uint8_t* faults) = 0;
};
template <int NL, int W>
struct Gsp : GspBase {
    using GD = Guided<NL, W>;
    using IO = StateIO<NL>;
    GuidedArena<NL, W> R; GSelfPlay sp; SelfPlayRec rec; uint32_t n_sims; double c_puct;
    std::vector<Quad> soa; std::vector<uint32_t> mdone; std::vector<tafl_play> plays;
    // tafl_gselfplay_begin: the arena of tafl_gmcts_begin, k_gselfplay_init, and the first round
    int init(const tafl_rules* r, uint8_t side, const tafl_state* st, uint32_t G, uint32_t sims_, uint32_t edges_per_node, double cp, const tafl_selfplay_opts* o, uint32_t n_moves,
             uint64_t base, ExHost* ex) {
        if (R.init(r, side, G, sims_, edges_per_node)) return -1;
        n_sims = sims_; c_puct = cp;
        mdone.resize(G); soa.resize((size_t)IO::QUADS * G); plays.assign((size_t)n_moves * G, tafl_play{});
        sp.moves_done = mdone.data(); sp.plays = plays.data(); sp.n_moves = n_moves;
        rec = make_rec(ex, o, base);
        for (uint32_t g = 0; g < G; ++g) {
            DState<NL> s; state_from_abi<NL>(st[g], s); IO::store_soa(soa.data(), G, g, s);
            DState<NL> t; IO::load_soa(soa.data(), G, g, t); GD::selfplay_init(R.M, g, t, sp);
        }
        step(nullptr, nullptr);
        return 0;
    }
    uint32_t step(const float* priors, const float* values) override {
        return R.round(priors, values, *this, [&](uint32_t g, const float* pr, float v, GuidedStats& gs) { GD::selfplay_step(R.M, g, soa.data(), pr, v, R.A, c_puct, n_sims, sp, rec, R.C, gs); });
    }
    void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) override { R.leaves(boards, sides, waiting); }
    void end(tafl_state* st, tafl_play* out_plays, uint32_t* moves, uint8_t* faults) override {
        for (uint32_t g = 0; g < R.M.G; ++g) {
            if (st) { DState<NL> t; IO::load_soa(soa.data(), R.M.G, g, t); state_to_abi<NL>(t, (uint8_t)R.n, st[g]); }
            if (moves) moves[g] = mdone[g] & ~kGspStopped;
            if (faults) faults[g] = R.fault[g];
        }
        if (out_plays) memcpy(out_plays, plays.data(), sizeof(tafl_play) * plays.size());
    }
};

extern "C" {
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
}
