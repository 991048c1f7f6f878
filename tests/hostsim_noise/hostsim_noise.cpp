// hostsim_noise.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  Dirichlet noise at the root of a guided search (include/taflhip.h
// tafl_root_noise) on the host: the lock-step search (k_gmcts_step<NL, W, true>), the guided self-play run (k_gselfplay_step<NL, W, true>),
// the eta rows (k_root_noise_eval) and the dense root priors (k_gmcts_root_priors), one game after the other around the product's per-game
// functions of tafl_guided.hpp.  The host's libm and the device's math library may round log / exp / cos differently, so eta is not
// comparable bit for bit between the two; each side's searches are compared with a twin fed that side's own eta.
#include "../hostsim/hostsim_common.hpp"
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_host.hpp"

static RootNoise noise_of(const tafl_root_noise* c) {
    RootNoise nz; nz.alpha = c->alpha; nz.epsilon = c->epsilon; nz.seed = c->seed; nz.gid = c->game_id_base; nz.move_no = c->move_no;
    return nz;
}

struct NoiseBase : GuidedCounts {
    virtual ~NoiseBase() {}
    virtual uint32_t step(const float* priors, const float* values) = 0;
    virtual void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) = 0;
    virtual void root_children(tafl_root_child* out, uint32_t max_children, uint32_t* out_n) = 0;
    virtual void root_priors(double* out) = 0;
    virtual void end(tafl_state* st, tafl_play* plays, uint32_t* moves, uint8_t* faults) = 0;
};
// n_moves == 0: a lock-step search (tafl_gmcts_begin / tafl_gmcts_step); otherwise a run (tafl_gselfplay_begin / _step / _end).  `noise`
// == NULL: the existing noise-free functions.
template <int NL, int W>
struct NoiseSession : NoiseBase {
    using GD = Guided<NL, W>;
    using IO = StateIO<NL>;
    GuidedArena<NL, W> R; GSelfPlay sp; SelfPlayRec rec; uint32_t n_sims, n_moves; double c_puct; bool noisy; RootNoise nz;
    std::vector<Quad> soa; std::vector<uint32_t> mdone; std::vector<tafl_play> plays;
    int init(const tafl_rules* r, uint8_t side, const tafl_state* st, uint32_t G, uint32_t sims_, uint32_t edges_per_node, double cp, const tafl_root_noise* noise,
             const tafl_selfplay_opts* o, uint32_t n_moves_, uint64_t base, ExHost* ex) {
        if (R.init(r, side, G, sims_, edges_per_node)) return -1;
        n_sims = sims_; c_puct = cp; n_moves = n_moves_; noisy = noise != nullptr;
        if (noisy) nz = noise_of(noise);
        mdone.resize(G); soa.resize((size_t)IO::QUADS * G); plays.assign((size_t)n_moves * G, tafl_play{});
        sp.moves_done = mdone.data(); sp.plays = plays.data(); sp.n_moves = n_moves;
        if (n_moves) rec = make_rec(ex, o, base);
        for (uint32_t g = 0; g < G; ++g) {
            DState<NL> s; state_from_abi<NL>(st[g], s); IO::store_soa(soa.data(), G, g, s);
            if (n_moves) GD::selfplay_init(R.M, g, s, sp); else GD::init_game(R.M, g, s);
        }
        step(nullptr, nullptr);
        return 0;
    }
    uint32_t step(const float* priors, const float* values) override {
        return R.round(priors, values, *this, [&](uint32_t g, const float* pr, float v, GuidedStats& gs) {
            if (n_moves) {
                if (noisy) GD::selfplay_step(R.M, g, soa.data(), pr, v, R.A, c_puct, n_sims, sp, rec, R.C, gs, nz);
                else GD::selfplay_step(R.M, g, soa.data(), pr, v, R.A, c_puct, n_sims, sp, rec, R.C, gs);
            } else if (noisy) { RootNoise mine = nz; mine.gid += g; GD::step(R.M, g, pr, v, R.A, c_puct, n_sims, R.C, gs, mine); }
            else GD::step(R.M, g, pr, v, R.A, c_puct, n_sims, R.C, gs);
        });
    }
    void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) override { R.leaves(boards, sides, waiting); }
    void root_children(tafl_root_child* out, uint32_t max_children, uint32_t* out_n) override {
        for (uint32_t g = 0; g < R.M.G; ++g) out_n[g] = GD::root_children(R.M, g, out + (size_t)g * max_children, max_children);
    }
    void root_priors(double* out) override {
        memset(out, 0, sizeof(double) * (size_t)R.M.G * R.A);
        for (uint32_t g = 0; g < R.M.G; ++g) GD::root_priors(R.M, g, out + (size_t)g * R.A);
    }
    void end(tafl_state* st, tafl_play* out_plays, uint32_t* moves, uint8_t* faults) override {
        for (uint32_t g = 0; g < R.M.G; ++g) {
            if (st) { DState<NL> t; IO::load_soa(soa.data(), R.M.G, g, t); state_to_abi<NL>(t, (uint8_t)R.n, st[g]); }
            if (moves) moves[g] = mdone[g] & ~kGspStopped;
            if (faults) faults[g] = R.fault[g];
        }
        if (out_plays && !plays.empty()) memcpy(out_plays, plays.data(), sizeof(tafl_play) * plays.size());
    }
    // k_root_noise_eval
    static int eta(const tafl_rules* r, uint8_t side, const tafl_state* st, uint32_t G, const tafl_root_noise* noise, double* out) {
        Consts<NL> C; if (make_consts<NL, W>(*r, side, C)) return -1;
        const uint32_t A = (uint32_t)side * side * 2u * (side - 1u);
        memset(out, 0, sizeof(double) * (size_t)G * A);
        for (uint32_t g = 0; g < G; ++g) {
            DState<NL> s; state_from_abi<NL>(st[g], s);
            RootNoise mine = noise_of(noise); mine.gid += g;
            GD::noise_row(s, C, mine, out + (size_t)g * A);
        }
        return 0;
    }
};

extern "C" {
void* hsn_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, uint32_t G, uint32_t n_sims, uint32_t edges_per_node, double c_puct,
                const tafl_root_noise* noise, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t base, void* ex) {
    ExHost* x = (ExHost*)ex;
    if ((x && (x->G != G || x->n != n)) || (n_moves && !o)) return nullptr;
    NoiseBase* s = nullptr; int rc = -2;
    if (word_bits == 64) { auto* p = new NoiseSession<2, 7>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, noise, o, n_moves, base, x); s = p; }
    else if (word_bits == 128) { auto* p = new NoiseSession<4, 11>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, noise, o, n_moves, base, x); s = p; }
    else if (word_bits == 256) { auto* p = new NoiseSession<8, 15>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, noise, o, n_moves, base, x); s = p; }
    if (rc) { delete s; return nullptr; }
    return s;
}
void hsn_free(void* h) { delete (NoiseBase*)h; }
uint32_t hsn_step(void* h, const float* priors, const float* values) { return ((NoiseBase*)h)->step(priors, values); }
void hsn_leaves(void* h, uint8_t* boards, uint8_t* sides, uint8_t* waiting) { ((NoiseBase*)h)->leaves(boards, sides, waiting); }
void hsn_root_children(void* h, tafl_root_child* out, uint32_t max_children, uint32_t* out_n) { ((NoiseBase*)h)->root_children(out, max_children, out_n); }
void hsn_root_priors(void* h, double* out) { ((NoiseBase*)h)->root_priors(out); }
// the batch states, the plays [m * G + g], the moves made, out4 = sims, predicts, terminal hits, faults, and the games' fault flags
void hsn_end(void* h, tafl_state* st, tafl_play* plays, uint32_t* moves, uint64_t* out4, uint8_t* faults) {
    NoiseBase* s = (NoiseBase*)h; s->end(st, plays, moves, faults);
    out4[0] = s->sims; out4[1] = s->predicts; out4[2] = s->terminal_hits; out4[3] = s->faults;
}
int hsn_eta(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, uint32_t G, const tafl_root_noise* noise, double* out) {
    switch (word_bits) {
        case 64:  return NoiseSession<2, 7>::eta(r, n, st, G, noise, out);
        case 128: return NoiseSession<4, 11>::eta(r, n, st, G, noise, out);
        case 256: return NoiseSession<8, 15>::eta(r, n, st, G, noise, out);
        default:  return -2;
    }
}
// the examples buffer of a recording run (ExHost of hostsim_common.hpp)
void* hsn_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return new ExHost(G, n, max_moves, K); }
void hsn_ex_free(void* h) { delete (ExHost*)h; }
void hsn_ex_counts(void* h, uint32_t* len, uint64_t* counters) { ((ExHost*)h)->counts(len, counters); }
int hsn_ex_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits) { return ((ExHost*)h)->read(e, out5, board, actions, visits); }
}

#ifdef HSN_MAIN
// the stand-alone program of the ubsan target: a Brandubh start position, constant priors; a noisy search, a noisy run, the eta rows for
// alpha 0.3 and 0.03; prints a checksum so that nothing is optimised away
#include <stdio.h>
int main() {
    tafl_rules r; tafl_state st[3];
    if (preset_rules("brandubh", &r)) { printf("no preset\n"); return 1; }
    for (int g = 0; g < 3; ++g) if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st[g], nullptr)) { printf("bad fen\n"); return 1; }
    const uint32_t A = 7 * 7 * 12;
    std::vector<float> pri((size_t)3 * A, 1.0f), val(3, 0.25f);
    double acc = 0.0;
    for (double alpha : {0.3, 0.03, 1.0, 2.5}) {
        tafl_root_noise nz; memset(&nz, 0, sizeof nz); nz.alpha = alpha; nz.epsilon = 0.25; nz.seed = 7; nz.game_id_base = 100; nz.move_no = 3;
        std::vector<double> eta((size_t)3 * A);
        if (hsn_eta(&r, 7, 64, st, 3, &nz, eta.data())) { printf("eta failed\n"); return 1; }
        for (double v : eta) acc += v;
        tafl_selfplay_opts o; memset(&o, 0, sizeof o); o.sample_seed = 5; o.temp_moves = 1;
        for (uint32_t n_moves : {0u, 2u}) {
            void* h = hsn_begin(&r, 7, 64, st, 3, 12, 128, 1.25, &nz, &o, n_moves, 9, nullptr);
            if (!h) { printf("begin failed\n"); return 1; }
            uint32_t w = 3, rounds = 0;
            while (w && rounds++ < 200) w = hsn_step(h, pri.data(), val.data());
            std::vector<double> p((size_t)3 * A); hsn_root_priors(h, p.data());
            for (double v : p) acc += v;
            hsn_free(h);
        }
    }
    printf("checksum %.6f\n", acc);
    return 0;
}
#endif
