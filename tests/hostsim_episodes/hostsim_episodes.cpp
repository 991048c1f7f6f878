// hostsim_episodes.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  A guided self-play run in episodes (include/taflhip.h
// tafl_gselfplay_begin_episodes) on the host: the round (k_gselfplay_episodes<NL, W> and <NL, W, true>) and then the close-and-reopen
// (k_gselfplay_reopen) over all lanes, one after the other, around the product's per-game functions of tafl_guided.hpp; the examples buffer
// with its open_from array and tafl_examples_finalize (examples_settle of tafl_examples.hpp).
#include "../hostsim/hostsim_common.hpp"
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_host.hpp"

// tafl_examples of an episodes run: ExHost and the open_from array (zero at create)
struct ExEp : ExHost {
    std::vector<uint32_t> open_from;
    ExEp(uint32_t G_, uint8_t n_, uint32_t max_moves_, uint32_t K_) : ExHost(G_, n_, max_moves_, K_), open_from(G_, 0u) {}
};

struct EpBase : GuidedCounts {
    virtual ~EpBase() {}
    virtual uint32_t step(const float* priors, const float* values) = 0;
    virtual void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) = 0;
    virtual void end(tafl_state* st, tafl_play* plays, uint32_t* moves, uint8_t* faults, uint32_t* episodes, uint64_t* counters) = 0;
};
template <int NL, int W>
struct EpSession : EpBase {
    using GD = Guided<NL, W>;
    using IO = StateIO<NL>;
    GuidedArena<NL, W> R; GSelfPlay sp; GEpisodes ep; SelfPlayRec rec; uint32_t n_sims; double c_puct; bool noisy; RootNoise nz;
    std::vector<Quad> soa, open; std::vector<uint32_t> mdone, episode, ep_start; std::vector<tafl_play> plays; unsigned long long epc[EP_COUNT];
    // tafl_gselfplay_begin_episodes: the arena, k_gselfplay_init, the copy of the openings, and the first round
    int init(const tafl_rules* r, uint8_t side, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t sims_, uint32_t edges_per_node, double cp,
             const tafl_root_noise* noise, const tafl_selfplay_opts* o, uint32_t lane_moves, uint64_t base, uint64_t id_stride, uint32_t episode_moves, ExEp* ex) {
        if (R.init(r, side, G, sims_, edges_per_node)) return -1;
        n_sims = sims_; c_puct = cp; noisy = noise != nullptr;
        if (noisy) { nz.alpha = noise->alpha; nz.epsilon = noise->epsilon; nz.seed = noise->seed; nz.gid = noise->game_id_base; nz.move_no = noise->move_no; }
        mdone.assign(G, 0); episode.assign(G, 0); ep_start.assign(G, 0); soa.resize((size_t)IO::QUADS * G); open.resize((size_t)IO::QUADS * G);
        plays.assign((size_t)lane_moves * G, tafl_play{}); memset(epc, 0, sizeof epc);
        sp.moves_done = mdone.data(); sp.plays = plays.data(); sp.n_moves = lane_moves;
        ep.episode_moves = episode_moves; ep.episode = episode.data(); ep.ep_start = ep_start.data(); ep.openings = open.data(); ep.ep_counters = epc;
        ep.id_stride = id_stride ? id_stride : (uint64_t)G; ep.open_from = ex ? ex->open_from.data() : nullptr;
        rec = SelfPlayRec{};
        if (ex) rec.ex = ex->mem();
        rec.sample_seed = o->sample_seed; rec.game_id_base = base; rec.temp_moves = o->temp_moves; rec.move_base = o->move_base;
        for (uint32_t g = 0; g < G; ++g) {
            DState<NL> s; state_from_abi<NL>(st[g], s); IO::store_soa(soa.data(), G, g, s);
            DState<NL> t; state_from_abi<NL>((openings ? openings : st)[g], t); IO::store_soa(open.data(), G, g, t);
            GD::selfplay_init(R.M, g, s, sp);
        }
        step(nullptr, nullptr);
        return 0;
    }
    uint32_t step(const float* priors, const float* values) override {
        uint32_t waiting = R.round(priors, values, *this, [&](uint32_t g, const float* pr, float v, GuidedStats& gs) {
            if (noisy) GD::selfplay_step_episodes(R.M, g, soa.data(), pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz);
            else GD::selfplay_step_episodes(R.M, g, soa.data(), pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs);
        });
        for (uint32_t g = 0; g < R.M.G; ++g) waiting += GD::selfplay_reopen(R.M, g, soa.data(), sp, ep, rec) ? 1u : 0u;
        return waiting;
    }
    void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) override { R.leaves(boards, sides, waiting); }
    void end(tafl_state* st, tafl_play* out_plays, uint32_t* moves, uint8_t* faults, uint32_t* episodes, uint64_t* counters) override {
        for (uint32_t g = 0; g < R.M.G; ++g) {
            if (st) { DState<NL> t; IO::load_soa(soa.data(), R.M.G, g, t); state_to_abi<NL>(t, (uint8_t)R.n, st[g]); }
            if (moves) moves[g] = mdone[g] & ~(kGspStopped | kGspEpisodeEnded);
            if (faults) faults[g] = R.fault[g];
            if (episodes) episodes[g] = episode[g];
        }
        if (counters) for (int i = 0; i < EP_COUNT; ++i) counters[i] = epc[i];
        if (out_plays && !plays.empty()) memcpy(out_plays, plays.data(), sizeof(tafl_play) * plays.size());
    }
};
// k_examples_finalize: one game after the other, the flags word of its current state
template <int NL>
static int finalize_as(ExEp* ex, const tafl_state* st) {
    const ExamplesMem X = ex->mem();
    for (uint32_t g = 0; g < ex->G; ++g) { DState<NL> s; state_from_abi<NL>(st[g], s); examples_settle(X, g, ex->open_from[g], s.flags); }
    return 0;
}

extern "C" {
void* hse_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t n_sims, uint32_t edges_per_node,
                double c_puct, const tafl_root_noise* noise, const tafl_selfplay_opts* o, uint32_t lane_moves, uint64_t base, uint64_t id_stride, uint32_t episode_moves, void* ex) {
    ExEp* x = (ExEp*)ex;
    if ((x && (x->G != G || x->n != n)) || !o || o->move_base != 0 || lane_moves == 0) return nullptr;
    EpBase* s = nullptr; int rc = -2;
    if (word_bits == 64) { auto* p = new EpSession<2, 7>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, noise, o, lane_moves, base, id_stride, episode_moves, x); s = p; }
#ifndef HSE_MAIN      /* (the sanitizer program plays Brandubh only) */
    else if (word_bits == 128) { auto* p = new EpSession<4, 11>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, noise, o, lane_moves, base, id_stride, episode_moves, x); s = p; }
    else if (word_bits == 256) { auto* p = new EpSession<8, 15>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, noise, o, lane_moves, base, id_stride, episode_moves, x); s = p; }
#endif
    if (rc) { delete s; return nullptr; }
    return s;
}
void hse_free(void* h) { delete (EpBase*)h; }
uint32_t hse_step(void* h, const float* priors, const float* values) { return ((EpBase*)h)->step(priors, values); }
void hse_leaves(void* h, uint8_t* boards, uint8_t* sides, uint8_t* waiting) { ((EpBase*)h)->leaves(boards, sides, waiting); }
// the batch states, the plays [m * G + g], the moves made, out4 = sims, predicts, terminal hits, faults, the lanes' fault flags, the episodes
// closed or cut per lane and the counters attacker wins, defender wins, draws, cut
void hse_end(void* h, tafl_state* st, tafl_play* plays, uint32_t* moves, uint64_t* out4, uint8_t* faults, uint32_t* episodes, uint64_t* counters) {
    EpBase* s = (EpBase*)h; s->end(st, plays, moves, faults, episodes, counters);
    out4[0] = s->sims; out4[1] = s->predicts; out4[2] = s->terminal_hits; out4[3] = s->faults;
}
void* hse_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return new ExEp(G, n, max_moves, K); }
void hse_ex_free(void* h) { delete (ExEp*)h; }
void hse_ex_counts(void* h, uint32_t* len, uint64_t* counters, uint32_t* open_from) {
    ExEp* x = (ExEp*)h; x->counts(len, counters);
    if (open_from) for (uint32_t g = 0; g < x->G; ++g) open_from[g] = x->open_from[g];
}
int hse_ex_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits, float* z, uint8_t* fin) {
    ExEp* x = (ExEp*)h;
    if (x->read(e, out5, board, actions, visits)) return -1;
    *z = x->z[e]; *fin = x->fin[e];
    return 0;
}
int hse_ex_finalize(void* ex, uint32_t word_bits, const tafl_state* st) {
    switch (word_bits) {
        case 64:  return finalize_as<2>((ExEp*)ex, st);
#ifndef HSE_MAIN
        case 128: return finalize_as<4>((ExEp*)ex, st);
        case 256: return finalize_as<8>((ExEp*)ex, st);
#endif
        default:  return -2;
    }
}
}

#ifdef HSE_MAIN
// the stand-alone program of the sanitizer target: Brandubh, 6 lanes from positions some random plies into the game, constant priors, a
// lane budget of 40 with episodes capped at 9 moves, without and with root noise; then finalize.  Prints what it counted.
#include <stdio.h>
int main() {
    tafl_rules r; const uint32_t G = 6, A = 7 * 7 * 12, budget = 40;
    if (preset_rules("brandubh", &r)) { printf("no preset\n"); return 1; }
    Consts<2> C; if (make_consts<2, 7>(r, 7, C)) { printf("no consts\n"); return 1; }
    std::vector<tafl_state> st(G);
    for (uint32_t g = 0; g < G; ++g) {
        if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st[g], nullptr)) { printf("bad fen\n"); return 1; }
        DState<2> s; state_from_abi<2>(st[g], s);
        Ops<2, 7>::random_advance(s, 21, g, 9 * g, C, false);
        state_to_abi<2>(s, 7, st[g]);
    }
    std::vector<float> pri((size_t)G * A, 1.0f), val(G, 0.25f);
    unsigned long long acc = 0;
    for (int noisy = 0; noisy < 2; ++noisy) {
        tafl_root_noise nz; memset(&nz, 0, sizeof nz); nz.alpha = 0.3; nz.epsilon = 0.25; nz.seed = 7;
        tafl_selfplay_opts o; memset(&o, 0, sizeof o); o.sample_seed = 5; o.temp_moves = 4;
        void* ex = hse_ex_new(G, 7, budget - 3, 8);                       // (a buffer that drops and overflows)
        void* h = hse_begin(&r, 7, 64, st.data(), nullptr, G, 12, 128, 1.25, noisy ? &nz : nullptr, &o, budget, 100, 0, 9, ex);
        if (!h) { printf("begin failed\n"); return 1; }
        uint32_t w = 1, rounds = 0;
        while (w && rounds++ < 100000) w = hse_step(h, pri.data(), val.data());
        std::vector<tafl_state> out(G); std::vector<tafl_play> plays((size_t)G * budget); std::vector<uint32_t> moves(G), eps(G); std::vector<uint8_t> faults(G);
        uint64_t c4[4], ec[4];
        hse_end(h, out.data(), plays.data(), moves.data(), c4, faults.data(), eps.data(), ec);
        hse_ex_finalize(ex, 64, out.data());
        for (uint32_t g = 0; g < G; ++g) acc += moves[g] + 100u * eps[g];
        printf("noise %d: rounds %u sims %llu episodes closed %llu+%llu+%llu cut %llu\n", noisy, rounds, (unsigned long long)c4[0], (unsigned long long)ec[0],
               (unsigned long long)ec[1], (unsigned long long)ec[2], (unsigned long long)ec[3]);
        hse_free(h); hse_ex_free(ex);
    }
    printf("checksum %llu\n", acc);
    return 0;
}
#endif
