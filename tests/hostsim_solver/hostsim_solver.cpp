// hostsim_solver.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  A guided self-play run with exact win/loss proofs (include/taflhip.h
// tafl_solver) on the host: the solver round (k_gselfplay_solver<NL, W, NOISE, EPISODES>: the product's selfplay_step_solver) over all
// lanes, one after the other, and for an episodes run the close-and-reopen (Guided::selfplay_reopen) after it; with or without root noise,
// a playout cap and forced playouts, as gselfplay_begin latches the settings.  Without the solver the session runs what
// tests/hostsim_forced runs.  The examples buffer is tests/hostsim_episodes' ExEp.
#include "../hostsim/hostsim_common.hpp"
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_host.hpp"

struct ExEp : ExHost {
    std::vector<uint32_t> open_from;
    ExEp(uint32_t G_, uint8_t n_, uint32_t max_moves_, uint32_t K_) : ExHost(G_, n_, max_moves_, K_), open_from(G_, 0u) {}
};

struct SvBase : GuidedCounts {
    unsigned long long capc[CAP_COUNT] = {0, 0}, fpc[FP_COUNT] = {0, 0, 0, 0}, svc[SV_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    virtual void root_children(tafl_root_child* out, uint32_t max_children, uint32_t* out_n) = 0;
    virtual ~SvBase() {}
    virtual uint32_t step(const float* priors, const float* values) = 0;
    virtual void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) = 0;
    virtual void end(tafl_state* st, tafl_play* plays, uint32_t* moves, uint8_t* faults, uint32_t* episodes, uint64_t* counters) = 0;
};
template <int NL, int W>
struct SvSession : SvBase {
    using GD = Guided<NL, W>;
    using IO = StateIO<NL>;
    GuidedArena<NL, W> R; GSelfPlay sp; GEpisodes ep; SelfPlayRec rec; uint32_t n_sims; double c_puct; bool noisy, episodes, capped, forced, solver; RootNoise nz; PlayoutCap pc; ForcedPlayouts fp; SolverCfg sv;
    std::vector<Quad> soa, open; std::vector<uint32_t> mdone, episode, ep_start; std::vector<tafl_play> plays; unsigned long long epc[EP_COUNT];
    // tafl_gselfplay_begin / tafl_gselfplay_begin_episodes (eps != 0) with the batch's noise and cap settings latched: the arena is sized
    // by n_sims, k_gselfplay_init, the copy of the openings, and the first round
    int init(const tafl_rules* r, uint8_t side, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t sims_, uint32_t edges_per_node, double cp,
             const tafl_root_noise* noise, const tafl_playout_cap* cap, const tafl_forced_playouts* fcfg, const tafl_solver* scfg, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t base, int eps,
             uint64_t id_stride, uint32_t episode_moves, ExEp* ex) {
        if (R.init(r, side, G, sims_, edges_per_node)) return -1;
        n_sims = sims_; c_puct = cp; noisy = noise != nullptr; episodes = eps != 0; capped = cap != nullptr; forced = fcfg != nullptr; solver = scfg != nullptr;
        nz = RootNoise{}; pc = PlayoutCap{}; fp = ForcedPlayouts{};
        if (noisy) { nz.alpha = noise->alpha; nz.epsilon = noise->epsilon; nz.seed = noise->seed; nz.gid = noise->game_id_base; nz.move_no = noise->move_no; }
        if (capped) { pc.seed = cap->seed; pc.fast_sims = cap->fast_sims; pc.full_per_65536 = cap->full_per_65536; }
        else { pc.fast_sims = sims_; pc.full_per_65536 = 65536u; }                  // (gselfplay_begin: a forced run without a cap passes "every move full")
        pc.counters = capc;
        if (forced) { fp.k = fcfg->k; fp.counters = fpc; }                             // (without it the solver rounds get k == 0 and no counters, as from gselfplay_begin)
        sv = SolverCfg{}; if (solver) sv.counters = svc;
        mdone.assign(G, 0); episode.assign(G, 0); ep_start.assign(G, 0); soa.resize((size_t)IO::QUADS * G); open.resize((size_t)IO::QUADS * G);
        plays.assign((size_t)n_moves * G, tafl_play{}); memset(epc, 0, sizeof epc);
        sp.moves_done = mdone.data(); sp.plays = plays.data(); sp.n_moves = n_moves;
        ep = GEpisodes{};
        ep.episode_moves = episode_moves; ep.episode = episode.data(); ep.ep_start = ep_start.data(); ep.openings = open.data(); ep.ep_counters = epc;
        ep.id_stride = id_stride ? id_stride : (uint64_t)G; ep.open_from = ex ? ex->open_from.data() : nullptr;
        rec = make_rec(ex, o, base);
        for (uint32_t g = 0; g < G; ++g) {
            DState<NL> s; state_from_abi<NL>(st[g], s); IO::store_soa(soa.data(), G, g, s);
            DState<NL> t; state_from_abi<NL>((openings ? openings : st)[g], t); IO::store_soa(open.data(), G, g, t);
            GD::selfplay_init(R.M, g, s, sp);
        }
        step(nullptr, nullptr);
        return 0;
    }
    // gselfplay_launch: the capped round of the run's shape, or without a cap the round the library launches today
    void one(uint32_t g, const float* pr, float v, GuidedStats& gs) {
        Quad* s = soa.data();
        if (solver) {
            if (episodes) { if (noisy) GD::template selfplay_step_solver<true, true>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp, sv);
                            else GD::template selfplay_step_solver<false, true>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp, sv); }
            else { if (noisy) GD::template selfplay_step_solver<true, false>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp, sv);
                   else GD::template selfplay_step_solver<false, false>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp, sv); }
        } else if (forced) {
            if (episodes) { if (noisy) GD::template selfplay_step_forced<true, true>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp);
                            else GD::template selfplay_step_forced<false, true>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp); }
            else { if (noisy) GD::template selfplay_step_forced<true, false>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp);
                   else GD::template selfplay_step_forced<false, false>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc, fp); }
        } else if (capped) {
            if (episodes) { if (noisy) GD::template selfplay_step_capped<true, true>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc);
                            else GD::template selfplay_step_capped<false, true>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc); }
            else { if (noisy) GD::template selfplay_step_capped<true, false>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc);
                   else GD::template selfplay_step_capped<false, false>(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz, pc); }
        } else if (episodes) {
            if (noisy) GD::selfplay_step_episodes(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs, nz);
            else GD::selfplay_step_episodes(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs);
        } else {
            if (noisy) GD::selfplay_step(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, rec, R.C, gs, nz);
            else GD::selfplay_step(R.M, g, s, pr, v, R.A, c_puct, n_sims, sp, rec, R.C, gs);
        }
    }
    uint32_t step(const float* priors, const float* values) override {
        uint32_t waiting = R.round(priors, values, *this, [&](uint32_t g, const float* pr, float v, GuidedStats& gs) { one(g, pr, v, gs); });
        if (episodes) for (uint32_t g = 0; g < R.M.G; ++g) waiting += GD::selfplay_reopen(R.M, g, soa.data(), sp, ep, rec) ? 1u : 0u;
        return waiting;
    }
    void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) override { R.leaves(boards, sides, waiting); }
    // the root's edge block as the run left it: after a run of ONE move (the lane stops before a fresh arena is made) the pruned counts n'
    void root_children(tafl_root_child* out, uint32_t max_children, uint32_t* out_n) override {
        for (uint32_t g = 0; g < R.M.G; ++g) out_n[g] = GD::root_children(R.M, g, out + (size_t)g * max_children, max_children);
    }
    void end(tafl_state* st, tafl_play* out_plays, uint32_t* moves, uint8_t* faults, uint32_t* episodes_out, uint64_t* counters) override {
        for (uint32_t g = 0; g < R.M.G; ++g) {
            if (st) { DState<NL> t; IO::load_soa(soa.data(), R.M.G, g, t); state_to_abi<NL>(t, (uint8_t)R.n, st[g]); }
            if (moves) moves[g] = mdone[g] & ~(kGspStopped | kGspEpisodeEnded);
            if (faults) faults[g] = R.fault[g];
            if (episodes_out) episodes_out[g] = episode[g];
        }
        if (counters) for (int i = 0; i < EP_COUNT; ++i) counters[i] = epc[i];
        if (out_plays && !plays.empty()) memcpy(out_plays, plays.data(), sizeof(tafl_play) * plays.size());
    }
};

extern "C" {
// what tafl_gselfplay_set_playout_cap and the begin check: 0 ok, -1 TAFL_ERR_INVALID_ARG, -5 TAFL_ERR_UNSUPPORTED
int hss_cap_check(const tafl_playout_cap* cap, uint32_t n_sims) {
    if (cap->fast_sims < 2u || cap->fast_sims > 0xFFFFu || cap->full_per_65536 > 65536u) return -1;
    if (cap->flags != 0 || cap->_reserved[0] != 0 || cap->_reserved[1] != 0 || cap->_reserved[2] != 0) return -5;
    return cap->fast_sims > n_sims ? -1 : 0;
}
// what tafl_gselfplay_set_forced_playouts checks
int hss_forced_check(const tafl_forced_playouts* f) {
    if (!(f->k > 0.0) || !(f->k <= 64.0)) return -1;
    if (f->flags != 0) return -5;
    for (uint32_t r : f->_reserved) if (r != 0) return -5;
    return 0;
}
// what tafl_gselfplay_set_solver checks
int hss_solver_check(const tafl_solver* c) {
    if (c->flags != 0) return -5;
    for (uint32_t r : c->_reserved) if (r != 0) return -5;
    return 0;
}
// the sizes the proofs must not change (tafl_solver rule 7)
void hss_sizes(uint32_t* out2) { out2[0] = (uint32_t)sizeof(GNode); out2[1] = (uint32_t)sizeof(GEdge); }
void* hss_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t n_sims, uint32_t edges_per_node,
                double c_puct, const tafl_root_noise* noise, const tafl_playout_cap* cap, const tafl_forced_playouts* fcfg, const tafl_solver* scfg, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t base,
                int episodes, uint64_t id_stride, uint32_t episode_moves, void* ex) {
    ExEp* x = (ExEp*)ex;
    if ((x && (x->G != G || x->n != n)) || !o || n_moves == 0 || (episodes && o->move_base != 0) || (cap && hss_cap_check(cap, n_sims)) || (fcfg && hss_forced_check(fcfg)) || (scfg && hss_solver_check(scfg))) return nullptr;
    SvBase* s = nullptr; int rc = -2;
    if (word_bits == 64) { auto* p = new SvSession<2, 7>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, noise, cap, fcfg, scfg, o, n_moves, base, episodes, id_stride, episode_moves, x); s = p; }
#ifndef HSS_MAIN      /* (the sanitizer program plays Brandubh only) */
    else if (word_bits == 128) { auto* p = new SvSession<4, 11>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, noise, cap, fcfg, scfg, o, n_moves, base, episodes, id_stride, episode_moves, x); s = p; }
    else if (word_bits == 256) { auto* p = new SvSession<8, 15>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, noise, cap, fcfg, scfg, o, n_moves, base, episodes, id_stride, episode_moves, x); s = p; }
#endif
    if (rc) { delete s; return nullptr; }
    return s;
}
void hss_free(void* h) { delete (SvBase*)h; }
uint32_t hss_step(void* h, const float* priors, const float* values) { return ((SvBase*)h)->step(priors, values); }
void hss_leaves(void* h, uint8_t* boards, uint8_t* sides, uint8_t* waiting) { ((SvBase*)h)->leaves(boards, sides, waiting); }
void hss_root_children(void* h, tafl_root_child* out, uint32_t max_children, uint32_t* out_n) { ((SvBase*)h)->root_children(out, max_children, out_n); }
// as hsf_end of tests/hostsim_forced, and sv8 = the eight counters of tafl_solver_stats in its order
void hss_end(void* h, tafl_state* st, tafl_play* plays, uint32_t* moves, uint64_t* out4, uint8_t* faults, uint32_t* episodes, uint64_t* counters, uint64_t* cap2, uint64_t* fp4,
             uint64_t* sv8) {
    SvBase* s = (SvBase*)h; s->end(st, plays, moves, faults, episodes, counters);
    out4[0] = s->sims; out4[1] = s->predicts; out4[2] = s->terminal_hits; out4[3] = s->faults;
    cap2[0] = s->capc[CAP_FULL]; cap2[1] = s->capc[CAP_FAST];
    for (int i = 0; i < FP_COUNT; ++i) fp4[i] = s->fpc[i];
    for (int i = 0; i < SV_COUNT; ++i) sv8[i] = s->svc[i];
}
void* hss_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return new ExEp(G, n, max_moves, K); }
void hss_ex_free(void* h) { delete (ExEp*)h; }
void hss_ex_counts(void* h, uint32_t* len, uint64_t* counters, uint32_t* open_from) {
    ExEp* x = (ExEp*)h; x->counts(len, counters);
    if (open_from) for (uint32_t g = 0; g < x->G; ++g) open_from[g] = x->open_from[g];
}
int hss_ex_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits, float* z, uint8_t* fin) {
    ExEp* x = (ExEp*)h;
    if (x->read(e, out5, board, actions, visits)) return -1;
    *z = x->z[e]; *fin = x->fin[e];
    return 0;
}
}

#ifdef HSS_MAIN
// the stand-alone program of the sanitizer target: Brandubh, 8 lanes from positions late in random games (so that terminals are in
// reach), constant priors, S = 24; one solver plain run of 10 moves and one solver episodes run with root noise, a cap (fast_sims 3, half
// of the moves full) and forced playouts (k = 2), a lane budget of 40 and episodes capped at 9 moves, into a buffer that drops and
// overflows.  Prints what it counted.
#include <stdio.h>
int main() {
    tafl_rules r; const uint32_t G = 8, A = 7 * 7 * 12;
    if (preset_rules("brandubh", &r)) { printf("no preset\n"); return 1; }
    Consts<2> C; if (make_consts<2, 7>(r, 7, C)) { printf("no consts\n"); return 1; }
    std::vector<tafl_state> st(G);
    for (uint32_t g = 0; g < G; ++g) {
        uint32_t plies = 0;                                                 // the last position of random game g that is still going, a few plies back
        for (uint32_t p = 1; p < 400; ++p) {
            if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st[g], nullptr)) { printf("bad fen\n"); return 1; }
            DState<2> s; state_from_abi<2>(st[g], s);
            Ops<2, 7>::random_advance(s, 77, g, p, C, false);
            if (TAFL_F_STATUS(s.flags) != TAFL_STATUS_ONGOING) break;
            plies = p;
        }
        plies = plies > g % 3u ? plies - g % 3u : 0u;
        if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st[g], nullptr)) { printf("bad fen\n"); return 1; }
        DState<2> s; state_from_abi<2>(st[g], s);
        Ops<2, 7>::random_advance(s, 77, g, plies, C, false);
        state_to_abi<2>(s, 7, st[g]);
    }
    std::vector<float> pri((size_t)G * A, 1.0f), val(G, 0.25f);
    unsigned long long acc = 0;
    for (int eps = 0; eps < 2; ++eps) {
        const uint32_t budget = eps ? 40 : 10;
        tafl_root_noise nz; memset(&nz, 0, sizeof nz); nz.alpha = 0.3; nz.epsilon = 0.25; nz.seed = 7;
        tafl_playout_cap cap; memset(&cap, 0, sizeof cap); cap.seed = 11; cap.fast_sims = 3; cap.full_per_65536 = 32768;
        tafl_forced_playouts fc; memset(&fc, 0, sizeof fc); fc.k = 2.0;
        tafl_solver sc; memset(&sc, 0, sizeof sc);
        tafl_selfplay_opts o; memset(&o, 0, sizeof o); o.sample_seed = 5; o.temp_moves = 4; o.move_base = eps ? 0 : 2;
        void* ex = hss_ex_new(G, 7, eps ? 6 : 2, 4);                       // (a buffer that drops and overflows)
        void* h = hss_begin(&r, 7, 64, st.data(), nullptr, G, 24, 128, 1.25, eps ? &nz : nullptr, eps ? &cap : nullptr, eps ? &fc : nullptr, &sc, &o, budget, 100, eps, 0, eps ? 9 : 0, ex);
        if (!h) { printf("begin failed\n"); return 1; }
        uint32_t w = 1, rounds = 0;
        while (w && rounds++ < 100000) w = hss_step(h, pri.data(), val.data());
        std::vector<tafl_state> out(G); std::vector<tafl_play> plays((size_t)G * budget); std::vector<uint32_t> moves(G), epn(G), len(G); std::vector<uint8_t> faults(G);
        uint64_t c4[4], ec[4], cc[2], f4[4], s8[8], xc[EX_COUNTERS];
        hss_end(h, out.data(), plays.data(), moves.data(), c4, faults.data(), epn.data(), ec, cc, f4, s8);
        hss_ex_counts(ex, len.data(), xc, nullptr);
        unsigned long long made = 0;
        for (uint32_t g = 0; g < G; ++g) { acc += moves[g] + 100u * epn[g]; made += moves[g]; }
        if (cc[0] + cc[1] != made || s8[SV_MOVES] != made) { printf("the counters do not add up to the moves made\n"); return 1; }
        printf("%s: rounds %u sims %llu skipped %llu moves %llu roots won %llu lost %llu nodes won %llu lost %llu pruned visits %llu children %llu forced sims %llu dropped %llu overflowed %llu faults %llu\n",
               eps ? "episodes with noise, a cap and forced playouts" : "plain", rounds, (unsigned long long)c4[0], (unsigned long long)s8[SV_SKIPPED_SIMS], made,
               (unsigned long long)s8[SV_ROOT_WON], (unsigned long long)s8[SV_ROOT_LOST], (unsigned long long)s8[SV_NODES_WON], (unsigned long long)s8[SV_NODES_LOST],
               (unsigned long long)s8[SV_PRUNED_VISITS], (unsigned long long)s8[SV_PRUNED_CHILDREN], (unsigned long long)f4[0], (unsigned long long)xc[0], (unsigned long long)xc[1],
               (unsigned long long)c4[3]);
        hss_free(h); hss_ex_free(ex);
    }
    printf("checksum %llu\n", acc);
    return 0;
}
#endif
