// hostsim_match.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  A match run (include/taflhip.h tafl_gmatch_*) on the host: the
// partition of the waiting lanes by owner as the obvious sequential loop around Guided::match_owner, the round (k_gmatch_round: the
// product's selfplay_step_episodes given the lane's row of its owner's compact batch), the tally (Guided::match_tally) and the
// close-and-reopen (Guided::selfplay_reopen) over all lanes, one after the other.  The examples buffer is tests/hostsim_episodes' ExEp.
#include "../hostsim/hostsim_common.hpp"
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_host.hpp"

struct ExEp : ExHost {
    std::vector<uint32_t> open_from;
    ExEp(uint32_t G_, uint8_t n_, uint32_t max_moves_, uint32_t K_) : ExHost(G_, n_, max_moves_, K_), open_from(G_, 0u) {}
};

struct MatchBase : GuidedCounts {
    virtual ~MatchBase() {}
    virtual void leaves(uint8_t* const boards[2], uint8_t* const sides[2], uint32_t* const lanes[2], uint32_t counts[2]) = 0;
    virtual void step(const float* const priors[2], const float* const values[2]) = 0;
    virtual void end(tafl_state* st, tafl_play* plays, uint32_t* moves, uint8_t* faults, uint32_t* episodes, uint64_t* counters, uint64_t* games) = 0;
};
template <int NL, int W>
struct MatchSession : MatchBase {
    using GD = Guided<NL, W>;
    using IO = StateIO<NL>;
    GuidedArena<NL, W> R; GSelfPlay sp; GEpisodes ep; SelfPlayRec rec; GMatch mt; uint32_t n_sims; double c_puct;
    std::vector<Quad> soa, open; std::vector<uint32_t> mdone, episode, ep_start, row_of; std::vector<tafl_play> plays; unsigned long long epc[EP_COUNT], games[2 * EP_COUNT];
    // tafl_gmatch_begin: tafl_gselfplay_begin_episodes (arena, init, the copy of the openings, the first round) and the match's own buffers
    int init(const tafl_rules* r, uint8_t side, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t sims_, uint32_t edges_per_node, double cp,
             const tafl_selfplay_opts* o, uint32_t lane_moves, uint64_t base, uint64_t id_stride, uint32_t episode_moves, uint32_t swap, ExEp* ex) {
        if (R.init(r, side, G, sims_, edges_per_node)) return -1;
        n_sims = sims_; c_puct = cp;
        mdone.assign(G, 0); episode.assign(G, 0); ep_start.assign(G, 0); row_of.assign(G, kMatchNoRow); soa.resize((size_t)IO::QUADS * G); open.resize((size_t)IO::QUADS * G);
        plays.assign((size_t)lane_moves * G, tafl_play{}); memset(epc, 0, sizeof epc); memset(games, 0, sizeof games);
        sp.moves_done = mdone.data(); sp.plays = plays.data(); sp.n_moves = lane_moves;
        ep.episode_moves = episode_moves; ep.episode = episode.data(); ep.ep_start = ep_start.data(); ep.openings = open.data(); ep.ep_counters = epc;
        ep.id_stride = id_stride ? id_stride : (uint64_t)G; ep.open_from = ex ? ex->open_from.data() : nullptr;
        mt.swap = swap; mt.row_of = row_of.data(); mt.games = games;
        rec = SelfPlayRec{};
        if (ex) rec.ex = ex->mem();
        rec.sample_seed = o->sample_seed; rec.game_id_base = base; rec.temp_moves = o->temp_moves; rec.move_base = o->move_base;
        for (uint32_t g = 0; g < G; ++g) {
            DState<NL> s; state_from_abi<NL>(st[g], s); IO::store_soa(soa.data(), G, g, s);
            DState<NL> t; state_from_abi<NL>((openings ? openings : st)[g], t); IO::store_soa(open.data(), G, g, t);
            GD::selfplay_init(R.M, g, s, sp);
        }
        const float* none[2] = {nullptr, nullptr};
        step(none, none);
        return 0;
    }
    // tafl_gmatch_leaves: the partition, then the planes of each row
    void leaves(uint8_t* const boards[2], uint8_t* const sides[2], uint32_t* const lanes[2], uint32_t counts[2]) override {
        const uint32_t G = R.M.G, n = R.n;
        counts[0] = counts[1] = 0;
        for (uint32_t g = 0; g < G; ++g) {
            row_of[g] = kMatchNoRow;
            if (R.M.kind[g] != 1) continue;
            const uint32_t e = GD::match_owner(rec.game_id_base, g, episode[g], mt.swap, GD::batch_flags(soa.data(), G, g)), row = counts[e]++;
            row_of[g] = (e << 31) | row;
            lanes[e][row] = g;
            DState<NL> s; IO::load_rec(R.M.node_state + ((size_t)R.M.leaf[g] * G + g) * IO::QUADS, s);
            for (uint32_t r = 0; r < n; ++r) for (uint32_t c = 0; c < n; ++c) boards[e][((size_t)row * n + r) * n + c] = (uint8_t)Ops<NL, W>::board_byte(s, r, c, R.C);
            sides[e][row] = (uint8_t)((s.flags & TAFL_F_SIDE) ? TAFL_DEFENDER : TAFL_ATTACKER);
        }
    }
    // tafl_gmatch_step: k_gmatch_round, k_gmatch_tally, k_gselfplay_reopen
    void step(const float* const priors[2], const float* const values[2]) override {
        for (uint32_t g = 0; g < R.M.G; ++g) {
            GuidedStats gs; memset(&gs, 0, sizeof gs);
            const uint32_t r = row_of[g];
            const float* pr = nullptr; float v = 0.f;
            if (r != kMatchNoRow && priors[r >> 31] && values[r >> 31]) { pr = priors[r >> 31] + (size_t)(r & kMatchRowMask) * R.A; v = values[r >> 31][r & kMatchRowMask]; }
            GD::selfplay_step_episodes(R.M, g, soa.data(), pr, v, R.A, c_puct, n_sims, sp, ep, rec, R.C, gs);
            sims += gs.sims; predicts += gs.predicts; terminal_hits += gs.terminal_hits; faults += gs.faults;
        }
        for (uint32_t g = 0; g < R.M.G; ++g) GD::match_tally(R.M, g, soa.data(), sp, ep, rec, mt);
        for (uint32_t g = 0; g < R.M.G; ++g) GD::selfplay_reopen(R.M, g, soa.data(), sp, ep, rec);
        std::fill(row_of.begin(), row_of.end(), kMatchNoRow);
    }
    void end(tafl_state* st, tafl_play* out_plays, uint32_t* moves, uint8_t* fl, uint32_t* episodes, uint64_t* counters, uint64_t* out_games) override {
        for (uint32_t g = 0; g < R.M.G; ++g) {
            if (st) { DState<NL> t; IO::load_soa(soa.data(), R.M.G, g, t); state_to_abi<NL>(t, (uint8_t)R.n, st[g]); }
            if (moves) moves[g] = mdone[g] & ~(kGspStopped | kGspEpisodeEnded);
            if (fl) fl[g] = R.fault[g];
            if (episodes) episodes[g] = episode[g];
        }
        if (counters) for (int i = 0; i < EP_COUNT; ++i) counters[i] = epc[i];
        if (out_games) for (int i = 0; i < 2 * EP_COUNT; ++i) out_games[i] = games[i];
        if (out_plays && !plays.empty()) memcpy(out_plays, plays.data(), sizeof(tafl_play) * plays.size());
    }
};

extern "C" {
void* hsm_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t n_sims, uint32_t edges_per_node,
                double c_puct, const tafl_selfplay_opts* o, uint32_t lane_moves, uint64_t base, uint64_t id_stride, uint32_t episode_moves, uint32_t swap, void* ex) {
    ExEp* x = (ExEp*)ex;
    if ((x && (x->G != G || x->n != n)) || !o || o->move_base != 0 || lane_moves == 0 || swap > 1) return nullptr;
    MatchBase* s = nullptr; int rc = -2;
    if (word_bits == 64) { auto* p = new MatchSession<2, 7>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, o, lane_moves, base, id_stride, episode_moves, swap, x); s = p; }
#ifndef HSM_MAIN      /* (the sanitizer program plays Brandubh only) */
    else if (word_bits == 128) { auto* p = new MatchSession<4, 11>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, o, lane_moves, base, id_stride, episode_moves, swap, x); s = p; }
    else if (word_bits == 256) { auto* p = new MatchSession<8, 15>(); rc = p->init(r, n, st, openings, G, n_sims, edges_per_node, c_puct, o, lane_moves, base, id_stride, episode_moves, swap, x); s = p; }
#endif
    if (rc) { delete s; return nullptr; }
    return s;
}
void hsm_free(void* h) { delete (MatchBase*)h; }
// boards / sides / lanes of evaluator 0 and of evaluator 1 (room for G rows each), counts[2]
void hsm_leaves(void* h, uint8_t* boards0, uint8_t* sides0, uint32_t* lanes0, uint8_t* boards1, uint8_t* sides1, uint32_t* lanes1, uint32_t* counts) {
    uint8_t* const b[2] = {boards0, boards1}; uint8_t* const s[2] = {sides0, sides1}; uint32_t* const l[2] = {lanes0, lanes1};
    ((MatchBase*)h)->leaves(b, s, l, counts);
}
void hsm_step(void* h, const float* priors0, const float* values0, const float* priors1, const float* values1) {
    const float* const p[2] = {priors0, priors1}; const float* const v[2] = {values0, values1};
    ((MatchBase*)h)->step(p, v);
}
// as hse_end of tests/hostsim_episodes, and games[2 * 4]
void hsm_end(void* h, tafl_state* st, tafl_play* plays, uint32_t* moves, uint64_t* out4, uint8_t* faults, uint32_t* episodes, uint64_t* counters, uint64_t* games) {
    MatchBase* s = (MatchBase*)h; s->end(st, plays, moves, faults, episodes, counters, games);
    out4[0] = s->sims; out4[1] = s->predicts; out4[2] = s->terminal_hits; out4[3] = s->faults;
}
void* hsm_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return new ExEp(G, n, max_moves, K); }
void hsm_ex_free(void* h) { delete (ExEp*)h; }
void hsm_ex_counts(void* h, uint32_t* len, uint64_t* counters, uint32_t* open_from) {
    ExEp* x = (ExEp*)h; x->counts(len, counters);
    if (open_from) for (uint32_t g = 0; g < x->G; ++g) open_from[g] = x->open_from[g];
}
int hsm_ex_example(void* h, uint32_t e, uint32_t* out5, uint8_t* board, uint32_t* actions, uint32_t* visits, float* z, uint8_t* fin) {
    ExEp* x = (ExEp*)h;
    if (x->read(e, out5, board, actions, visits)) return -1;
    *z = x->z[e]; *fin = x->fin[e];
    return 0;
}
}

#ifdef HSM_MAIN
// the stand-alone program of the sanitizer target: Brandubh, 7 lanes from positions some random plies into the game, two constant
// evaluators that differ, a lane budget of 40 with episodes capped at 9 moves, swap 0 and 1.  Prints what it counted.
#include <stdio.h>
int main() {
    tafl_rules r; const uint32_t G = 7, A = 7 * 7 * 12, budget = 40;
    if (preset_rules("brandubh", &r)) { printf("no preset\n"); return 1; }
    Consts<2> C; if (make_consts<2, 7>(r, 7, C)) { printf("no consts\n"); return 1; }
    std::vector<tafl_state> st(G);
    for (uint32_t g = 0; g < G; ++g) {
        if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st[g], nullptr)) { printf("bad fen\n"); return 1; }
        DState<2> s; state_from_abi<2>(st[g], s);
        Ops<2, 7>::random_advance(s, 21, g, 9 * g, C, false);
        state_to_abi<2>(s, 7, st[g]);
    }
    std::vector<float> p0((size_t)G * A, 1.0f), v0(G, 0.25f), p1((size_t)G * A), v1(G, -0.25f);
    for (size_t i = 0; i < p1.size(); ++i) p1[i] = 1.0f + (float)((i % A) % 7);
    unsigned long long acc = 0;
    for (uint32_t swap = 0; swap < 2; ++swap) {
        tafl_selfplay_opts o; memset(&o, 0, sizeof o); o.sample_seed = 5; o.temp_moves = 4;
        void* ex = hsm_ex_new(G, 7, budget - 3, 8);                       // (a buffer that drops and overflows)
        void* h = hsm_begin(&r, 7, 64, st.data(), nullptr, G, 12, 128, 1.25, &o, budget, 100, 0, 9, swap, ex);
        if (!h) { printf("begin failed\n"); return 1; }
        std::vector<uint8_t> b0((size_t)G * 49), b1((size_t)G * 49), s0(G), s1(G); std::vector<uint32_t> l0(G), l1(G);
        uint32_t cnt[2], rounds = 0;
        for (;;) {
            hsm_leaves(h, b0.data(), s0.data(), l0.data(), b1.data(), s1.data(), l1.data(), cnt);
            if (!(cnt[0] + cnt[1]) || rounds++ > 100000) break;
            hsm_step(h, p0.data(), v0.data(), p1.data(), v1.data());
        }
        std::vector<tafl_state> out(G); std::vector<tafl_play> plays((size_t)G * budget); std::vector<uint32_t> moves(G), eps(G); std::vector<uint8_t> faults(G);
        uint64_t c4[4], ec[4], gm[8];
        hsm_end(h, out.data(), plays.data(), moves.data(), c4, faults.data(), eps.data(), ec, gm);
        for (uint32_t g = 0; g < G; ++g) acc += moves[g] + 100u * eps[g];
        printf("swap %u: rounds %u sims %llu games [%llu %llu %llu %llu] [%llu %llu %llu %llu]\n", swap, rounds, (unsigned long long)c4[0], (unsigned long long)gm[0],
               (unsigned long long)gm[1], (unsigned long long)gm[2], (unsigned long long)gm[3], (unsigned long long)gm[4], (unsigned long long)gm[5], (unsigned long long)gm[6],
               (unsigned long long)gm[7]);
        hsm_free(h); hsm_ex_free(ex);
    }
    printf("checksum %llu\n", acc);
    return 0;
}
#endif
