// tafl_gmcts.hip — guided MCTS: the search whose leaves an external evaluator scores (tafl_guided.hpp), kernels and tafl_gmcts_* entry points.
#include "tafl_internal.hpp"


template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_init(Consts<NL> C, const Quad* soa, GuidedMem M) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, M.G, g, st);
    Guided<NL, W>::init_game(M, g, st);
}
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_step(Consts<NL> C, GuidedMem M, const float* priors, const float* values, uint32_t A, double c_puct,
                                                           uint32_t n_sims, unsigned long long* stats) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::step(M, g, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, C, gs);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// the same round with Dirichlet noise mixed into the root priors (tafl_root_noise; nz.gid holds the game id base): instantiations of their
// own, chosen at launch, so that the kernels above stay as they are
template <int NL, int W, bool NOISE>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_step(Consts<NL> C, GuidedMem M, const float* priors, const float* values, uint32_t A, double c_puct,
                                                           uint32_t n_sims, unsigned long long* stats, RootNoise nz) {
    static_assert(NOISE, "the noise-free round is k_gmcts_step<NL, W>");
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    nz.gid += g;
    Guided<NL, W>::step(M, g, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, C, gs, nz);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// eta for every game's batch state (tafl_root_noise_eval) and the dense root priors (tafl_gmcts_root_priors); `out` is zeroed before
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_root_noise_eval(Consts<NL> C, const Quad* soa, uint32_t n, RootNoise nz, double* out, uint32_t A) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
    nz.gid += g;
    Guided<NL, W>::noise_row(st, C, nz, out + (size_t)g * A);
}
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_root_priors(Consts<NL> C, GuidedMem M, double* out, uint32_t A) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    Guided<NL, W>::root_priors(M, g, out + (size_t)g * A);
}
// network input of the waiting leaves: board_to_matrix planes (game/main.rs:55-83), side to move, waiting flag; one thread per tile
template <int NL, int W>
__global__ __launch_bounds__(256) void k_gmcts_leaves(Consts<NL> C, GuidedMem M, uint8_t* boards, uint8_t* sides, uint8_t* waiting) {
    const uint32_t nn = C.n * C.n;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)M.G * nn) return;
    const uint32_t g = (uint32_t)(i / nn), t = (uint32_t)(i % nn), r = t / C.n, c = t % C.n, bit = r * (uint32_t)W + c;
    const bool wait = M.kind[g] == 1;
    const uint32_t L = wait ? M.leaf[g] : 0u;
    const uint32_t* rec = (const uint32_t*)(M.node_state + ((size_t)L * M.G + g) * StateIO<NL>::QUADS);   // att[NL], def[NL], rep[4], meta[4]
    const uint32_t aw = rec[bit >> 5], dw = rec[NL + (bit >> 5)], flags = rec[2 * NL + 7];
    // a waiting leaf is shown under its symmetry (tafl_eval_symmetry): the byte of tile t goes to tile sym_tile(s, t) of the game's row
    size_t o = i;
    if (M.sym && wait) {
        const uint32_t s = M.sym[g];
        uint32_t r2 = (s & 4u) ? c : r, c2 = (s & 4u) ? r : c;
        if (s & 1u) r2 = C.n - 1u - r2;
        if (s & 2u) c2 = C.n - 1u - c2;
        o = (size_t)g * nn + r2 * C.n + c2;
    }
    boards[o] = (uint8_t)board_value((aw >> (bit & 31)) & 1u, (dw >> (bit & 31)) & 1u, r, c, C.n, flags);
    if (t == 0) { sides[g] = (uint8_t)((flags & TAFL_F_SIDE) ? TAFL_DEFENDER : TAFL_ATTACKER); waiting[g] = wait ? 1 : 0; }
}
// the symmetry every waiting leaf is shown under (tafl_gmcts_leaf_symmetry): 0 for a game that does not wait, and with the setting off
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_leaf_symmetry(GuidedMem M, uint8_t* out) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    out[g] = (M.sym && M.kind[g] == 1) ? M.sym[g] : (uint8_t)0;
}
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_root_children(Consts<NL> C, GuidedMem M, tafl_root_child* out, uint32_t max_children, uint32_t* out_n) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    out_n[g] = Guided<NL, W>::root_children(M, g, out + (size_t)g * max_children, max_children);
}
// dense root visit counts and the probs of src/mcts.py:43-53 (any temperature; temp == 0 as in k_mcts_policy)
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_root_dense(Consts<NL> C, GuidedMem M, uint32_t* visits, double* probs, uint32_t A, int one_hot, double inv_temp,
                                                                 uint64_t tie_seed, uint64_t base) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    const GNode h = M.hdr[g];
    if (!h.expanded) return;
    const GEdge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
    // the legal edges are stored in ascending action order, zeros included: a zero count adds 0.0 to the sum (0 ** x == 0 for x > 0)
    double sum = 0.0; uint32_t best = 0, ties = 0; bool any_n = false;
    for (uint32_t j = 0; j < h.n_legal; ++j) {
        const GEdge e = eb[j];
        if (!one_hot && e.n != 0) sum += temp_weight(e.n, inv_temp);
        if (e.n > best) { best = e.n; ties = 1; } else if (e.n == best && best > 0) ++ties;
        any_n |= e.n != 0;
    }
    uint32_t pick = 0;
    if (one_hot && tie_seed != 0 && ties > 1) pick = tie_pick(tie_seed, base + g, ties);
    uint32_t seen = 0;
    for (uint32_t j = 0; j < h.n_legal; ++j) {
        const GEdge e = eb[j];
        if (visits) visits[(size_t)g * A + e.action] = e.n;
        if (probs && any_n) {
            double p;
            if (one_hot) { const bool is_max = e.n == best; p = (is_max && seen == pick) ? 1.0 : 0.0; seen += is_max ? 1u : 0u; }
            else p = e.n != 0 ? temp_weight(e.n, inv_temp) / sum : 0.0;
            probs[(size_t)g * A + e.action] = p;
        }
    }
}

// subtree reuse in guided mode: keep-init and advance (k_mcts_keep_init / k_mcts_advance on the guided arena)
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_keep_init(Consts<NL> C, const Quad* soa, GuidedMem M) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    if (M.node_top[g] == 0) { DState<NL> st; StateIO<NL>::load_soa(soa, M.G, g, st); Guided<NL, W>::init_game(M, g, st); }
    else Guided<NL, W>::keep_init(M, g);
}
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_advance(Consts<NL> C, GuidedMem M, Quad* soa, GEdge* dst, uint32_t* idmap, const uint32_t* actions, int live,
                                                              uint32_t A, tafl_play* out_plays, tafl_effects* eff, uint32_t* bad) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    const GNode h = M.hdr[g];
    const GEdge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
    uint32_t a = actions ? actions[g] : TAFL_ACTION_NONE, child = 0;
    if (live && h.expanded) {
        uint32_t best = 0;
        for (uint32_t j = 0; j < h.n_legal; ++j) {                  // ascending action order: the first maximum
            const GEdge e = eb[j];
            if (actions ? e.action == a : e.n > best) { best = e.n; child = e.child; a = e.action; if (actions) break; }
        }
    }
    DState<NL> st; StateIO<NL>::load_soa(soa, M.G, g, st);
    tafl_play p; tafl_effects e;
    const bool played = advance_play<NL, W>(C, st, a, A, p, e);
    if (played) StateIO<NL>::store_soa(soa, M.G, g, st);
    const bool alone = !played && (a == TAFL_ACTION_NONE || e.code == TAFL_PLAY_GAME_OVER);
    if (live && alone) Guided<NL, W>::keep_edges(M, dst, g);
    else {
        bool fresh = !(live && played && child != 0);
        if (!fresh) {
            Guided<NL, W>::reroot(M, dst, idmap, g, child);
            if (!same_state<NL>(M.node_state + (size_t)g * StateIO<NL>::QUADS, st)) { atomicAdd(bad, 1u); fresh = true; }
        }
        if (fresh) Guided<NL, W>::init_game(M, g, st);
    }
    if (out_plays) out_plays[g] = p;
    if (eff) eff[g] = e;
}

// guided self-play at each game's own pace (tafl_gselfplay_*): one game per lane.  k_gselfplay_step is k_gmcts_step
// with the move made in the same launch: the lane that owns a game whose search is complete chooses, records, plays and begins the next search.
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_init(Consts<NL> C, const Quad* soa, GuidedMem M, GSelfPlay sp) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, M.G, g, st);
    Guided<NL, W>::selfplay_init(M, g, st, sp);
}
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_step(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                               uint32_t n_sims, GSelfPlay sp, SelfPlayRec rec, unsigned long long* stats) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::selfplay_step(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, rec, C, gs);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
template <int NL, int W, bool NOISE>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_step(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                               uint32_t n_sims, GSelfPlay sp, SelfPlayRec rec, unsigned long long* stats, RootNoise nz) {
    static_assert(NOISE, "the noise-free round is k_gselfplay_step<NL, W>");
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::selfplay_step(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, rec, C, gs, nz);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// the round of an episodes run (tafl_gselfplay_begin_episodes), without and with root noise: kernels of their own, so
// that the ones above stay as they are
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_episodes(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                                   uint32_t n_sims, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::selfplay_step_episodes(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, ep, rec, C, gs);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
template <int NL, int W, bool NOISE>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_episodes(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                                   uint32_t n_sims, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats, RootNoise nz) {
    static_assert(NOISE, "the noise-free round is k_gselfplay_episodes<NL, W>");
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::selfplay_step_episodes(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, ep, rec, C, gs, nz);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// the round of a capped run (tafl_gselfplay_set_playout_cap), plain or episodes, without or with root noise: kernels
// of their own, so that the ones above stay as they are.  `ep` is read by the EPISODES instantiations alone, `nz` by the NOISE ones.
template <int NL, int W, bool NOISE, bool EPISODES>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_capped(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                                 uint32_t n_sims, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats, RootNoise nz, PlayoutCap pc) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::template selfplay_step_capped<NOISE, EPISODES>(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, ep, rec, C,
                                                                  gs, nz, pc);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// the round of a run with forced playouts (tafl_gselfplay_set_forced_playouts), again kernels of their own.  They
// go through the capped path: a run without a cap passes a PlayoutCap under which every move is full
template <int NL, int W, bool NOISE, bool EPISODES>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_forced(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                                 uint32_t n_sims, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats, RootNoise nz, PlayoutCap pc,
                                                                 ForcedPlayouts fp) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::template selfplay_step_forced<NOISE, EPISODES>(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, ep, rec, C,
                                                                  gs, nz, pc, fp);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// the round of a run with exact win/loss proofs (tafl_gselfplay_set_solver), kernels of their own once more.  They
// go through the capped path and take the run's cap and forced playouts at run time: "every move full" without a cap, k == 0 without forcing
template <int NL, int W, bool NOISE, bool EPISODES>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_solver(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                                 uint32_t n_sims, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats, RootNoise nz, PlayoutCap pc,
                                                                 ForcedPlayouts fp, SolverCfg sv) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::template selfplay_step_solver<NOISE, EPISODES>(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, sp, ep, rec, C,
                                                                  gs, nz, pc, fp, sv);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// close and reopen, right after the round on the same stream: the lanes whose episode ended settle its examples, count it, take their
// opening and wait with a fresh root (Guided::selfplay_reopen); every other lane leaves at its first load
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_reopen(GuidedMem M, Quad* soa, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    if (Guided<NL, W>::selfplay_reopen(M, g, soa, sp, ep, rec)) atomicAdd(&stats[GS_WAITING], 1ull);
}

// ---- match play: two evaluators in an episodes run (tafl_gmatch_*) -----------------------------------------------
// The evaluators' dense batches are a stable two-way partition of the waiting lanes by owner (Guided::match_owner), in two launches of
// 256-lane workgroups.  k_gmatch_rank: the rank of a lane among the lanes of its workgroup with the same owner - a wave ballot and mbcnt
// inside the wave, the four wave counts through LDS - goes to row_of, the workgroup's two counts to block_counts.  k_gmatch_place: every
// workgroup sums the counts of the workgroups before it (and all of them: the totals), adds its offset to the ranks and writes
// lanes[e][row].  No atomic decides a row, so the rows are in ascending lane order.
#define TAFL_MATCH_BLOCK 256
#define TAFL_MATCH_WAVES (TAFL_MATCH_BLOCK / 64)
template <int NL, int W>
__global__ __launch_bounds__(TAFL_MATCH_BLOCK) void k_gmatch_rank(GuidedMem M, const Quad* soa, const uint32_t* episode, uint64_t game_id_base, uint32_t swap, uint32_t* row_of,
                                                                  uint32_t* block_counts) {
    __shared__ uint32_t wave_cnt[2][TAFL_MATCH_WAVES];
    const uint32_t g = blockIdx.x * TAFL_MATCH_BLOCK + threadIdx.x, wave = threadIdx.x >> 6;
    uint32_t e = 2u;                                               // 2: the lane does not wait
    if (g < M.G && M.kind[g] == 1) e = Guided<NL, W>::match_owner(game_id_base, g, episode[g], swap, Guided<NL, W>::batch_flags(soa, M.G, g));
    const unsigned long long b0 = __ballot(e == 0u), b1 = __ballot(e == 1u), mine = e == 0u ? b0 : b1;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
    if ((threadIdx.x & 63u) == 0u) { wave_cnt[0][wave] = (uint32_t)__popcll(b0); wave_cnt[1][wave] = (uint32_t)__popcll(b1); }
    __syncthreads();
    if (e < 2u) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; ++w) before += wave_cnt[e][w];
        row_of[g] = (e << 31) | (before + rank);
    } else if (g < M.G) row_of[g] = kMatchNoRow;
    if (threadIdx.x < 2u) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < TAFL_MATCH_WAVES; ++w) sum += wave_cnt[threadIdx.x][w];
        block_counts[2u * blockIdx.x + threadIdx.x] = sum;
    }
}
__global__ __launch_bounds__(TAFL_MATCH_BLOCK) void k_gmatch_place(uint32_t G, uint32_t n_blocks, const uint32_t* block_counts, uint32_t* row_of, uint32_t* lanes, uint32_t* counts) {
    __shared__ uint32_t part[4][TAFL_MATCH_WAVES];                 // per wave: evaluator 0 / 1 before this workgroup, evaluator 0 / 1 in all
    uint32_t s[4] = {0u, 0u, 0u, 0u};
    for (uint32_t t = threadIdx.x; t < n_blocks; t += TAFL_MATCH_BLOCK) {
        const uint32_t c0 = block_counts[2u * t], c1 = block_counts[2u * t + 1u];
        if (t < blockIdx.x) { s[0] += c0; s[1] += c1; }
        s[2] += c0; s[3] += c1;
    }
    TAFL_UNROLL for (int k = 0; k < 4; ++k) {
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off);
        if ((threadIdx.x & 63u) == 0u) part[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    uint32_t tot[4];
    TAFL_UNROLL for (int k = 0; k < 4; ++k) { tot[k] = 0; for (uint32_t w = 0; w < TAFL_MATCH_WAVES; ++w) tot[k] += part[k][w]; }
    const uint32_t g = blockIdx.x * TAFL_MATCH_BLOCK + threadIdx.x;
    if (g < G) {
        const uint32_t r = row_of[g];
        if (r != kMatchNoRow) {
            const uint32_t e = r >> 31, row = (r & kMatchRowMask) + tot[e];
            if (row < G) { row_of[g] = (e << 31) | row; lanes[(size_t)e * G + row] = g; }      // (row < count_e <= G by construction)
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { counts[0] = tot[2]; counts[1] = tot[3]; }
}
// the evaluators' network input: k_gmcts_leaves with one thread per (row, tile) of the two compact batches, evaluator 0's rows first.  Rows
// beyond the counts exit; the waiting flags are written up to each capacity.  The host has checked counts[e] <= cap[e].
struct MatchOut { uint8_t* boards[2]; uint8_t* sides[2]; uint8_t* waiting[2]; uint32_t* lanes[2]; uint32_t cap[2]; };
template <int NL, int W>
__global__ __launch_bounds__(256) void k_gmatch_leaves(Consts<NL> C, GuidedMem M, const uint32_t* lanes, const uint32_t* counts, MatchOut o) {
    const uint32_t nn = C.n * C.n;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const uint32_t cnt[2] = {counts[0], counts[1]};
    TAFL_UNROLL for (int e = 0; e < 2; ++e)
        if (o.waiting[e]) for (size_t r = i; r < o.cap[e]; r += threads) o.waiting[e][r] = r < cnt[e] ? 1 : 0;
    if (i >= (size_t)M.G * nn) return;
    const uint32_t R = (uint32_t)(i / nn), t = (uint32_t)(i % nn), r = t / C.n, c = t % C.n, bit = r * (uint32_t)W + c;
    if (R >= cnt[0] + cnt[1] || cnt[0] > M.G || cnt[1] > M.G) return;
    const uint32_t e = R >= cnt[0] ? 1u : 0u, row = e ? R - cnt[0] : R;
    if (row >= o.cap[e]) return;
    const uint32_t g = lanes[(size_t)e * M.G + row];
    if (g >= M.G) return;
    const uint32_t L = M.leaf[g];
    const uint32_t* rec = (const uint32_t*)(M.node_state + ((size_t)L * M.G + g) * StateIO<NL>::QUADS);   // att[NL], def[NL], rep[4], meta[4]
    const uint32_t aw = rec[bit >> 5], dw = rec[NL + (bit >> 5)], flags = rec[2 * NL + 7];
    if (o.boards[e]) o.boards[e][(size_t)row * nn + t] = (uint8_t)board_value((aw >> (bit & 31)) & 1u, (dw >> (bit & 31)) & 1u, r, c, C.n, flags);
    if (t == 0) {
        if (o.sides[e]) o.sides[e][row] = (uint8_t)((flags & TAFL_F_SIDE) ? TAFL_DEFENDER : TAFL_ATTACKER);
        if (o.lanes[e]) o.lanes[e][row] = g;
    }
}
// the round of a match run: k_gselfplay_episodes with the lane's evaluation read from its row of its owner's compact batch
struct MatchIn { const float* priors[2]; const float* values[2]; };
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmatch_round(Consts<NL> C, GuidedMem M, Quad* soa, MatchIn in, const uint32_t* row_of, uint32_t A, double c_puct,
                                                             uint32_t n_sims, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    const uint32_t r = row_of[g];
    const float* pr = nullptr; float v = 0.f;
    if (r != kMatchNoRow) {
        const float* p = in.priors[r >> 31]; const float* vs = in.values[r >> 31];
        if (p && vs) { pr = p + (size_t)(r & kMatchRowMask) * A; v = vs[r & kMatchRowMask]; }
    }
    Guided<NL, W>::selfplay_step_episodes(M, g, soa, pr, v, A, c_puct, n_sims, sp, ep, rec, C, gs);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// the tally, between the round and k_gselfplay_reopen on the same stream (Guided::match_tally)
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmatch_tally(GuidedMem M, const Quad* soa, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, GMatch mt) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    Guided<NL, W>::match_tally(M, g, soa, sp, ep, rec, mt);
}

// the arena of a search from fresh roots: max_sims + 1 nodes and (max_sims + 1) x edges_per_node edges per game; the guided stats are zeroed
static int gmcts_arena(tafl_batch* b, uint32_t max_sims, uint32_t edges_per_node, const char* name) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n; const size_t q = (size_t)quads_of(c);
    const uint32_t node_cap = max_sims + 1;
    const unsigned long long ecap = (unsigned long long)node_cap * edges_per_node;
    if (ecap > 0xFFFFFFFFull) return fail(TAFL_ERR_CAPACITY, std::string(name) + ": edge arena too large");
    NEED(b->g_node_state, sizeof(Quad) * q * node_cap * n); NEED(b->g_hdr, sizeof(GNode) * (size_t)node_cap * n);
    NEED(b->g_pedge, sizeof(uint32_t) * (size_t)node_cap * n); NEED(b->g_edges, sizeof(GEdge) * (size_t)ecap * n);
    NEED(b->g_node_top, 4 * (size_t)n); NEED(b->g_edge_top, 4 * (size_t)n); NEED(b->g_leaf, 4 * (size_t)n); NEED(b->g_kind, n); NEED(b->g_fault, n);
    NEED(b->g_sims, 4 * (size_t)n); NEED(b->g_stats, sizeof(unsigned long long) * GS_COUNT);
    GuidedMem& M = b->gmem;
    b->g_node_state.bind(M.node_state); b->g_hdr.bind(M.hdr); b->g_pedge.bind(M.pedge); b->g_edges.bind(M.edges);
    b->g_node_top.bind(M.node_top); b->g_edge_top.bind(M.edge_top); b->g_leaf.bind(M.leaf); b->g_kind.bind(M.kind);
    b->g_fault.bind(M.fault); b->g_sims.bind(M.sims_done); M.G = n; M.node_cap = node_cap; M.edge_cap = (uint32_t)ecap;
    HIPCHK(hipMemsetAsync(b->g_stats.p, 0, sizeof(unsigned long long) * GS_COUNT, c->stream));
    return TAFL_OK;
}
// the evaluator's answer where the step kernels read it: host arrays are copied to g_priors / g_values, device pointers (and none) pass through
static int stage_evaluation(tafl_batch* b, const float*& priors, const float*& values, int in_is_device) {
    if (!priors || in_is_device) return TAFL_OK;
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, A = tafl_action_size(c);
    NEED(b->g_priors, sizeof(float) * (size_t)n * A); NEED(b->g_values, sizeof(float) * (size_t)n);
    HIPCHK(hipMemcpyAsync(b->g_priors.p, priors, sizeof(float) * (size_t)n * A, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b->g_values.p, values, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    priors = b->g_priors.as<const float>(); values = b->g_values.as<const float>();
    return TAFL_OK;
}
// the games now waiting for predict(), as the last step kernel counted them
static int gmcts_waiting(tafl_batch* b, uint32_t* out_waiting) {
    if (!out_waiting) return TAFL_OK;
    tafl_ctx* c = b->ctx;
    unsigned long long w = 0;
    HIPCHK(hipMemcpyAsync(&w, b->g_stats.as<unsigned long long>() + GS_WAITING, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out_waiting = (uint32_t)w;
    return TAFL_OK;
}

// a tafl_root_noise the library accepts
static int noise_check(const tafl_root_noise* cfg, const char* name) {
    if (!(cfg->alpha > 0.0) || !(cfg->alpha < INFINITY) || !(cfg->epsilon > 0.0) || !(cfg->epsilon <= 1.0))
        return fail(TAFL_ERR_INVALID_ARG, std::string(name) + ": alpha must be positive and finite, epsilon in (0, 1]");
    if (cfg->flags != 0 || cfg->_reserved != 0) return fail(TAFL_ERR_UNSUPPORTED, std::string(name) + ": flags and the reserved word must be 0");
    return TAFL_OK;
}
static RootNoise noise_arg(const tafl_root_noise& cfg) {
    RootNoise nz; nz.alpha = cfg.alpha; nz.epsilon = cfg.epsilon; nz.seed = cfg.seed; nz.gid = cfg.game_id_base; nz.move_no = cfg.move_no;
    return nz;
}

// a begin latches the batch's eval-symmetry setting into the arena's argument struct (after gmcts_arena has bound the rest): off, or one
// byte per game, the seed and the game id base of the search (cfg's) or run (its own)
static int evalsym_latch(tafl_batch* b, uint64_t game_id_base) {
    tafl_ctx* c = b->ctx; GuidedMem& M = b->gmem;
    M.sym = nullptr; M.sym_seed = 0; M.sym_gid = 0; M.sym_n = 0;
    if (!b->evalsym_set) return TAFL_OK;
    NEED(b->g_sym, b->n);
    HIPCHK(hipMemsetAsync(b->g_sym.p, 0, b->n, c->stream));
    b->g_sym.bind(M.sym); M.sym_seed = b->evalsym_cfg.seed; M.sym_gid = game_id_base; M.sym_n = c->n;
    return TAFL_OK;
}

// a tafl_playout_cap the library accepts
static int cap_check(const tafl_playout_cap* cfg) {
    if (cfg->fast_sims < 2u || cfg->fast_sims > 0xFFFFu || cfg->full_per_65536 > 65536u)
        return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_set_playout_cap: fast_sims must be 2 .. 65535 and full_per_65536 at most 65536");
    if (cfg->flags != 0 || cfg->_reserved[0] != 0 || cfg->_reserved[1] != 0 || cfg->_reserved[2] != 0)
        return fail(TAFL_ERR_UNSUPPORTED, "tafl_playout_cap: flags and reserved words must be 0");
    return TAFL_OK;
}

// a tafl_forced_playouts the library accepts
static int forced_check(const tafl_forced_playouts* cfg) {
    if (!(cfg->k > 0.0) || !(cfg->k <= 64.0)) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_set_forced_playouts: k must be finite, above 0 and at most 64");
    if (cfg->flags != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_forced_playouts: flags and reserved words must be 0");
    for (uint32_t r : cfg->_reserved) if (r != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_forced_playouts: flags and reserved words must be 0");
    return TAFL_OK;
}

extern "C" {

int tafl_gselfplay_set_solver(tafl_batch* b, const tafl_solver* cfg) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_set_solver: null batch");
    if (!cfg) { b->solver_set = false; return TAFL_OK; }
    if (cfg->flags != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_solver: flags and reserved words must be 0");
    for (uint32_t r : cfg->_reserved) if (r != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_solver: flags and reserved words must be 0");
    b->solver_set = true;
    return TAFL_OK;
}

int tafl_gselfplay_solver_stats(tafl_batch* b, tafl_solver_stats* out) {
    if (!b || !b->gsp_has || !b->gsp_solver_on || !out)
        return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_solver_stats: no run with the solver on this batch (tafl_gselfplay_set_solver, then a begin)");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long h[SV_COUNT];
    HIPCHK(hipMemcpyAsync(h, b->gsp_solver_counters.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->root_won = h[SV_ROOT_WON]; out->root_lost = h[SV_ROOT_LOST]; out->skipped_sims = h[SV_SKIPPED_SIMS]; out->nodes_won = h[SV_NODES_WON];
    out->nodes_lost = h[SV_NODES_LOST]; out->pruned_visits = h[SV_PRUNED_VISITS]; out->pruned_children = h[SV_PRUNED_CHILDREN]; out->moves = h[SV_MOVES];
    return TAFL_OK;
}

int tafl_gselfplay_set_forced_playouts(tafl_batch* b, const tafl_forced_playouts* cfg) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_set_forced_playouts: null batch");
    if (!cfg) { b->forced_set = false; return TAFL_OK; }
    if (const int rc = forced_check(cfg)) return rc;
    b->forced_set = true; b->forced_cfg = *cfg;
    return TAFL_OK;
}

int tafl_gselfplay_forced_playouts_stats(tafl_batch* b, tafl_forced_playouts_stats* out) {
    if (!b || !b->gsp_has || !b->gsp_forced_on || !out)
        return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_forced_playouts_stats: no run with forced playouts on this batch (tafl_gselfplay_set_forced_playouts, then a begin)");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long h[FP_COUNT];
    HIPCHK(hipMemcpyAsync(h, b->gsp_forced_counters.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->forced_sims = h[FP_FORCED_SIMS]; out->pruned_visits = h[FP_PRUNED_VISITS]; out->pruned_children = h[FP_PRUNED_CHILDREN]; out->full_moves = h[FP_FULL_MOVES];
    return TAFL_OK;
}

int tafl_gselfplay_set_playout_cap(tafl_batch* b, const tafl_playout_cap* cfg) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_set_playout_cap: null batch");
    if (!cfg) { b->cap_set = false; return TAFL_OK; }
    if (const int rc = cap_check(cfg)) return rc;
    b->cap_set = true; b->cap_cfg = *cfg;
    return TAFL_OK;
}

int tafl_gselfplay_playout_cap_stats(tafl_batch* b, tafl_playout_cap_stats* out) {
    if (!b || !b->gsp_has || !b->gsp_cap_on || !out) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_playout_cap_stats: no capped run on this batch (tafl_gselfplay_set_playout_cap, then a begin)");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long h[CAP_COUNT];
    HIPCHK(hipMemcpyAsync(h, b->gsp_cap_counters.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof *out);
    out->full_moves = h[CAP_FULL]; out->fast_moves = h[CAP_FAST];
    return TAFL_OK;
}

int tafl_gmcts_set_eval_symmetry(tafl_batch* b, const tafl_eval_symmetry* cfg) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_set_eval_symmetry: null batch");
    if (!cfg) { b->evalsym_set = false; return TAFL_OK; }
    if (cfg->flags != 0 || cfg->_reserved[0] != 0 || cfg->_reserved[1] != 0 || cfg->_reserved[2] != 0)
        return fail(TAFL_ERR_UNSUPPORTED, "tafl_eval_symmetry: flags and reserved words must be 0");
    b->evalsym_set = true; b->evalsym_cfg = *cfg;
    return TAFL_OK;
}

int tafl_gmcts_leaf_symmetry(tafl_batch* b, uint8_t* out_sym, int out_is_device) {
    if (!b || !b->g_has || !out_sym) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_leaf_symmetry: bad argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    uint8_t* d;
    STAGED(d, b->g_wait, out_sym, n, out_is_device);
    LAUNCH_PER_GAME(k_gmcts_leaf_symmetry, c, n, b->gmem, d);
    HIPCHK(hipGetLastError());
    if (!out_is_device) COPY_OUT(out_sym, d, n, c->stream);
    return sync_ok(c);
}

int tafl_gmcts_set_root_noise(tafl_batch* b, const tafl_root_noise* cfg) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_set_root_noise: null batch");
    if (!cfg) { b->noise_set = false; return TAFL_OK; }
    if (const int rc = noise_check(cfg, "tafl_gmcts_set_root_noise")) return rc;
    b->noise_set = true; b->noise_cfg = *cfg;
    return TAFL_OK;
}

int tafl_root_noise_eval(tafl_batch* b, const tafl_root_noise* cfg, double* out_eta, int out_is_device) {
    if (!b || !cfg || !out_eta) return fail(TAFL_ERR_INVALID_ARG, "tafl_root_noise_eval: null argument");
    if (const int rc = noise_check(cfg, "tafl_root_noise_eval")) return rc;
    if (const int rc = join_search(b)) return rc;
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, A = tafl_action_size(c); const size_t count = (size_t)n * A;
    HIPCHK(hipSetDevice(c->device));
    double* d;
    STAGED(d, b->policy, out_eta, count, out_is_device);
    HIPCHK(hipMemsetAsync(d, 0, sizeof(double) * count, c->stream));
    const RootNoise nz = noise_arg(*cfg);
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_root_noise_eval<t.NL, t.W>), c, n, t.CC, b->soa, n, nz, d, A); });
    HIPCHK(hipGetLastError());
    if (!out_is_device) COPY_OUT(out_eta, d, count, c->stream);
    return sync_ok(c);
}

int tafl_gmcts_root_priors(tafl_batch* b, double* out, int out_is_device) {
    if (!b || !b->g_has || !out) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_root_priors: bad argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, A = tafl_action_size(c); const size_t count = (size_t)n * A;
    HIPCHK(hipSetDevice(c->device));
    double* d;
    STAGED(d, b->policy, out, count, out_is_device);
    HIPCHK(hipMemsetAsync(d, 0, sizeof(double) * count, c->stream));
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_root_priors<t.NL, t.W>), c, n, t.CC, b->gmem, d, A); });
    HIPCHK(hipGetLastError());
    if (!out_is_device) COPY_OUT(out, d, count, c->stream);
    return sync_ok(c);
}

int tafl_gmcts_begin(tafl_batch* b, uint32_t max_sims, uint32_t edges_per_node) { return tafl_gmcts_begin_ex(b, max_sims, edges_per_node, 0); }

// TAFL_GMCTS_KEEP_TREE on a retained tree: the arena grows (contents kept) to the largest kept tree + max_sims + 1 nodes and + (max_sims + 1)
// x edges_per_node edges, and only the per-search fields are reset
static int gmcts_begin_keep(tafl_batch* b, uint32_t max_sims, uint32_t edges_per_node) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n; const size_t q = (size_t)quads_of(c);
    GuidedMem& M = b->gmem;
    uint32_t mx[2];
    int rc = arena_max(b, M.node_top, M.edge_top, mx);
    if (rc) return rc;
    const unsigned long long nodes = (unsigned long long)mx[0] + max_sims + 1, ecap = (unsigned long long)mx[1] + ((unsigned long long)max_sims + 1) * edges_per_node;
    if (nodes > 0xFFFFFFFFull || ecap > 0xFFFFFFFFull) return fail(TAFL_ERR_CAPACITY, "tafl_gmcts_begin_ex: the retained tree and the new simulations exceed the arena's index range");
    rc = arena_grow(b, {ArenaArray(b->g_node_state, sizeof(Quad) * q, M.node_state), ArenaArray(b->g_hdr, sizeof(GNode), M.hdr), ArenaArray(b->g_pedge, sizeof(uint32_t), M.pedge)},
                    M.node_cap, nodes, ArenaArray(b->g_edges, sizeof(GEdge), M.edges), b->g_edges_alt, M.edge_cap, ecap);
    if (rc != TAFL_OK) return rc;
    HIPCHK(hipMemsetAsync(b->g_stats.p, 0, sizeof(unsigned long long) * GS_COUNT, c->stream));
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_keep_init<t.NL, t.W>), c, n, t.CC, b->soa, M); });
    HIPCHK(hipGetLastError());
    b->g_max_sims = max_sims;
    return TAFL_OK;
}

int tafl_gmcts_begin_ex(tafl_batch* b, uint32_t max_sims, uint32_t edges_per_node, uint32_t flags) {
    if (!b || max_sims == 0 || edges_per_node == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_begin: bad argument");
    if (flags & ~(uint32_t)TAFL_GMCTS_KEEP_TREE) return fail(TAFL_ERR_UNSUPPORTED, "tafl_gmcts_begin_ex: unknown flags");
    if ((flags & TAFL_GMCTS_KEEP_TREE) && b->noise_set) return fail(TAFL_ERR_UNSUPPORTED, "tafl_gmcts_begin_ex: root noise on a retained tree is not supported (tafl_gmcts_set_root_noise(NULL) first)");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    b->gsp_active = false;                                   // (a guided self-play run on this arena is closed)
    b->gsp_targets = ExampleTargetsMem{}; b->gsp_open_from = nullptr; b->gsp_targets_ex = nullptr;      // (the closed run holds its examples object no longer)
    b->g_noise_on = b->noise_set;                            // the search latches the noise setting
    if (b->noise_set) b->g_noise = noise_arg(b->noise_cfg);
    HIPCHK(hipSetDevice(c->device));
    if (flags & TAFL_GMCTS_KEEP_TREE) { if (const int rc = join_search(b)) return rc; }
    if (const int rc = evalsym_latch(b, b->evalsym_cfg.game_id_base)) return rc;      // and the eval symmetry (a retained tree: its new leaves)
    if ((flags & TAFL_GMCTS_KEEP_TREE) && b->g_has && b->g_tree_live) {
        b->g_tree_live = false;
        const int rc = gmcts_begin_keep(b, max_sims, edges_per_node);
        if (rc == TAFL_OK) b->g_tree_live = true;
        return rc;
    }
    b->g_tree_live = false;
    if (const int rc = gmcts_arena(b, max_sims, edges_per_node, "tafl_gmcts_begin")) return rc;
    GuidedMem& M = b->gmem;
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_init<t.NL, t.W>), c, n, t.CC, b->soa, M); });
    HIPCHK(hipGetLastError());
    b->g_has = true; b->g_max_sims = max_sims; b->g_tree_live = true;
    return TAFL_OK;
}

int tafl_gmcts_step(tafl_batch* b, const float* priors, const float* values, int in_is_device, double c_puct, uint32_t n_sims, uint32_t* out_waiting) {
    if (!b || !b->g_has) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_step: tafl_gmcts_begin first");
    if (n_sims > b->g_max_sims) return fail(TAFL_ERR_CAPACITY, "tafl_gmcts_step: n_sims exceeds the reserved simulations");
    if ((priors == nullptr) != (values == nullptr)) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_step: priors and values go together");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, A = tafl_action_size(c);
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = stage_evaluation(b, priors, values, in_is_device)) return rc;
    unsigned long long* st = b->g_stats.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(st + GS_WAITING, 0, sizeof(unsigned long long), c->stream));
    if (b->gmem.sym) { if (const int rc = gsym_launch_step(b, priors, values, A, c_puct, n_sims, st)) return rc; }      // the search latched the eval symmetry
    else if (b->g_noise_on) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_step<t.NL, t.W, true>), c, n, t.CC, b->gmem, priors, values, A, c_puct, n_sims, st, b->g_noise); });
    else dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_step<t.NL, t.W>), c, n, t.CC, b->gmem, priors, values, A, c_puct, n_sims, st); });
    HIPCHK(hipGetLastError());
    return gmcts_waiting(b, out_waiting);
}

int tafl_gmcts_leaves(tafl_batch* b, uint8_t* boards, uint8_t* sides, uint8_t* waiting, int out_is_device) {
    if (!b || !b->g_has || !boards || !sides || !waiting) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_leaves: bad argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n; const size_t total = (size_t)n * c->n * c->n;
    HIPCHK(hipSetDevice(c->device));
    uint8_t *db, *ds, *dw;
    STAGED(db, b->g_boards, boards, total, out_is_device);
    STAGED(ds, b->g_sides, sides, n, out_is_device);
    STAGED(dw, b->g_wait, waiting, n, out_is_device);
    dispatch<BATCH, false>(c, [&](auto t) { hipLaunchKernelGGL((k_gmcts_leaves<t.NL, t.W>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, t.CC, b->gmem, db, ds, dw); });
    HIPCHK(hipGetLastError());
    if (!out_is_device) {
        COPY_OUT(boards, db, total, c->stream);
        COPY_OUT(sides, ds, n, c->stream);
        COPY_OUT(waiting, dw, n, c->stream);
    }
    return sync_ok(c);
}

int tafl_gmcts_root_children(tafl_batch* b, tafl_root_child* out, uint32_t max_children, uint32_t* out_n) {
    if (!b || !b->g_has || !out || !out_n || max_children == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_root_children: bad argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->children, sizeof(tafl_root_child) * (size_t)n * max_children); NEED(b->children_n, sizeof(uint32_t) * n);
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_root_children<t.NL, t.W>), c, n, t.CC, b->gmem, b->children.as<tafl_root_child>(), max_children, b->children_n.as<uint32_t>()); });
    HIPCHK(hipGetLastError());
    COPY_OUT(out, b->children.p, (size_t)n * max_children, c->stream);
    COPY_OUT(out_n, b->children_n.p, n, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t g = 0; g < n; ++g) if (out_n[g] > max_children) return fail(TAFL_ERR_CAPACITY, "tafl_gmcts_root_children: max_children too small");
    return TAFL_OK;
}

static int gmcts_dense(tafl_batch* b, uint32_t* visits, double* probs, double temp, int out_is_device, uint64_t tie_seed = 0, uint64_t game_id_base = 0) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, A = tafl_action_size(c); const size_t count = (size_t)n * A;
    HIPCHK(hipSetDevice(c->device));
    uint32_t* dv; double* dp;
    STAGED(dv, b->visits, visits, count, out_is_device);
    STAGED(dp, b->policy, probs, count, out_is_device);
    if (dv) HIPCHK(hipMemsetAsync(dv, 0, sizeof(uint32_t) * count, c->stream));
    if (dp) HIPCHK(hipMemsetAsync(dp, 0, sizeof(double) * count, c->stream));
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_root_dense<t.NL, t.W>), c, n, t.CC, b->gmem, dv, dp, A, temp == 0.0 ? 1 : 0, temp == 0.0 ? 1.0 : 1.0 / temp, tie_seed, game_id_base); });
    HIPCHK(hipGetLastError());
    if (!out_is_device) {
        COPY_OUT(visits, dv, count, c->stream);
        COPY_OUT(probs, dp, count, c->stream);
    }
    return sync_ok(c);
}
int tafl_gmcts_root_visits(tafl_batch* b, uint32_t* out, int out_is_device) {
    if (!b || !b->g_has || !out) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_root_visits: bad argument");
    return gmcts_dense(b, out, nullptr, 1.0, out_is_device);
}
int tafl_gmcts_policy_ex(tafl_batch* b, double temp, uint64_t tie_seed, uint64_t game_id_base, double* out, int out_is_device) {
    if (!b || !b->g_has || !out) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_policy: bad argument");
    if (!(temp >= 0.0)) return fail(TAFL_ERR_INVALID_ARG, "temp must be >= 0");
    return gmcts_dense(b, nullptr, out, temp, out_is_device, tie_seed, game_id_base);
}
int tafl_gmcts_policy(tafl_batch* b, double temp, double* out, int out_is_device) { return tafl_gmcts_policy_ex(b, temp, 0, 0, out, out_is_device); }

// play + re-root of the retained guided tree (tree_advance)
int tafl_gmcts_advance(tafl_batch* b, const uint32_t* actions, tafl_play* out_plays, tafl_effects* out_effects) {
    if (!b || !b->g_has) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_advance: tafl_gmcts_begin first");
    if (const int rc = join_search(b)) return rc;
    b->gsp_active = false;
    b->gsp_targets = ExampleTargetsMem{}; b->gsp_open_from = nullptr; b->gsp_targets_ex = nullptr;      // (the closed run holds its examples object no longer)
    const bool live = b->g_tree_live;
    if (!actions && !live) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_advance: actions == NULL needs a retained tree");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    GuidedMem& M = b->gmem;
    return tree_advance(b, "tafl_gmcts_advance", b->g_edges, b->g_edges_alt, b->g_idmap, M.node_cap, actions, out_plays, out_effects,
        [&](const uint32_t* acts, uint32_t A, tafl_play* dplays, tafl_effects* deff, uint32_t* bad) {
            dispatch<BATCH, false>(c, [&](auto t) {
                LAUNCH_PER_GAME((k_gmcts_advance<t.NL, t.W>), c, b->n, t.CC, M, b->soa, b->g_edges_alt.as<GEdge>(), b->g_idmap.as<uint32_t>(), acts, live ? 1 : 0, A, dplays, deff, bad); });
        },
        [&] { b->g_edges.bind(M.edges); b->g_tree_live = true; b->tree_live = false; });                      // (the rollout-mode tree belongs to the states before the play)
}

int tafl_gmcts_tree_nodes(tafl_batch* b, uint32_t* out) {
    if (!b || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    if (!b->g_has || !b->g_tree_live) { memset(out, 0, sizeof(uint32_t) * b->n); return TAFL_OK; }
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    COPY_OUT(out, b->gmem.node_top, b->n, c->stream);
    return sync_ok(c);
}

int tafl_gmcts_get_stats(tafl_batch* b, tafl_gmcts_stats* out) {
    if (!b || !b->g_has || !out) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmcts_get_stats: bad argument");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long h[GS_COUNT];
    HIPCHK(hipMemcpyAsync(h, b->g_stats.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof *out);
    out->sims = h[GS_SIMS]; out->predicts = h[GS_PREDICTS]; out->terminal_hits = h[GS_TERMINAL]; out->faults = h[GS_FAULTS];
    out->select_depth_sum = h[GS_DEPTH]; out->waiting = h[GS_WAITING];
    return TAFL_OK;
}

// ---- guided self-play at each game's own pace -----------------------------------------------------------------
// the recorder of search statistics (Guided record_stats): one lane per game, after the round and its reopen, on
// the same stream; launched only for a run whose examples object carries the arrays
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_record_stats(GuidedMem M, ExamplesMem X, ExampleStatsMem S) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    record_stats(M, g, X, S);
}
// the recorder of episode boundaries (vt_mark_boundary): one lane per game, behind the recorder above, hence after
// the reopen of every family; launched only for a run whose examples object carries value targets
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_mark_boundary(ExamplesMem X, ExampleTargetsMem T, const uint32_t* open_from) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= X.G) return;
    vt_mark_boundary(X, T, open_from, g);
}
static int gselfplay_mark_boundary(tafl_batch* b) {
    if (!b->gsp_targets.ep_end) return TAFL_OK;
    b->gsp_targets_ex->vt_valid = false;                     // (a round may append examples the targets know nothing of)
    LAUNCH_PER_GAME(k_gselfplay_mark_boundary, b->ctx, b->n, b->gsp_rec.ex, b->gsp_targets, b->gsp_open_from);
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}
static int gselfplay_record_stats(tafl_batch* b) {
    if (!b->gsp_stats.cq) return TAFL_OK;
    LAUNCH_PER_GAME(k_gselfplay_record_stats, b->ctx, b->n, b->gmem, b->gsp_rec.ex, b->gsp_stats);
    HIPCHK(hipGetLastError());
    return gselfplay_mark_boundary(b);
}
static int gselfplay_rounds(tafl_batch* b, const float* dp, const float* dv);
static int gselfplay_launch(tafl_batch* b, const float* dp, const float* dv) {
    if (const int rc = gselfplay_rounds(b, dp, dv)) return rc;
    return gselfplay_record_stats(b);
}
static int gselfplay_rounds(tafl_batch* b, const float* dp, const float* dv) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, A = tafl_action_size(c);
    unsigned long long* st = b->g_stats.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(st + GS_WAITING, 0, sizeof(unsigned long long), c->stream));
    if (b->gmem.sym) return gsym_launch_selfplay(b, dp, dv, A, st);      // the run latched the eval symmetry: rounds (and reopen) of their own
    if (b->gsp_solver_on) {                                     // exact proofs: rounds of their own (whatever the noise, the cap and the forcing), then the reopen
        const bool nz = b->g_noise_on, ep = b->gsp_episodes;
#define TAFL_SOLVER(NZ, EP) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_solver<t.NL, t.W, NZ, EP>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_ep, b->gsp_rec, st, b->g_noise, b->gsp_cap, b->gsp_forced, b->gsp_solver); })
        if (ep) { if (nz) TAFL_SOLVER(true, true); else TAFL_SOLVER(false, true); }
        else { if (nz) TAFL_SOLVER(true, false); else TAFL_SOLVER(false, false); }
#undef TAFL_SOLVER
        if (ep) {
            HIPCHK(hipGetLastError());
            dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_reopen<t.NL, t.W>), c, n, b->gmem, b->soa, b->gsp, b->gsp_ep, b->gsp_rec, st); });
        }
    }
    else if (b->gsp_forced_on) {                                // forced playouts: rounds of their own (with or without a cap), then the reopen
        const bool nz = b->g_noise_on, ep = b->gsp_episodes;
#define TAFL_FORCED(NZ, EP) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_forced<t.NL, t.W, NZ, EP>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_ep, b->gsp_rec, st, b->g_noise, b->gsp_cap, b->gsp_forced); })
        if (ep) { if (nz) TAFL_FORCED(true, true); else TAFL_FORCED(false, true); }
        else { if (nz) TAFL_FORCED(true, false); else TAFL_FORCED(false, false); }
#undef TAFL_FORCED
        if (ep) {
            HIPCHK(hipGetLastError());
            dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_reopen<t.NL, t.W>), c, n, b->gmem, b->soa, b->gsp, b->gsp_ep, b->gsp_rec, st); });
        }
    }
    else if (b->gsp_cap_on) {                                   // a capped run: rounds of its own, then the reopen of an episodes run as below
        const bool nz = b->g_noise_on, ep = b->gsp_episodes;
#define TAFL_CAPPED(NZ, EP) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_capped<t.NL, t.W, NZ, EP>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_ep, b->gsp_rec, st, b->g_noise, b->gsp_cap); })
        if (ep) { if (nz) TAFL_CAPPED(true, true); else TAFL_CAPPED(false, true); }
        else { if (nz) TAFL_CAPPED(true, false); else TAFL_CAPPED(false, false); }
#undef TAFL_CAPPED
        if (ep) {
            HIPCHK(hipGetLastError());
            dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_reopen<t.NL, t.W>), c, n, b->gmem, b->soa, b->gsp, b->gsp_ep, b->gsp_rec, st); });
        }
    }
    else if (b->gsp_episodes) {
        if (b->g_noise_on) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_episodes<t.NL, t.W, true>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_ep, b->gsp_rec, st, b->g_noise); });
        else dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_episodes<t.NL, t.W>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_ep, b->gsp_rec, st); });
        HIPCHK(hipGetLastError());
        dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_reopen<t.NL, t.W>), c, n, b->gmem, b->soa, b->gsp, b->gsp_ep, b->gsp_rec, st); });
    }
    else if (b->g_noise_on) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_step<t.NL, t.W, true>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_rec, st, b->g_noise); });
    else dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_step<t.NL, t.W>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_rec, st); });
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}

// tafl_gselfplay_begin, and with `eo` tafl_gselfplay_begin_episodes (`openings` then names the batch whose states are the openings)
static int gselfplay_begin(tafl_batch* b, uint32_t n_sims, uint32_t edges_per_node, double c_puct, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t game_id_base,
                           tafl_examples* ex, const tafl_episode_opts* eo, tafl_batch* openings) {
    if (!b || !o || n_sims == 0 || edges_per_node == 0 || n_moves == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin: bad argument");
    if (n_sims > 0xFFFFu) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin: n_sims must be below 65536 (Nsa is stored in 16 bits)");
    if (o->flags != 0 || o->_reserved[0] != 0 || o->_reserved[1] != 0 || o->_reserved[2] != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_selfplay_opts: flags and reserved words must be 0");
    if ((unsigned long long)o->move_base + n_moves > 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin: move_base + n_moves exceeds 32 bits");
    if (ex && (ex->n_games != b->n || ex->ctx->device != b->ctx->device || ex->ctx->n != b->ctx->n))
        return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin: the examples object was created for another batch size, board or device");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    if (eo) {
        if (eo->flags != 0 || eo->_reserved[0] != 0 || eo->_reserved[1] != 0 || eo->_reserved[2] != 0 || eo->_reserved[3] != 0)
            return fail(TAFL_ERR_UNSUPPORTED, "tafl_episode_opts: flags and reserved words must be 0");
        if (o->move_base != 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin_episodes: move_base must be 0 (move numbers are per episode)");
        if (openings->n != n || openings->ctx->device != c->device || openings->ctx->n != c->n || openings->ctx->nl != c->nl)
            return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin_episodes: the openings batch has another size, board or device");
    }
    b->gsp_active = false; b->gsp_has = false;                 // (a begin that fails from here on leaves no run to step, end or ask for stats)
    b->gm_on = false; b->gm_leaves = false;                    // (tafl_gmatch_begin marks its run after this function)
    if (b->cap_set && b->cap_cfg.fast_sims > n_sims) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin: the playout cap's fast_sims exceeds n_sims");
    if (const int rc = join_search(b)) return rc;
    if (eo && openings != b) {
        if (const int rc = join_search(openings)) return rc;
        if (openings->ctx != c) { HIPCHK(hipSetDevice(openings->ctx->device)); HIPCHK(hipStreamSynchronize(openings->ctx->stream)); }
    }
    if (ex) { HIPCHK(hipSetDevice(ex->ctx->device)); HIPCHK(hipStreamSynchronize(ex->ctx->stream)); }      // (clears and gathers of another context's stream)
    HIPCHK(hipSetDevice(c->device));
    b->tree_live = false; b->g_tree_live = false; b->ran = false;      // the run plays away from the roots of both retained trees
    if (const int rc = gmcts_arena(b, n_sims, edges_per_node, "tafl_gselfplay_begin")) return rc;
    if (const int rc = evalsym_latch(b, game_id_base)) return rc;      // the run latches the eval symmetry; its game ids are the run's own
    NEED(b->gsp_moves_done, sizeof(uint32_t) * (size_t)n); NEED(b->gsp_plays, sizeof(tafl_play) * (size_t)n * n_moves);
    b->gsp_moves_done.bind(b->gsp.moves_done); b->gsp_plays.bind(b->gsp.plays); b->gsp.n_moves = n_moves;
    b->gsp_episodes = eo != nullptr; b->gsp_ep = GEpisodes{};
    if (eo) {
        const size_t state_bytes = sizeof(Quad) * (size_t)quads_of(c) * n;
        NEED(b->gsp_episode, sizeof(uint32_t) * (size_t)n); NEED(b->gsp_ep_start, sizeof(uint32_t) * (size_t)n); NEED(b->gsp_openings, state_bytes);
        NEED(b->gsp_ep_counters, sizeof(unsigned long long) * EP_COUNT);
        GEpisodes& ep = b->gsp_ep;
        b->gsp_episode.bind(ep.episode); b->gsp_ep_start.bind(ep.ep_start); b->gsp_ep_counters.bind(ep.ep_counters);
        ep.openings = b->gsp_openings.as<const Quad>(); ep.open_from = ex ? ex->open_from.as<uint32_t>() : nullptr;
        ep.episode_moves = eo->episode_moves; ep.id_stride = eo->id_stride ? eo->id_stride : (uint64_t)n;
        HIPCHK(hipMemsetAsync(b->gsp_episode.p, 0, sizeof(uint32_t) * (size_t)n, c->stream));
        HIPCHK(hipMemsetAsync(b->gsp_ep_start.p, 0, sizeof(uint32_t) * (size_t)n, c->stream));
        HIPCHK(hipMemsetAsync(b->gsp_ep_counters.p, 0, sizeof(unsigned long long) * EP_COUNT, c->stream));
        HIPCHK(hipMemcpyAsync(b->gsp_openings.p, openings->soa, state_bytes, hipMemcpyDeviceToDevice, c->stream));      // the copy the run reopens from
    }
    b->gsp_rec = SelfPlayRec{};
    if (ex) b->gsp_rec.ex = ex->mem;
    b->gsp_stats = ExampleStatsMem{};
    if (ex && (ex->flags & TAFL_EXAMPLES_SEARCH_STATS)) {      // the recorder deals with what this run appends: seen = len
        b->gsp_stats = ex->smem;
        HIPCHK(hipMemcpyAsync(ex->seen.p, ex->len.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    }
    b->gsp_targets = ExampleTargetsMem{}; b->gsp_open_from = nullptr; b->gsp_targets_ex = nullptr;
    if (ex && (ex->flags & TAFL_EXAMPLES_VALUE_TARGETS)) {     // the boundary the object's open_from names as the run begins; its targets are stale from here on
        b->gsp_targets = ex->tmem; b->gsp_open_from = ex->open_from.as<const uint32_t>(); b->gsp_targets_ex = ex;
        if (const int rc = gselfplay_mark_boundary(b)) return rc;
    }
    b->gsp_rec.sample_seed = o->sample_seed; b->gsp_rec.game_id_base = game_id_base; b->gsp_rec.temp_moves = o->temp_moves; b->gsp_rec.move_base = o->move_base;
    b->gsp_sims = n_sims; b->gsp_cpuct = c_puct;
    b->g_noise_on = b->noise_set;                            // the run latches the noise setting; gid and M are the run's own
    if (b->noise_set) b->g_noise = noise_arg(b->noise_cfg);
    b->gsp_cap_on = b->cap_set; b->gsp_cap = PlayoutCap{};   // and the playout cap
    b->gsp_forced_on = b->forced_set; b->gsp_forced = ForcedPlayouts{};      // and forced playouts, whose rounds take a PlayoutCap in any case
    b->gsp_solver_on = b->solver_set; b->gsp_solver = SolverCfg{};          // and the solver, whose rounds take a PlayoutCap and a ForcedPlayouts (k == 0: none) in any case
    if (b->cap_set || b->forced_set || b->solver_set) {
        NEED(b->gsp_cap_counters, sizeof(unsigned long long) * CAP_COUNT);
        HIPCHK(hipMemsetAsync(b->gsp_cap_counters.p, 0, sizeof(unsigned long long) * CAP_COUNT, c->stream));
        if (b->cap_set) { b->gsp_cap.seed = b->cap_cfg.seed; b->gsp_cap.fast_sims = b->cap_cfg.fast_sims; b->gsp_cap.full_per_65536 = b->cap_cfg.full_per_65536; }
        else { b->gsp_cap.fast_sims = n_sims; b->gsp_cap.full_per_65536 = 65536u; }      // (every move is full)
        b->gsp_cap_counters.bind(b->gsp_cap.counters);
    }
    if (b->forced_set) {
        NEED(b->gsp_forced_counters, sizeof(unsigned long long) * FP_COUNT);
        HIPCHK(hipMemsetAsync(b->gsp_forced_counters.p, 0, sizeof(unsigned long long) * FP_COUNT, c->stream));
        b->gsp_forced.k = b->forced_cfg.k;
        b->gsp_forced_counters.bind(b->gsp_forced.counters);
    }
    if (b->solver_set) {
        NEED(b->gsp_solver_counters, sizeof(unsigned long long) * SV_COUNT);
        HIPCHK(hipMemsetAsync(b->gsp_solver_counters.p, 0, sizeof(unsigned long long) * SV_COUNT, c->stream));
        b->gsp_solver_counters.bind(b->gsp_solver.counters);
    }
    HIPCHK(hipMemsetAsync(b->gsp_plays.p, 0, sizeof(tafl_play) * (size_t)n * n_moves, c->stream));
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_init<t.NL, t.W>), c, n, t.CC, b->soa, b->gmem, b->gsp); });
    HIPCHK(hipGetLastError());
    b->g_has = true; b->g_max_sims = n_sims;
    if (const int rc = gselfplay_launch(b, nullptr, nullptr)) return rc;      // the first round: every live root waits for its evaluation
    b->gsp_has = true; b->gsp_active = true; b->gsp_first = true;
    return TAFL_OK;
}

int tafl_gselfplay_begin(tafl_batch* b, uint32_t n_sims, uint32_t edges_per_node, double c_puct, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t game_id_base,
                         tafl_examples* ex) {
    return gselfplay_begin(b, n_sims, edges_per_node, c_puct, o, n_moves, game_id_base, ex, nullptr, nullptr);
}

int tafl_gselfplay_begin_episodes(tafl_batch* b, uint32_t n_sims, uint32_t edges_per_node, double c_puct, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t game_id_base,
                                  tafl_examples* ex, const tafl_episode_opts* eo, tafl_batch* openings) {
    if (!b || !eo) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_begin_episodes: bad argument");
    return gselfplay_begin(b, n_sims, edges_per_node, c_puct, o, n_moves, game_id_base, ex, eo, openings ? openings : b);
}

int tafl_gselfplay_episode_stats(tafl_batch* b, uint32_t* out_episodes, tafl_episode_stats* out) {
    if (!b || !b->gsp_has || !b->gsp_episodes || !out) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_episode_stats: tafl_gselfplay_begin_episodes first");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long h[EP_COUNT];
    HIPCHK(hipMemcpyAsync(h, b->gsp_ep_counters.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    COPY_OUT(out_episodes, b->gsp_episode.p, b->n, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof *out);
    out->attacker_wins = h[EP_ATTACKER]; out->defender_wins = h[EP_DEFENDER]; out->draws = h[EP_DRAW]; out->cut = h[EP_CUT];
    return TAFL_OK;
}

int tafl_gselfplay_step(tafl_batch* b, const float* priors, const float* values, int in_is_device, uint32_t* out_waiting) {
    if (!b || !b->gsp_active) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_step: no run is open on this batch (tafl_gselfplay_begin first; a write to the batch states closes a run)");
    if (b->gm_on) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_step: the open run is a match (tafl_gmatch_leaves / tafl_gmatch_step)");
    if ((priors == nullptr) != (values == nullptr)) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_step: priors and values go together");
    if (b->gsp_first != (priors == nullptr)) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_step: the first step after tafl_gselfplay_begin, and only that one, takes priors = values = NULL");
    HIPCHK(hipSetDevice(b->ctx->device));
    if (b->gsp_first) { b->gsp_first = false; return gmcts_waiting(b, out_waiting); }      // (tafl_gselfplay_begin ran that round)
    if (const int rc = stage_evaluation(b, priors, values, in_is_device)) return rc;
    if (const int rc = gselfplay_launch(b, priors, values)) return rc;
    return gmcts_waiting(b, out_waiting);
}

int tafl_gselfplay_end(tafl_batch* b, tafl_play* out_plays, uint32_t* out_moves) {
    if (!b || !b->gsp_has) return fail(TAFL_ERR_INVALID_ARG, "tafl_gselfplay_end: tafl_gselfplay_begin first");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    b->gsp_active = false;
    b->gsp_targets = ExampleTargetsMem{}; b->gsp_open_from = nullptr; b->gsp_targets_ex = nullptr;      // (the closed run holds its examples object no longer)
    HIPCHK(hipSetDevice(c->device));
    COPY_OUT(out_plays, b->gsp_plays.p, (size_t)n * b->gsp.n_moves, c->stream);
    COPY_OUT(out_moves, b->gsp_moves_done.p, n, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out_moves) for (uint32_t g = 0; g < n; ++g) out_moves[g] &= ~(kGspStopped | kGspEpisodeEnded);
    return TAFL_OK;
}

// ---- match play: two evaluators in an episodes run ---------------------------------------------------------------
int tafl_gmatch_begin(tafl_batch* b, uint32_t n_sims, uint32_t edges_per_node, double c_puct, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t game_id_base,
                      tafl_examples* ex, const tafl_episode_opts* eo, tafl_batch* openings, const tafl_match_opts* mo) {
    if (!b || !eo || !mo) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_begin: bad argument");
    if (mo->swap > 1u) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_begin: swap must be 0 or 1");
    if (mo->flags != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_match_opts: flags and reserved words must be 0");
    for (uint32_t r : mo->_reserved) if (r != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_match_opts: flags and reserved words must be 0");
    if (b->noise_set) return fail(TAFL_ERR_UNSUPPORTED, "tafl_gmatch_begin: root noise is set on the batch (tafl_gmcts_set_root_noise(NULL) first)");
    if (b->cap_set) return fail(TAFL_ERR_UNSUPPORTED, "tafl_gmatch_begin: a playout cap is set on the batch (tafl_gselfplay_set_playout_cap(NULL) first)");
    if (b->solver_set) return fail(TAFL_ERR_UNSUPPORTED, "tafl_gmatch_begin: the solver is set on the batch (tafl_gselfplay_set_solver(NULL) first)");
    if (b->forced_set) return fail(TAFL_ERR_UNSUPPORTED, "tafl_gmatch_begin: forced playouts are set on the batch (tafl_gselfplay_set_forced_playouts(NULL) first)");
    if (b->evalsym_set) return fail(TAFL_ERR_UNSUPPORTED, "tafl_gmatch_begin: the eval symmetry is set on the batch (tafl_gmcts_set_eval_symmetry(NULL) first)");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    if (const int rc = gselfplay_begin(b, n_sims, edges_per_node, c_puct, o, n_moves, game_id_base, ex, eo, openings ? openings : b)) return rc;
    b->gsp_active = false; b->gsp_has = false;                 // (the run counts as open once its match buffers exist)
    const uint32_t n_blocks = (n + TAFL_MATCH_BLOCK - 1) / TAFL_MATCH_BLOCK;
    NEED(b->gm_row_of, sizeof(uint32_t) * (size_t)n); NEED(b->gm_lanes, sizeof(uint32_t) * 2 * (size_t)n); NEED(b->gm_blocks, sizeof(uint32_t) * 2 * (size_t)n_blocks);
    NEED(b->gm_counts, sizeof(uint32_t) * 2); NEED(b->gm_games, sizeof(unsigned long long) * 2 * EP_COUNT);
    b->gm.swap = mo->swap; b->gm_row_of.bind(b->gm.row_of); b->gm_games.bind(b->gm.games);
    HIPCHK(hipMemsetAsync(b->gm_games.p, 0, sizeof(unsigned long long) * 2 * EP_COUNT, c->stream));
    b->gsp_has = true; b->gsp_active = true; b->gsp_first = false; b->gm_on = true; b->gm_leaves = false;
    return TAFL_OK;
}

int tafl_gmatch_leaves(tafl_batch* b, const tafl_match_io* io, int out_is_device, uint32_t out_count[2]) {
    if (!b || !b->gsp_active || !b->gm_on) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_leaves: no match run is open on this batch (tafl_gmatch_begin first; a write to the batch states closes a run)");
    if (!io || !out_count) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_leaves: null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, nn = (uint32_t)c->n * c->n;
    const uint32_t n_blocks = (n + TAFL_MATCH_BLOCK - 1) / TAFL_MATCH_BLOCK;
    HIPCHK(hipSetDevice(c->device));
    b->gm_leaves = false;
    uint32_t* row_of = b->gm_row_of.as<uint32_t>(); uint32_t* lanes = b->gm_lanes.as<uint32_t>(); uint32_t* blocks = b->gm_blocks.as<uint32_t>(); uint32_t* counts = b->gm_counts.as<uint32_t>();
    dispatch<BATCH, false>(c, [&](auto t) {
        hipLaunchKernelGGL((k_gmatch_rank<t.NL, t.W>), dim3(n_blocks), dim3(TAFL_MATCH_BLOCK), 0, c->stream, b->gmem, (const Quad*)b->soa, (const uint32_t*)b->gsp_ep.episode,
                           b->gsp_rec.game_id_base, b->gm.swap, row_of, blocks); });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_gmatch_place, dim3(n_blocks), dim3(TAFL_MATCH_BLOCK), 0, c->stream, n, n_blocks, (const uint32_t*)blocks, row_of, lanes, counts);
    HIPCHK(hipGetLastError());
    uint32_t cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, counts, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out_count[0] = cnt[0]; out_count[1] = cnt[1];
    if (cnt[0] > io->cap[0] || cnt[1] > io->cap[1]) return fail(TAFL_ERR_CAPACITY, "tafl_gmatch_leaves: an evaluator has more waiting leaves than its cap (cap = batch size is always enough)");
    // host pointers: the rows are staged behind one another in the buffers of tafl_gmcts_leaves (count_0 + count_1 <= n) and the waiting
    // flags are written on the host
    MatchOut mo;
    for (int e = 0; e < 2; ++e) {
        mo.boards[e] = io->boards[e]; mo.sides[e] = io->sides[e]; mo.waiting[e] = out_is_device ? io->waiting[e] : nullptr; mo.lanes[e] = out_is_device ? io->lanes[e] : nullptr;
        mo.cap[e] = io->cap[e];
    }
    if (!out_is_device) {
        NEED(b->g_boards, (size_t)n * nn); NEED(b->g_sides, n);
        for (int e = 0; e < 2; ++e) {
            const uint32_t first = e ? cnt[0] : 0u;
            if (io->boards[e]) mo.boards[e] = b->g_boards.as<uint8_t>() + (size_t)first * nn;
            if (io->sides[e]) mo.sides[e] = b->g_sides.as<uint8_t>() + first;
        }
    }
    const size_t total = (size_t)n * nn;
    dispatch<BATCH, false>(c, [&](auto t) {
        hipLaunchKernelGGL((k_gmatch_leaves<t.NL, t.W>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, t.CC, b->gmem, (const uint32_t*)lanes, (const uint32_t*)counts, mo); });
    HIPCHK(hipGetLastError());
    if (!out_is_device) {
        for (int e = 0; e < 2; ++e) {
            if (cnt[e]) {
                COPY_OUT(io->boards[e], mo.boards[e], (size_t)cnt[e] * nn, c->stream);
                COPY_OUT(io->sides[e], mo.sides[e], cnt[e], c->stream);
                COPY_OUT(io->lanes[e], lanes + (size_t)e * n, cnt[e], c->stream);
            }
            if (io->waiting[e]) for (uint32_t r = 0; r < io->cap[e]; ++r) io->waiting[e][r] = r < cnt[e] ? 1 : 0;
        }
    }
    if (const int rc = sync_ok(c)) return rc;
    b->gm_count[0] = cnt[0]; b->gm_count[1] = cnt[1]; b->gm_leaves = true;
    return TAFL_OK;
}

int tafl_gmatch_step(tafl_batch* b, const float* const priors[2], const float* const values[2], int in_is_device) {
    if (!b || !b->gsp_active || !b->gm_on) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_step: no match run is open on this batch (tafl_gmatch_begin first; a write to the batch states closes a run)");
    if (!b->gm_leaves) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_step: tafl_gmatch_leaves first (once per step)");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, A = tafl_action_size(c);
    MatchIn in;
    for (int e = 0; e < 2; ++e) {
        in.priors[e] = priors ? priors[e] : nullptr; in.values[e] = values ? values[e] : nullptr;
        if (b->gm_count[e] && (!in.priors[e] || !in.values[e])) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_step: priors and values of an evaluator with waiting leaves are missing");
        if (!b->gm_count[e]) in.priors[e] = in.values[e] = nullptr;
    }
    HIPCHK(hipSetDevice(c->device));
    if (!in_is_device) {                                        // exactly count_e rows of each evaluator, behind one another in g_priors / g_values
        const size_t rows = (size_t)b->gm_count[0] + b->gm_count[1];
        NEED(b->g_priors, sizeof(float) * std::max<size_t>(rows, 1) * A); NEED(b->g_values, sizeof(float) * std::max<size_t>(rows, 1));
        for (int e = 0; e < 2; ++e) {
            if (!b->gm_count[e]) continue;
            const size_t first = e ? b->gm_count[0] : 0u, cnt = b->gm_count[e];
            float* dp = b->g_priors.as<float>() + first * A; float* dv = b->g_values.as<float>() + first;
            HIPCHK(hipMemcpyAsync(dp, in.priors[e], sizeof(float) * cnt * A, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(dv, in.values[e], sizeof(float) * cnt, hipMemcpyHostToDevice, c->stream));
            in.priors[e] = dp; in.values[e] = dv;
        }
    }
    b->gm_leaves = false;
    unsigned long long* st = b->g_stats.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(st + GS_WAITING, 0, sizeof(unsigned long long), c->stream));
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmatch_round<t.NL, t.W>), c, n, t.CC, b->gmem, b->soa, in, (const uint32_t*)b->gm.row_of, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_ep, b->gsp_rec, st); });
    HIPCHK(hipGetLastError());
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmatch_tally<t.NL, t.W>), c, n, b->gmem, (const Quad*)b->soa, b->gsp, b->gsp_ep, b->gsp_rec, b->gm); });
    HIPCHK(hipGetLastError());
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_reopen<t.NL, t.W>), c, n, b->gmem, b->soa, b->gsp, b->gsp_ep, b->gsp_rec, st); });
    HIPCHK(hipGetLastError());
    if (const int rc = gselfplay_record_stats(b)) return rc;
    return in_is_device ? TAFL_OK : sync_ok(c);                // (host arrays may be reused once the call returns)
}

int tafl_gmatch_get_stats(tafl_batch* b, tafl_match_stats* out) {
    if (!b || !b->gsp_has || !b->gm_on || !out) return fail(TAFL_ERR_INVALID_ARG, "tafl_gmatch_get_stats: tafl_gmatch_begin first");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long h[2 * EP_COUNT];
    HIPCHK(hipMemcpyAsync(h, b->gm_games.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof *out);
    for (int a = 0; a < 2; ++a) for (int r = 0; r < EP_COUNT; ++r) out->games[a][r] = h[a * EP_COUNT + r];
    return TAFL_OK;
}

}  // extern "C"
