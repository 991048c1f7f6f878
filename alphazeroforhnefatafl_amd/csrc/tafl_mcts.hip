// tafl_mcts.hip — rollout-mode search: the MCTS kernels, the search driver (tafl_mcts_run and its kin, tafl_selfplay_run), the readers of
// a search's results, and subtree reuse (arena growth, re-root).
#include "tafl_internal.hpp"

// ---- MCTS kernels ---------------------------------------------------------------------------------
enum { ST_SIMS = 0, ST_ROLLOUTS, ST_PLIES, ST_DEPTH, ST_SCANNED, ST_TERMINAL, ST_FAULTS, ST_SPEC_ISSUED, ST_REASON0 = 8, ST_SPEC_HITS = 24, ST_EXEC = 25, ST_DONE = 26, ST_COUNT = 28 };
// control words of a search in flight (device memory, one set per batch): the width cap of the prediction pass is steered ON THE DEVICE
// from the hit rate of the last window, so that a whole search can be enqueued without a single read-back (tafl_mcts_run_async)
enum { CT_WCAP = 0, CT_LAST_ISSUED, CT_LAST_HITS, CT_NEXT_CHECK, CT_COUNT };
static_assert(CT_COUNT == 4, "SearchPlan::ctrl0");
__device__ __forceinline__ unsigned long long ld_counter(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ void stat_add(unsigned long long* stats, int idx, uint32_t v) {
    const uint32_t s = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&stats[idx], (unsigned long long)s);
}

template <int NLS, int WS, int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_init(Consts<NL> C, const Quad* soa, MctsMem M) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    DState<NL> st; load_batch_state<NLS, WS, NL, W>(soa, M.G, g, C.n, st);
    Ops<NL, W>::mcts_init_game(M, g, st, C);
}

// tree phase of the simulation pipeline: consume finished playouts (backup), run as many further simulations as can be
// served by ready slots, then issue the next slots (tafl_ops.hpp mcts_tree_step)
// SP: a self-play run (tafl_selfplay_run): a game whose search is done plays its most visited root play on the batch state (soa, layout
// <NLS, WS>) and starts its next search in the same launch; its plan counts from the launch in which that search began
// REC: a recording run (tafl_selfplay_record): the advance also draws the play and appends the move's training example (Ops::selfplay_advance_rec)
template <int NLS, int WS, int NL, int W, int PRESET, bool SP, bool REC = false>
__device__ __forceinline__ void mcts_tree_launch(const Consts<NL>& Carg, const MctsMem& M, double c_puct, uint32_t n_sims, uint32_t round, uint32_t planned, uint32_t probe_every,
                                                 uint32_t target, unsigned long long* stats, const unsigned long long* ctrl, uint32_t* work, uint32_t* work_count,
                                                 uint32_t g_begin, uint32_t g_end, Quad* soa, const SelfPlay& sp, const SelfPlayRec* rec = nullptr) {
    const uint32_t g = g_begin + blockIdx.x * TAFL_BLOCK + threadIdx.x;     // this launch serves games g_begin .. g_end - 1
    // the tree phase of one half of the batch runs beside the other half's playouts (2 - 4 waves per SIMD): it is one latency-bound wave
    // per SIMD on the critical path of its half, so its instructions go first
    __builtin_amdgcn_s_setprio(3);
    TAFL_PICK_CONSTS(C, Carg);
    LaneStats ls; ls.sims = ls.rollouts = ls.rollout_plies = ls.depth = ls.scanned = ls.terminal_hits = ls.faults = ls.reason = 0;
    ls.reason_hist4 = 0; ls.spec_issued = ls.spec_hits = 0;
    bool live = g < g_end && (M.sim_next[g] < n_sims || M.kind[g] == 1);
    if constexpr (SP) {
        const bool adv = g < g_end && !live && sp.moves_done[g] < sp.n_moves;
        if (__ballot(live || adv) == 0ull) return;
        int r = 0;
        if constexpr (REC) { if (adv) r = Ops<NL, W>::template selfplay_advance_rec<NLS, WS>(M, g, soa, sp, *rec, n_sims, round, C); }
        else if (adv) r = Ops<NL, W>::template selfplay_advance<NLS, WS>(M, g, soa, sp, n_sims, round, C);
        live = live || r == 1;                                // the new search takes its first step in this launch
        const unsigned long long fin = __ballot(r == 2);      // games that made their last play
        if ((threadIdx.x & 63u) == 0 && fin) atomicAdd(&stats[ST_DONE], (unsigned long long)__popcll(fin));
    } else {
        (void)soa; (void)sp;
        if (__ballot(live) == 0ull) return;                   // whole wave finished: nothing to do, nothing to count
    }
    // Plan (wave-uniform): inside the plan a game issues ceil(remaining / rounds left) slots.  Past it: 1 = "use every slot that exists"
    // (wasted playouts are free on an emptying device) for short searches and, for long ones, once three quarters of the games are done;
    // until then 0 = every game keeps to what its own hit history allows (a long search whose predictions fail runs far beyond the plan
    // with every game still alive: S = 1000 runs 44 M sims/s this way, 39 M otherwise).  Both only steer WHEN playouts run, never a result.
    uint32_t rounds_left;
    if constexpr (SP) { const uint32_t rel = live ? round - sp.start_round[g] : 0u; rounds_left = rel < planned ? planned - rel : 0u; }      // per game (the device never empties before the run's end)
    else if (round < planned) rounds_left = planned - round;
    else rounds_left = (probe_every == 0u || 4ull * ld_counter(&stats[ST_DONE]) >= 3ull * (unsigned long long)M.G) ? 1u : 0u;
    const uint32_t wcap = (uint32_t)ld_counter(&ctrl[CT_WCAP]);
    // the undo log of the prediction pass: LDS, one log per lane, word-interleaved (tafl_ops.hpp LogMem)
    extern __shared__ uint32_t tree_lds[];
    LogMem lm; lm.base = tree_lds; lm.stride = TAFL_BLOCK; lm.lane = threadIdx.x & 63u; lm.cap = TAFL_MCTS_UNDO_CAP;
    if (live) Ops<NL, W>::mcts_tree_step(M, g, c_puct, n_sims, rounds_left, Ops<NL, W>::mcts_scenarios(rounds_left, planned), wcap, C, ls, lm);
    if constexpr (!SP) {   // games that completed their last simulation in this launch (a finished game is never live again: counted once)
        const unsigned long long fin = __ballot(live && M.sim_next[g] >= n_sims && M.kind[g] != 1);
        if ((threadIdx.x & 63u) == 0 && fin) atomicAdd(&stats[ST_DONE], (unsigned long long)__popcll(fin));
    }
    // dense work lists of the playouts this round has to run, one list per priority class (MctsMem::spec_cls; work[c * stride ..], work_count[c];
    // entry = slot << 27 | game): the playout kernel walks them in class order up to what the device holds at once, so that the most
    // speculative playouts are the ones left for the next round when more is asked for.  One atomic per wave and slot; the loads of all
    // slots, then the atomics of all slots are in flight together (a dependent chain of eight was 8 round trips to L2).
    const uint32_t stride = g_end - g_begin;
    const uint32_t lane = threadIdx.x & 63u;
    uint8_t kd[TAFL_MCTS_MAX_SLOTS], cl[TAFL_MCTS_MAX_SLOTS];
    TAFL_UNROLL for (uint32_t j = 0; j < TAFL_MCTS_MAX_SLOTS; ++j) {
        const size_t o = (size_t)(j < M.spec_k ? j : 0u) * M.G + g;
        kd[j] = (live && j < M.spec_k) ? M.spec_kind[o] : (uint8_t)0;
        cl[j] = (live && j < M.spec_k) ? M.spec_cls[o] : (uint8_t)0;
    }
    // the slot of this game whose requested playout has priority class c (a game's requested playouts have distinct classes)
    uint32_t sl[TAFL_MCTS_MAX_SLOTS];
    TAFL_UNROLL for (uint32_t c = 0; c < TAFL_MCTS_MAX_SLOTS; ++c) {
        sl[c] = 0xFFu;
        TAFL_UNROLL for (uint32_t j = 0; j < TAFL_MCTS_MAX_SLOTS; ++j) sl[c] = (kd[j] == 1 && cl[j] == c) ? j : sl[c];
    }
    unsigned long long bal[TAFL_MCTS_MAX_SLOTS]; uint32_t base[TAFL_MCTS_MAX_SLOTS];
    TAFL_UNROLL for (uint32_t j = 0; j < TAFL_MCTS_MAX_SLOTS; ++j) {
        bal[j] = __ballot(sl[j] != 0xFFu);
        base[j] = 0;
        if (bal[j] != 0ull && (int)lane == __ffsll((long long)bal[j]) - 1) base[j] = atomicAdd(&work_count[j], (uint32_t)__popcll(bal[j]));
    }
    TAFL_UNROLL for (uint32_t j = 0; j < TAFL_MCTS_MAX_SLOTS; ++j) {
        if (bal[j] == 0ull) continue;
        const uint32_t b0 = (uint32_t)__shfl((int)base[j], __ffsll((long long)bal[j]) - 1);
        if ((bal[j] >> lane) & 1ull) work[(size_t)j * stride + b0 + (uint32_t)__popcll(bal[j] & ((1ull << lane) - 1ull))] = (sl[j] << 27) | g;
    }
    stat_add(stats, ST_SIMS, ls.sims); stat_add(stats, ST_DEPTH, ls.depth); stat_add(stats, ST_SCANNED, ls.scanned);
    stat_add(stats, ST_TERMINAL, ls.terminal_hits); stat_add(stats, ST_FAULTS, ls.faults);
    stat_add(stats, ST_ROLLOUTS, ls.rollouts); stat_add(stats, ST_PLIES, ls.rollout_plies);
    stat_add(stats, ST_SPEC_ISSUED, ls.spec_issued); stat_add(stats, ST_SPEC_HITS, ls.spec_hits);
    for (uint32_t r = 0; r < 16; ++r) stat_add(stats, ST_REASON0 + r, (uint32_t)((ls.reason_hist4 >> (4u * r)) & 15ull));
}
template <int NL, int W, int PRESET>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_tree(Consts<NL> Carg, MctsMem M, double c_puct, uint32_t n_sims, uint32_t round, uint32_t planned, uint32_t probe_every,
                                                          uint32_t target, unsigned long long* stats, const unsigned long long* ctrl, uint32_t* work, uint32_t* work_count,
                                                          uint32_t g_begin, uint32_t g_end) {
    SelfPlay none; none.moves_done = nullptr; none.start_round = nullptr; none.plays = nullptr; none.n_moves = 0;
    mcts_tree_launch<NL, W, NL, W, PRESET, false>(Carg, M, c_puct, n_sims, round, planned, probe_every, target, stats, ctrl, work, work_count, g_begin, g_end, nullptr, none);
}
template <int NLS, int WS, int NL, int W, int PRESET>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_tree_selfplay(Consts<NL> Carg, MctsMem M, double c_puct, uint32_t n_sims, uint32_t round, uint32_t planned, uint32_t probe_every,
                                                                   uint32_t target, unsigned long long* stats, const unsigned long long* ctrl, uint32_t* work, uint32_t* work_count,
                                                                   uint32_t g_begin, uint32_t g_end, Quad* soa, SelfPlay sp) {
    mcts_tree_launch<NLS, WS, NL, W, PRESET, true>(Carg, M, c_puct, n_sims, round, planned, probe_every, target, stats, ctrl, work, work_count, g_begin, g_end, soa, sp);
}

// the recording run's tree phase (tafl_selfplay_record): an instantiation of its own, so that k_mcts_tree_selfplay stays what it was
template <int NLS, int WS, int NL, int W, int PRESET>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_tree_selfplay_rec(Consts<NL> Carg, MctsMem M, double c_puct, uint32_t n_sims, uint32_t round, uint32_t planned, uint32_t probe_every,
                                                                       uint32_t target, unsigned long long* stats, const unsigned long long* ctrl, uint32_t* work, uint32_t* work_count,
                                                                       uint32_t g_begin, uint32_t g_end, Quad* soa, SelfPlay sp, SelfPlayRec rec) {
    mcts_tree_launch<NLS, WS, NL, W, PRESET, true, true>(Carg, M, c_puct, n_sims, round, planned, probe_every, target, stats, ctrl, work, work_count, g_begin, g_end, soa, sp, &rec);
}

// the dominant kernel: one seeded random playout per entry of the round's work list (slot, game), state resident in registers.
// spec_k slots per game put up to spec_k waves on every SIMD.
template <int NL, int W, int PRESET>
__global__ TAFL_KATTR __launch_bounds__(TAFL_BLOCK, TAFL_ROLLOUT_WAVES) void k_mcts_rollout(Consts<NL> Carg, MctsMem M, uint64_t seed, uint64_t base, uint32_t sim_offset,
                                                                       uint32_t max_plies, const uint32_t* work, const uint32_t* work_count, uint32_t* next_count,
                                                                       uint32_t stride, uint32_t capacity, unsigned long long* stats, uint32_t* trace,
                                                                       unsigned long long* ctrl, uint32_t round, uint32_t planned, uint32_t probe_every) {
    // entry i of the concatenated per-class work lists; entries beyond `capacity` (what the device holds at once) wait for the next round
    uint32_t pre[TAFL_MCTS_MAX_SLOTS + 1];
    pre[0] = 0;
    TAFL_UNROLL for (uint32_t t = 0; t < TAFL_MCTS_MAX_SLOTS; ++t) pre[t + 1] = pre[t] + work_count[t];
    const uint32_t cnt = pre[TAFL_MCTS_MAX_SLOTS] < capacity ? pre[TAFL_MCTS_MAX_SLOTS] : capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (trace) { trace[0] = pre[TAFL_MCTS_MAX_SLOTS]; trace[1] = cnt; }                // this round: requested, run
        TAFL_UNROLL for (uint32_t t = 0; t < TAFL_MCTS_MAX_SLOTS; ++t) next_count[t] = 0;     // the next round's counters (the other buffer)
        // Width control of long searches (ctrl is handed to the first partition's launches only): every `probe_every` rounds inside the plan,
        // every few rounds past it, the share of predictions that came true since the last look sets how many predicted simulations a game
        // may run beside the pending one (a prediction costs a child expansion in the tree phase and, when it fails, a playout: S = 1000 runs
        // 50.6 M sims/s with the thresholds below, 45.5 M when the windows with 45 - 75 % hits get three predictions instead of one, S = 256
        // 63.8 M with them and 62.0 M with narrower ones; measured in round 2 with the same rule on the host).
        if (ctrl && probe_every && (unsigned long long)round + 1ull >= ctrl[CT_NEXT_CHECK]) {
            const unsigned long long issued = ld_counter(&stats[ST_SPEC_ISSUED]), hits = ld_counter(&stats[ST_SPEC_HITS]);
            const unsigned long long di = issued - ctrl[CT_LAST_ISSUED], dh = hits - ctrl[CT_LAST_HITS];
            ctrl[CT_LAST_ISSUED] = issued; ctrl[CT_LAST_HITS] = hits;
            unsigned long long wcap = ctrl[CT_WCAP];
            if (di > (unsigned long long)M.G / 4ull) wcap = 100ull * dh > 85ull * di ? M.spec_k - 1u : 100ull * dh > 75ull * di ? 3u : 100ull * dh > 70ull * di ? 2u : 1u;
            else if (wcap < M.spec_k - 1u) wcap += 1ull;                  // hardly anything was predicted: probe one wider
            __hip_atomic_store(&ctrl[CT_WCAP], wcap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ctrl[CT_NEXT_CHECK] = (unsigned long long)round + 1ull + (round + 1u < planned ? probe_every : (planned >= 32u ? 4u : 2u));
        }
    }
    if (blockIdx.x * TAFL_BLOCK >= cnt) return;
    const uint32_t i = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    TAFL_PICK_CONSTS(C, Carg);
    const auto lut = playout_tables<NL, W, PRESET>();            // (every lane of the workgroup is still here)
    const bool has = i < cnt;
    uint32_t cls = 0, off = 0;
    TAFL_UNROLL for (uint32_t t = 1; t < TAFL_MCTS_MAX_SLOTS; ++t) { const bool ge = i >= pre[t]; cls = ge ? t : cls; off = ge ? pre[t] : off; }
    const uint32_t e = has ? work[(size_t)cls * stride + (i - off)] : 0u;
    const uint32_t j = e >> 27, g = e & 0x07FFFFFFu;
    if (has) Ops<NL, W>::mcts_slot_rollout(M, j, g, seed, base + g, sim_offset, max_plies, C, lut, KernelPlayout());
    if ((threadIdx.x & 63) == 0) atomicAdd(&stats[ST_EXEC], (unsigned long long)__popcll(__ballot(has)));
}

// The fused form of the two kernels above: one wave owns 64 / K games for a whole chunk of rounds and alternates, without any
// grid-wide synchronisation, between the tree phase (its games on the first 64 / K lanes) and the playout phase (K slots x 64 / K
// games on all 64 lanes).  Nothing is shared between waves, so no wave ever waits for another: the tree phase of one wave hides
// under the playouts of the other wave on its SIMD, the per-round launches disappear, and a wave leaves as soon as its own games
// are done.  Same per-game functions, same memory layout, same results as the two-kernel path.
template <int NL, int W, int PRESET, int K>
__global__ TAFL_KATTR __launch_bounds__(TAFL_BLOCK, TAFL_ROLLOUT_WAVES) void k_mcts_fused(Consts<NL> Carg, MctsMem M, double c_puct, uint32_t n_sims, uint64_t seed,
                                                                     uint64_t base, uint32_t sim_offset, uint32_t max_plies, uint32_t max_rounds,
                                                                     unsigned long long* stats) {
    constexpr uint32_t GPW = TAFL_BLOCK / K;                      // games per wave
    const uint32_t lane = threadIdx.x;
    const uint32_t tg = blockIdx.x * GPW + lane;                  // tree phase: lane < GPW serves game tg
    const uint32_t rj = lane / GPW, rg = blockIdx.x * GPW + (lane % GPW);   // playout phase: slot rj of game rg
    TAFL_PICK_CONSTS(C, Carg);
    const auto lut = playout_tables<NL, W, PRESET>();
    LaneStats ls; ls.sims = ls.rollouts = ls.rollout_plies = ls.depth = ls.scanned = ls.terminal_hits = ls.faults = ls.reason = 0;
    ls.reason_hist4 = 0; ls.spec_issued = ls.spec_hits = 0;
    uint32_t executed = 0, finished = 0;
    extern __shared__ uint32_t tree_lds[];                        // undo log of the prediction pass (tafl_ops.hpp LogMem)
    LogMem lm; lm.base = tree_lds; lm.stride = TAFL_BLOCK; lm.lane = lane; lm.cap = K > 1 ? TAFL_MCTS_UNDO_CAP_FUSED : 0u;
    for (uint32_t round = 0; round < max_rounds; ++round) {
        const bool live = lane < GPW && tg < M.G && (M.sim_next[tg] < n_sims || M.kind[tg] == 1);
        if (__ballot(live) == 0ull) break;                        // every game of this wave has finished
        if (live) Ops<NL, W>::mcts_tree_step(M, tg, c_puct, n_sims, 0u, 2u, K, C, ls, lm);
        finished += (uint32_t)__popcll(__ballot(live && M.sim_next[tg] >= n_sims && M.kind[tg] != 1));
        if ((round & 3u) == 3u) {                                 // the packed 4-bit reason counters hold 15: at most 2 playouts are consumed per round
            for (uint32_t r = 0; r < 16; ++r) stat_add(stats, ST_REASON0 + r, (uint32_t)((ls.reason_hist4 >> (4u * r)) & 15ull));
            ls.reason_hist4 = 0;
        }
        __threadfence();                                          // slot records written by the tree lanes are read by all lanes
        const bool work = rg < M.G && rj < M.spec_k && M.spec_kind[(size_t)rj * M.G + rg] == 1;
        const unsigned long long wb = __ballot(work);
        if (wb == 0ull) continue;
        if (work) Ops<NL, W>::mcts_slot_rollout(M, rj, rg, seed, base + rg, sim_offset, max_plies, C, lut, KernelPlayout());
        executed += (uint32_t)__popcll(wb);
        __threadfence();
    }
    stat_add(stats, ST_SIMS, ls.sims); stat_add(stats, ST_DEPTH, ls.depth); stat_add(stats, ST_SCANNED, ls.scanned);
    stat_add(stats, ST_TERMINAL, ls.terminal_hits); stat_add(stats, ST_FAULTS, ls.faults);
    stat_add(stats, ST_ROLLOUTS, ls.rollouts); stat_add(stats, ST_PLIES, ls.rollout_plies);
    stat_add(stats, ST_SPEC_ISSUED, ls.spec_issued); stat_add(stats, ST_SPEC_HITS, ls.spec_hits);
    for (uint32_t r = 0; r < 16; ++r) stat_add(stats, ST_REASON0 + r, (uint32_t)((ls.reason_hist4 >> (4u * r)) & 15ull));
    if (lane == 0 && executed) atomicAdd(&stats[ST_EXEC], (unsigned long long)executed);
    if (lane == 0 && finished) atomicAdd(&stats[ST_DONE], (unsigned long long)finished);
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_root_children(Consts<NL> C, MctsMem M, tafl_root_child* out, uint32_t max_children, uint32_t* out_n) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    out_n[g] = Ops<NL, W>::mcts_root_children(M, g, C, out + (size_t)g * max_children, max_children);
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_root_visits(Consts<NL> C, MctsMem M, uint32_t* out, uint32_t action_size) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    const NodeHdr h = M.hdr[g];
    const Edge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
    for (uint32_t j = 0; j < h.m; ++j) {
        const Edge e = eb[j];
        const NodeHdr ch = M.hdr[(size_t)e.child * M.G + g];
        Move m; m.from = ch.mv_from; m.dir = ch.mv_dir; m.dist = ch.mv_dist; m.to = 0;
        out[(size_t)g * action_size + Ops<NL, W>::action_of(m, C)] = e.n;
    }
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_best_play(Consts<NL> C, MctsMem M, tafl_play* out_plays, uint32_t* out_visits) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    const NodeHdr h = M.hdr[g];
    const Edge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
    uint32_t best = 0; tafl_play bp; bp.from_row = bp.from_col = bp.axis = 0; bp.disp = 0;
    for (uint32_t j = 0; j < h.m; ++j) {                       // first maximum (src/mcts.rs:216-227)
        const Edge e = eb[j];
        if (e.n > best) {
            const NodeHdr ch = M.hdr[(size_t)e.child * M.G + g];
            Move m; m.from = ch.mv_from; m.dir = ch.mv_dir; m.dist = ch.mv_dist; m.to = 0;
            best = e.n; bp = Ops<NL, W>::to_play(m);
        }
    }
    out_plays[g] = bp; out_visits[g] = best;
}

// board_to_matrix (game/main.rs:55-83): corners 20, throne 30, soldier +1, king +5, one uint8 per tile, row-major n x n.
// One lane per tile: consecutive lanes write consecutive bytes.
// self-play step on the device: every game plays the most visited root play of its last search (first maximum, src/mcts.rs:216-227)
// on its batch state (do_valid_play); games whose root has no visited child (finished games) stay as they are
// NL, W: the batch layout (the play is applied to the batch state); WA: row stride of the search arena the root's plays are recorded in
template <int NL, int W, int WA>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_play_best(Consts<NL> C, MctsMem M, Quad* soa, tafl_play* out_plays, tafl_effects* eff) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    const NodeHdr h = M.hdr[g];
    const Edge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
    uint32_t best = 0; Move bm; bm.from = bm.to = bm.dir = bm.dist = 0;
    for (uint32_t j = 0; j < h.m; ++j) {
        const Edge e = eb[j];
        if (e.n > best) { const NodeHdr ch = M.hdr[(size_t)e.child * M.G + g]; best = e.n; bm.from = ch.mv_from; bm.dir = ch.mv_dir; bm.dist = ch.mv_dist; }
    }
    if constexpr (WA != W) bm.from = restride_sq<WA, W>(bm.from);
    DState<NL> st; StateIO<NL>::load_soa(soa, M.G, g, st);
    tafl_effects e; Ops<NL, W>::caps_to_effects(bz<NL>(), 0, e);
    tafl_play p; p.from_row = p.from_col = p.axis = 0; p.disp = 0;
    int code = TAFL_PLAY_GAME_OVER;
    if (best > 0 && TAFL_F_STATUS(st.flags) == TAFL_STATUS_ONGOING) {
        bm.to = (uint32_t)((int)bm.from + Engine<NL, W>::delta(bm.dir) * (int)bm.dist);
        p = Ops<NL, W>::to_play(bm);
        StepOut<NL> so; Moves<NL> nx;
        Engine<NL, W>::apply(st, bm, C, &so, nx);
        Ops<NL, W>::caps_to_effects(so.captures, so.n_captures, e);
        StateIO<NL>::store_soa(soa, M.G, g, st);
        code = TAFL_PLAY_OK;
    }
    Ops<NL, W>::status_to_effects(st, code, e);
    if (eff) eff[g] = e;
    if (out_plays) out_plays[g] = p;
}

// ---- subtree reuse (TAFL_MCTS_FLAG_KEEP_TREE) ------------------------------------------------------------------
// keep-init: a search that continues the retained tree (k_mcts_init for the games without one)
template <int NLS, int WS, int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_keep_init(Consts<NL> C, const Quad* soa, MctsMem M) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    if (M.node_top[g] == 0) { DState<NL> st; load_batch_state<NLS, WS, NL, W>(soa, M.G, g, C.n, st); Ops<NL, W>::mcts_init_game(M, g, st, C); }
    else Ops<NL, W>::mcts_keep_init(M, g);
}
// out[0] = max a[g], out[1] = max b[g] (kept nodes and edges of a retained tree: what the next search's arena must hold beside its own)
__global__ __launch_bounds__(256) void k_max2(const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    atomicMax(&out[0], a[g]); atomicMax(&out[1], b[g]);
}
// tafl_mcts_advance, one game per lane: play actions[g] (NULL: the most visited root child, first maximum) on the batch state and re-root
// the retained tree at that child (Ops::mcts_reroot).  live == 0: the arena holds no tree for these states (every game gets a fresh root).
// Every game's edges end up in `dst` (the caller swaps the arenas).  bad[0] counts kept roots whose state differs from the new batch state
// (never expected: such a game gets a fresh root).  Batch layout <NLS, WS>, arena layout <NL, W>.
template <int NLS, int WS, int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_advance(Consts<NLS> Cb, Consts<NL> Ca, MctsMem M, Quad* soa, Edge* dst, uint32_t* idmap,
                                                             const uint32_t* actions, int live, uint32_t A, tafl_play* out_plays, tafl_effects* eff, uint32_t* bad) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    using OA = Ops<NL, W>;
    const NodeHdr h = M.hdr[g];
    const Edge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
    uint32_t a = actions ? actions[g] : TAFL_ACTION_NONE, child = 0;
    if (live) {
        uint32_t best = 0;
        for (uint32_t j = 0; j < h.m; ++j) {
            const Edge e = eb[j];
            const NodeHdr ch = M.hdr[(size_t)e.child * M.G + g];
            Move m; m.from = ch.mv_from; m.dir = ch.mv_dir; m.dist = ch.mv_dist; m.to = 0;
            const uint32_t ea = OA::action_of(m, Ca);
            if (actions ? (ea == a && child == 0) : e.n > best) { best = e.n; child = e.child; a = ea; }
        }
    }
    DState<NLS> st; StateIO<NLS>::load_soa(soa, M.G, g, st);
    tafl_play p; tafl_effects e;
    const bool played = advance_play<NLS, WS>(Cb, st, a, A, p, e);
    if (played) StateIO<NLS>::store_soa(soa, M.G, g, st);
    const bool alone = !played && (a == TAFL_ACTION_NONE || e.code == TAFL_PLAY_GAME_OVER);      // nothing to play: the game is left alone
    if (live && alone) OA::mcts_keep_edges(M, dst, g);
    else {
        DState<NL> ast; load_batch_state<NLS, WS, NL, W>(soa, M.G, g, Cb.n, ast);
        bool fresh = !(live && played && child != 0);
        if (!fresh) {
            OA::mcts_reroot(M, dst, idmap, g, child);
            if (!same_state<NL>(M.node_state + (size_t)g * StateIO<NL>::QUADS, ast)) { atomicAdd(bad, 1u); fresh = true; }
        }
        if (fresh) OA::mcts_init_game(M, g, ast, Ca);           // never visited, an illegal action, or no tree: a root the tables have never seen
    }
    if (out_plays) out_plays[g] = p;
    if (eff) eff[g] = e;
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_mcts_policy(Consts<NL> C, MctsMem M, double* out, uint32_t action_size, int one_hot, double inv_temp,
                                                            uint64_t tie_seed, uint64_t base) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    const NodeHdr h = M.hdr[g];
    const Edge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
    double sum = 0.0; uint32_t best = 0, ties = 0;
    for (uint32_t j = 0; j < h.m; ++j) {
        const Edge e = eb[j];
        if (!one_hot) sum += temp_weight(e.n, inv_temp);
        if (e.n > best) { best = e.n; ties = 1; } else if (e.n == best && best > 0) ++ties;
    }
    uint32_t pick = 0;
    if (one_hot && tie_seed != 0 && ties > 1) pick = tie_pick(tie_seed, base + g, ties);
    uint32_t seen = 0;
    for (uint32_t j = 0; j < h.m; ++j) {
        const Edge e = eb[j];
        const NodeHdr ch = M.hdr[(size_t)e.child * M.G + g];
        Move m; m.from = ch.mv_from; m.dir = ch.mv_dir; m.dist = ch.mv_dist; m.to = 0;
        double p;
        if (one_hot) { const bool is_max = best > 0 && e.n == best; p = (is_max && seen == pick) ? 1.0 : 0.0; seen += is_max ? 1u : 0u; }
        else p = temp_weight(e.n, inv_temp) / sum;
        out[(size_t)g * action_size + Ops<NL, W>::action_of(m, C)] = p;
    }
    // all counts zero (the root was terminal): every action is a maximum (np.argwhere order); first, or the seeded choice among all actions
    if (one_hot && best == 0) out[(size_t)g * action_size + (tie_seed != 0 ? tie_pick(tie_seed, base + g, action_size) : 0u)] = 1.0;
}

// ---- host: arena capacity ----------------------------------------------------------------------------------------------------------------
static int arena_quads(const tafl_ctx* c) { return c->preset == PRESET_COPENHAGEN13 ? (2 * 6 + 8) / 4 : quads_of(c); }
int arena_max(tafl_batch* b, const uint32_t* node_top, const uint32_t* edge_top, uint32_t out[2]) {
    tafl_ctx* c = b->ctx;
    NEED(b->small, 64);
    HIPCHK(hipMemsetAsync(b->small.p, 0, 8, c->stream));
    hipLaunchKernelGGL(k_max2, dim3((b->n + 255) / 256), dim3(256), 0, c->stream, node_top, edge_top, b->n, b->small.as<uint32_t>());
    HIPCHK(hipGetLastError());
    COPY_OUT(out, b->small.p, 2, c->stream);
    return sync_ok(c);
}
// a device buffer grown to `bytes` with its first `keep` bytes kept (DevBuf::ensure drops the contents)
static int grow_keep(DevBuf& d, size_t bytes, size_t keep, hipStream_t s) {
    if (bytes <= d.cap) return TAFL_OK;
    DevBuf g;
    if (g.ensure(bytes)) return fail(TAFL_ERR_OOM, "hipMalloc(arena growth) failed");
    if (keep && (hipMemcpyAsync(g.p, d.p, keep, hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
        return fail(TAFL_ERR_HIP, "arena growth: copy failed");
    d = std::move(g);
    return TAFL_OK;
}
// an edge arena [g * stride + e] of G games moved to a larger stride, contents kept (a strided copy)
static int grow_stride(DevBuf& d, size_t elem, uint32_t G, uint32_t old_stride, uint32_t new_stride, hipStream_t s) {
    if (new_stride <= old_stride) return TAFL_OK;
    DevBuf g;
    if (g.ensure(elem * new_stride * G)) return fail(TAFL_ERR_OOM, "hipMalloc(edge arena growth) failed");
    if (hipMemcpy2DAsync(g.p, elem * new_stride, d.p, elem * old_stride, elem * old_stride, G, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail(TAFL_ERR_HIP, "edge arena growth: copy failed");
    d = std::move(g);
    return TAFL_OK;
}
// The node arrays are node-major, so their contents are a prefix of the larger ones; the edge arena gets a larger per-game stride (and the
// alternate edge arena of a re-root, which has the old stride, is released).  Nothing is ever pruned.
int arena_grow(tafl_batch* b, std::initializer_list<ArenaArray> node_arrays, uint32_t& node_cap, unsigned long long nodes,
               const ArenaArray& edge_array, DevBuf& edges_alt, uint32_t& edge_cap, unsigned long long edges) {
    hipStream_t s = b->ctx->stream; const size_t n = b->n;
    // every pointer follows its buffer as soon as that buffer has moved: a later failure (TAFL_ERR_OOM) leaves a consistent arena
    // of the old capacity with its tree intact
    if (nodes > node_cap) {
        for (const ArenaArray& a : node_arrays) {
            const int rc = grow_keep(*a.buf, (size_t)nodes * n * a.elem, (size_t)node_cap * n * a.elem, s);
            a.follow();
            if (rc != TAFL_OK) return rc;
        }
        node_cap = (uint32_t)nodes;
    }
    if (edges > edge_cap) {
        const int rc = grow_stride(*edge_array.buf, edge_array.elem, b->n, edge_cap, (uint32_t)edges, s);
        edge_array.follow();
        if (rc != TAFL_OK) return rc;
        edge_cap = (uint32_t)edges;
        edges_alt.release();
    }
    return TAFL_OK;
}
// the rollout-mode arena grown to `nodes` nodes and `edges` edges per game with the last search's tree kept (its readers stay valid, a
// retained tree stays retained)
static int mcts_grow(tafl_batch* b, unsigned long long nodes, unsigned long long edges) {
    MctsMem& M = b->mem;
    const int rc = arena_grow(b, {ArenaArray(b->node_state, (size_t)arena_quads(b->ctx) * sizeof(Quad), M.node_state), ArenaArray(b->hdr, sizeof(NodeHdr), M.hdr)}, M.node_cap, nodes,
                              ArenaArray(b->edges, sizeof(Edge), M.edges), b->edges_alt, M.edge_cap, edges);
    if (rc != TAFL_OK) return rc;
    const uint32_t by_nodes = M.node_cap - 1, by_edges = M.edge_cap / 4 - 1;
    b->reserved_sims = by_nodes < by_edges ? by_nodes : by_edges;
    return TAFL_OK;
}

// keep_tree: the caller may still read (or continue) the last search's tree; a search that starts afresh passes false
static int mcts_reserve(tafl_batch* b, uint32_t max_sims, bool keep_tree) {
    if (!b || max_sims == 0 || max_sims > 60000) return fail(TAFL_ERR_INVALID_ARG, "max_sims must be in 1..60000");
    tafl_ctx* c = b->ctx; const size_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    if (b->has_mem && b->reserved_sims >= max_sims) return TAFL_OK;
    // growing frees the arena a search in flight runs on (its plan keeps its own copy of the pointers): join it first
    if (const int rc = join_search(b)) return rc;
    const size_t node_cap = (size_t)max_sims + 1, edge_cap = 4 * ((size_t)max_sims + 1);
    if (keep_tree && b->has_mem && (b->ran || b->tree_live)) return mcts_grow(b, node_cap, edge_cap);      // the last search's tree moves with the arena
    b->tree_live = false;
    const size_t k = b->spec_k, aq = (size_t)arena_quads(c);
    MctsMem& M = b->mem;
    NEED(b->node_state, node_cap * n * aq * sizeof(Quad));
    NEED(b->hdr, node_cap * n * sizeof(NodeHdr));
    NEED(b->edges, edge_cap * n * sizeof(Edge));
    NEED(b->node_top, n * 4); NEED(b->edge_top, n * 4); NEED(b->leaf, n * 4);
    NEED(b->kind, n); NEED(b->fault, n);
    NEED(b->stats, sizeof(unsigned long long) * ST_COUNT);
    NEED(b->sim_next, n * 4); NEED(b->spec_state, k * n * aq * sizeof(Quad)); NEED(b->spec_value, k * n); NEED(b->spec_kind, k * n); NEED(b->spec_meta, k * n * 4);
    NEED(b->spec_reason, k * n); NEED(b->spec_plies, k * n * 4); NEED(b->spec_ref, k * n * 4); NEED(b->spec_cls, k * n); NEED(b->spec_pend, n * 4); NEED(b->spec_bias, n * 4);
    NEED(b->work, k * n * 4); NEED(b->work_count, 4 * 2 * TAFL_MCTS_MAX_SLOTS * TAFL_MCTS_MAX_PARTS); NEED(b->trace, 8 * TAFL_MCTS_TRACE_ROUNDS);
    NEED(b->ctrl, sizeof(unsigned long long) * CT_COUNT); NEED(b->sim_base, n * 4);
    b->node_state.bind(M.node_state); b->hdr.bind(M.hdr); b->edges.bind(M.edges);
    b->node_top.bind(M.node_top); b->edge_top.bind(M.edge_top); b->leaf.bind(M.leaf); b->kind.bind(M.kind); b->fault.bind(M.fault);
    b->sim_base.bind(M.sim_base); b->sim_next.bind(M.sim_next); b->spec_state.bind(M.spec_state); b->spec_value.bind(M.spec_value); b->spec_meta.bind(M.spec_meta);
    b->spec_kind.bind(M.spec_kind); b->spec_reason.bind(M.spec_reason); b->spec_plies.bind(M.spec_plies);
    b->spec_ref.bind(M.spec_ref); b->spec_cls.bind(M.spec_cls); b->spec_pend.bind(M.spec_pend); b->spec_bias.bind(M.spec_bias);
    M.spec_k = b->spec_k;
    M.G = b->n; M.node_cap = (uint32_t)node_cap; M.edge_cap = (uint32_t)edge_cap;
    M.flags = 0;
    b->has_mem = true; b->reserved_sims = max_sims;
    return TAFL_OK;
}

// A search that continues the retained trees needs room for the largest of them plus its own growth: n_sims + 1 nodes, and edges for
// 3 x the kept edges (a kept block that grows is copied once to twice its size before its new children pay for the next doubling) + the
// 4 (n_sims + 1) of a fresh search.  The arena grows with its contents kept; nothing is ever pruned: a tree that cannot fit fails the call
// before anything is launched.
static int mcts_keep_capacity(tafl_batch* b, uint32_t n_sims) {
    if (n_sims > 60000) return fail(TAFL_ERR_INVALID_ARG, "n_sims must be in 1..60000");
    uint32_t mx[2];
    if (const int rc = arena_max(b, b->mem.node_top, b->mem.edge_top, mx)) return rc;
    const unsigned long long nodes = (unsigned long long)mx[0] + n_sims + 1, edges = 3ull * mx[1] + 4ull * ((unsigned long long)n_sims + 1);
    if (nodes > kMctsMaxNodes) return fail(TAFL_ERR_CAPACITY, "TAFL_MCTS_FLAG_KEEP_TREE: the retained tree and the new simulations exceed 2^20 nodes");
    if (edges > 0xFFFFFFFFull) return fail(TAFL_ERR_CAPACITY, "TAFL_MCTS_FLAG_KEEP_TREE: the edge arena would exceed 2^32 edges per game");
    return mcts_grow(b, nodes, edges);
}

// ---- the search driver -------------------------------------------------------------------------------------------------------------
// tafl_mcts_run_async enqueues a whole search - the planned rounds plus the rounds its stragglers usually need - on the batch's own
// streams WITHOUT reading anything back: plan and width control live on the device (k_mcts_tree / k_mcts_rollout read the counters
// themselves), launches for a finished batch return at once.  tafl_mcts_wait joins the streams, reads the counters and, while games are
// still unfinished, runs further rounds: a search always completes (or the call fails), however many rounds its slowest game needs.
// tafl_mcts_run = the two back to back.  Results never depend on how a search was enqueued.
static int search_streams(tafl_batch* b, uint32_t parts) {
    if (b->n_sstreams == 0) {
        HIPCHK(hipEventCreateWithFlags(&b->ev_start, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&b->ev_half, hipEventDisableTiming));
    }
    while (b->n_sstreams < parts) {
        const uint32_t k = b->n_sstreams;
        HIPCHK(hipStreamCreateWithFlags(&b->sstream[k], hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&b->ev_fork[k], hipEventDisableTiming));
        b->n_sstreams = k + 1;
    }
    return TAFL_OK;
}

// rounds [next_round, next_round + count) of the two-kernel pipeline: per round and partition one tree launch (one game per lane: backups,
// real selections, slot matching, prediction of the next slots, dense work lists) and one playout launch over the work lists
static int mcts_enqueue_rounds(tafl_batch* b, uint32_t count, bool stagger) {
    tafl_ctx* c = b->ctx; SearchPlan& sp = b->plan; const tafl_mcts_params* p = &sp.p;
    unsigned long long* st = b->stats.as<unsigned long long>(); unsigned long long* ctrl = b->ctrl.as<unsigned long long>();
    const MctsMem& M = sp.M;
    for (uint32_t r = 0; r < count; ++r) {
        const uint32_t i = sp.next_round;
        if (i >= sp.max_rounds) return fail(TAFL_ERR_CAPACITY, "tafl_mcts: the search did not finish within its round bound");
        b->trace_rounds = i + 1;
        for (uint32_t k = 0; k < sp.parts; ++k) {
            const SearchPart& pk = sp.P[k];
            uint32_t* wc_now = pk.wc + (i & 1u) * TAFL_MCTS_MAX_SLOTS; uint32_t* wc_next = pk.wc + ((i + 1u) & 1u) * TAFL_MCTS_MAX_SLOTS;
            {
                SpanGuard sg(c, KC_MCTS_TREE, pk.s);
                dispatch<ARENA, true>(c, [&](auto t) {
                    // the tree launch; a self-play run's kernels also get the batch states and the run's records
                    auto launch = [&](auto kernel, auto... more) {
                        hipLaunchKernelGGL(kernel, dim3(pk.grid_tree), dim3(TAFL_BLOCK), TAFL_UNDO_LDS_BYTES(TAFL_MCTS_UNDO_CAP), pk.s, t.CC, M, p->c_puct, p->n_sims, i, sp.planned,
                                           sp.probe_every, sp.slots, st, ctrl, pk.wl, wc_now, pk.g0, pk.g1, more...);
                    };
                    if (sp.selfplay.n_moves && sp.recording) launch(k_mcts_tree_selfplay_rec<t.NLS, t.WS, t.NL, t.W, t.PRESET>, b->soa, sp.selfplay, sp.rec);
                    else if (sp.selfplay.n_moves) launch(k_mcts_tree_selfplay<t.NLS, t.WS, t.NL, t.W, t.PRESET>, b->soa, sp.selfplay);
                    else launch(k_mcts_tree<t.NL, t.W, t.PRESET>); });
            }
            // partition k+1 starts behind partition k's first tree launch: from then on the tree phases are spread over a round
            if (stagger && k + 1 < sp.parts) {
                if (hipEventRecord(b->ev_fork[k + 1], pk.s) != hipSuccess || hipStreamWaitEvent(sp.P[k + 1].s, b->ev_fork[k + 1], 0) != hipSuccess) return fail(TAFL_ERR_HIP, "tafl_mcts: stream fork failed");
            }
            {
                SpanGuard sg(c, KC_MCTS_ROLLOUT, pk.s);
                uint32_t* tr = (k == 0 && i < TAFL_MCTS_TRACE_ROUNDS) ? b->trace.as<uint32_t>() + 2 * i : nullptr;      // the first partition's rounds are traced
                dispatch<ARENA, true>(c, [&](auto t) {
                    hipLaunchKernelGGL((k_mcts_rollout<t.NL, t.W, t.PRESET>), dim3(pk.grid_roll), dim3(TAFL_BLOCK), 0, pk.s, t.CC, M, p->seed,
                                       sp.base, p->sim_offset, p->max_rollout_plies, pk.wl, wc_now, wc_next, pk.g1 - pk.g0, pk.cap, st, tr,
                                       k == 0 ? ctrl : nullptr, i, sp.planned, sp.probe_every); });
            }
        }
        stagger = false;
        sp.next_round = i + 1;
        if (!b->half_recorded && 2u * (i + 1u) >= sp.planned) {          // a search started "after" this one begins here (tafl_mcts_run_async_after)
            if (hipEventRecord(b->ev_half, sp.P[0].s) != hipSuccess) return fail(TAFL_ERR_HIP, "tafl_mcts: hipEventRecord failed");
            b->half_recorded = true;
        }
    }
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}
static int mcts_enqueue_fused(tafl_batch* b, uint32_t rounds) {
    tafl_ctx* c = b->ctx; SearchPlan& sp = b->plan; const tafl_mcts_params* p = &sp.p; const uint32_t n = b->n;
    unsigned long long* st = b->stats.as<unsigned long long>(); const MctsMem& M = sp.M; hipStream_t s0 = sp.P[0].s;
    SpanGuard sg(c, KC_MCTS_ROLLOUT, s0);
    // two slots: 32 games per wave and an undo log in LDS; one slot: 64 games per wave, nothing is predicted
    const bool two = sp.slots == 2;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(two ? (n + 31) / 32 : grid_of(n)), dim3(TAFL_BLOCK), two ? TAFL_UNDO_LDS_BYTES(TAFL_MCTS_UNDO_CAP_FUSED) : 0, s0, c->c2, M, p->c_puct, p->n_sims,
                           p->seed, sp.base, p->sim_offset, p->max_rollout_plies, rounds, st);
    };
    if (c->preset == PRESET_BRANDUBH7) { if (two) launch(k_mcts_fused<2, 7, PRESET_BRANDUBH7, 2>); else launch(k_mcts_fused<2, 7, PRESET_BRANDUBH7, 1>); }
    else { if (two) launch(k_mcts_fused<2, 7, PRESET_NONE, 2>); else launch(k_mcts_fused<2, 7, PRESET_NONE, 1>); }
    sp.next_round += rounds;
    return TAFL_OK;
}

// -- the steps of mcts_begin_enqueue, in the order it takes them --
static int search_check_args(const tafl_batch* b, const tafl_mcts_params* p, const tafl_batch* after) {
    if (!b || !p) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    if (p->flags & ~(uint32_t)TAFL_MCTS_FLAGS_KNOWN) return fail(TAFL_ERR_UNSUPPORTED, "tafl_mcts_params.flags: unknown bits set");
    if (p->n_sims == 0) return fail(TAFL_ERR_INVALID_ARG, "n_sims must be > 0");
    if (after && after->ctx->device != b->ctx->device) return fail(TAFL_ERR_INVALID_ARG, "tafl_mcts_run_async_after: the two batches live on different devices");
    return TAFL_OK;
}
// tuning fields of `flags` (results never depend on them): which pipeline, and the playout slots per game that were asked for (0: default)
static int search_check_tuning(const tafl_ctx* c, const tafl_mcts_params* p, uint32_t n_moves, bool* fused, uint32_t* slots) {
    const uint32_t pipe = TAFL_MCTS_TUNE_PIPELINE_OF(p->flags);
    *slots = TAFL_MCTS_TUNE_SLOTS_OF(p->flags);
    if (pipe > TAFL_MCTS_PIPELINE_TWO_KERNEL) return fail(TAFL_ERR_UNSUPPORTED, "tafl_mcts_params.flags: unknown pipeline");
    // default: the two-kernel pipeline; 7x7 boards have playouts so short (Brandubh: ~65 plies) that the per-round launches and the
    // exposed tree phase cost more than the fused kernel's two waves per SIMD (measured: 92 M vs 31 M sims/s on 7x7)
    // The fused kernel is built for 64-bit boards only (7x7): on wider boards its tree phase does not fit the register file beside the
    // playout loop (256 VGPRs and spills) and the two-kernel pipeline is faster anyway (13x13: 44.9 M vs 37.4 M sims/s).
    if (pipe == TAFL_MCTS_PIPELINE_FUSED && c->nl != 2) return fail(TAFL_ERR_UNSUPPORTED, "the fused pipeline exists for 64-bit boards (word_bits 64) only");
    if (n_moves && pipe == TAFL_MCTS_PIPELINE_FUSED) return fail(TAFL_ERR_UNSUPPORTED, "tafl_selfplay_run uses the two-kernel pipeline");
    *fused = !n_moves && (pipe == TAFL_MCTS_PIPELINE_FUSED || (pipe == TAFL_MCTS_PIPELINE_DEFAULT && c->nl == 2 && *slots <= 2));
    if (*fused && *slots == 0) *slots = 2;
    if (*fused && *slots > 2) return fail(TAFL_ERR_UNSUPPORTED, "the fused pipeline has 1 or 2 playout slots per game");
    return TAFL_OK;
}
// the playouts a round of the two-kernel pipeline may run (this search's share of what the device holds at once) and, where the caller
// left them open, the slots per game that fill it
static int search_capacity_and_slots(tafl_batch* b, const tafl_mcts_params* p, uint32_t* capacity, uint32_t* slots) {
    tafl_ctx* c = b->ctx;
    if (c->rollout_capacity == 0) {
        int blocks = 0; hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, c->device));
        dispatch<ARENA, true>(c, [&](auto t) { if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_mcts_rollout<t.NL, t.W, t.PRESET>, TAFL_BLOCK, 0) != hipSuccess) blocks = 0; });
        if (blocks < 1) blocks = 8;
        c->rollout_capacity = (uint32_t)blocks * (uint32_t)prop.multiProcessorCount * TAFL_BLOCK;
    }
    *capacity = c->rollout_capacity;
    // batches that are searched side by side (tafl_mcts_run_async) each take their share of the device: a round that fills its share
    // EXACTLY keeps every SIMD at the same number of waves - a few workgroups more and some SIMDs carry one wave more than the others,
    // and the whole round takes that wave's time (1 / 2 / 3 / 4 waves per SIMD: 1.0 / 1.5 / 2.0 / 2.55 ms per 512-ply round)
    if (TAFL_MCTS_TUNE_SHARE_OF(p->flags) > 1) { *capacity = *capacity / TAFL_MCTS_TUNE_SHARE_OF(p->flags) / TAFL_BLOCK * TAFL_BLOCK; if (*capacity < TAFL_BLOCK) *capacity = TAFL_BLOCK; }
    if (*slots == 0) {                                           // what fills the device exactly: 4 slots per game at 65 536 games on 11x11
        *slots = *capacity / b->n;
        if (*slots < 1) *slots = 1;
    }
    return TAFL_OK;
}
// The batch is cut into partitions (two by default) that run the same pipeline on their own streams, started one tree launch apart: the
// tree phase of a partition (latency- and divergence-bound, one wave per 64 games) then runs under the playouts of the others instead
// of on an idle device, and the partitions' rounds interleave instead of ending together.  Each partition may fill its share of the
// device.  Small batches stay in one piece.
static uint32_t search_part_count(uint32_t n, bool fused, uint32_t flags) {
    uint32_t parts = (!fused && n >= 8192u) ? 2u : 1u;             // measured at 65 536 games, S = 64: 1: 56.9, 2: 64.6, 3: 61.2, 4: 61.0, 8: 35.7 M sims/s
    if (!fused && TAFL_MCTS_TUNE_PARTS_OF(flags)) { parts = TAFL_MCTS_TUNE_PARTS_OF(flags); if (parts > TAFL_MCTS_MAX_PARTS) parts = TAFL_MCTS_MAX_PARTS; }
    if (parts > grid_of(n)) parts = grid_of(n);
    return parts;
}
// the partition table of a two-kernel search: whole waves of 64 games, the first (waves mod parts) partitions one wave larger; every
// partition gets its stream, its share of `capacity` and its piece of the work lists
static void search_partition(tafl_batch* b, uint32_t capacity) {
    SearchPlan& sp = b->plan; const uint32_t n = b->n, parts = sp.parts;
    uint32_t* wlist = b->work.as<uint32_t>(); uint32_t* wcount = b->work_count.as<uint32_t>();
    const uint32_t waves = grid_of(n), per = waves / parts, extra = waves % parts;
    uint32_t w0 = 0; size_t wl_off = 0;
    for (uint32_t k = 0; k < parts; ++k) {
        SearchPart& P = sp.P[k];
        const uint32_t wk = per + (k < extra ? 1u : 0u);
        P.g0 = w0 * TAFL_BLOCK; P.g1 = (w0 + wk) * TAFL_BLOCK < n ? (w0 + wk) * TAFL_BLOCK : n;
        w0 += wk;
        const uint32_t cnt = P.g1 - P.g0;
        P.cap = parts > 1 ? (uint32_t)((unsigned long long)capacity * cnt / n / TAFL_BLOCK * TAFL_BLOCK) : capacity;
        if (P.cap < TAFL_BLOCK) P.cap = TAFL_BLOCK;
        const unsigned long long most = (unsigned long long)cnt * sp.M.spec_k;
        P.grid_tree = grid_of(cnt);
        P.grid_roll = (uint32_t)(((most < P.cap ? most : P.cap) + TAFL_BLOCK - 1) / TAFL_BLOCK);
        P.s = b->sstream[k];
        P.wl = wlist + wl_off; wl_off += (size_t)cnt * sp.M.spec_k;
        P.wc = wcount + (size_t)k * 2 * TAFL_MCTS_MAX_SLOTS;              // two counter sets per partition: the playout launch of a round clears the next round's
    }
}
// Fused pipeline (k_mcts_fused): one wave owns 64 / K games for a whole chunk of rounds and leaves as soon as its games are done;
// n_sims + 1 rounds always suffice (every round completes at least one simulation of every live game)
static int search_enqueue_fused(tafl_batch* b) {
    SearchPlan& sp = b->plan; hipStream_t s0 = b->sstream[0];
    sp.P[0].s = s0; sp.planned = sp.p.n_sims + 1; sp.max_rounds = sp.p.n_sims + 1; sp.probe_every = 0;
    uint32_t left = sp.p.n_sims + 1, chunk_len = 8;
    while (left > 0) {
        const uint32_t rounds = chunk_len < left ? chunk_len : left;
        if (const int rc = mcts_enqueue_fused(b, rounds)) return rc;
        left -= rounds;
        if (chunk_len < 16) chunk_len *= 2;
        if (!b->half_recorded && 2u * sp.next_round >= sp.planned) { HIPCHK(hipEventRecord(b->ev_half, s0)); b->half_recorded = true; }
    }
    HIPCHK(hipGetLastError());
    sp.active = true;
    return TAFL_OK;
}
// Two-kernel pipeline.  The search is planned for ceil(n_sims / slots) rounds (+ slack, below); every game issues ceil(remaining / rounds left) slots, so
// games that lost a round to a misprediction catch up instead of trailing behind in nearly empty rounds.
static int search_enqueue_two_kernel(tafl_batch* b, uint32_t capacity, uint32_t n_moves) {
    SearchPlan& sp = b->plan; const tafl_mcts_params* p = &sp.p; const uint32_t n = b->n; hipStream_t s0 = b->sstream[0];
    // A long search gets one round of slack in eight: its rounds are then not quite full, so that a game that lost a round to a failed
    // prediction finds room for the extra playout that lets it catch up inside the plan (S = 256: 95.5 -> 98.3 M sims/s, S = 1000:
    // 73.2 -> 74.0 M; a short search loses more to the longer plan than it wins: S = 64 97.1 -> 91.9 M with 18 rounds instead of 16).
    const uint32_t tight = (p->n_sims + sp.slots - 1) / sp.slots;
    const uint32_t planned = tight + (tight >= 32u ? tight / 8u : 0u);
    search_partition(b, capacity);
    // every round runs min(capacity, requested) playouts, the pending leaf of every waiting game first (class 0): progress is guaranteed
    // a large batch always has stragglers that need a few rounds more than the plan (65 536 games: 5 - 6)
    const uint32_t tail_guess = n >= 32768u ? 6u : n >= 4096u ? 4u : n >= 512u ? 2u : 1u;
    const unsigned long long rounds_bound = ((unsigned long long)p->n_sims + 2 + tail_guess) * (1 + (unsigned long long)n / (capacity ? capacity : 1));
    sp.max_rounds = rounds_bound > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)rounds_bound;
    sp.planned = planned;
    // long searches: width control every 16 rounds (k_mcts_rollout)
    sp.probe_every = planned >= 64 ? 16u : 0u;
    sp.ctrl0[CT_WCAP] = sp.M.spec_k - 1u; sp.ctrl0[CT_LAST_ISSUED] = sp.ctrl0[CT_LAST_HITS] = 0ull; sp.ctrl0[CT_NEXT_CHECK] = sp.probe_every ? sp.probe_every : ~0ull;
    HIPCHK(hipMemcpyAsync(b->ctrl.p, sp.ctrl0, sizeof sp.ctrl0, hipMemcpyHostToDevice, s0));      // (the source lives in the batch until the search is joined)
    HIPCHK(hipMemsetAsync(b->trace.p, 0, 8 * TAFL_MCTS_TRACE_ROUNDS, s0));
    HIPCHK(hipMemsetAsync(b->work_count.p, 0, sizeof(uint32_t) * 2 * TAFL_MCTS_MAX_SLOTS * TAFL_MCTS_MAX_PARTS, s0));
    uint32_t first = planned + tail_guess;
    if (n_moves) {
        // a self-play run: n_moves searches per game, each game at its own pace (k_mcts_tree_selfplay); most games need planned + 0..1 rounds per search
        NEED(b->sp_moves_done, sizeof(uint32_t) * (size_t)n); NEED(b->sp_start_round, sizeof(uint32_t) * (size_t)n); NEED(b->sp_plays, sizeof(tafl_play) * (size_t)n * n_moves);
        b->sp_moves_done.bind(sp.selfplay.moves_done); b->sp_start_round.bind(sp.selfplay.start_round); b->sp_plays.bind(sp.selfplay.plays);
        HIPCHK(hipMemsetAsync(b->sp_moves_done.p, 0, sizeof(uint32_t) * (size_t)n, s0)); HIPCHK(hipMemsetAsync(b->sp_start_round.p, 0, sizeof(uint32_t) * (size_t)n, s0));
        HIPCHK(hipMemsetAsync(b->sp_plays.p, 0, sizeof(tafl_play) * (size_t)n * n_moves, s0));
        const unsigned long long all = (unsigned long long)sp.max_rounds * n_moves;
        sp.max_rounds = all > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)all;
        const unsigned long long want = (unsigned long long)(planned + 1u) * n_moves + tail_guess;
        first = want > sp.max_rounds ? sp.max_rounds : (uint32_t)want;
    }
    if (first > sp.max_rounds) first = sp.max_rounds;
    if (const int rc = mcts_enqueue_rounds(b, first, sp.parts > 1)) return rc;
    sp.active = true;
    return TAFL_OK;
}

static int mcts_begin_enqueue(tafl_batch* b, const tafl_mcts_params* p, uint64_t game_id_base, tafl_batch* after, uint32_t n_moves, const SelfPlayRec* rec) {
    int rc = search_check_args(b, p, after);
    if (rc != TAFL_OK) return rc;
    if ((rc = join_search(b)) != TAFL_OK) return rc;       // one search per batch at a time
    // TAFL_MCTS_FLAG_KEEP_TREE on a retained tree: the search continues it (a dropped tree: a fresh search)
    const bool keep = (p->flags & TAFL_MCTS_FLAG_KEEP_TREE) && b->tree_live && b->has_mem;
    if (keep) { if ((rc = mcts_keep_capacity(b, p->n_sims)) != TAFL_OK) return rc; }
    else if ((rc = mcts_reserve(b, p->n_sims, false)) != TAFL_OK) return rc;
    b->tree_live = false;
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    SearchPlan& sp = b->plan;
    sp.p = *p; sp.base = game_id_base; sp.next_round = 0; sp.fused = false;
    sp.recording = n_moves && rec; if (sp.recording) sp.rec = *rec;
    sp.selfplay.n_moves = n_moves; sp.selfplay.moves_done = nullptr; sp.selfplay.start_round = nullptr; sp.selfplay.plays = nullptr;
    MctsMem& M = sp.M; M = b->mem;
    M.node_cap = keep ? b->mem.node_cap : p->n_sims + 1; M.edge_cap = b->mem.edge_cap; M.flags = p->flags & TAFL_MCTS_FLAG_FPU_INF;
    bool fused = false; uint32_t slots = 0, capacity = 0;
    if ((rc = search_check_tuning(c, p, n_moves, &fused, &slots)) != TAFL_OK) return rc;
    if (!fused && (rc = search_capacity_and_slots(b, p, &capacity, &slots)) != TAFL_OK) return rc;
    if (slots > b->spec_k) slots = b->spec_k;
    sp.fused = fused; sp.slots = slots;
    sp.parts = search_part_count(n, fused, p->flags);
    if ((rc = search_streams(b, sp.parts)) != TAFL_OK) return rc;
    // the search starts behind everything enqueued on the context's stream so far (uploads, steps ...) and, if asked for, behind the first
    // half of another batch's search in flight
    HIPCHK(hipEventRecord(b->ev_start, c->stream));
    HIPCHK(hipStreamWaitEvent(b->sstream[0], b->ev_start, 0));
    if (after && after != b && after->plan.active && after->half_recorded) HIPCHK(hipStreamWaitEvent(b->sstream[0], after->ev_half, 0));
    b->half_recorded = false;
    hipStream_t s0 = b->sstream[0];
    HIPCHK(hipMemsetAsync(b->stats.p, 0, sizeof(unsigned long long) * ST_COUNT, s0));
    M.spec_k = fused ? slots : b->spec_k;
    dispatch<ARENA, false>(c, [&](auto t) {
        if (keep) hipLaunchKernelGGL((k_mcts_keep_init<t.NLS, t.WS, t.NL, t.W>), dim3(grid_of(n)), dim3(TAFL_BLOCK), 0, s0, t.CC, b->soa, M);
        else hipLaunchKernelGGL((k_mcts_init<t.NLS, t.WS, t.NL, t.W>), dim3(grid_of(n)), dim3(TAFL_BLOCK), 0, s0, t.CC, b->soa, M); });
    b->ran = false; b->trace_rounds = 0;
    return fused ? search_enqueue_fused(b) : search_enqueue_two_kernel(b, capacity, n_moves);
}

// the launches of a search that is not in flight (any more) must not outlive the call that gave it up: nobody would join them
static void search_streams_drain(tafl_batch* b) {
    for (uint32_t k = 0; k < b->n_sstreams; ++k) (void)hipStreamSynchronize(b->sstream[k]);
}
// A failing return of mcts_begin_enqueue leaves plan.active == false, whatever it had enqueued by then (the stats memset, the init kernel,
// the control block copy, rounds on every partition's stream): the streams are drained before the error is reported, so that no launch
// runs on while the caller frees, grows or rewrites what it reads.  (A failure BEFORE the join of an earlier search leaves that search
// in flight and active: it is joined like any other.)
int mcts_begin(tafl_batch* b, const tafl_mcts_params* p, uint64_t game_id_base, tafl_batch* after, uint32_t n_moves, const SelfPlayRec* rec) {
    const int rc = mcts_begin_enqueue(b, p, game_id_base, after, n_moves, rec);
    if (rc != TAFL_OK && b && !b->plan.active) search_streams_drain(b);
    return rc;
}
int selfplay_finish(tafl_batch* b, int rc, uint32_t n_moves, tafl_play* out_plays) {
    if (rc == TAFL_OK) rc = tafl_mcts_wait(b);
    b->ran = false;                                          // the trees belong to roots that have been played away from
    b->tree_live = false; b->g_tree_live = false; b->gsp_active = false;
    if (rc) return rc;
    if (out_plays) {
        COPY_OUT(out_plays, b->sp_plays.p, (size_t)b->n * n_moves, b->ctx->stream);
        HIPCHK(hipStreamSynchronize(b->ctx->stream));
    }
    return TAFL_OK;
}

// every reader of a search's results joins a search in flight first; non-zero = there is no finished search to read
static int search_done(tafl_batch* b) {
    if (b->plan.active && tafl_mcts_wait(b) != TAFL_OK) return 1;
    return b->ran ? 0 : 1;
}
// the counters of the last finished search / self-play run, for the two entry points that read them
static int search_stats_ready(tafl_batch* b) {
    if (b->plan.active && tafl_mcts_wait(b) != TAFL_OK) return TAFL_ERR_HIP;
    if (!b->stats_ok) return fail(TAFL_ERR_INVALID_ARG, "no MCTS run on this batch");
    HIPCHK(hipSetDevice(b->ctx->device));
    return TAFL_OK;
}

extern "C" {

int tafl_mcts_reserve(tafl_batch* b, uint32_t max_sims) { return mcts_reserve(b, max_sims, true); }
int tafl_mcts_run_async(tafl_batch* b, const tafl_mcts_params* p, uint64_t game_id_base) { return mcts_begin(b, p, game_id_base, nullptr); }
int tafl_mcts_run_async_after(tafl_batch* b, const tafl_mcts_params* p, uint64_t game_id_base, tafl_batch* other) { return mcts_begin(b, p, game_id_base, other); }

int tafl_mcts_wait(tafl_batch* b) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "null batch");
    SearchPlan& sp = b->plan;
    if (!sp.active) return b->ran ? TAFL_OK : fail(TAFL_ERR_INVALID_ARG, "tafl_mcts_wait: no search was started on this batch");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    sp.active = false;                                                      // whatever happens below, the plan is over
    for (;;) {
        for (uint32_t k = 0; k < sp.parts; ++k) HIPCHK(hipStreamSynchronize(sp.P[k].s));
        unsigned long long h[ST_COUNT];
        HIPCHK(hipMemcpyAsync(h, b->stats.p, sizeof h, hipMemcpyDeviceToHost, sp.P[0].s));
        HIPCHK(hipStreamSynchronize(sp.P[0].s));
        if (h[ST_DONE] >= (unsigned long long)n) break;                     // every game has consumed its last playout
        if (sp.fused) return fail(TAFL_ERR_HIP, "tafl_mcts_wait: the fused search ended with unfinished games");
        // stragglers: a few more rounds, then look again (a round of a nearly finished batch is a lone wave per partition)
        const int rc = mcts_enqueue_rounds(b, sp.planned >= 32 ? 4u : 2u, false);
        if (rc) { search_streams_drain(b); return rc; }
    }
    b->ran = true; b->stats_ok = true;
    b->tree_live = sp.selfplay.n_moves == 0;                                 // (a self-play run leaves no tree for the current states)
    return TAFL_OK;
}

int tafl_mcts_run(tafl_batch* b, const tafl_mcts_params* p, uint64_t game_id_base) {
    const int rc = mcts_begin(b, p, game_id_base, nullptr);
    return rc ? rc : tafl_mcts_wait(b);
}

// n_moves x { tafl_mcts_run with sim_offset + move * n_sims; tafl_mcts_play_best } for every game, without leaving the device and without a
// barrier between the moves: a game starts its next search as soon as its own is done (SelfPlay, tafl_ops.hpp)
int tafl_selfplay_run(tafl_batch* b, const tafl_mcts_params* p, uint32_t n_moves, uint64_t game_id_base, tafl_play* out_plays) {
    if (!b || !p || n_moves == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_run: bad argument");
    if (p->flags & TAFL_MCTS_FLAG_KEEP_TREE) return fail(TAFL_ERR_UNSUPPORTED, "tafl_selfplay_run: TAFL_MCTS_FLAG_KEEP_TREE is not supported (no re-root inside a self-play run)");
    if ((unsigned long long)n_moves * p->n_sims + p->sim_offset > 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_run: sim_offset + n_moves * n_sims exceeds 32 bits");
    return selfplay_finish(b, mcts_begin(b, p, game_id_base, nullptr, n_moves), n_moves, out_plays);
}

// measurement: playouts requested / run in every round of the last two-kernel search (0 rounds after a fused search)
int tafl_mcts_round_trace(tafl_batch* b, uint32_t* requested, uint32_t* run, uint32_t cap, uint32_t* n_rounds) {
    if (!b || !n_rounds) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    if (const int rc = search_stats_ready(b)) return rc;
    tafl_ctx* c = b->ctx;
    const uint32_t k = b->trace_rounds < TAFL_MCTS_TRACE_ROUNDS ? b->trace_rounds : TAFL_MCTS_TRACE_ROUNDS;
    std::vector<uint32_t> h((size_t)2 * (k ? k : 1));
    if (k) { COPY_OUT(h.data(), b->trace.p, 2 * (size_t)k, c->stream); HIPCHK(hipStreamSynchronize(c->stream)); }
    for (uint32_t i = 0; i < k && i < cap; ++i) { if (requested) requested[i] = h[2 * i]; if (run) run[i] = h[2 * i + 1]; }
    *n_rounds = k;
    return TAFL_OK;
}

int tafl_mcts_get_stats(tafl_batch* b, tafl_mcts_stats* out) {
    if (!b || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    if (const int rc = search_stats_ready(b)) return rc;
    tafl_ctx* c = b->ctx;
    unsigned long long h[ST_COUNT];
    HIPCHK(hipMemcpyAsync(h, b->stats.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof *out);
    out->sims = h[ST_SIMS]; out->rollouts = h[ST_ROLLOUTS]; out->rollout_plies = h[ST_PLIES]; out->tree_depth_sum = h[ST_DEPTH];
    out->children_scanned = h[ST_SCANNED]; out->terminal_hits = h[ST_TERMINAL]; out->faults = h[ST_FAULTS];
    out->spec_issued = h[ST_SPEC_ISSUED]; out->spec_hits = h[ST_SPEC_HITS];
    for (int i = 0; i < 16; ++i) out->reason_hist[i] = h[ST_REASON0 + i];
    return TAFL_OK;
}

int tafl_mcts_root_children(tafl_batch* b, tafl_root_child* out, uint32_t max_children, uint32_t* out_n) {
    if (!b || !out || !out_n || max_children == 0 || search_done(b)) return fail(TAFL_ERR_INVALID_ARG, "bad argument / no MCTS run");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->children, sizeof(tafl_root_child) * (size_t)n * max_children); NEED(b->children_n, sizeof(uint32_t) * n);
    HIPCHK(hipMemsetAsync(b->children.p, 0, sizeof(tafl_root_child) * (size_t)n * max_children, c->stream));
    dispatch<ARENA, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_mcts_root_children<t.NL, t.W>), c, n, t.CC, b->mem, b->children.as<tafl_root_child>(), max_children, b->children_n.as<uint32_t>()); });
    HIPCHK(hipGetLastError());
    COPY_OUT(out, b->children.p, (size_t)n * max_children, c->stream);
    COPY_OUT(out_n, b->children_n.p, n, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t g = 0; g < n; ++g) if (out_n[g] > max_children) return fail(TAFL_ERR_CAPACITY, "max_children too small for some game");
    return TAFL_OK;
}

int tafl_mcts_root_visits(tafl_batch* b, uint32_t* out) {
    if (!b || !out || search_done(b)) return fail(TAFL_ERR_INVALID_ARG, "bad argument / no MCTS run");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, as = tafl_action_size(c);
    HIPCHK(hipSetDevice(c->device));
    NEED(b->visits, sizeof(uint32_t) * (size_t)n * as);
    HIPCHK(hipMemsetAsync(b->visits.p, 0, sizeof(uint32_t) * (size_t)n * as, c->stream));
    dispatch<ARENA, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_mcts_root_visits<t.NL, t.W>), c, n, t.CC, b->mem, b->visits.as<uint32_t>(), as); });
    HIPCHK(hipGetLastError());
    COPY_OUT(out, b->visits.p, (size_t)n * as, c->stream);
    return sync_ok(c);
}

// probs of src/mcts.py:40-53 computed on the host from the device's root visit counts (float64, same op order)
int tafl_mcts_policy(tafl_batch* b, double temp, double* out) {
    if (!b || !out || search_done(b) || temp < 0) return fail(TAFL_ERR_INVALID_ARG, "bad argument / no MCTS run");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, as = tafl_action_size(c);
    std::vector<uint32_t> counts((size_t)n * as);
    int rc = tafl_mcts_root_visits(b, counts.data());
    if (rc) return rc;
    for (uint32_t g = 0; g < n; ++g) {
        const uint32_t* cg = counts.data() + (size_t)g * as; double* og = out + (size_t)g * as;
        if (temp == 0) {
            uint32_t best = 0, arg = 0;
            for (uint32_t a = 0; a < as; ++a) if (cg[a] > best) { best = cg[a]; arg = a; }
            for (uint32_t a = 0; a < as; ++a) og[a] = 0.0;
            og[arg] = 1.0;
        } else {
            const double ex = 1.0 / temp; double sum = 0.0;
            for (uint32_t a = 0; a < as; ++a) { og[a] = pow((double)cg[a], ex); sum += og[a]; }
            for (uint32_t a = 0; a < as; ++a) og[a] = og[a] / sum;
        }
    }
    return TAFL_OK;
}

int tafl_mcts_best_play(tafl_batch* b, tafl_play* out_plays, uint32_t* out_visits) {
    if (!b || !out_plays || search_done(b)) return fail(TAFL_ERR_INVALID_ARG, "bad argument / no MCTS run");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->best_plays, sizeof(tafl_play) * n); NEED(b->best_visits, sizeof(uint32_t) * n);
    dispatch<ARENA, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_mcts_best_play<t.NL, t.W>), c, n, t.CC, b->mem, b->best_plays.as<tafl_play>(), b->best_visits.as<uint32_t>()); });
    HIPCHK(hipGetLastError());
    COPY_OUT(out_plays, b->best_plays.p, n, c->stream);
    COPY_OUT(out_visits, b->best_visits.p, n, c->stream);
    return sync_ok(c);
}

int tafl_mcts_play_best(tafl_batch* b, tafl_play* out_plays, tafl_effects* out_effects) {
    if (!b || search_done(b)) return fail(TAFL_ERR_INVALID_ARG, "bad argument / no MCTS run");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    tafl_play* dplays; tafl_effects* deff;
    STAGED(dplays, b->best_plays, out_plays, n, 0);
    STAGED(deff, b->effects, out_effects, n, 0);
    dispatch<ARENA, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_mcts_play_best<t.NLS, t.WS, t.W>), c, n, batch_consts<t.NLS>(c), b->mem, b->soa, dplays, deff); });
    HIPCHK(hipGetLastError());
    COPY_OUT(out_plays, dplays, n, c->stream);
    COPY_OUT(out_effects, deff, n, c->stream);
    if (out_plays || out_effects) HIPCHK(hipStreamSynchronize(c->stream));
    b->ran = false;                                   // the tree belongs to the previous roots
    b->tree_live = false; b->g_tree_live = false; b->gsp_active = false;
    return TAFL_OK;
}

// play + re-root of the retained tree (tree_advance)
int tafl_mcts_advance(tafl_batch* b, const uint32_t* actions, tafl_play* out_plays, tafl_effects* out_effects) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "null batch");
    int rc = join_search(b);
    if (rc != TAFL_OK) return rc;
    b->gsp_active = false;
    const bool live = b->tree_live && b->has_mem;
    if (!actions && !live) return fail(TAFL_ERR_INVALID_ARG, "tafl_mcts_advance: actions == NULL needs a retained tree (run a search first)");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!b->has_mem && (rc = tafl_mcts_reserve(b, 1)) != TAFL_OK) return rc;
    return tree_advance(b, "tafl_mcts_advance", b->edges, b->edges_alt, b->idmap, b->mem.node_cap, actions, out_plays, out_effects,
        [&](const uint32_t* acts, uint32_t A, tafl_play* dplays, tafl_effects* deff, uint32_t* bad) {
            dispatch<ARENA, false>(c, [&](auto t) {
                LAUNCH_PER_GAME((k_mcts_advance<t.NLS, t.WS, t.NL, t.W>), c, b->n, batch_consts<t.NLS>(c), t.CC, b->mem, b->soa,
                                   b->edges_alt.as<Edge>(), b->idmap.as<uint32_t>(), acts, live ? 1 : 0, A, dplays, deff, bad); });
        },
        [&] { b->edges.bind(b->mem.edges); b->tree_live = true; b->ran = true; b->g_tree_live = false; });      // (the guided tree belongs to the states before the play)
}

int tafl_mcts_tree_nodes(tafl_batch* b, uint32_t* out) {
    if (!b || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    if (const int rc = join_search(b)) return rc;
    if (!b->tree_live) { memset(out, 0, sizeof(uint32_t) * b->n); return TAFL_OK; }
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    COPY_OUT(out, b->mem.node_top, b->n, c->stream);
    return sync_ok(c);
}

int tafl_mcts_policy_device_ex(tafl_batch* b, double temp, uint64_t tie_seed, uint64_t game_id_base, double* out, int out_is_device) {
    if (!b || !out || search_done(b)) return fail(TAFL_ERR_INVALID_ARG, "bad argument / no MCTS run");
    if (!(temp >= 0.0)) return fail(TAFL_ERR_INVALID_ARG, "temp must be >= 0");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, as = tafl_action_size(c); const size_t count = (size_t)n * as;
    HIPCHK(hipSetDevice(c->device));
    double* dst;
    STAGED(dst, b->policy, out, count, out_is_device);
    HIPCHK(hipMemsetAsync(dst, 0, sizeof(double) * count, c->stream));
    const double inv = temp == 0.0 ? 1.0 : 1.0 / temp;                  // 1. / temp of mcts.py:50
    dispatch<ARENA, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_mcts_policy<t.NL, t.W>), c, n, t.CC, b->mem, dst, as, temp == 0.0 ? 1 : 0, inv, tie_seed, game_id_base); });
    HIPCHK(hipGetLastError());
    if (!out_is_device) COPY_OUT(out, dst, count, c->stream);
    return sync_ok(c);
}
int tafl_mcts_policy_device(tafl_batch* b, double temp, double* out, int out_is_device) { return tafl_mcts_policy_device_ex(b, temp, 0, 0, out, out_is_device); }

}  // extern "C"
