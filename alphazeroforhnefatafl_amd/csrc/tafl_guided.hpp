// tafl_guided.hpp — MCTS with an external evaluator: src/mcts.py:55-136 where nnet.predict (mcts.py:85) is the CALLER's
// network, evaluated for all games of the batch at once between two kernel launches.
//
// One lock-step round per game:   [expand the pending leaf with the priors / value just delivered, back the value up]
//                                 -> [run searches from the root until one reaches a node that is not in Ps (a leaf that
//                                    needs predict) — searches that end in a terminal node are completed on the way]
// so that every launch leaves at most one leaf per game waiting for the network.  The arithmetic is mcts.py's, in float64
// and in its order of operations:
//   Ps[s] = Ps[s] * valids                  priors arrive as float32, `* valids` widens them to float64       mcts.py:87
//   sum_Ps_s = np.sum(Ps[s])                numpy's PAIRWISE summation over the dense action vector           mcts.py:88
//   Ps[s] /= sum   |  (Ps[s] + valids) / np.sum(..)  when every valid move was masked                      mcts.py:89-98
//   u = Qsa + cpuct*Ps*sqrt(Ns)/(1+Nsa)  |  cpuct*Ps*sqrt(Ns + EPS),  strict >, ascending action index      mcts.py:109-119
//   Qsa = (Nsa*Qsa + v)/(Nsa+1), Nsa += 1, Ns += 1, return -v                                             mcts.py:127-136
// The value is taken as a Python float (float(v)); the tree is explicit (no transposition table), as in the rollout mode.
//
// Storage differs from the rollout mode (tafl_ops.hpp): with non-uniform priors the visited children are no longer a prefix
// of the legal list, so a node owns one edge per LEGAL move, in canonical (= ascending action index) order.
//
// Dirichlet noise at the root (include/taflhip.h tafl_root_noise) is a tail of the root's expansion, compiled only into
// the NOISE instantiations (step / selfplay_step with a RootNoise argument); the functions without it are what they were.
//
// A guided self-play run records its examples and draws its plays with the functions of tafl_examples.hpp (example_append,
// visit_draw, which own the example layout and the board encoding); this file only walks the root's edge block for them.
//
// Evaluation under a random board symmetry (include/taflhip.h tafl_eval_symmetry) is compiled only into the SYM
// instantiations (the kernels of tafl_gmcts_sym.hip): where a leaf starts to wait its symmetry is drawn into GuidedMem::sym, and
// expand_as reads the prior of a legal move at the permuted index.  The functions without the flag are what they were.
//
// Exact win/loss proofs (MCTS-Solver: include/taflhip.h tafl_solver) are compiled only into the SOLVER
// instantiations (selfplay_step_solver).  A node's proof lives in bits 1-2 of GNode::expanded (a terminal's is its term code), the
// losing-move / winning-move mark of an edge in bits 2-3 of GEdge::dir, mirrored there through pedge when the child is proven, so the
// selection scan reads it from the record it loads anyway.  The functions without the flag are what they were.
#pragma once
#include "tafl_ops.hpp"

namespace tafl {

struct GNode {                   // 16 bytes
    uint32_t parent;             // node id of the parent (0 for the root)
    uint32_t edge_base;          // first edge of this node inside the game's edge arena
    uint32_t ns;                 // Ns[s]
    uint16_t n_legal;            // |Vs[s]|
    uint8_t  term;               // 0 not ended, 1 Es=+1, 2 Es=-1, 3 draw
    uint8_t  expanded;           // s in Ps
};
struct GEdge {                   // 32 bytes
    double p, q;                 // Ps[s][a], Qsa
    uint32_t n, child;           // Nsa (0 = (s,a) not in Qsa), node of the next state (0 = not created yet)
    uint32_t action;             // dense action index
    uint16_t from; uint8_t dir, dist;
};
struct GuidedMem {
    Quad* node_state;            // [(k * G + g) * QUADS]
    GNode* hdr;                  // [k * G + g]
    uint32_t* pedge;             // [k * G + g] index (inside the game's edge arena) of the edge parent -> this node
    GEdge* edges;                // [g * edge_cap + e]
    uint32_t* node_top;          // [G]
    uint32_t* edge_top;          // [G]
    uint32_t* leaf;              // [G] node waiting for predict()
    uint8_t* kind;               // [G] 0 nothing pending, 1 leaf waits for predict, 3 all simulations done
    uint8_t* fault;              // [G] arena overflow / no selectable action: the game stops searching
    uint32_t* sims_done;         // [G]
    uint32_t G, node_cap, edge_cap;
    // evaluation under a random board symmetry (include/taflhip.h tafl_eval_symmetry): read by the SYM
    // instantiations of the rounds alone, which run only when sym != nullptr; the leaves kernel and the getter test the pointer
    uint8_t* sym = nullptr;      // [G] the symmetry the leaf that waits is shown under: written where kind[g] becomes 1
    uint64_t sym_seed = 0, sym_gid = 0;   // the game id of game g is sym_gid + g
    uint32_t sym_n = 0;          // the board's side length (the close-and-reopen kernel has no Consts)
};
struct GuidedStats { uint32_t sims, predicts, terminal_hits, faults, depth; };
// per-run state of a guided self-play run (tafl_gselfplay_*)
constexpr uint32_t kGspStopped = 0x80000000u;    // GSelfPlay::moves_done: the game makes no further move in this run
constexpr uint32_t kGspEpisodeEnded = 0x40000000u;   // episodes run: the lane's episode is over or cut, k_gselfplay_reopen closes it and opens the next
enum { EP_ATTACKER = 0, EP_DEFENDER, EP_DRAW, EP_CUT, EP_COUNT };
struct GSelfPlay {
    uint32_t* moves_done;        // [G] moves made in this run | kGspStopped
    tafl_play* plays;            // [m * G + g] the play of move m (all-zero: not made)
    uint32_t n_moves;
};
// what an episodes run (tafl_gselfplay_begin_episodes) adds to it: an argument of the episodes kernels alone
struct GEpisodes {
    uint32_t episode_moves;      // an episode that has made this many moves and is still going is cut (0: no cap)
    uint32_t* episode;           // [G] k: episodes of the lane that are closed or cut = the number of the one that is open
    uint32_t* ep_start;          // [G] moves the lane had made when its open episode began
    const Quad* openings;        // quad-plane SoA [QUADS][G]: the position every episode of lane g begins from
    unsigned long long* ep_counters;   // [EP_COUNT]
    uint64_t id_stride;          // game id of episode k of lane g = game_id_base + k * id_stride + g
    uint32_t* open_from;         // [G] of the examples object (null: nothing is recorded): first example of the lane's open episode
};
// what a match run (tafl_gmatch_begin) adds to an episodes run: an argument of the match kernels alone
constexpr uint32_t kMatchNoRow = 0xFFFFFFFFu;    // GMatch::row_of: the lane has no row in either evaluator's batch
constexpr uint32_t kMatchRowMask = 0x7FFFFFFFu;  // otherwise evaluator << 31 | row
struct GMatch {
    uint32_t swap;               // 0 or 1: which evaluator takes the attackers in episode 0 of the lane with the even global number
    uint32_t* row_of;            // [G] where the evaluation of the lane's waiting leaf stands (tafl_gmatch_leaves writes it)
    unsigned long long* games;   // [2 * EP_COUNT]: games[a * EP_COUNT + r], episodes closed or cut with evaluator a as the attackers
};
// playout cap randomization (include/taflhip.h tafl_playout_cap): an argument of the capped rounds alone
enum { CAP_FULL = 0, CAP_FAST, CAP_COUNT };
struct PlayoutCap {
    uint64_t seed;
    uint32_t fast_sims;          // simulations of a fast move (a full one searches the run's n_sims)
    uint32_t full_per_65536;     // a move is full iff the high 16 bits of its class word are below this
    unsigned long long* counters;   // [CAP_COUNT] moves made per class
};
// the class of move M of game gid, a pure function of (seed, gid, M): the game key is that of selfplay_rand with kCapKey folded in, so for
// equal seeds the class stream differs from the sample stream and from the noise stream
constexpr uint64_t kCapKey = 0x504C41594F555443ull;
static TAFL_HD bool cap_is_full(const PlayoutCap& pc, uint64_t gid, uint32_t move_no) {
    using E = Engine<2, 7>;
    return (E::ply_rand(E::sim_key(E::game_key(pc.seed, gid) ^ kCapKey, move_no), 0u) >> 16) < pc.full_per_65536;
}
// forced playouts and policy target pruning (include/taflhip.h tafl_forced_playouts): an argument of the forced rounds alone
enum { FP_FORCED_SIMS = 0, FP_PRUNED_VISITS, FP_PRUNED_CHILDREN, FP_FULL_MOVES, FP_COUNT };
struct ForcedPlayouts {
    double k;                       // a visited root edge is forced while n * n < (k * p) * Ns
    unsigned long long* counters;   // [FP_COUNT]
};
// exact win/loss proofs (include/taflhip.h tafl_solver): an argument of the solver rounds alone
enum { SV_ROOT_WON = 0, SV_ROOT_LOST, SV_SKIPPED_SIMS, SV_NODES_WON, SV_NODES_LOST, SV_PRUNED_VISITS, SV_PRUNED_CHILDREN, SV_MOVES, SV_COUNT };
struct SolverCfg { unsigned long long* counters; };   // [SV_COUNT]
enum { PROOF_NONE = 0, PROOF_WON = 1, PROOF_LOST = 2 };          // for the side to move at the node; GNode::expanded = expanded | proof << 1
constexpr uint8_t kDirMask = 3u, kEdgeLosing = 4u, kEdgeWinning = 8u;   // GEdge::dir = dir | marks: the child is WON / the child is LOST
enum { SL_SKIPPED = 0, SL_NODES_WON, SL_NODES_LOST, SL_COUNT };  // what one lane counts during one call of step_as
// Dirichlet noise at the root (include/taflhip.h tafl_root_noise): what the search of one game mixes into Ps[root]
struct RootNoise {
    double alpha, epsilon;
    uint64_t seed, gid;          // gid = game_id_base + g
    uint32_t move_no;            // M
};
// the symmetry a leaf with the leaf key `h` (Engine::state_hash) is shown under in game gid: a pure function of (seed, gid, position)
constexpr uint64_t kSymKey = 0x53594D4D45545259ull;
static TAFL_HD uint32_t eval_symmetry_of(uint64_t seed, uint64_t gid, uint32_t h) {
    using E = Engine<2, 7>;
    return E::ply_rand(E::sim_key(E::game_key(seed, gid) ^ kSymKey, h), 0u) >> 29;
}
constexpr uint32_t kNoiseTries = 16;         // rejection rounds of one Gamma variate before its fallback
constexpr uint32_t kNoiseWordsPerTry = 5;    // uniform words one round consumes; the words of the boost follow at kNoiseTries * kNoiseWordsPerTry

// the uniform word `draw` of the noise stream of (seed, gid, M, action a): the taflmix32 family of tafl_core.hpp.  The game key is that of
// selfplay_rand with kNoiseKey folded in, so for equal seeds the two streams hang off different game keys; below it one simulation key per
// move number, one per action, and the draw index as the ply.
constexpr uint64_t kNoiseKey = 0x4449524943484C45ull;
static TAFL_HD uint32_t noise_word(uint32_t ak, uint32_t draw) { return Engine<2, 7>::ply_rand(ak, draw); }
static TAFL_HD uint32_t noise_action_key(const RootNoise& nz, uint32_t a) {
    using E = Engine<2, 7>;
    const uint32_t mk = E::sim_key(E::game_key(nz.seed, nz.gid) ^ kNoiseKey, nz.move_no);
    return E::sim_key((uint64_t)mk | ((uint64_t)E::fmix32(mk + 0x9E3779B9u) << 32), a);
}
// a uniform in (0, 1) with 53 random bits from two words: ((w0 >> 5) * 2^26 + (w1 >> 6) + 0.5) * 2^-53
static TAFL_HD double noise_uniform(uint32_t w0, uint32_t w1) { return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6) + 0.5) * (1.0 / 9007199254740992.0); }
// One Gamma(alpha, 1) variate, a pure function of (seed, gid, M, a).  Marsaglia & Tsang (2000) for shape k = alpha (alpha >= 1) or
// alpha + 1 (alpha < 1, then multiplied by U^(1/alpha)): d = k - 1/3, c = 1/sqrt(9 d); a round draws a normal x (Box-Muller: words 0-2)
// and a uniform u (words 3-4), v = (1 + c x)^3, and accepts d v when v > 0 and log u < x^2/2 + d - d v + d log v.  A round accepts with
// probability > 0.95 for every d >= 2/3; after kNoiseTries rounds without one the variate is d (v = 1): probability < 0.05^16 < 2e-21.
// For small alpha the boost exp(log U / alpha) underflows to 0 for most actions, which is a valid value.
static TAFL_HD double noise_gamma(const RootNoise& nz, uint32_t a) {
    const uint32_t ak = noise_action_key(nz, a);
    const bool boost = nz.alpha < 1.0;
    const double d = (boost ? nz.alpha + 1.0 : nz.alpha) - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = d;
    for (uint32_t t = 0; t < kNoiseTries; ++t) {
        const uint32_t w = t * kNoiseWordsPerTry;
        const double r = sqrt(-2.0 * log(noise_uniform(noise_word(ak, w), noise_word(ak, w + 1u))));
        const double x = r * cos(6.283185307179586 * (((double)noise_word(ak, w + 2u) + 0.5) * (1.0 / 4294967296.0)));
        const double u = noise_uniform(noise_word(ak, w + 3u), noise_word(ak, w + 4u));
        const double t1 = 1.0 + c * x, v = t1 * t1 * t1;
        if (v > 0.0 && log(u) < 0.5 * x * x + d - d * v + d * log(v)) { g = d * v; break; }
    }
    if (boost) {
        const uint32_t w = kNoiseTries * kNoiseWordsPerTry;
        g = g * exp(log(noise_uniform(noise_word(ak, w), noise_word(ak, w + 1u))) / nz.alpha);
    }
    return g;
}
// eta_i from gamma_i, the sequential sum s of the root's variates and the number n of its legal actions
static TAFL_HD double noise_eta(double gamma, double s, uint32_t n) { return (s > 0.0 && s < __builtin_inf()) ? gamma / s : 1.0 / (double)n; }

// The recorder of search statistics (tafl_examples.hpp ExampleStatsMem), for game g AFTER a self-play round of any family: if the round
// appended an example (len[g] has passed seen[g]; a round appends at most one, a move needs its root's evaluation) that holds a policy,
// Qsa and Ps of its stored children are read from the block of the root the move was made from.  That block still stands: init_game resets
// edge_top and writes no edge, the block begins at edge 0 of the game's arena (the root is the first node a search expands) and the next
// expansion needs an evaluation, hence a later round.  The stored actions ascend and each is in the block, so child k's edge is the next
// one with its action; the pruning rounds edit n in that block in place and leave q and p.  The walk never leaves the game's arena: it
// is bounded by edge_cap and not by the root's n_legal, which init_game has overwritten - an action that were not in the block (none is)
// would be looked for among the stale edges behind it and, not found, store zeros.
static TAFL_HD void record_stats(const GuidedMem& M, uint32_t g, const ExamplesMem& X, const ExampleStatsMem& S) {
    const uint32_t len = X.len[g] < X.max_moves ? X.len[g] : X.max_moves, seen = S.seen[g];
    if (len == seen) return;
    S.seen[g] = len;
    if (len < seen) return;                                      // (the object was cleared under the run)
    const uint32_t j = len - 1u, info = X.info[(size_t)j * X.G + g], nc = example_stored_children(X, info);
    const GEdge* eb = &M.edges[(size_t)g * M.edge_cap];
    uint32_t i = 0;
    for (uint32_t k = 0; k < nc; ++k) {
        const size_t at = ((size_t)j * X.K + k) * X.G + g;
        const uint32_t a = X.pol[at] & 0xFFFFu;
        while (i < M.edge_cap && eb[i].action != a) ++i;
        float q = 0.0f, p = 0.0f;
        if (i < M.edge_cap) { q = (float)eb[i].q; p = (float)eb[i].p; ++i; }
        S.cq[at] = q; S.cp[at] = p;
    }
}

template <int NL, int W>
struct Guided {
    using E = Engine<NL, W>;
    using O = Ops<NL, W>;
    using S = DState<NL>;
    using K = Consts<NL>;
    using IO = StateIO<NL>;

    // (writes no edge: record_stats above reads the block of the root a move was just made from AFTER this has run for the next root)
    static TAFL_HD void init_game(const GuidedMem& M, uint32_t g, const S& root) {
        GNode h; h.parent = 0; h.edge_base = 0; h.ns = 0; h.n_legal = 0; h.term = O::term_code(root); h.expanded = 0;
        M.hdr[g] = h; M.pedge[g] = 0;
        IO::store_rec(M.node_state + (size_t)g * IO::QUADS, root);
        M.node_top[g] = 1; M.edge_top[g] = 0; M.leaf[g] = 0; M.kind[g] = 0; M.fault[g] = 0; M.sims_done[g] = 0;
    }

    // SYM: the leaf `st` of game g starts to wait (kind[g] has just become 1): draw its symmetry
    static TAFL_HD void leaf_symmetry(const GuidedMem& M, uint32_t g, const S& st) {
        M.sym[g] = (uint8_t)eval_symmetry_of(M.sym_seed, M.sym_gid + g, E::state_hash(st, M.sym_n));
    }

    // np.sum over the dense action vector whose only non-zero entries are e[0..cnt) (ascending action index); `add1`
    // adds 1.0 to every entry first (the `Ps + valids` of mcts.py:97).  numpy: DOUBLE_pairwise_sum, blocks of <= 128
    // elements with 8 interleaved accumulators, halves split at a multiple of 8; adding the zeros in between is exact.
    static TAFL_HD double leaf_sum(const GEdge* e, uint32_t cnt, uint32_t& cur, uint32_t lo, uint32_t n, bool add1) {
        const uint32_t hi = lo + n;
        if (n < 8) {
            double res = 0.;
            while (cur < cnt && e[cur].action < hi) { res += add1 ? e[cur].p + 1.0 : e[cur].p; ++cur; }
            return res;
        }
        double r0 = 0., r1 = 0., r2 = 0., r3 = 0., r4 = 0., r5 = 0., r6 = 0., r7 = 0.;
        const uint32_t bulk = lo + (n - (n % 8u));
        while (cur < cnt && e[cur].action < bulk) {
            const double v = add1 ? e[cur].p + 1.0 : e[cur].p;
            const uint32_t j = (e[cur].action - lo) & 7u;
            r0 += j == 0 ? v : 0.; r1 += j == 1 ? v : 0.; r2 += j == 2 ? v : 0.; r3 += j == 3 ? v : 0.;
            r4 += j == 4 ? v : 0.; r5 += j == 5 ? v : 0.; r6 += j == 6 ? v : 0.; r7 += j == 7 ? v : 0.;
            ++cur;
        }
        double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        while (cur < cnt && e[cur].action < hi) { res += add1 ? e[cur].p + 1.0 : e[cur].p; ++cur; }
        return res;
    }
    static TAFL_HD double np_sum_sparse(const GEdge* e, uint32_t cnt, uint32_t A, bool add1) {
        struct Frame { uint32_t lo, n; uint32_t stage; double left; };
        // the recursion's frames: a per-lane stack indexed at run time.  In registers that is scratch memory (it was 400 of this kernel's
        // 496 B per lane); on the device it lives in LDS, one column per lane of the 64-thread workgroup
#if defined(__HIP_DEVICE_COMPILE__)
        __shared__ Frame stk_lds[16 * 64];
        Frame* const stk = stk_lds + (threadIdx.x & 63u);
        constexpr int SS = 64;
#else
        Frame stk_host[16]; Frame* const stk = stk_host;
        constexpr int SS = 1;
#endif
        int sp = 0; uint32_t cur = 0; double ret = 0.;
        stk[sp * SS].lo = 0; stk[sp * SS].n = A; stk[sp * SS].stage = 0; stk[sp * SS].left = 0.; ++sp;
        while (sp > 0) {
            Frame& f = stk[(sp - 1) * SS];
            if (f.n <= 128u) { ret = leaf_sum(e, cnt, cur, f.lo, f.n, add1); --sp; continue; }
            uint32_t n2 = f.n / 2u; n2 -= n2 % 8u;
            if (f.stage == 0) { f.stage = 1; Frame& c = stk[sp * SS]; c.lo = f.lo; c.n = n2; c.stage = 0; c.left = 0.; ++sp; }
            else if (f.stage == 1) { f.left = ret; f.stage = 2; Frame& c = stk[sp * SS]; c.lo = f.lo + n2; c.n = f.n - n2; c.stage = 0; c.left = 0.; ++sp; }
            else { ret = f.left + ret; --sp; }
        }
        return 0.0 + ret;                                       // np.add.reduce: identity + pairwise sum
    }

    // mcts.py:127-136 unwound iteratively from node `cur` (whose search returned v) to the root
    static TAFL_HD void backup(const GuidedMem& M, uint32_t g, uint32_t cur, double v) {
        while (cur != 0) {
            const uint32_t par = M.hdr[(size_t)cur * M.G + g].parent;
            GEdge* e = &M.edges[(size_t)g * M.edge_cap + M.pedge[(size_t)cur * M.G + g]];
            if (e->n > 0) { e->q = ((double)e->n * e->q + v) / (double)(e->n + 1); e->n += 1; }
            else { e->q = v; e->n = 1; }
            M.hdr[(size_t)par * M.G + g].ns += 1;
            v = -v;
            cur = par;
        }
    }

    // the solver rounds' backup (tafl_solver rule 3): the same walk, and behind every edge update the proof `cp` of the node just left
    // is mirrored into that edge and may prove the parent: WON by a LOST child, LOST once every legal move has a WON child
    static TAFL_HD void backup_solver(const GuidedMem& M, uint32_t g, uint32_t cur, double v, uint32_t cp, uint32_t* sl) {
        while (cur != 0) {
            const uint32_t par = M.hdr[(size_t)cur * M.G + g].parent;
            GEdge* e = &M.edges[(size_t)g * M.edge_cap + M.pedge[(size_t)cur * M.G + g]];
            if (e->n > 0) { e->q = ((double)e->n * e->q + v) / (double)(e->n + 1); e->n += 1; }
            else { e->q = v; e->n = 1; }
            GNode* ph = &M.hdr[(size_t)par * M.G + g];
            ph->ns += 1;
            if (cp != PROOF_NONE) {
                e->dir = (uint8_t)(e->dir | (cp == PROOF_WON ? kEdgeLosing : kEdgeWinning));
                uint32_t np = PROOF_NONE;
                if ((ph->expanded >> 1) == PROOF_NONE) {
                    if (cp == PROOF_LOST) np = PROOF_WON;
                    else {
                        const GEdge* pb = &M.edges[(size_t)g * M.edge_cap + ph->edge_base];
                        bool all = true;
                        for (uint32_t j = 0; j < ph->n_legal; ++j) all = all && (pb[j].dir & kEdgeLosing) != 0;
                        if (all) np = PROOF_LOST;
                    }
                    if (np != PROOF_NONE) {
                        ph->expanded = (uint8_t)(ph->expanded | (np << 1));
                        if (par != 0) sl[np == PROOF_WON ? SL_NODES_WON : SL_NODES_LOST] += 1u;
                    }
                }
                cp = np;
            }
            v = -v;
            cur = par;
        }
    }

    // mcts.py:83-102 for the pending leaf, with the network's answer
    static TAFL_HD bool expand(const GuidedMem& M, uint32_t g, const float* priors, uint32_t A, const K& C) { return expand_as<false>(M, g, priors, A, C, nullptr); }
    // NOISE: when the leaf is node 0, P' = (1 - epsilon) P + epsilon eta (tafl_root_noise): the raw variates wait in the fresh edges' q
    // between the two passes (mix == false: this search takes no noise - a fast move of a capped run)
    // SYM (the rounds of a search or run that latched tafl_eval_symmetry): the evaluator saw this leaf under symmetry s = sym[g], so the
    // prior of action a stands at sym_action(s, a) of its answer; the move is at hand as (from, dir, dist), which sym_move_action takes
    template <bool NOISE, bool SYM = false>
    static TAFL_HD bool expand_as(const GuidedMem& M, uint32_t g, const float* priors, uint32_t A, const K& C, const RootNoise* nz, bool mix = true) {
        const uint32_t L = M.leaf[g];
        S st; IO::load_rec(M.node_state + ((size_t)L * M.G + g) * IO::QUADS, st);
        const uint32_t base = M.edge_top[g];
        GEdge* e = &M.edges[(size_t)g * M.edge_cap + base];
        const uint32_t side = st.flags & TAFL_F_SIDE;
        [[maybe_unused]] uint32_t s = 0;
        if constexpr (SYM) s = M.sym[g];
        Move cur = E::canon_start();
        uint32_t cnt = 0;
        while (E::canon_next(st, side, C, cur)) {                 // getValidMoves, canonical = ascending action index
            if (base + cnt >= M.edge_cap) return false;
            const uint32_t a = O::action_of(cur, C);
            uint32_t pa = a;
            if constexpr (SYM) pa = sym_move_action(s, cur.from / (uint32_t)W, cur.from % (uint32_t)W, cur.dir, cur.dist, C.n);
            GEdge ne; ne.p = (double)priors[pa] * 1.0; ne.q = 0.0; ne.n = 0; ne.child = 0; ne.action = a;
            ne.from = (uint16_t)cur.from; ne.dir = (uint8_t)cur.dir; ne.dist = (uint8_t)cur.dist;
            e[cnt++] = ne;
        }
        const double sum = np_sum_sparse(e, cnt, A, false);
        if (sum > 0) { for (uint32_t i = 0; i < cnt; ++i) e[i].p /= sum; }
        else {
            const double s2 = np_sum_sparse(e, cnt, A, true);
            for (uint32_t i = 0; i < cnt; ++i) e[i].p = (e[i].p + 1.0) / s2;
        }
        if constexpr (NOISE) {
            if (L == 0 && mix) {
                double s = 0.0;
                for (uint32_t i = 0; i < cnt; ++i) { const double gm = noise_gamma(*nz, e[i].action); e[i].q = gm; s += gm; }
                const double keep = 1.0 - nz->epsilon;
                for (uint32_t i = 0; i < cnt; ++i) { e[i].p = keep * e[i].p + nz->epsilon * noise_eta(e[i].q, s, cnt); e[i].q = 0.0; }
            }
        }
        GNode* h = &M.hdr[(size_t)L * M.G + g];
        h->edge_base = base; h->n_legal = (uint16_t)cnt; h->ns = 0; h->expanded = 1;
        M.edge_top[g] = base + cnt;
        return true;
    }

    // One round for game g.  `priors` = this game's row of the network output (may be null when nothing is pending).
    static TAFL_HD void step(const GuidedMem& M, uint32_t g, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                             const K& C, GuidedStats& gs) { step_as<false>(M, g, priors, value, A, c_puct, n_sims, C, gs, nullptr); }
    // the round with the root noise `nz` of this game's search
    static TAFL_HD void step(const GuidedMem& M, uint32_t g, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                             const K& C, GuidedStats& gs, const RootNoise& nz) { step_as<true>(M, g, priors, value, A, c_puct, n_sims, C, gs, &nz); }
    // FORCED (the forced rounds, include/taflhip.h tafl_forced_playouts rule 1): in the search of a full move (`mix`) a visited edge of
    // node 0 with n * n < (k * p) * Ns scores +inf, so the first such edge is selected; *forced counts the simulations this happened to
    // SOLVER (the solver rounds, include/taflhip.h tafl_solver rules 1-5): terminals prove their parents, backup_solver carries the
    // proofs up, the scan of a node skips its losing moves, and a proven root ends the search; sl[SL_COUNT] counts for this lane.  The
    // forced-playouts argument is a run-time one there: k == 0 forces nothing
    // SYM: leaves are expanded through the permuted index (expand_as) and a leaf that starts to wait draws its symmetry
    template <bool NOISE, bool FORCED = false, bool SOLVER = false, bool SYM = false>
    static TAFL_HD void step_as(const GuidedMem& M, uint32_t g, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                const K& C, GuidedStats& gs, const RootNoise* nz, bool mix = true, const ForcedPlayouts* fp = nullptr, uint32_t* forced = nullptr,
                                uint32_t* sl = nullptr) {
        if (M.fault[g]) { M.kind[g] = 3; return; }
        uint32_t sims = M.sims_done[g];
        if (M.kind[g] == 1) {
            if (!priors || !expand_as<NOISE, SYM>(M, g, priors, A, C, nz, mix)) { M.fault[g] = 1; gs.faults += 1; M.kind[g] = 3; return; }
            gs.predicts += 1;
            if constexpr (SOLVER) backup_solver(M, g, M.leaf[g], -(double)value, PROOF_NONE, sl);
            else backup(M, g, M.leaf[g], -(double)value);         // return -v (mcts.py:102) into the callers
            ++sims; gs.sims += 1;
        }
        M.kind[g] = 3;
        while (sims < n_sims) {
            if constexpr (SOLVER) { if ((M.hdr[g].expanded >> 1) != PROOF_NONE) { sl[SL_SKIPPED] += n_sims - sims; sims = n_sims; break; } }   // rule 5
            uint32_t cur = 0; bool waiting = false;
            for (uint32_t depth = 0; depth <= M.node_cap; ++depth) {
                const GNode h = M.hdr[(size_t)cur * M.G + g];
                if (h.term) {                                                                              // mcts.py:79-81
                    if constexpr (SOLVER) backup_solver(M, g, cur, -O::term_value(h.term), h.term == 1 ? PROOF_WON : h.term == 2 ? PROOF_LOST : PROOF_NONE, sl);
                    else backup(M, g, cur, -O::term_value(h.term));
                    gs.terminal_hits += 1; break;
                }
                if (!(SOLVER ? h.expanded & 1 : h.expanded)) {                                                // mcts.py:83-85
                    M.leaf[g] = cur; M.kind[g] = 1; waiting = true;
                    if constexpr (SYM) { S ls; IO::load_rec(M.node_state + ((size_t)cur * M.G + g) * IO::QUADS, ls); leaf_symmetry(M, g, ls); }
                    break;
                }
                gs.depth += 1;
                GEdge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
                const double sq = sqrt((double)h.ns), sq0 = sqrt((double)h.ns + TAFL_MCTS_EPS);
                double cur_best = -__builtin_inf(); int best = -1;
                bool force = false; double kns = 0.0;
                if constexpr (FORCED) { force = mix && cur == 0u && (!SOLVER || fp->k > 0.0); kns = (double)h.ns; }
                // eight edge records in flight at a time (the scan is bound by memory latency), evaluated in ascending action order
                for (uint32_t j0 = 0; j0 < h.n_legal; j0 += 8) {
                    double ep[8], eq[8]; uint32_t en[8]; [[maybe_unused]] uint8_t ed[8];
                    TAFL_UNROLL for (uint32_t t = 0; t < 8; ++t) {
                        const GEdge* e = &eb[(j0 + t < h.n_legal) ? j0 + t : j0]; ep[t] = e->p; eq[t] = e->q; en[t] = e->n;
                        if constexpr (SOLVER) ed[t] = e->dir;
                    }
                    TAFL_UNROLL for (uint32_t t = 0; t < 8; ++t) {
                        double u = en[t] > 0 ? eq[t] + c_puct * ep[t] * sq / (double)(1 + en[t]) : c_puct * ep[t] * sq0;
                        if constexpr (FORCED) { if (force && en[t] > 0 && (double)en[t] * (double)en[t] < (fp->k * ep[t]) * kns) u = __builtin_inf(); }
                        bool open = j0 + t < h.n_legal;
                        if constexpr (SOLVER) open = open && (ed[t] & kEdgeLosing) == 0;          // rule 4: a losing move is not selected
                        if (open && u > cur_best) { cur_best = u; best = (int)(j0 + t); }
                    }
                }
                if (best < 0) { M.fault[g] = 1; gs.faults += 1; M.sims_done[g] = sims; return; }
                if constexpr (FORCED) { if (force && cur_best == __builtin_inf()) *forced += 1u; }
                uint32_t child = eb[best].child;
                if (child == 0) {                                     // getNextState (mcts.py:122-123): first visit of this edge
                    const uint32_t id = M.node_top[g];
                    if (id >= M.node_cap) { M.fault[g] = 1; gs.faults += 1; M.sims_done[g] = sims; return; }
                    S st; IO::load_rec(M.node_state + ((size_t)cur * M.G + g) * IO::QUADS, st);
                    Move mv; mv.from = eb[best].from; mv.dir = SOLVER ? eb[best].dir & kDirMask : eb[best].dir; mv.dist = eb[best].dist;
                    mv.to = (uint32_t)((int)mv.from + E::delta(mv.dir) * (int)mv.dist);
                    Moves<NL> nx;
                    E::apply(st, mv, C, nullptr, nx);
                    GNode nh; nh.parent = cur; nh.edge_base = 0; nh.ns = 0; nh.n_legal = 0; nh.term = O::term_code(st); nh.expanded = 0;
                    M.hdr[(size_t)id * M.G + g] = nh;
                    M.pedge[(size_t)id * M.G + g] = h.edge_base + (uint32_t)best;
                    IO::store_rec(M.node_state + ((size_t)id * M.G + g) * IO::QUADS, st);
                    M.node_top[g] = id + 1;
                    eb[best].child = id; child = id;
                }
                cur = child;
            }
            if (waiting) break;
            ++sims; gs.sims += 1;
        }
        M.sims_done[g] = sims;
    }

    // ---- subtree reuse (TAFL_GMCTS_KEEP_TREE) -------------------------------------------------------------
    // per-search fields of a retained tree (nodes, edges, priors and values stay)
    static TAFL_HD void keep_init(const GuidedMem& M, uint32_t g) { M.leaf[g] = 0; M.kind[g] = 0; M.fault[g] = 0; M.sims_done[g] = 0; }
    static constexpr uint32_t NO_NODE = 0xFFFFFFFFu;
    // Node c (a child of the root) becomes the root of game g, as Ops::mcts_reroot: ids are decided by one upward sweep (a parent's id is
    // lower than its children's), nodes move in place in ascending order, the edge blocks of the kept expanded nodes are written densely
    // into the second arena `dst`.  pedge is stored relative to the parent's block between the two passes (the parent's old edge_base is
    // gone once it has moved).
    static TAFL_HD void reroot(const GuidedMem& M, GEdge* dst, uint32_t* idmap, uint32_t g, uint32_t c) {
        const uint32_t top = M.node_top[g];
        idmap[(size_t)c * M.G + g] = 0;
        uint32_t cnt = 1;
        for (uint32_t k = c + 1; k < top; ++k) {
            const uint32_t p = M.hdr[(size_t)k * M.G + g].parent;
            const bool keep = p >= c && p < k && idmap[(size_t)p * M.G + g] != NO_NODE;
            idmap[(size_t)k * M.G + g] = keep ? cnt++ : NO_NODE;
            if (keep) M.pedge[(size_t)k * M.G + g] -= M.hdr[(size_t)p * M.G + g].edge_base;
        }
        uint32_t etop = 0;
        for (uint32_t k = c; k < top; ++k) {
            const uint32_t nk = idmap[(size_t)k * M.G + g];
            if (nk == NO_NODE) continue;
            GNode h = M.hdr[(size_t)k * M.G + g];
            const uint32_t rel = M.pedge[(size_t)k * M.G + g];
            uint32_t nbase = 0;
            if (h.expanded) {
                const GEdge* src = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
                GEdge* de = &dst[(size_t)g * M.edge_cap + etop];
                for (uint32_t j = 0; j < h.n_legal; ++j) {
                    GEdge e = src[j];
                    e.child = (e.child > k && e.child < top) ? idmap[(size_t)e.child * M.G + g] : 0u;
                    de[j] = e;
                }
                nbase = etop; etop += h.n_legal;
            }
            uint32_t pe = 0;
            if (k == c) h.parent = 0;
            else { h.parent = idmap[(size_t)h.parent * M.G + g]; pe = M.hdr[(size_t)h.parent * M.G + g].edge_base + rel; }   // (the parent has moved already)
            h.edge_base = nbase;
            M.hdr[(size_t)nk * M.G + g] = h;
            M.pedge[(size_t)nk * M.G + g] = pe;
            if (nk != k) {
                const Quad* s = M.node_state + ((size_t)k * M.G + g) * IO::QUADS;
                Quad* d = M.node_state + ((size_t)nk * M.G + g) * IO::QUADS;
                TAFL_UNROLL for (int q = 0; q < IO::QUADS; ++q) d[q] = s[q];
            }
        }
        M.node_top[g] = cnt; M.edge_top[g] = etop;
    }
    static TAFL_HD void keep_edges(const GuidedMem& M, GEdge* dst, uint32_t g) {
        const uint32_t n = M.edge_top[g];
        for (uint32_t j = 0; j < n; ++j) dst[(size_t)g * M.edge_cap + j] = M.edges[(size_t)g * M.edge_cap + j];
    }

    // the dense row eta that a search from `st` under `nz` mixes into its root priors: zero off the legal actions, all zero for a game
    // that is over; the variates wait in the row between the two passes
    static TAFL_HD void noise_row(const S& st, const K& C, const RootNoise& nz, double* row) {
        if (O::term_code(st)) return;
        const uint32_t side = st.flags & TAFL_F_SIDE;
        Move cur = E::canon_start();
        uint32_t cnt = 0; double s = 0.0;
        while (E::canon_next(st, side, C, cur)) { const uint32_t a = O::action_of(cur, C); const double gm = noise_gamma(nz, a); row[a] = gm; s += gm; ++cnt; }
        cur = E::canon_start();
        while (E::canon_next(st, side, C, cur)) { const uint32_t a = O::action_of(cur, C); row[a] = noise_eta(row[a], s, cnt); }
    }
    // the dense Ps[root] as the root's edges hold it (nothing is written for a root that is not expanded)
    static TAFL_HD void root_priors(const GuidedMem& M, uint32_t g, double* row) {
        const GNode h = M.hdr[g];
        if (!h.expanded) return;
        const GEdge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
        for (uint32_t j = 0; j < h.n_legal; ++j) row[eb[j].action] = eb[j].p;
    }

    // visited root edges in ascending action order (mcts.py:40-41)
    static TAFL_HD uint32_t root_children(const GuidedMem& M, uint32_t g, tafl_root_child* out, uint32_t max_children) {
        const GNode h = M.hdr[g];
        if (!h.expanded) return 0;
        const GEdge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
        uint32_t k = 0;
        for (uint32_t j = 0; j < h.n_legal; ++j) {
            const GEdge e = eb[j];
            if (e.n == 0) continue;
            if (k < max_children) {
                Move m; m.from = e.from; m.dir = e.dir; m.dist = e.dist; m.to = 0;
                tafl_root_child rc; rc.play = O::to_play(m); rc.action = e.action; rc.visits = e.n; rc.q = e.q;
                out[k] = rc;
            }
            ++k;
        }
        return k;
    }

    // ---- guided self-play at each game's own pace (tafl_gselfplay_*) -----------------------------------------
    // Policy target pruning (include/taflhip.h tafl_forced_playouts rule 2) of the finished root `h` of a full move, in place: every
    // visited edge but the first most visited one gives back up to F visits, one at a time, while its PUCT value with one visit fewer
    // stays below that of the most visited edge; an edge pruned to a single visit is pruned to none.  Counts what it took away.
    static TAFL_HD void forced_prune(GEdge* eb, const GNode& h, double c_puct, const ForcedPlayouts& fp) {
        uint32_t best = 0, b = 0;
        for (uint32_t j = 0; j < h.n_legal; ++j) { const uint32_t v = eb[j].n; if (v > best) { best = v; b = j; } }
        if (best == 0u) return;
        const double ns = (double)h.ns, sq = sqrt(ns);
        const double ustar = eb[b].q + c_puct * eb[b].p * sq / (double)(1 + eb[b].n);
        uint32_t visits = 0, children = 0;
        for (uint32_t j = 0; j < h.n_legal; ++j) {
            const uint32_t nj = eb[j].n;
            if (nj == 0u || j == b) continue;
            const double p = eb[j].p, q = eb[j].q, x = (fp.k * p) * ns;
            uint32_t F = (uint32_t)sqrt(x);                           // sqrt(x) rounded up, decided by the integer comparison
            while ((double)F * (double)F < x) ++F;
            while (F > 0u && (double)(F - 1u) * (double)(F - 1u) >= x) --F;
            uint32_t m = nj;
            for (uint32_t i = 0; i < F && m != 0u; ++i) {
                if (q + c_puct * p * sq / (double)(1 + (m - 1u)) < ustar) m -= 1u; else break;
            }
            if (m < nj && m <= 1u) m = 0u;
            if (m != nj) { eb[j].n = m; visits += nj - m; children += m == 0u; }
        }
        if (visits) TAFL_COUNT_ADD(&fp.counters[FP_PRUNED_VISITS], visits);
        if (children) TAFL_COUNT_ADD(&fp.counters[FP_PRUNED_CHILDREN], children);
    }
    // Solver pruning (include/taflhip.h tafl_solver rule 6) of the finished root `h`, in place: a WON root keeps the visits of its first
    // winning move alone; otherwise the losing moves give up theirs, provided a visited edge remains that is no losing move.  The marks
    // leave the block with it, so everything after reads plain dir and n' as it reads n.  Counts the proven roots and what it took away.
    static TAFL_HD void solver_prune(GEdge* eb, const GNode& h, const SolverCfg& sv) {
        const uint32_t proof = h.expanded >> 1;
        uint32_t visits = 0, children = 0;
        if (proof == PROOF_WON) {
            bool found = false;
            for (uint32_t j = 0; j < h.n_legal; ++j) {
                const uint32_t nj = eb[j].n;
                if (!found && (eb[j].dir & kEdgeWinning)) { found = true; continue; }
                if (nj != 0u) { eb[j].n = 0u; visits += nj; children += 1u; }
            }
        } else {
            bool other = false;
            for (uint32_t j = 0; j < h.n_legal; ++j) other = other || (!(eb[j].dir & kEdgeLosing) && eb[j].n != 0u);
            if (other)
                for (uint32_t j = 0; j < h.n_legal; ++j) {
                    const uint32_t nj = eb[j].n;
                    if ((eb[j].dir & kEdgeLosing) && nj != 0u) { eb[j].n = 0u; visits += nj; children += 1u; }
                }
        }
        for (uint32_t j = 0; j < h.n_legal; ++j) { const uint8_t d = eb[j].dir; if (d & ~kDirMask) eb[j].dir = (uint8_t)(d & kDirMask); }
        if (proof == PROOF_WON) TAFL_COUNT_ADD(&sv.counters[SV_ROOT_WON], 1);
        if (proof == PROOF_LOST) TAFL_COUNT_ADD(&sv.counters[SV_ROOT_LOST], 1);
        if (visits) TAFL_COUNT_ADD(&sv.counters[SV_PRUNED_VISITS], visits);
        if (children) TAFL_COUNT_ADD(&sv.counters[SV_PRUNED_CHILDREN], children);
    }
    // visit_draw (tafl_examples.hpp) over the root's edge block (one edge per LEGAL move, the unvisited ones in between): the index inside the block
    static TAFL_HD uint32_t selfplay_pick(const GEdge* eb, uint32_t n_legal, uint32_t N, uint32_t r) { return visit_draw(n_legal, N, r, [&](uint32_t j) { return eb[j].n; }); }
    // the start of a run for game g: a fresh root from its batch state; a game that is over makes no move
    static TAFL_HD void selfplay_init(const GuidedMem& M, uint32_t g, const S& root, const GSelfPlay& sp) {
        init_game(M, g, root);
        const bool over = TAFL_F_STATUS(root.flags) != TAFL_STATUS_ONGOING;
        if (over) M.kind[g] = 3;
        sp.moves_done[g] = over ? kGspStopped : 0u;
    }
    // One round of the run for game g: `step`; if that completes the game's search, the play of move M = move_base + moves made is chosen
    // (the most visited edge, first maximum, or for M < temp_moves the draw of selfplay_pick), its example is appended, the play is made on
    // the batch state `soa`, and - while the game goes on and has moves left - the next search begins from a fresh root, which waits for
    // its evaluation at once.  The state after the play is the record of the played edge's child, which `step` made with Engine::apply
    // (= do_valid_play) when the edge was first visited.  A game that faults, is over, has no visited root edge or has made n_moves moves stops.
    static TAFL_HD void selfplay_step(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                      const GSelfPlay& sp, const SelfPlayRec& rec, const K& C, GuidedStats& gs) {
        selfplay_step_as<false, false>(M, g, soa, priors, value, A, c_puct, n_sims, sp, rec, C, gs, nullptr, nullptr);
    }
    // the round with root noise: alpha, epsilon and seed of `nz`; gid and M are the run's (rec.game_id_base + g, rec.move_base + moves made)
    static TAFL_HD void selfplay_step(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                      const GSelfPlay& sp, const SelfPlayRec& rec, const K& C, GuidedStats& gs, const RootNoise& nz) {
        selfplay_step_as<true, false>(M, g, soa, priors, value, A, c_puct, n_sims, sp, rec, C, gs, &nz, nullptr);
    }
    // the round of an episodes run (tafl_gselfplay_begin_episodes), without and with root noise: gid and M are those of the lane's open
    // episode, and a game that ends (or an episode that reaches its cap) with budget left marks the lane kGspEpisodeEnded instead of
    // stopping it; selfplay_reopen does the rest
    static TAFL_HD void selfplay_step_episodes(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                               const GSelfPlay& sp, const GEpisodes& ep, const SelfPlayRec& rec, const K& C, GuidedStats& gs) {
        selfplay_step_as<false, true>(M, g, soa, priors, value, A, c_puct, n_sims, sp, rec, C, gs, nullptr, &ep);
    }
    static TAFL_HD void selfplay_step_episodes(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                               const GSelfPlay& sp, const GEpisodes& ep, const SelfPlayRec& rec, const K& C, GuidedStats& gs, const RootNoise& nz) {
        selfplay_step_as<true, true>(M, g, soa, priors, value, A, c_puct, n_sims, sp, rec, C, gs, &nz, &ep);
    }
    // CAP: the round of a capped run (include/taflhip.h tafl_playout_cap).  The class of the move whose search is open at entry keeps the
    // noise and the example to a full move and counts the move when it is made.  A fast move searches pc->fast_sims simulations: when its
    // root is about to be expanded (the search has done nothing yet) its sims_done starts at n_sims - fast_sims, so that `step` and the
    // test that the search is complete keep the run's uniform n_sims
    // FORCED: the round of a run with forced playouts (include/taflhip.h tafl_forced_playouts).  The search of a full move forces at
    // the root (step_as); when it is complete the visit counts of the root's edges are pruned in place (forced_prune: the block is dead
    // once the move is made), so the scan, the draw and the example below read n' as they read n
    // SOLVER: the round of a run with exact proofs (include/taflhip.h tafl_solver).  Every search, full or fast, proves what it can
    // (step_as); when it is complete solver_prune edits the root's visit counts in place, before forced_prune, and the rest reads n'.
    // Forced playouts are a run-time matter there (fp->k == 0: none)
    // SYM: every search of the run shows its leaves under their symmetries (step_as)
    template <bool NOISE, bool EPISODES, bool CAP = false, bool FORCED = false, bool SOLVER = false, bool SYM = false>
    static TAFL_HD void selfplay_step_as(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                         const GSelfPlay& sp, const SelfPlayRec& rec, const K& C, GuidedStats& gs, const RootNoise* nz, const GEpisodes* ep,
                                         const PlayoutCap* pc = nullptr, const ForcedPlayouts* fp = nullptr, const SolverCfg* sv = nullptr) {
        uint32_t md = sp.moves_done[g];
        if (md & kGspStopped) return;
        // EPISODES: the game id and the first move of the lane's open episode (rec.move_base is 0); they hold for the whole call, a new
        // episode begins in selfplay_reopen
        uint64_t gid = rec.game_id_base + g; uint32_t m0 = 0;
        if constexpr (EPISODES) {
            if (md & kGspEpisodeEnded) return;
            gid += (uint64_t)ep->episode[g] * ep->id_stride; m0 = ep->ep_start[g];
        }
        // (only the first pass of the loop below expands a leaf, so the move number of the search that is open now serves the whole call)
        RootNoise mine;
        if constexpr (NOISE) { mine = *nz; mine.gid = gid; mine.move_no = EPISODES ? md - m0 : rec.move_base + md; }
        // (CAP: likewise the class of that move; the second pass begins the next search with sims_done = 0 and ends at its unexpanded root)
        bool full = true;
        if constexpr (CAP) {
            full = cap_is_full(*pc, gid, EPISODES ? md - m0 : rec.move_base + md);
            if (!full && M.kind[g] == 1 && M.leaf[g] == 0u) M.sims_done[g] = n_sims - pc->fast_sims;      // (fast_sims <= n_sims: the begin checks it)
        }
        // (a loop so that `step` is inlined once: its second pass is the first round of the next search and ends at the unexpanded root;
        // record_stats depends on that: no expansion, hence no edge write, between a move and the end of the round.  Subtree reuse in a
        // run, or a search that expands before its evaluation, would have to record before it overwrites the block)
        for (;;) {
            if constexpr (SOLVER) {
                uint32_t forced = 0, sl[SL_COUNT] = {0u, 0u, 0u};
                step_as<NOISE, true, true, SYM>(M, g, priors, value, A, c_puct, n_sims, C, gs, NOISE ? &mine : nullptr, full, fp, &forced, sl);
                if (forced) TAFL_COUNT_ADD(&fp->counters[FP_FORCED_SIMS], forced);
                if (sl[SL_SKIPPED]) TAFL_COUNT_ADD(&sv->counters[SV_SKIPPED_SIMS], sl[SL_SKIPPED]);
                if (sl[SL_NODES_WON]) TAFL_COUNT_ADD(&sv->counters[SV_NODES_WON], sl[SL_NODES_WON]);
                if (sl[SL_NODES_LOST]) TAFL_COUNT_ADD(&sv->counters[SV_NODES_LOST], sl[SL_NODES_LOST]);
            } else if constexpr (FORCED) {
                uint32_t forced = 0;
                step_as<NOISE, true, false, SYM>(M, g, priors, value, A, c_puct, n_sims, C, gs, NOISE ? &mine : nullptr, full, fp, &forced);
                if (forced) TAFL_COUNT_ADD(&fp->counters[FP_FORCED_SIMS], forced);
            } else step_as<NOISE, false, false, SYM>(M, g, priors, value, A, c_puct, n_sims, C, gs, NOISE ? &mine : nullptr, full);
            if (M.fault[g]) { sp.moves_done[g] = md | kGspStopped; return; }
            if (M.kind[g] == 1 || M.sims_done[g] < n_sims) return;           // its search goes on
            const GNode h = M.hdr[g];
            if constexpr (SOLVER) { if (h.expanded) solver_prune(&M.edges[(size_t)g * M.edge_cap + h.edge_base], h, *sv); }
            if constexpr (FORCED) { if (full && h.expanded && (!SOLVER || fp->k > 0.0)) forced_prune(&M.edges[(size_t)g * M.edge_cap + h.edge_base], h, c_puct, *fp); }
            const GEdge* eb = &M.edges[(size_t)g * M.edge_cap + h.edge_base];
            uint32_t best = 0, pick = 0, total = 0, m = 0;
            if (h.expanded)
                for (uint32_t j = 0; j < h.n_legal; ++j) {
                    const uint32_t v = eb[j].n;
                    if (v > best) { best = v; pick = j; }
                    total += v; m += v != 0u;
                }
            if (m == 0) { sp.moves_done[g] = md | kGspStopped; return; }   // (n_sims == 1: the root was evaluated, no edge visited)
            const uint32_t move_no = EPISODES ? md - m0 : rec.move_base + md;
            if (move_no < rec.temp_moves) pick = selfplay_pick(eb, h.n_legal, total, selfplay_rand(rec.sample_seed, gid, move_no));
            const GEdge pe = eb[pick];
            S st;
            if (rec.ex.len && full) {                                        // (tafl_examples.hpp; a guided edge carries its action, unvisited edges lie in between)
                IO::load_soa(soa, M.G, g, st);
                example_append<NL, W>(rec.ex, g, st, C.n, m, pe.action, move_no, [&](auto&& put) {
                    for (uint32_t i = 0; i < h.n_legal; ++i) if (eb[i].n != 0u) put(eb[i].action, eb[i].n);
                });
            }
            IO::load_rec(M.node_state + ((size_t)pe.child * M.G + g) * IO::QUADS, st);
            IO::store_soa(soa, M.G, g, st);
            Move mv; mv.from = pe.from; mv.dir = pe.dir; mv.dist = pe.dist; mv.to = 0;
            sp.plays[(size_t)md * M.G + g] = O::to_play(mv);
            if constexpr (CAP) TAFL_COUNT_ADD(&pc->counters[full ? CAP_FULL : CAP_FAST], 1);
            if constexpr (FORCED) { if (full && (!SOLVER || fp->k > 0.0)) TAFL_COUNT_ADD(&fp->counters[FP_FULL_MOVES], 1); }
            if constexpr (SOLVER) TAFL_COUNT_ADD(&sv->counters[SV_MOVES], 1);
            md += 1u;
            if constexpr (EPISODES) {
                if (md >= sp.n_moves) { sp.moves_done[g] = md | kGspStopped; return; }      // the budget is used up: the episode stays open
                if (TAFL_F_STATUS(st.flags) != TAFL_STATUS_ONGOING || (ep->episode_moves != 0u && md - m0 >= ep->episode_moves)) { sp.moves_done[g] = md | kGspEpisodeEnded; return; }
            } else if (md >= sp.n_moves || TAFL_F_STATUS(st.flags) != TAFL_STATUS_ONGOING) { sp.moves_done[g] = md | kGspStopped; return; }
            sp.moves_done[g] = md;
            init_game(M, g, st);
            priors = nullptr;
        }
    }
    // the capped rounds (tafl_gselfplay_set_playout_cap): plain or episodes, without or with root noise
    template <bool NOISE, bool EPISODES>
    static TAFL_HD void selfplay_step_capped(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                             const GSelfPlay& sp, const GEpisodes& ep, const SelfPlayRec& rec, const K& C, GuidedStats& gs, const RootNoise& nz, const PlayoutCap& pc) {
        selfplay_step_as<NOISE, EPISODES, true>(M, g, soa, priors, value, A, c_puct, n_sims, sp, rec, C, gs, NOISE ? &nz : nullptr, EPISODES ? &ep : nullptr, &pc);
    }
    // the forced rounds (tafl_gselfplay_set_forced_playouts): always through the capped path - a run without a cap passes "every move full"
    template <bool NOISE, bool EPISODES>
    static TAFL_HD void selfplay_step_forced(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                             const GSelfPlay& sp, const GEpisodes& ep, const SelfPlayRec& rec, const K& C, GuidedStats& gs, const RootNoise& nz, const PlayoutCap& pc,
                                             const ForcedPlayouts& fp) {
        selfplay_step_as<NOISE, EPISODES, true, true>(M, g, soa, priors, value, A, c_puct, n_sims, sp, rec, C, gs, NOISE ? &nz : nullptr, EPISODES ? &ep : nullptr, &pc, &fp);
    }
    // the solver rounds (tafl_gselfplay_set_solver): through the capped path as the forced rounds are, with the cap and the forced
    // playouts of the run at run time - "every move full" without a cap, k == 0 without forced playouts
    template <bool NOISE, bool EPISODES>
    static TAFL_HD void selfplay_step_solver(const GuidedMem& M, uint32_t g, Quad* soa, const float* priors, float value, uint32_t A, double c_puct, uint32_t n_sims,
                                             const GSelfPlay& sp, const GEpisodes& ep, const SelfPlayRec& rec, const K& C, GuidedStats& gs, const RootNoise& nz, const PlayoutCap& pc,
                                             const ForcedPlayouts& fp, const SolverCfg& sv) {
        selfplay_step_as<NOISE, EPISODES, true, true, true>(M, g, soa, priors, value, A, c_puct, n_sims, sp, rec, C, gs, NOISE ? &nz : nullptr, EPISODES ? &ep : nullptr, &pc, &fp, &sv);
    }
    // a fresh root that waits for its evaluation: what `step` leaves when it meets the unexpanded root of an ongoing game
    template <bool SYM = false>
    static TAFL_HD void root_waits(const GuidedMem& M, uint32_t g, const S& root) {
        init_game(M, g, root); M.kind[g] = 1;
        if constexpr (SYM) leaf_symmetry(M, g, root);
    }
    // Close and reopen (include/taflhip.h tafl_gselfplay_begin_episodes) for a lane that selfplay_step_episodes marked kGspEpisodeEnded: the
    // examples of the episode get their result when its game is over (examples_settle; a cut episode keeps z = 0, final = 0), the
    // result counters and the lane's episode number go up, the batch state becomes the opening and the new episode's root waits.  A
    // lane whose opening is over stops.  Returns true when a root now waits.
    template <bool SYM = false>
    static TAFL_HD bool selfplay_reopen(const GuidedMem& M, uint32_t g, Quad* soa, const GSelfPlay& sp, const GEpisodes& ep, const SelfPlayRec& rec) {
        const uint32_t md = sp.moves_done[g];
        if (!(md & kGspEpisodeEnded) || (md & kGspStopped)) return false;
        const uint32_t moves = md & ~kGspEpisodeEnded;
        S st; IO::load_soa(soa, M.G, g, st);
        const uint32_t status = TAFL_F_STATUS(st.flags);
        if (rec.ex.len) {
            if (status != TAFL_STATUS_ONGOING) examples_settle(rec.ex, g, ep.open_from[g], st.flags);
            ep.open_from[g] = rec.ex.len[g];
        }
        const uint32_t what = status == TAFL_STATUS_ONGOING ? (uint32_t)EP_CUT : status == TAFL_STATUS_DRAW ? (uint32_t)EP_DRAW : TAFL_F_WINNER(st.flags) != 0u ? (uint32_t)EP_DEFENDER : (uint32_t)EP_ATTACKER;
        TAFL_COUNT_ADD(&ep.ep_counters[what], 1);
        ep.episode[g] += 1u;
        IO::load_soa(ep.openings, M.G, g, st);
        if (TAFL_F_STATUS(st.flags) != TAFL_STATUS_ONGOING) { sp.moves_done[g] = moves | kGspStopped; return false; }
        IO::store_soa(soa, M.G, g, st);
        root_waits<SYM>(M, g, st);
        ep.ep_start[g] = moves; sp.moves_done[g] = moves;
        return true;
    }

    // ---- match play: two evaluators in an episodes run (tafl_gmatch_*) ---------------------------------------
    // the flags word of lane g's batch state alone (the last word of the last quad plane)
    static TAFL_HD uint32_t batch_flags(const Quad* soa, uint32_t G, uint32_t g) { return soa[(size_t)(IO::QUADS - 1) * G + g].w; }
    // the evaluator that plays the attackers in episode k of the lane with the global number game_id_base + g
    static TAFL_HD uint32_t match_seat(uint64_t game_id_base, uint32_t g, uint32_t k, uint32_t swap) { return (uint32_t)((game_id_base + g + k + swap) & 1u); }
    // the evaluator of every leaf of the lane's current search: the one that owns the side to move at the search's root, which is the
    // lane's batch state (`flags` is its flags word)
    static TAFL_HD uint32_t match_owner(uint64_t game_id_base, uint32_t g, uint32_t k, uint32_t swap, uint32_t flags) {
        return (match_seat(game_id_base, g, k, swap) + ((flags & TAFL_F_SIDE) ? 1u : 0u)) & 1u;
    }
    // between the round and selfplay_reopen: a lane whose episode the round closed or cut counts it for the evaluator that played the
    // attackers, the result read from the batch state as selfplay_reopen reads it (ep.episode[g] is still the number of that episode)
    static TAFL_HD void match_tally(const GuidedMem& M, uint32_t g, const Quad* soa, const GSelfPlay& sp, const GEpisodes& ep, const SelfPlayRec& rec, const GMatch& mt) {
        const uint32_t md = sp.moves_done[g];
        if (!(md & kGspEpisodeEnded) || (md & kGspStopped)) return;
        const uint32_t flags = batch_flags(soa, M.G, g), status = TAFL_F_STATUS(flags);
        const uint32_t what = status == TAFL_STATUS_ONGOING ? (uint32_t)EP_CUT : status == TAFL_STATUS_DRAW ? (uint32_t)EP_DRAW : TAFL_F_WINNER(flags) != 0u ? (uint32_t)EP_DEFENDER : (uint32_t)EP_ATTACKER;
        TAFL_COUNT_ADD(&mt.games[match_seat(rec.game_id_base, g, ep.episode[g], mt.swap) * EP_COUNT + what], 1);
    }
};

}  // namespace tafl
