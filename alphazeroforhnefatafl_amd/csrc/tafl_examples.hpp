// tafl_examples.hpp — training examples recorded by a self-play run (tafl_selfplay_record and tafl_gselfplay_*, DESIGN.md sections 12-13):
// the device-resident buffer, the result of an example and the eight symmetries of the square on tiles and dense actions.  Two decisions
// that both search modes and the network-input kernels share are made here and nowhere else:
//   board_value     the board_to_matrix encoding of a tile (k_encode_boards, k_gmcts_leaves and example_append call it)
//   example_append  the layout of a recorded example; Ops (tafl_ops.hpp) and Guided (tafl_guided.hpp) only enumerate their root children
// and so is the draw of a play in proportion to the visit counts (visit_draw).  __host__ __device__ like everything in tafl_ops.hpp: the
// kernels run these functions one game (or one example, or one tile) per lane, tests/hostsim runs the same code on the CPU.
#pragma once
#include <math.h>
#include "tafl_core.hpp"

#define TAFL_DRAW_VALUE 1e-4     /* getGameEnded draw convention, DESIGN.md: the value of a drawn terminal in the search and z of a drawn game */

namespace tafl {

#if defined(__HIP_DEVICE_COMPILE__)
#define TAFL_COUNT_ADD(p, v) atomicAdd((p), (unsigned long long)(v))
#else
#define TAFL_COUNT_ADD(p, v) (*(p) += (v))
#endif

// Example (j, g) - the j-th example of game g - has index e = j * G + g in every per-example array (a wave's stores are contiguous).
enum { EX_DROPPED = 0, EX_OVERFLOWED = 1, EX_BAD_INDEX = 2, EX_COUNTERS = 4 };
constexpr uint32_t kExOverflow = 1u << 24;       // ExamplesMem::info: the root had more than K visited children, none is stored
struct ExamplesMem {
    uint32_t* len;               // [G] examples of game g
    uint32_t* boards;            // [(j * BW + w) * G + g] board_to_matrix bytes of the position before the play, four tiles per word (tile t: byte t & 3 of word t >> 2)
    uint32_t* info;              // [e] n_children | side to move (TAFL_ATTACKER / TAFL_DEFENDER) << 16 | kExOverflow
    uint32_t* played;            // [e] dense action index of the play made | N = sum of the stored Nsa << 16
    uint32_t* move_no;           // [e] number of the move in the episode (move_base + move inside the run)
    uint32_t* pol;               // [(j * K + k) * G + g] k-th visited root child in canonical order: action | Nsa << 16
    float* z;                    // [e] result seen from the example's side to move (tafl_examples_finalize)
    uint8_t* fin;                // [e] 1: z is final
    unsigned long long* counters;   // [EX_COUNTERS]
    uint32_t G, max_moves, K, BW;
};
// Search statistics per stored child (include/taflhip.h TAFL_EXAMPLES_SEARCH_STATS), of an object created with the
// flag.  A struct of its own and not a part of ExamplesMem: the self-play rounds take ExamplesMem by value and stay what they were; only
// the recorder kernel that runs after a guided round (Guided::record_stats) and the readers below take this one.
struct ExampleStatsMem {
    float* cq;                   // [(j * K + k) * G + g] Qsa of the k-th stored child, laid out like pol
    float* cp;                   // [(j * K + k) * G + g] Ps of the k-th stored child as the root's edges held it
    uint32_t* seen;              // [G] examples of game g the recorder has dealt with (a run sets it to len at its begin)
};
// what a recording run adds to SelfPlay: ex.len == nullptr records nothing (the plays are still drawn)
struct SelfPlayRec {
    ExamplesMem ex;
    uint64_t sample_seed, game_id_base;
    uint32_t temp_moves, move_base;
};

// board_to_matrix (game/main.rs:55-83) of tile (r, c) of an n x n board: corner 20, throne 30, + 1 for a piece, + 5 for the king.  `att` /
// `def`: the tile holds an attacker / a defender (the king is a defender); flags: the state's flags word (it names the king's tile).
static TAFL_HD uint32_t board_value(bool att, bool def, uint32_t r, uint32_t c, uint32_t n, uint32_t flags) {
    uint32_t v = 0;
    if ((r == 0 || r == n - 1u) && (c == 0 || c == n - 1u)) v = 20;
    if (r == n / 2u && c == n / 2u) v = 30;
    if (def) v += (r == TAFL_F_KROW(flags) && c == TAFL_F_KCOL(flags)) ? 5u : 1u; else if (att) v += 1u;
    return v;
}

// Appends the example of the move game g is about to make from `st` (W columns per row): m visited root children, `played` = dense action
// of the play.  each(put) calls put(action, Nsa) for every visited root child in canonical order; it is called only if the children fit
// in K (otherwise the example is marked kExOverflow and stores none).
template <int NL, int W, class Each>
static TAFL_HD void example_append(const ExamplesMem& X, uint32_t g, const DState<NL>& st, uint32_t n, uint32_t m, uint32_t played, uint32_t move_no, Each&& each) {
    const uint32_t j = X.len[g];
    if (j >= X.max_moves) { TAFL_COUNT_ADD(&X.counters[EX_DROPPED], 1); return; }
    const size_t e = (size_t)j * X.G + g;
    uint32_t w = 0, t = 0;
    for (uint32_t r = 0; r < n; ++r)
        for (uint32_t c = 0; c < n; ++c) {
            const uint32_t bit = r * (uint32_t)W + c;
            w |= board_value(test(st.att, bit), test(st.def, bit), r, c, n, st.flags) << (8u * (t & 3u));
            if ((t & 3u) == 3u) { X.boards[((size_t)j * X.BW + (t >> 2)) * X.G + g] = w; w = 0; }
            ++t;
        }
    if (t & 3u) X.boards[((size_t)j * X.BW + (t >> 2)) * X.G + g] = w;
    const bool over = m > X.K;
    uint32_t total = 0, k = 0;
    if (over) TAFL_COUNT_ADD(&X.counters[EX_OVERFLOWED], 1);
    else each([&](uint32_t a, uint32_t v) { X.pol[((size_t)j * X.K + k) * X.G + g] = a | (v << 16); total += v; ++k; });
    X.info[e] = (over ? kExOverflow : m) | (((st.flags & TAFL_F_SIDE) ? (uint32_t)TAFL_DEFENDER : (uint32_t)TAFL_ATTACKER) << 16);
    X.played[e] = played | (total << 16); X.move_no[e] = move_no; X.z[e] = 0.0f; X.fin[e] = 0;
    X.len[g] = j + 1u;
}

// The two scalars a training row derives from its stored children (include/taflhip.h "search value and policy surprise"; the text there
// is normative).  Both are 0 for an example without a stored policy (overflowed, or no children).
//   value     N = sum Nsa; acc = 0; for k ascending: acc = acc + (double)Nsa_k * (double)cq_k; value = (float)(acc / (double)N)
//   surprise  pi_k = (double)Nsa_k / (double)N; s = sum_k pi_k * (log(pi_k) - log(max((double)cp_k, 2^-126))), ascending, in double;
//             surprise = (float)max(s, 0.0): KL(pi || P) over the stored children
// `info` is the example's info word.  No FMA contraction on either build, so value is the same bits on the host and on the device.
static TAFL_HD uint32_t example_stored_children(const ExamplesMem& X, uint32_t info) {
    const uint32_t nc = (info & kExOverflow) ? 0u : (info & 0xFFFFu);
    return nc <= X.K ? nc : 0u;
}
static TAFL_HD void example_search_stats(const ExamplesMem& X, const ExampleStatsMem& S, uint32_t j, uint32_t g, uint32_t info, float& value, float& surprise) {
    const uint32_t nc = example_stored_children(X, info);
    value = 0.0f; surprise = 0.0f;
    uint32_t N = 0;
    for (uint32_t k = 0; k < nc; ++k) N += X.pol[((size_t)j * X.K + k) * X.G + g] >> 16;
    if (N == 0u) return;
    double acc = 0.0, s = 0.0;
    for (uint32_t k = 0; k < nc; ++k) {
        const size_t at = ((size_t)j * X.K + k) * X.G + g;
        const double v = (double)(X.pol[at] >> 16), pi = v / (double)N, pr = (double)S.cp[at];
        acc = acc + v * (double)S.cq[at];
        s = s + pi * (log(pi) - log(pr > 0x1p-126 ? pr : 0x1p-126));
    }
    value = (float)(acc / (double)N);
    surprise = (float)(s > 0.0 ? s : 0.0);
}

// ---- value targets from search values (include/taflhip.h TAFL_EXAMPLES_VALUE_TARGETS; the text there is normative) ----
// The arrays of an object created with the flag, a struct of its own for the reason ExampleStatsMem is one.
struct ExampleTargetsMem {
    uint8_t* ep_end;             // [e] 1: the example is the last of its lane's episode (vt_mark_boundary)
    float* vt;                   // [e] the target (between the two passes of tafl_examples_value_targets: the example's search value)
    uint8_t* kind;               // [e] 0 no target, 1 from a closed episode, 2 from an unfinished one (between the passes: 1 = takes part)
};
enum { VT_CLOSED = 0, VT_UNFINISHED = 1, VT_ROWS = 2, VT_SETTLED = 3, VT_COUNTERS = 4 };
// The boundary recorder, for game g at the begin of a run and after every round and its reopen: the value open_from[g] holds marks the
// example before it.  Stateless, so a value that stands for many rounds, or that a reopen without a new example repeats, marks once.
static TAFL_HD void vt_mark_boundary(const ExamplesMem& X, const ExampleTargetsMem& T, const uint32_t* open_from, uint32_t g) {
    const uint32_t o = open_from[g];
    if (o == 0u || o > X.len[g] || o > X.max_moves) return;
    const size_t e = (size_t)(o - 1u) * X.G + g;
    if (!T.ep_end[e]) T.ep_end[e] = 1;
}
// value of example_search_stats alone (the same operations, hence the same bits); false: N == 0, the example takes no part
static TAFL_HD bool example_search_value(const ExamplesMem& X, const ExampleStatsMem& S, uint32_t j, uint32_t g, uint32_t info, float& value) {
    const uint32_t nc = example_stored_children(X, info);
    value = 0.0f;
    uint32_t N = 0;
    for (uint32_t k = 0; k < nc; ++k) N += X.pol[((size_t)j * X.K + k) * X.G + g] >> 16;
    if (N == 0u) return false;
    double acc = 0.0;
    for (uint32_t k = 0; k < nc; ++k) {
        const size_t at = ((size_t)j * X.K + k) * X.G + g;
        acc = acc + (double)(X.pol[at] >> 16) * (double)S.cq[at];
    }
    value = (float)(acc / (double)N);
    return true;
}
// pass 1, entry e of the per-example arrays: the search value and the participation bit are staged in vt and kind
static TAFL_HD void vt_stage(const ExamplesMem& X, const ExampleStatsMem& S, const ExampleTargetsMem& T, uint32_t e) {
    const uint32_t g = e % X.G, j = e / X.G;
    if (j >= X.max_moves || j >= X.len[g]) return;
    float v;
    const bool part = example_search_value(X, S, j, g, X.info[e], v);
    T.vt[e] = v; T.kind[e] = part ? 1 : 0;
}
static TAFL_HD double vt_lam_pow(double lambda, uint32_t d) {
    double r = 1.0, b = lambda;
    for (uint32_t bit = 0; bit < 16u; ++bit) { if ((d >> bit) & 1u) r = r * b; b = b * b; }
    return r;
}
// pass 2, one lane per game walks its examples backward; what it carries from example j + 1 to example j
struct VtChain { double A, L, u_last, u_next; uint32_t mv_next, have, closed; };
enum { VT_EV_ROW = 1u, VT_EV_CLOSED = 2u, VT_EV_UNFINISHED = 4u, VT_EV_SETTLED = 8u };
// example (j, g) of the backward walk: writes vt and kind (and z, fin when an unfinished episode is settled); returns what to count
static TAFL_HD uint32_t vt_step(const ExamplesMem& X, const ExampleTargetsMem& T, uint32_t j, uint32_t g, double lambda, bool settle, VtChain& c) {
    const size_t e = (size_t)j * X.G + g;
    if (T.ep_end[e]) c.have = 0u;                                  // the last example of an episode: nothing follows it in the chain
    if (!T.kind[e]) { T.vt[e] = 0.0f; return 0u; }
    const double s = ((X.info[e] >> 16) & 0xFFu) == (uint32_t)TAFL_ATTACKER ? 1.0 : -1.0, u = s * (double)T.vt[e];
    const uint32_t mv = X.move_no[e];
    uint32_t ev = VT_EV_ROW;
    if (!c.have) {
        c.have = 1u; c.closed = X.fin[e] == 1 ? 1u : 0u; c.A = 0.0; c.L = 1.0; c.u_last = u;
        ev |= c.closed ? VT_EV_CLOSED : VT_EV_UNFINISHED;
    } else {
        uint32_t d = c.mv_next > mv ? c.mv_next - mv : 1u;
        if (d > 65535u) d = 65535u;
        const double p = vt_lam_pow(lambda, d);
        c.A = (1.0 - p) * c.u_next + p * c.A;
        c.L = p * c.L;
    }
    c.u_next = u; c.mv_next = mv;
    const double term = c.closed ? (double)X.z[e] : s * c.u_last;
    T.vt[e] = (float)(s * c.A + c.L * term); T.kind[e] = c.closed ? 1 : 2;
    if (!c.closed && settle) { X.z[e] = (float)(s * c.u_last); X.fin[e] = 2; ev |= VT_EV_SETTLED; }
    return ev;
}

// The entry a move is drawn with, among n entries of which entry j has count(j) visits: k = mulhi(r, N) = (r * N) >> 32 with N = the sum of
// the counts, and the draw is the first entry in canonical (= ascending action) order whose running sum exceeds k: entry j is drawn for
// floor-exact count(j) / N of the 2^32 values of r.  Integers only.  Entries without visits (the unvisited edges of a guided root) add
// nothing to the running sum, so skipping them cannot change which entry passes first.  Both callers (Ops::selfplay_pick, Guided::selfplay_pick) pass N = the sum of the counts with
// N > 0; then k < N and the running sum always passes it, so the fallback (the last visited entry) is never reached.
template <class Count>
static TAFL_HD uint32_t visit_draw(uint32_t n, uint32_t N, uint32_t r, Count&& count) {
    const uint32_t k = Engine<2, 7>::mulhi(r, N);
    uint32_t run = 0, last = 0;
    for (uint32_t j = 0; j < n; ++j) { const uint32_t v = count(j); if (v == 0) continue; run += v; last = j; if (run > k) return j; }
    return last;
}

// ---- the eight symmetries of the square -----------------------------------------------------------------------------------------
// bit 2 of sym transposes (r, c) -> (c, r) first, then bit 0 mirrors the rows r -> n-1-r, then bit 1 mirrors the columns c -> n-1-c.
// Tiles are r * n + c.
static TAFL_HD uint32_t sym_tile(uint32_t sym, uint32_t t, uint32_t n) {
    uint32_t r = t / n, c = t % n;
    if (sym & 4u) { const uint32_t x = r; r = c; c = x; }
    if (sym & 1u) r = n - 1u - r;
    if (sym & 2u) c = n - 1u - c;
    return r * n + c;
}
// dense action (include/taflhip.h: (from tile) * 2(n-1) + slot, slots V+ V- H+ H- by distance) -> from tile and destination tile
static TAFL_HD void action_tiles(uint32_t a, uint32_t n, uint32_t& from, uint32_t& to) {
    const uint32_t nm = n - 1u, t = a / (2u * nm), s = a % (2u * nm), r = t / n, c = t % n;
    from = t;
    if (s < nm - r) to = (r + s + 1u) * n + c;
    else if (s < nm) to = (r - (s - (nm - r) + 1u)) * n + c;
    else if (s < nm + (nm - c)) to = r * n + c + (s - nm + 1u);
    else to = r * n + c - (s - nm - (nm - c) + 1u);
}
static TAFL_HD uint32_t tiles_action(uint32_t from, uint32_t to, uint32_t n) {
    const uint32_t nm = n - 1u, r = from / n, c = from % n, r2 = to / n, c2 = to % n;
    uint32_t s;
    if (c2 == c) s = r2 > r ? r2 - r - 1u : (nm - r) + (r - r2) - 1u;
    else s = c2 > c ? nm + (c2 - c) - 1u : nm + (nm - c) + (c - c2) - 1u;
    return from * 2u * nm + s;
}
// an action under a symmetry: its from and to tiles transformed and encoded again
static TAFL_HD uint32_t sym_action(uint32_t sym, uint32_t a, uint32_t n) {
    uint32_t from, to; action_tiles(a, n, from, to);
    return tiles_action(sym_tile(sym, from, n), sym_tile(sym, to, n), n);
}

// the same for a move that is at hand as (row, column, direction, distance) of its from tile (directions: 0 r+, 1 r-, 2 c+, 3 c-, the
// order of the slots): the tile is transformed once, the direction by what each step of the symmetry does to it - the transposition
// swaps vertical and horizontal, a mirror reverses the directions along its axis - and the distance stays.  No division.
static TAFL_HD uint32_t sym_move_action(uint32_t sym, uint32_t r, uint32_t c, uint32_t dir, uint32_t dist, uint32_t n) {
    if (sym & 4u) { const uint32_t x = r; r = c; c = x; dir ^= 2u; }
    if (sym & 1u) { r = n - 1u - r; if (dir < 2u) dir ^= 1u; }
    if (sym & 2u) { c = n - 1u - c; if (dir >= 2u) dir ^= 1u; }
    const uint32_t nm = n - 1u;
    const uint32_t slot = dir == 0u ? dist - 1u : dir == 1u ? (nm - r) + dist - 1u : dir == 2u ? nm + dist - 1u : nm + (nm - c) + dist - 1u;
    return (r * n + c) * 2u * nm + slot;
}

// z of an example whose side to move was `side` (TAFL_ATTACKER / TAFL_DEFENDER), from the game's current flags word: +1 that side won,
// -1 it lost, TAFL_DRAW_VALUE (1e-4) a draw; fin = 0 and z = 0 while the game is going on
static TAFL_HD float example_outcome(uint32_t flags, uint32_t side, uint8_t& fin) {
    const uint32_t status = TAFL_F_STATUS(flags);
    fin = status != TAFL_STATUS_ONGOING ? 1 : 0;
    if (status == TAFL_STATUS_WIN) return ((TAFL_F_WINNER(flags) != 0u) == (side != 0u)) ? 1.0f : -1.0f;
    return status == TAFL_STATUS_DRAW ? (float)TAFL_DRAW_VALUE : 0.0f;
}

// z and the final mark of the examples `from` .. len[g] of game g from the flags word of the position their game stands at (the rule of
// tafl_examples_finalize; an episodes run settles the examples of an episode that has just ended with it)
static TAFL_HD void examples_settle(const ExamplesMem& X, uint32_t g, uint32_t from, uint32_t flags) {
    const uint32_t len = X.len[g] < X.max_moves ? X.len[g] : X.max_moves;
    for (uint32_t j = from; j < len; ++j) {
        const size_t e = (size_t)j * X.G + g;
        uint8_t fin; const float z = example_outcome(flags, (X.info[e] >> 16) & 0xFFu, fin);
        X.z[e] = z; X.fin[e] = fin;
    }
}

// the word (sample_seed, global game id, move number in the episode) draws the play of a move with: independent of the sharding
static TAFL_HD uint32_t selfplay_rand(uint64_t sample_seed, uint64_t game_id, uint32_t move_no) {
    using E = Engine<2, 7>;
    return E::ply_rand(E::sim_key(E::game_key(sample_seed, game_id), move_no), 0u);
}

}  // namespace tafl
