// tafl_pool.hpp — the training pool (tafl_pool_*): a ring of finished training examples in HBM, filled from a
// tafl_examples object and sampled uniformly under random board symmetries.  What is decided per example, per row and per drawn row is
// here: which recorded example an ingest takes (pool_take), the words of a row (pool_row_word), the draw (pool_draw), which slots are
// live (pool_slot_live) and what a row writes into a minibatch (pool_out_tile, pool_out_pi).  __host__ __device__ like tafl_examples.hpp:
// the kernels of tafl_pool.hip run these functions one example / word / tile / policy entry per lane, tests/hostsim_pool runs them in
// serial loops on the CPU.
#pragma once
#include <vector>
#include "tafl_examples.hpp"

namespace tafl {

// what an ingest does with the entry e of the per-example arrays
enum { POOL_NONE = 0, POOL_TAKEN = 1, POOL_OPEN = 2, POOL_OVERFLOW = 3 };
// A row, RW = pool_row_words words, contiguous: BW board words as example_append wrote them, then the PR_HEAD words below, then Kp policy
// words action | Nsa << 16 in canonical order (zero beyond n_children), then zeros up to a multiple of four words (16 bytes).
enum { PR_INFO = 0, PR_N = 1, PR_MOVE_NO = 2, PR_GENERATION = 3, PR_Z = 4, PR_HEAD = 5 };
enum { POOL_BAD_SLOT = 0, POOL_COUNTERS = 1 };
constexpr uint64_t kPoolDrawKey = 0x504F4F4C44524157ull;      // "POOLDRAW"
struct PoolMem {
    uint32_t* rows;                  // [slot * RW + w]
    unsigned long long* counters;    // [POOL_COUNTERS]
    uint32_t C, Kp, BW, RW;
};
static TAFL_HD uint32_t pool_row_words(uint32_t BW, uint32_t Kp) { return (BW + (uint32_t)PR_HEAD + Kp + 3u) & ~3u; }

// the take predicate: entry e < G * max_moves of `X` holds no example (beyond its lane's len), an example without a policy, an example
// whose result is open, or one the pool takes.  `info` receives the example's info word.
static TAFL_HD uint32_t pool_take(const ExamplesMem& X, uint32_t e, uint32_t& info) {
    const uint32_t g = e % X.G, j = e / X.G;
    info = 0;
    if (j >= X.max_moves || j >= X.len[g]) return POOL_NONE;
    info = X.info[e];
    if (info & kExOverflow) return POOL_OVERFLOW;
    return X.fin[e] ? POOL_TAKEN : POOL_OPEN;
}

// word w < RW of the row of example (j, g) (info word `info`) taken by the ingest number `generation`
static TAFL_HD uint32_t pool_row_word(const ExamplesMem& X, uint32_t j, uint32_t g, uint32_t info, uint32_t w, uint32_t generation) {
    if (w < X.BW) return X.boards[((size_t)j * X.BW + w) * X.G + g];
    const size_t e = (size_t)j * X.G + g;
    const uint32_t h = w - X.BW;
    if (h == PR_INFO) return info & 0x00FFFFFFu;
    if (h == PR_N) return X.played[e] >> 16;
    if (h == PR_MOVE_NO) return X.move_no[e];
    if (h == PR_GENERATION) return generation;
    if (h == PR_Z) { union { float f; uint32_t u; } c; c.f = X.z[e]; return c.u; }
    const uint32_t k = h - PR_HEAD;
    return (k < X.K && k < (info & 0xFFFFu)) ? X.pol[((size_t)j * X.K + k) * X.G + g] : 0u;
}

// the slot the example of rank r of an ingest of T taken examples goes to, in a pool of C slots that had taken `written` rows before:
// false for the examples that would be overwritten by the same ingest (they are never stored)
static TAFL_HD bool pool_place(uint64_t written, uint32_t r, uint32_t T, uint32_t C, uint32_t& slot) {
    if (r < T - (T < C ? T : C)) return false;
    slot = (uint32_t)((written + r) % C);
    return true;
}

// The draw of row `row` of the sample (seed, step): integers only, a pure function of its arguments.  a = the age rank (0 = the oldest
// live row).  live in 1..C.
static TAFL_HD void pool_draw(uint64_t seed, uint64_t step, uint32_t row, uint64_t written, uint64_t live, uint32_t C, uint32_t flags, uint32_t& slot, uint32_t& sym) {
    using E = Engine<2, 7>;
    const uint32_t dk = E::sim_key(E::game_key(seed, step) ^ kPoolDrawKey, row);
    const uint32_t a = E::mulhi(E::ply_rand(dk, 0u), (uint32_t)live);
    slot = (uint32_t)((written - live + a) % C);
    sym = (flags & 1u) ? E::ply_rand(dk, 1u) >> 29 : 0u;
}
// slot s holds one of the rows [written - live, written)
static TAFL_HD bool pool_slot_live(uint32_t s, uint64_t written, uint64_t live, uint32_t C) {
    if (s >= C) return false;
    const uint32_t first = (uint32_t)((written - live) % C);
    const uint64_t age = s >= first ? (uint64_t)(s - first) : (uint64_t)s + (C - first);
    return age < live;
}

// what a row writes into a minibatch under the symmetry sym: tile t of the board goes to `dst` with the returned byte, policy entry
// k < n_children goes to the dense action `a` with the returned probability - the bytes tafl_examples_gather writes
static TAFL_HD uint8_t pool_out_tile(const uint32_t* row, uint32_t t, uint32_t n, uint32_t sym, uint32_t& dst) {
    dst = sym ? sym_tile(sym, t, n) : t;
    return (uint8_t)(row[t >> 2] >> (8u * (t & 3u)));
}
static TAFL_HD float pool_out_pi(const uint32_t* row, uint32_t BW, uint32_t k, uint32_t n, uint32_t sym, uint32_t& a) {
    const uint32_t w = row[BW + (uint32_t)PR_HEAD + k];
    a = sym ? sym_action(sym, w & 0xFFFFu, n) : (w & 0xFFFFu);
    return (float)((double)(w >> 16) / (double)row[BW + (uint32_t)PR_N]);
}
static TAFL_HD uint32_t pool_row_children(const uint32_t* row, uint32_t BW) { return row[BW + (uint32_t)PR_INFO] & 0xFFFFu; }
static TAFL_HD uint8_t pool_row_side(const uint32_t* row, uint32_t BW) { return (uint8_t)((row[BW + (uint32_t)PR_INFO] >> 16) & 0xFFu); }
static TAFL_HD float pool_row_z(const uint32_t* row, uint32_t BW) { union { float f; uint32_t u; } c; c.u = row[BW + (uint32_t)PR_Z]; return c.f; }


// The host's bookkeeping of a pool (tafl_pool_ingest, tafl_pool_trim, tafl_pool_get_stats): the live rows are [written - live, written),
// and per ingest that may still have a live row, the row number its rows end before.  Rows are in age order and generations are
// monotone, so what a trim keeps is a suffix.
struct PoolBook {
    struct Gen { uint64_t generation, end; };
    uint64_t written = 0, live = 0, ingests = 0;
    std::vector<Gen> gens;               // ascending
    void clear() { written = live = ingests = 0; gens.clear(); }
    // an ingest took T rows into a pool of C slots (T = 0 still is a generation)
    void took(uint64_t T, uint32_t C) {
        written += T; ingests += 1;
        live = live + T < C ? live + T : C;
        gens.push_back(Gen{ingests, written});
        (void)oldest_generation();
    }
    // only the rows of the newest `keep` >= 1 ingests stay live
    void trim(uint64_t keep) {
        if (keep >= ingests) return;
        uint64_t cut = 0;                // where the last generation that is not kept ends
        for (const Gen& g : gens) if (g.generation <= ingests - keep) cut = g.end;
        if (cut > written - live) live = written - cut;
        (void)oldest_generation();
    }
    // the generation of the oldest live row (0: no live row); drops the entries of ingests without a live row
    uint64_t oldest_generation() {
        if (live == 0) { gens.clear(); return 0; }
        size_t k = 0;
        while (k < gens.size() && gens[k].end <= written - live) ++k;
        gens.erase(gens.begin(), gens.begin() + k);
        return gens.empty() ? 0 : gens.front().generation;
    }
};

}  // namespace tafl
