// tafl_pool.hpp — the training pool (tafl_pool_*): a ring of finished training examples in HBM, filled from a
// tafl_examples object and sampled uniformly under random board symmetries.  What is decided per example, per row and per drawn row is
// here: which recorded example an ingest takes (pool_take), the words of a row (pool_row_word), the draw (pool_draw), which slots are
// live (pool_slot_live) and what a row writes into a minibatch (pool_out_tile, pool_out_pi); for weighted sampling the masked weight
// (pool_eff), the weighted draw (pool_wdraw) and the steps of its search (pool_wsearch_*, pool_wpick); for de-duplication the key of
// a row, the table insert and the group's mean result (pooldd_*).  __host__ __device__ like
// tafl_examples.hpp: the kernels of tafl_pool.hip run these functions one example / word / tile / policy entry / probe per lane,
// tests/hostsim_pool and tests/hostsim_pool_weights run them in serial loops on the CPU.
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

// ---- weighted sampling (tafl_pool_set_weighting / _set_weights / _sample_weighted): one uint32 weight per slot, a draw in proportion ----
// eff(s) = wt[s] where slot s is live, else 0; W(s) = the sum of eff below s in SLOT order (64 bits), total = W(C).  The prefix structure
// holds, per tile of POOLW_TILE slots, the sum of eff and the exclusive prefix of the sums; a draw searches the tiles' prefixes 64 at a
// time (one probe per lane of a wave), then the 256 weights of the tile, four per lane.
constexpr uint64_t kPoolWDrawKey = 0x504F4F4C57445257ull;     // "POOLWDRW"
enum { POOLW_TILE = 256, POOLW_LANES = 64, POOLW_PER_LANE = 4 };
enum { PW_TOTAL = 0, PW_POSITIVE = 1, PW_BAD_SLOT = 2, PW_WORDS = 3 };
struct PoolWeights {
    uint32_t* wt;                    // [NT * POOLW_TILE]: the slots C .. NT * POOLW_TILE - 1 are never live
    unsigned long long* tile_sum;    // [NT]
    unsigned long long* tile_pre;    // [NT] exclusive
    uint32_t* tile_pos;              // [NT] live slots of the tile with a weight above 0
    unsigned long long* res;         // [PW_WORDS]
    uint32_t NT;
};
static TAFL_HD uint32_t pool_weight_tiles(uint32_t C) { return (uint32_t)(((uint64_t)C + POOLW_TILE - 1) / POOLW_TILE); }
// pool_slot_live with the first live slot, (written - live) mod C, worked out once
static TAFL_HD uint32_t pool_first_live(uint64_t written, uint64_t live, uint32_t C) { return (uint32_t)((written - live) % C); }
static TAFL_HD bool pool_slot_live_from(uint32_t s, uint32_t first, uint64_t live, uint32_t C) {
    if (s >= C) return false;
    const uint64_t age = s >= first ? (uint64_t)(s - first) : (uint64_t)s + (C - first);
    return age < live;
}
static TAFL_HD uint32_t pool_eff(uint32_t w, uint32_t s, uint32_t first, uint64_t live, uint32_t C) { return pool_slot_live_from(s, first, live, C) ? w : 0u; }
// the high 64 bits of a * b
static TAFL_HD uint64_t pool_mulhi64(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
// the weighted draw of row `row` of the sample (seed, step): k < total, the slot is the one s with W(s) <= k < W(s) + eff(s)
static TAFL_HD void pool_wdraw(uint64_t seed, uint64_t step, uint32_t row, uint64_t total, uint32_t flags, uint64_t& k, uint32_t& sym) {
    using E = Engine<2, 7>;
    const uint32_t dk = E::sim_key(E::game_key(seed, step) ^ kPoolWDrawKey, row);
    const uint64_t r = (uint64_t)E::ply_rand(dk, 2u) << 32 | E::ply_rand(dk, 3u);
    k = pool_mulhi64(r, total);
    sym = (flags & 1u) ? E::ply_rand(dk, 1u) >> 29 : 0u;
}
// The search for the last tile t of [lo, hi) with tile_pre[t] <= k (tile_pre[lo] <= k holds), 64 probes per step: lane `lane` probes
// lo + lane * stride; the prefixes ascend, so the lanes whose probe is inside the range and <= k are the first c >= 1 lanes, and the tile
// lies in the stride behind the last of them.  hi - lo shrinks to at most ceil((hi - lo) / 64) per step: three steps for 16 384 tiles.
static TAFL_HD uint32_t pool_wsearch_stride(uint32_t lo, uint32_t hi) { return (hi - lo + (uint32_t)POOLW_LANES - 1u) / (uint32_t)POOLW_LANES; }
static TAFL_HD bool pool_wsearch_probe(uint32_t lo, uint32_t hi, uint32_t lane, uint32_t& idx) {
    const uint64_t i = (uint64_t)lo + (uint64_t)lane * pool_wsearch_stride(lo, hi);
    idx = (uint32_t)i;
    return i < hi;
}
static TAFL_HD void pool_wsearch_narrow(uint32_t& lo, uint32_t& hi, uint32_t c) {
    const uint32_t stride = pool_wsearch_stride(lo, hi);
    lo += ((c ? c : 1u) - 1u) * stride;
    if (hi - lo > stride) hi = lo + stride;
}
// inside a lane's four slots: the last j whose weights below it sum to at most `rem` (rem < the lane's sum); w = that slot's weight
static TAFL_HD uint32_t pool_wpick(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, uint64_t rem, uint32_t& w) {
    const uint64_t p1 = e0, p2 = p1 + e1, p3 = p2 + e2;
    uint32_t j = 0; w = e0;
    if (p1 <= rem) { j = 1; w = e1; }
    if (p2 <= rem) { j = 2; w = e2; }
    if (p3 <= rem) { j = 3; w = e3; }
    return j;
}
// the slot the rank i < min(T, C) of the rows an ingest of T taken examples stores goes to (the ranks r >= T - min(T, C), pool_place)
static TAFL_HD uint32_t pool_stored_slot(uint64_t written, uint32_t i, uint32_t T, uint32_t C) { return (uint32_t)((written + (T - (T < C ? T : C)) + i) % C); }
// the weight tafl_pool_weights_from_surprise assigns to a row of surprise `surprise`: x = (double)surprise * per_nat,
// min(2^32 - 1, base + (x < 2^32 ? (uint64)x : 2^32 - 1))
static TAFL_HD uint32_t pool_surprise_weight(float surprise, uint32_t base, double per_nat) {
    const double x = (double)surprise * per_nat;
    const uint64_t add = x < 4294967296.0 ? (uint64_t)x : 0xFFFFFFFFull, w = (uint64_t)base + add;
    return w < 0xFFFFFFFFull ? (uint32_t)w : 0xFFFFFFFFu;
}

// ---- de-duplication (tafl_pool_dedup / _gather_dedup / _weights_from_dedup; the text in include/taflhip.h is normative) --
// Live rows with equal keys form a group; a key is a 64-bit hash of the side to move and the board bytes (under the symmetry that gives the
// smallest hash, with TAFL_POOL_DEDUP_SYMMETRIES).  The groups are found in an open-addressing table of integer counters, so that what a
// row reads back depends on the pool's contents alone, never on the order the rows were inserted in.
#if defined(__HIP_DEVICE_COMPILE__)
#define TAFL_POOLDD_CAS(p, cmp, v) atomicCAS((p), (unsigned long long)(cmp), (unsigned long long)(v))
#define TAFL_POOLDD_ADD(p, v) atomicAdd((p), (v))
#define TAFL_POOLDD_MAX(p, v) atomicMax((p), (v))
#else
#define TAFL_POOLDD_CAS(p, cmp, v) (*(p) == (unsigned long long)(cmp) ? (*(p) = (unsigned long long)(v), (unsigned long long)(cmp)) : *(p))
#define TAFL_POOLDD_ADD(p, v) (*(p) += (v))
#define TAFL_POOLDD_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#endif
enum { PDD_DISTINCT = 0, PDD_LARGEST = 1, PDD_COLLISIONS = 2, PDD_WORDS = 4 };
enum { POOLDD_ROWS = 32 };           // rows a workgroup of k_pooldd_key stages: eight lanes per row
// the table of one tafl_pool_dedup call: TS entries, all zero before the first insert (no key is 0)
struct PoolDedupTable {
    unsigned long long* key;         // [TS] 0: free
    uint32_t* count;                 // [TS] members
    uint32_t* wins;                  // [TS] members with z == 1.0f
    uint32_t* losses;                // [TS] members with z == -1.0f
    uint32_t* newest;                // [TS] the largest age rank of a member
    uint32_t TS;
};
static TAFL_HD size_t pooldd_table_bytes(uint32_t TS) { return 24 * (size_t)TS; }
static TAFL_HD PoolDedupTable pooldd_table(void* base, uint32_t TS) {
    PoolDedupTable T;
    T.key = static_cast<unsigned long long*>(base);
    T.count = reinterpret_cast<uint32_t*>(T.key + TS); T.wins = T.count + TS; T.losses = T.wins + TS; T.newest = T.losses + TS; T.TS = TS;
    return T;
}
// the table of a call over `live` rows: the power of two that is at least 2 * live (at least 64)
static TAFL_HD uint32_t pooldd_table_size(uint64_t live) { uint64_t ts = 64; while (ts < 2 * live) ts <<= 1; return (uint32_t)ts; }
// the splitmix64 finaliser
static TAFL_HD uint64_t pooldd_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// sym_tile is a bijection of the tiles; its inverse is sym_tile of this symmetry (the two rotations by a quarter turn swap, the others
// are their own inverse)
static TAFL_HD uint32_t pooldd_sym_inverse(uint32_t sym) { return (sym == 5u || sym == 6u) ? sym ^ 3u : sym; }
// sym_tile(sym, r * n + c, n) for a tile at hand as (r, c): no division
static TAFL_HD uint32_t pooldd_sym_rc(uint32_t sym, uint32_t r, uint32_t c, uint32_t n) {
    if (sym & 4u) { const uint32_t x = r; r = c; c = x; }
    if (sym & 1u) r = n - 1u - r;
    if (sym & 2u) c = n - 1u - c;
    return r * n + c;
}
// h(sym) of a row: the image under sym has byte b[t] at tile sym_tile(sym, t, n), so its tile u holds b[sym_tile(inverse, u, n)]; the
// image is folded word by word, four tiles per word, zero bytes beyond n * n.  `b`: the row's board bytes, tile t at b[t].
static TAFL_HD uint64_t pooldd_hash(const uint8_t* b, uint32_t sym, uint32_t n, uint32_t BW, uint32_t side) {
    const uint32_t inv = pooldd_sym_inverse(sym);
    uint64_t x = 0x9E3779B97F4A7C15ull ^ (uint64_t)side;
    uint32_t r = 0, c = 0;
    for (uint32_t i = 0; i < BW; ++i) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
            if (r >= n) break;
            w |= (uint32_t)b[inv ? pooldd_sym_rc(inv, r, c, n) : r * n + c] << (8u * k);
            if (++c == n) { c = 0; ++r; }
        }
        x = pooldd_mix64(x ^ (uint64_t)w);
    }
    return x;
}
// the key of a hash: its low key_bits bits (1..64, 0 means 64), 1 in place of 0
static TAFL_HD uint64_t pooldd_key(uint64_t h, uint32_t key_bits) {
    if (key_bits != 0u && key_bits < 64u) h &= (1ull << key_bits) - 1ull;
    return h ? h : 1ull;
}
// key and canon of a row, all by one caller (the kernel gives a symmetry to each of eight lanes and takes the minimum across them)
static TAFL_HD uint64_t pooldd_row_key(const uint32_t* row, uint32_t n, uint32_t BW, bool symmetries, uint32_t key_bits, uint32_t& canon) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(row);
    const uint32_t side = pool_row_side(row, BW);
    uint64_t best = pooldd_hash(b, 0u, n, BW, side);
    canon = 0;
    if (symmetries)
        for (uint32_t s = 1; s < 8u; ++s) { const uint64_t h = pooldd_hash(b, s, n, BW, side); if (h < best) { best = h; canon = s; } }
    return pooldd_key(best, key_bits);
}
// the rows a and b have the same side to move and the same canonical image (each under its own canon)
static TAFL_HD bool pooldd_same(const uint32_t* a, uint32_t canon_a, const uint32_t* b, uint32_t canon_b, uint32_t n, uint32_t BW) {
    if (pool_row_side(a, BW) != pool_row_side(b, BW)) return false;
    if (canon_a == canon_b) {                                                   // the same symmetry on both: the images are equal where the boards are, word by word
        for (uint32_t w = 0; w < BW; ++w) if (a[w] != b[w]) return false;
        return true;
    }
    const uint8_t* pa = reinterpret_cast<const uint8_t*>(a); const uint8_t* pb = reinterpret_cast<const uint8_t*>(b);
    const uint32_t ia = pooldd_sym_inverse(canon_a), ib = pooldd_sym_inverse(canon_b);
    for (uint32_t r = 0; r < n; ++r)
        for (uint32_t c = 0; c < n; ++c)
            if (pa[pooldd_sym_rc(ia, r, c, n)] != pb[pooldd_sym_rc(ib, r, c, n)]) return false;
    return true;
}
// where the probe of a key starts (a multiplicative hash, mapped to [0, TS) by the high half of a product: any TS) and goes on
static TAFL_HD uint32_t pooldd_start(uint64_t key, uint32_t TS) { return (uint32_t)pool_mulhi64(key * 0x9E3779B97F4A7C15ull, (uint64_t)TS); }
static TAFL_HD uint32_t pooldd_next(uint32_t pos, uint32_t TS) { return pos + 1u == TS ? 0u : pos + 1u; }
// `cnt` rows of the key, `wins` / `losses` of them won / lost, the newest of age rank `age`, join the key's entry; returns the entry.  The
// entry is found or claimed by linear probing (a free entry is claimed with a 64-bit compare-and-swap); all that is stored are sums and a
// maximum of integers.  The table has more entries than keys, so the probe ends; it is bounded by TS all the same.
static TAFL_HD uint32_t pooldd_insert(const PoolDedupTable& T, uint64_t key, uint32_t cnt, uint32_t wins, uint32_t losses, uint32_t age) {
    uint32_t pos = pooldd_start(key, T.TS);
    for (uint32_t i = 0; i < T.TS; ++i) {
        unsigned long long k = T.key[pos];
        if (k == 0ull) k = TAFL_POOLDD_CAS(&T.key[pos], 0ull, key);
        if (k == 0ull || k == key) break;
        pos = pooldd_next(pos, T.TS);
    }
    TAFL_POOLDD_ADD(&T.count[pos], cnt);
    if (wins) TAFL_POOLDD_ADD(&T.wins[pos], wins);
    if (losses) TAFL_POOLDD_ADD(&T.losses[pos], losses);
    TAFL_POOLDD_MAX(&T.newest[pos], age);
    return pos;
}
// the mean result of a group of m rows: integer counts and one division
static TAFL_HD float pooldd_zmean(uint32_t m, uint32_t wins, uint32_t losses) {
    return (float)(((double)wins - (double)losses + (double)(m - wins - losses) * (double)(float)TAFL_DRAW_VALUE) / (double)m);
}
// the weight tafl_pool_weights_from_dedup assigns to a live slot: w = its weight now, m = mult, is_rep = it is its group's representative
static TAFL_HD uint32_t pooldd_weight(uint32_t w, uint32_t m, bool is_rep, uint32_t scale, uint32_t flags) {
    if (m == 0u) m = 1u;                                                        // (no live slot of a valid result has it)
    if (flags & 2u) return is_rep ? scale : 0u;
    if (flags & 1u) { if (w == 0u) return 0u; const uint32_t q = w / m; return q ? q : 1u; }
    const uint32_t q = scale / m;
    return q ? q : 1u;
}

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
