// hostsim_search_stats.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  Search statistics per training row (include/taflhip.h "search
// value and policy surprise") on the host: the examples buffer of tests/hostsim_solver with the two arrays beside pol
// and the recorder's per-lane count; a session of that harness steps as it always did and, after every round, the product's record_stats
// runs for one lane after the other, as k_gselfplay_record_stats does behind the round kernels; the two scalars are the product's
// example_search_stats in the loop of k_examples_gather_stats.
#ifdef HQS_MAIN       /* the sanitizer program plays Brandubh only, as the solver harness's own program does: that one's main is set aside */
#define HSS_MAIN
#define main hss_program
#endif
#include "../hostsim_solver/hostsim_solver.cpp"
#ifdef HQS_MAIN
#undef main
#endif
#include "../hostsim_pool_weights/hostsim_pool_weights.cpp"

// every entry of the two arrays is filled with a pattern no run writes (a NaN with a payload)
static float hqs_pattern() { union { uint32_t u; float f; } c; c.u = 0x7FC0BEEFu; return c.f; }
struct ExStats : ExEp {
    std::vector<float> cq, cp; std::vector<uint32_t> seen;
    ExStats(uint32_t G_, uint8_t n_, uint32_t max_moves_, uint32_t K_) : ExEp(G_, n_, max_moves_, K_), cq((size_t)G_ * max_moves_ * K_, hqs_pattern()),
        cp((size_t)G_ * max_moves_ * K_, hqs_pattern()), seen(G_, 0u) {}
    ExampleStatsMem smem() { ExampleStatsMem S; S.cq = cq.data(); S.cp = cp.data(); S.seen = seen.data(); return S; }
};
// tests/hostsim_pool_weights' pool with the two per-slot arrays: the loops restate k_pool_ingest_stats, k_pool_gather_stats and
// k_poolw_from_surprise, the per-item functions are the product's
struct PoolSHost {
    PoolWHost w;
    bool on = false;
    std::vector<float> value, surprise;
    PoolSHost(uint32_t C, uint32_t Kp, uint8_t n) : w(C, Kp, n) {}
    int set_search_stats(bool enable) {
        if (w.pool.book.live != 0) return -1;
        if (!enable) { on = false; value.clear(); surprise.clear(); return 0; }
        if (!on) { value.assign(w.pool.M.C, 0.0f); surprise.assign(w.pool.M.C, 0.0f); on = true; }
        return 0;
    }
    // tafl_pool_ingest: the rows and the weights by the harnesses below, then k_pool_ingest_stats one example after the other.
    // `ex` null stands for an examples object without the flag (`plain` is that object)
    int ingest(ExStats* ex, ExHost* plain, uint64_t* out3) {
        if (on && !ex) return -1;
        const uint64_t written = w.pool.book.written;
        uint64_t o3[3];
        const int rc = w.ingest(ex ? ex : plain, o3);
        if (rc) return rc;
        if (out3) { out3[0] = o3[0]; out3[1] = o3[1]; out3[2] = o3[2]; }
        if (!on) return 0;
        const ExamplesMem X = ex->mem(); const ExampleStatsMem S = ex->smem();
        const uint32_t E = X.G * X.max_moves, T = (uint32_t)o3[0], C = w.pool.M.C, first = T - (T < C ? T : C);
        uint32_t r = 0, info;
        for (uint32_t e = 0; e < E; ++e) {
            if (pool_take(X, e, info) != POOL_TAKEN) continue;
            if (r >= first) {
                float v, s;
                example_search_stats(X, S, e / X.G, e % X.G, info, v, s);
                const uint32_t slot = pool_stored_slot(written, r - first, T, C);
                value[slot] = v; surprise[slot] = s;
            }
            ++r;
        }
        return 0;
    }
};
struct StatsRun { void* h; ExStats* ex; uint32_t word_bits; };

extern "C" {
void* hqs_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return new ExStats(G, n, max_moves, K); }
void hqs_ex_free(void* h) { delete (ExStats*)h; }
// hss_begin recording into `ex` (an ExStats): the recorder deals with what this run appends, seen = len, as gselfplay_begin sets it
void* hqs_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t n_sims, uint32_t edges_per_node,
                double c_puct, const tafl_root_noise* noise, const tafl_playout_cap* cap, const tafl_forced_playouts* fcfg, const tafl_solver* scfg, const tafl_selfplay_opts* o, uint32_t n_moves,
                uint64_t base, int episodes, uint64_t id_stride, uint32_t episode_moves, void* ex) {
    ExStats* x = (ExStats*)ex;
    if (!x) return nullptr;
    for (uint32_t g = 0; g < x->G && g < G; ++g) x->seen[g] = x->len[g] < x->max_moves ? x->len[g] : x->max_moves;
    void* h = hss_begin(r, n, word_bits, st, openings, G, n_sims, edges_per_node, c_puct, noise, cap, fcfg, scfg, o, n_moves, base, episodes, id_stride, episode_moves, (ExEp*)x);
    return h ? new StatsRun{h, x, word_bits} : nullptr;
}
void* hqs_session(void* run) { return ((StatsRun*)run)->h; }
void hqs_free(void* run) { StatsRun* s = (StatsRun*)run; hss_free(s->h); delete s; }
// one round (hss_step), then the recorder for every lane
uint32_t hqs_step(void* run, const float* priors, const float* values) {
    StatsRun* s = (StatsRun*)run;
    const uint32_t w = hss_step(s->h, priors, values);
    const ExamplesMem X = s->ex->mem(); const ExampleStatsMem S = s->ex->smem();
    SvBase* b = (SvBase*)s->h;
    const GuidedMem* M = nullptr;
    if (s->word_bits == 64) M = &static_cast<SvSession<2, 7>*>(b)->R.M;
#ifndef HSS_MAIN
    else if (s->word_bits == 128) M = &static_cast<SvSession<4, 11>*>(b)->R.M;
    else M = &static_cast<SvSession<8, 15>*>(b)->R.M;
#endif
    for (uint32_t g = 0; g < M->G; ++g) record_stats(*M, g, X, S);
    return w;
}
// tafl_examples_finalize against the positions `st` (one per lane): z and the final mark of every open example of lane g from st[g]
void hqs_ex_finalize(void* h, const tafl_state* st) {
    ExStats* x = (ExStats*)h;
    const ExamplesMem X = x->mem();
    for (uint32_t g = 0; g < x->G; ++g) { DState<2> s; state_from_abi<2>(st[g], s); examples_settle(X, g, x->open_from[g], s.flags); }
}
// the raw arrays, [max_moves * K * G] each, as the recorder left them (the pattern where nothing was stored)
void hqs_ex_raw(void* h, float* cq, float* cp) { ExStats* x = (ExStats*)h; memcpy(cq, x->cq.data(), 4 * x->cq.size()); memcpy(cp, x->cp.data(), 4 * x->cp.size()); }
// tafl_examples_read_stats: q, prior [count * K]; -1 for an index that names no example
int hqs_ex_read_stats(void* h, const uint32_t* index, uint32_t count, float* q, float* prior) {
    ExStats* x = (ExStats*)h;
    const ExamplesMem X = x->mem(); const ExampleStatsMem S = x->smem();
    for (uint32_t i = 0; i < count; ++i) { const uint32_t g = index[i] % X.G, j = index[i] / X.G; if (j >= X.max_moves || j >= X.len[g]) return -1; }
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t e = index[i], g = e % X.G, j = e / X.G, nc = example_stored_children(X, X.info[e]);
        for (uint32_t k = 0; k < X.K; ++k) {
            const size_t at = ((size_t)j * X.K + k) * X.G + g;
            q[(size_t)i * X.K + k] = k < nc ? S.cq[at] : 0.0f; prior[(size_t)i * X.K + k] = k < nc ? S.cp[at] : 0.0f;
        }
    }
    return 0;
}
// tafl_examples_gather_stats with device pointers (k_examples_gather_stats, one row after the other): returns the rows whose index
// named no example (they are zeros)
int hqs_ex_gather_stats(void* h, const uint32_t* index, uint32_t count, float* value, float* surprise) {
    ExStats* x = (ExStats*)h;
    const ExamplesMem X = x->mem(); const ExampleStatsMem S = x->smem();
    int bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t e = index[i], g = e % X.G, j = e / X.G;
        const bool ok = j < X.max_moves && j < X.len[g];
        float v = 0.0f, s = 0.0f;
        if (ok) example_search_stats(X, S, j, g, X.info[e], v, s); else { x->counters[EX_BAD_INDEX] += 1; ++bad; }
        value[i] = v; surprise[i] = s;
    }
    return bad;
}

void* hqs_pool_new(uint32_t C, uint32_t Kp, uint8_t n) { return (C == 0 || Kp == 0 || Kp > 0xFFFFu) ? nullptr : new PoolSHost(C, Kp, n); }
void hqs_pool_free(void* h) { delete (PoolSHost*)h; }
// the PoolWHost inside, for the hspw_* calls that neither ingest nor change this setting (weighting, trim, weights, draws, stats)
void* hqs_pool_weights(void* h) { return &((PoolSHost*)h)->w; }
int hqs_pool_set_search_stats(void* h, int on) { return ((PoolSHost*)h)->set_search_stats(on != 0); }
// `with_stats` 0: `ex` is taken as an examples object created without the flag
int hqs_pool_ingest(void* h, void* ex, int with_stats, uint64_t* out3) { return ((PoolSHost*)h)->ingest(with_stats ? (ExStats*)ex : nullptr, (ExHost*)(ExStats*)ex, out3); }
// tafl_pool_gather_stats: strict (host pointers) refuses a slot that is not live (-1); otherwise zeros, counted; returns the rows so counted
int hqs_pool_gather_stats(void* h, const uint32_t* slot, uint32_t count, float* value, float* surprise, int strict) {
    PoolSHost* p = (PoolSHost*)h;
    if (!p->on) return -1;
    const uint32_t f = p->w.first(), C = p->w.pool.M.C; const uint64_t live = p->w.pool.book.live;
    if (strict) for (uint32_t i = 0; i < count; ++i) if (!pool_slot_live_from(slot[i], f, live, C)) return -1;
    int bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const bool ok = pool_slot_live_from(slot[i], f, live, C);
        if (!ok) { p->w.pool.counters[POOL_BAD_SLOT] += 1; ++bad; }
        value[i] = ok ? p->value[slot[i]] : 0.0f; surprise[i] = ok ? p->surprise[slot[i]] : 0.0f;
    }
    return bad;
}
// tafl_pool_weights_from_surprise: -1 TAFL_ERR_INVALID_ARG, -5 TAFL_ERR_UNSUPPORTED
int hqs_pool_weights_from_surprise(void* h, const tafl_pool_surprise_weights* cfg) {
    PoolSHost* p = (PoolSHost*)h;
    if (!cfg || !p->w.on || !p->on || !(cfg->per_nat >= 0.0)) return -1;
    if (cfg->flags) return -5;
    for (uint32_t r : cfg->_reserved) if (r) return -5;
    const PoolMem& M = p->w.pool.M;
    const uint32_t f = p->w.first(); const uint64_t live = p->w.pool.book.live;
    for (uint32_t s = 0; s < M.C; ++s) {
        if (!pool_slot_live_from(s, f, live, M.C)) continue;
        if (cfg->generation != 0u && M.rows[(size_t)s * M.RW + M.BW + PR_GENERATION] != cfg->generation) continue;
        p->w.wt[s] = pool_surprise_weight(p->surprise[s], cfg->base, cfg->per_nat);
    }
    p->w.dirty = true;
    return 0;
}
}

#ifdef HQS_MAIN
// The stand-alone program of the sanitizer target: Brandubh, 8 lanes some plies into random games, constant priors, S = 24.  A solver
// episodes run with root noise, a cap and forced playouts records into a buffer with the statistics that drops (6 examples per lane) and
// overflows (K = 4); the examples are finalized against finished positions and gathered with indices beyond len and beyond the buffer.
#include <stdio.h>
int main() {
    tafl_rules r; const uint32_t G = 8, A = 7 * 7 * 12, K = 4, MM = 6;
    if (preset_rules("brandubh", &r)) { printf("no preset\n"); return 1; }
    Consts<2> C; if (make_consts<2, 7>(r, 7, C)) { printf("no consts\n"); return 1; }
    std::vector<tafl_state> st(G), over(G);
    for (uint32_t g = 0; g < G; ++g) {
        if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st[g], nullptr)) { printf("bad fen\n"); return 1; }
        DState<2> s; state_from_abi<2>(st[g], s);
        DState<2> e = s;
        Ops<2, 7>::random_advance(s, 77, g, 3 + 2 * g, C, false); state_to_abi<2>(s, 7, st[g]);
        Ops<2, 7>::random_advance(e, 77, g, 2000, C, false); state_to_abi<2>(e, 7, over[g]);
        if (TAFL_F_STATUS(e.flags) == TAFL_STATUS_ONGOING) { printf("game %u is not over\n", g); return 1; }
    }
    std::vector<float> pri((size_t)G * A, 1.0f), val(G, 0.25f);
    tafl_root_noise nz; memset(&nz, 0, sizeof nz); nz.alpha = 0.3; nz.epsilon = 0.25; nz.seed = 7;
    tafl_playout_cap cap; memset(&cap, 0, sizeof cap); cap.seed = 11; cap.fast_sims = 3; cap.full_per_65536 = 49152;
    tafl_forced_playouts fc; memset(&fc, 0, sizeof fc); fc.k = 2.0;
    tafl_solver sc; memset(&sc, 0, sizeof sc);
    tafl_selfplay_opts o; memset(&o, 0, sizeof o); o.sample_seed = 5; o.temp_moves = 4;
    void* ex = hqs_ex_new(G, 7, MM, K);
    void* h = hqs_begin(&r, 7, 64, st.data(), nullptr, G, 24, 128, 1.25, &nz, &cap, &fc, &sc, &o, 12, 100, 1, 0, 5, ex);
    if (!h) { printf("begin failed\n"); return 1; }
    uint32_t w = 1, rounds = 0;
    while (w && rounds++ < 100000) w = hqs_step(h, pri.data(), val.data());
    hqs_free(h);
    hqs_ex_finalize(ex, over.data());
    std::vector<uint32_t> len(G), index; uint64_t xc[EX_COUNTERS];
    hss_ex_counts(ex, len.data(), xc, nullptr);
    for (uint32_t e = 0; e < G * MM + 9; ++e) index.push_back((e * 5u) % (G * MM + 9));
    std::vector<float> v(index.size()), s(index.size());
    const int bad = hqs_ex_gather_stats(ex, index.data(), (uint32_t)index.size(), v.data(), s.data());
    double acc = 0.0;
    for (size_t i = 0; i < index.size(); ++i) { if (!(s[i] >= 0.0f) || !(v[i] >= -1.0f && v[i] <= 1.0f)) { printf("scalar out of range at %zu\n", i); return 1; } acc += v[i] + s[i]; }
    // a pool of 4 slots takes the finished examples (few: a cut episode stays open) three times, so that the ring wraps, with the statistics and the weighting on, is
    // gathered with dead slots, and its weights are set from the surprise by generation, for all rows with a saturating per_nat, and refused
    void* p = hqs_pool_new(4, 6, 7);
    uint64_t o3[3] = {0, 0, 0};
    if (hqs_pool_set_search_stats(p, 1)) { printf("set failed\n"); return 1; }
    if (hqs_pool_ingest(p, ex, 0, o3) != -1) { printf("ingest of an object without the arrays\n"); return 1; }
    hspw_set_weighting(hqs_pool_weights(p), 1, 7);
    for (int i = 0; i < 3; ++i) if (hqs_pool_ingest(p, ex, 1, o3)) { printf("ingest failed\n"); return 1; }
    if (hqs_pool_set_search_stats(p, 0) != -1) { printf("the setting changed with live rows\n"); return 1; }
    std::vector<uint32_t> slots; for (uint32_t k = 0; k < 25; ++k) slots.push_back(k);
    std::vector<float> pv(25), ps(25);
    if (hqs_pool_gather_stats(p, slots.data(), 25, pv.data(), ps.data(), 1) != -1) { printf("strict gather took a dead slot\n"); return 1; }
    const int dead = hqs_pool_gather_stats(p, slots.data(), 25, pv.data(), ps.data(), 0);
    tafl_pool_surprise_weights cfg; memset(&cfg, 0, sizeof cfg);
    cfg.base = 3; cfg.per_nat = 1000.0; cfg.generation = 3;
    if (hqs_pool_weights_from_surprise(p, &cfg)) { printf("weights failed\n"); return 1; }
    cfg.generation = 0; cfg.per_nat = 1e300; cfg.base = 0xFFFFFFF0u;
    if (hqs_pool_weights_from_surprise(p, &cfg)) { printf("weights failed\n"); return 1; }
    cfg.per_nat = -1.0;
    if (hqs_pool_weights_from_surprise(p, &cfg) != -1) { printf("a negative per_nat was taken\n"); return 1; }
    uint64_t s8[8]; hspw_stats(hqs_pool_weights(p), s8);
    printf("rounds %u examples dropped %llu overflowed %llu bad indices %d taken %llu dead slots %d total weight %llu\nchecksum %.6f\n", rounds, (unsigned long long)xc[0],
           (unsigned long long)xc[1], bad, (unsigned long long)o3[0], dead, (unsigned long long)s8[2], acc);
    hqs_pool_free(p);
    hqs_ex_free(ex);
    return 0;
}
#endif
