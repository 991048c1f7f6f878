// hostsim_value_targets.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  Value targets from search values (include/taflhip.h "value
// targets") on the host: the examples buffer of tests/hostsim_search_stats with ep_end, vt and kind beside it; a
// session of that harness steps as it always did and, after every round and its recorder, the product's vt_mark_boundary runs for one lane
// after the other, as k_gselfplay_mark_boundary does; the targets are the product's vt_stage and vt_step in the loops of
// k_examples_vt_stage and k_examples_vt_chain, the pool's pass restates k_pool_ingest_targets.
#ifdef HVT_MAIN       /* the sanitizer program plays Brandubh only (HSS_MAIN), and the solver harness's own program is set aside */
#define HSS_MAIN
#define main hss_program
#endif
#include "../hostsim_search_stats/hostsim_search_stats.cpp"
#ifdef HVT_MAIN
#undef main
#endif

struct ExVt : ExStats {
    std::vector<uint8_t> ep_end, kind; std::vector<float> vt;
    bool valid = false;
    ExVt(uint32_t G_, uint8_t n_, uint32_t max_moves_, uint32_t K_) : ExStats(G_, n_, max_moves_, K_), ep_end((size_t)G_ * max_moves_, 0), kind((size_t)G_ * max_moves_, 0),
        vt((size_t)G_ * max_moves_, 0.0f) {}
    ExampleTargetsMem tmem() { ExampleTargetsMem T; T.ep_end = ep_end.data(); T.vt = vt.data(); T.kind = kind.data(); return T; }
    void mark() { const ExamplesMem X = mem(); const ExampleTargetsMem T = tmem(); for (uint32_t g = 0; g < G; ++g) vt_mark_boundary(X, T, open_from.data(), g); }
    // tafl_examples_clear
    void clear() {
        std::fill(len.begin(), len.end(), 0u); memset(counters, 0, sizeof counters); std::fill(open_from.begin(), open_from.end(), 0u); std::fill(seen.begin(), seen.end(), 0u);
        std::fill(ep_end.begin(), ep_end.end(), (uint8_t)0); std::fill(vt.begin(), vt.end(), 0.0f); std::fill(kind.begin(), kind.end(), (uint8_t)0); valid = false;
    }
};
// tests/hostsim_search_stats' pool with the two per-slot arrays of tafl_pool_set_value_targets
struct PoolVHost {
    PoolSHost s;
    bool on = false;
    std::vector<float> vt; std::vector<uint8_t> kind;
    PoolVHost(uint32_t C, uint32_t Kp, uint8_t n) : s(C, Kp, n) {}
    int set_value_targets(bool enable) {
        if (s.w.pool.book.live != 0) return -1;
        if (!enable) { on = false; vt.clear(); kind.clear(); return 0; }
        if (!s.on) return -1;
        if (!on) { vt.assign(s.w.pool.M.C, 0.0f); kind.assign(s.w.pool.M.C, 0); on = true; }
        return 0;
    }
    // tafl_pool_ingest; with_targets 0 stands for an examples object created without TAFL_EXAMPLES_VALUE_TARGETS
    int ingest(ExVt* ex, int with_targets, uint64_t* out3) {
        if (on && !(with_targets && ex->valid)) return -1;
        const uint64_t written = s.w.pool.book.written;
        uint64_t o3[3];
        const int rc = s.ingest(ex, ex, o3);
        if (rc) return rc;
        if (out3) { out3[0] = o3[0]; out3[1] = o3[1]; out3[2] = o3[2]; }
        if (!on) return 0;
        const ExamplesMem X = ex->mem(); const ExampleTargetsMem T = ex->tmem();
        const uint32_t E = X.G * X.max_moves, Tn = (uint32_t)o3[0], C = s.w.pool.M.C, first = Tn - (Tn < C ? Tn : C);
        uint32_t r = 0, info;
        for (uint32_t e = 0; e < E; ++e) {
            if (pool_take(X, e, info) != POOL_TAKEN) continue;
            if (r >= first) { const uint32_t slot = pool_stored_slot(written, r - first, Tn, C); vt[slot] = T.vt[e]; kind[slot] = T.kind[e]; }
            ++r;
        }
        return 0;
    }
};
struct VtRun { void* h; ExVt* ex; };

extern "C" {
void* hvt_ex_new(uint32_t G, uint8_t n, uint32_t max_moves, uint32_t K) { return new ExVt(G, n, max_moves, K); }
void hvt_ex_free(void* h) { delete (ExVt*)h; }
void hvt_ex_clear(void* h) { ((ExVt*)h)->clear(); }
int hvt_ex_valid(void* h) { return ((ExVt*)h)->valid ? 1 : 0; }
// the object's ExStats (for the hqs_* and hss_* readers)
void* hvt_ex_stats(void* h) { return (ExStats*)(ExVt*)h; }
// hqs_begin recording into `ex` (an ExVt): the targets are stale from here on, and the boundary open_from names as the run begins is marked
void* hvt_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, const tafl_state* openings, uint32_t G, uint32_t n_sims, uint32_t edges_per_node,
                double c_puct, const tafl_root_noise* noise, const tafl_playout_cap* cap, const tafl_forced_playouts* fcfg, const tafl_solver* scfg, const tafl_selfplay_opts* o, uint32_t n_moves,
                uint64_t base, int episodes, uint64_t id_stride, uint32_t episode_moves, void* ex) {
    ExVt* x = (ExVt*)ex;
    if (!x) return nullptr;
    x->valid = false;
    x->mark();
    void* h = hqs_begin(r, n, word_bits, st, openings, G, n_sims, edges_per_node, c_puct, noise, cap, fcfg, scfg, o, n_moves, base, episodes, id_stride, episode_moves, (ExStats*)x);
    if (!h) return nullptr;
    x->mark();                                                  // (the first round, which the begin runs)
    return new VtRun{h, x};
}
void* hvt_run(void* run) { return ((VtRun*)run)->h; }
void hvt_free(void* run) { VtRun* s = (VtRun*)run; hqs_free(s->h); delete s; }
// one round and its recorder (hqs_step), then the boundary recorder for every lane
uint32_t hvt_step(void* run, const float* priors, const float* values) {
    VtRun* s = (VtRun*)run;
    const uint32_t w = hqs_step(s->h, priors, values);
    s->ex->valid = false;                                       // (every round of a run marks the targets stale)
    s->ex->mark();
    return w;
}
void hvt_ex_finalize(void* h, const tafl_state* st) { ExVt* x = (ExVt*)h; hqs_ex_finalize((ExStats*)x, st); x->valid = false; }
// tafl_examples_value_targets: -1 TAFL_ERR_INVALID_ARG, -5 TAFL_ERR_UNSUPPORTED; out4 = closed, unfinished, rows, settled
int hvt_value_targets(void* h, const tafl_value_targets_cfg* cfg, uint64_t* out4) {
    ExVt* x = (ExVt*)h;
    if (!cfg || !(cfg->lambda >= 0.0 && cfg->lambda <= 1.0)) return -1;
    if (cfg->flags & ~(uint32_t)TAFL_VT_SETTLE_UNFINISHED) return -5;
    for (uint32_t r : cfg->_reserved) if (r) return -5;
    const ExamplesMem X = x->mem(); const ExampleStatsMem S = x->smem(); const ExampleTargetsMem T = x->tmem();
    const uint32_t E = X.G * X.max_moves;
    for (uint32_t e = 0; e < E; ++e) vt_stage(X, S, T, e);
    uint64_t n[VT_COUNTERS] = {0, 0, 0, 0};
    for (uint32_t g = 0; g < X.G; ++g) {
        const uint32_t len = X.len[g] < X.max_moves ? X.len[g] : X.max_moves;
        VtChain c; memset(&c, 0, sizeof c); c.L = 1.0;
        for (uint32_t j = len; j-- > 0u;) {
            const uint32_t ev = vt_step(X, T, j, g, cfg->lambda, (cfg->flags & TAFL_VT_SETTLE_UNFINISHED) != 0u, c);
            n[VT_ROWS] += (ev & VT_EV_ROW) ? 1 : 0; n[VT_CLOSED] += (ev & VT_EV_CLOSED) ? 1 : 0; n[VT_UNFINISHED] += (ev & VT_EV_UNFINISHED) ? 1 : 0; n[VT_SETTLED] += (ev & VT_EV_SETTLED) ? 1 : 0;
        }
    }
    x->valid = true;
    if (out4) { out4[0] = n[VT_CLOSED]; out4[1] = n[VT_UNFINISHED]; out4[2] = n[VT_ROWS]; out4[3] = n[VT_SETTLED]; }
    return 0;
}
// tafl_examples_gather_targets: -1 for a stale result (when target or kind is asked for) and, strict (host pointers), for a bad index;
// otherwise zeros, counted; returns the rows so counted.  Any output may be null.
int hvt_gather_targets(void* h, const uint32_t* index, uint32_t count, float* target, uint8_t* kind, uint8_t* ep_end, int strict) {
    ExVt* x = (ExVt*)h;
    const ExamplesMem X = x->mem(); const ExampleTargetsMem T = x->tmem();
    if ((target || kind) && !x->valid) return -1;
    if (strict) for (uint32_t i = 0; i < count; ++i) { const uint32_t g = index[i] % X.G, j = index[i] / X.G; if (j >= X.max_moves || j >= X.len[g]) return -1; }
    int bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t e = index[i], g = e % X.G, j = e / X.G;
        const bool ok = j < X.max_moves && j < X.len[g];
        if (!ok) { x->counters[EX_BAD_INDEX] += 1; ++bad; }
        if (target) target[i] = ok ? T.vt[e] : 0.0f;
        if (kind) kind[i] = ok ? T.kind[e] : (uint8_t)0;
        if (ep_end) ep_end[i] = ok ? T.ep_end[e] : (uint8_t)0;
    }
    return bad;
}

void* hvt_pool_new(uint32_t C, uint32_t Kp, uint8_t n) { return (C == 0 || Kp == 0 || Kp > 0xFFFFu) ? nullptr : new PoolVHost(C, Kp, n); }
void hvt_pool_free(void* h) { delete (PoolVHost*)h; }
// the PoolSHost / PoolWHost inside, for the hqs_* and hspw_* calls that neither ingest nor change this setting
void* hvt_pool_stats(void* h) { return &((PoolVHost*)h)->s; }
void* hvt_pool_weights(void* h) { return &((PoolVHost*)h)->s.w; }
int hvt_pool_set_search_stats(void* h, int on) { PoolVHost* p = (PoolVHost*)h; const int rc = p->s.set_search_stats(on != 0); if (!rc && !on) { p->on = false; p->vt.clear(); p->kind.clear(); } return rc; }
int hvt_pool_set_value_targets(void* h, int on) { return ((PoolVHost*)h)->set_value_targets(on != 0); }
int hvt_pool_ingest(void* h, void* ex, int with_targets, uint64_t* out3) { return ((PoolVHost*)h)->ingest((ExVt*)ex, with_targets, out3); }
// tafl_pool_gather_targets: strict (host pointers) refuses a slot that is not live (-1); otherwise zeros, counted; returns the rows so counted
int hvt_pool_gather_targets(void* h, const uint32_t* slot, uint32_t count, float* target, uint8_t* kind, int strict) {
    PoolVHost* p = (PoolVHost*)h;
    if (!p->on) return -1;
    PoolWHost& w = p->s.w;
    const uint32_t f = w.first(), C = w.pool.M.C; const uint64_t live = w.pool.book.live;
    if (strict) for (uint32_t i = 0; i < count; ++i) if (!pool_slot_live_from(slot[i], f, live, C)) return -1;
    int bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const bool ok = pool_slot_live_from(slot[i], f, live, C);
        if (!ok) { w.pool.counters[POOL_BAD_SLOT] += 1; ++bad; }
        if (target) target[i] = ok ? p->vt[slot[i]] : 0.0f;
        if (kind) kind[i] = ok ? p->kind[slot[i]] : (uint8_t)0;
    }
    return bad;
}
}

#ifdef HVT_MAIN
// The stand-alone program of the sanitizer target: Brandubh, 8 lanes some plies into random games, constant priors, S = 16.  An episodes
// run that cuts after three moves records across reopens into a buffer of 6 examples per lane, which every lane fills (the budget is 12);
// a second run continues it.  The targets are computed, settled and gathered with indices beyond len and beyond the buffer; a pool of 5
// slots takes them three times, past the wrap, and is gathered with dead slots.
#include <stdio.h>
int main() {
    tafl_rules r; const uint32_t G = 8, A = 7 * 7 * 12, K = 24, MM = 6;
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
    tafl_selfplay_opts o; memset(&o, 0, sizeof o); o.sample_seed = 5; o.temp_moves = 4;
    void* ex = hvt_ex_new(G, 7, MM, K);
    uint32_t rounds = 0;
    for (int run = 0; run < 2; ++run) {
        void* h = hvt_begin(&r, 7, 64, st.data(), nullptr, G, 16, 128, 1.25, nullptr, nullptr, nullptr, nullptr, &o, 12, 100 + 1000 * run, 1, 0, 3, ex);
        if (!h) { printf("begin failed\n"); return 1; }
        uint32_t w = 1;
        while (w && rounds++ < 100000) w = hvt_step(h, pri.data(), val.data());
        hvt_free(h);
    }
    std::vector<uint32_t> len(G), index; uint64_t xc[EX_COUNTERS];
    hss_ex_counts(hvt_ex_stats(ex), len.data(), xc, nullptr);
    for (uint32_t g = 0; g < G; ++g) if (len[g] != MM) { printf("lane %u holds %u examples, not %u\n", g, len[g], MM); return 1; }
    for (uint32_t e = 0; e < G * MM + 9; ++e) index.push_back((e * 5u) % (G * MM + 9));
    std::vector<float> t(index.size()); std::vector<uint8_t> kd(index.size()), ee(index.size());
    if (hvt_gather_targets(ex, index.data(), (uint32_t)index.size(), t.data(), kd.data(), ee.data(), 0) != -1) { printf("a stale result was read\n"); return 1; }
    hvt_ex_finalize(ex, over.data());
    tafl_value_targets_cfg cfg; memset(&cfg, 0, sizeof cfg); cfg.lambda = 0.75;
    uint64_t o4[4], s4[4];
    if (hvt_value_targets(ex, &cfg, o4)) { printf("targets failed\n"); return 1; }
    cfg.flags = TAFL_VT_SETTLE_UNFINISHED;
    if (hvt_value_targets(ex, &cfg, s4)) { printf("targets failed\n"); return 1; }
    cfg.lambda = 1.5;
    if (hvt_value_targets(ex, &cfg, nullptr) != -1) { printf("lambda 1.5 was taken\n"); return 1; }
    if (hvt_gather_targets(ex, index.data(), (uint32_t)index.size(), t.data(), kd.data(), ee.data(), 1) != -1) { printf("strict gather took a bad index\n"); return 1; }
    const int bad = hvt_gather_targets(ex, index.data(), (uint32_t)index.size(), t.data(), kd.data(), ee.data(), 0);
    double acc = 0.0; uint32_t ends = 0;
    for (size_t i = 0; i < index.size(); ++i) { if (!(t[i] >= -1.0f && t[i] <= 1.0f) || kd[i] > 2) { printf("target out of range at %zu\n", i); return 1; } acc += t[i]; ends += ee[i]; }
    void* p = hvt_pool_new(5, K, 7);
    uint64_t o3[3] = {0, 0, 0};
    if (hvt_pool_set_value_targets(p, 1) != -1) { printf("the setting went on without the statistics\n"); return 1; }
    if (hvt_pool_set_search_stats(p, 1) || hvt_pool_set_value_targets(p, 1)) { printf("set failed\n"); return 1; }
    if (hvt_pool_ingest(p, ex, 0, o3) != -1) { printf("ingest of an object without the arrays\n"); return 1; }
    for (int i = 0; i < 3; ++i) if (hvt_pool_ingest(p, ex, 1, o3)) { printf("ingest failed\n"); return 1; }
    std::vector<uint32_t> slots; for (uint32_t k = 0; k < 25; ++k) slots.push_back(k);
    std::vector<float> pv(25); std::vector<uint8_t> pk(25);
    if (hvt_pool_gather_targets(p, slots.data(), 25, pv.data(), pk.data(), 1) != -1) { printf("strict gather took a dead slot\n"); return 1; }
    const int dead = hvt_pool_gather_targets(p, slots.data(), 25, pv.data(), pk.data(), 0);
    printf("rounds %u dropped %llu episodes closed %llu unfinished %llu rows %llu settled %llu boundaries %u bad indices %d taken %llu dead slots %d\nchecksum %.6f\n", rounds,
           (unsigned long long)xc[0], (unsigned long long)o4[0], (unsigned long long)o4[1], (unsigned long long)o4[2], (unsigned long long)s4[3], ends, bad, (unsigned long long)o3[0], dead, acc);
    hvt_pool_free(p);
    hvt_ex_free(ex);
    return 0;
}
#endif
