// hostsim_pool_weights.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  Weighted sampling of the training pool (include/taflhip.h
// tafl_pool_set_weighting / _set_weights / _sample_weighted) on the host, on top of tests/hostsim_pool's PoolHost: the per-item functions
// are the product's (tafl_pool.hpp: pool_eff, pool_wdraw, pool_wsearch_*, pool_wpick, pool_stored_slot), the loops around them restate
// the kernels of tafl_pool.hip - k_poolw_ingest, k_poolw_zero / k_poolw_max, k_poolw_tiles + k_poolw_scan (the tile structure) and
// k_poolw_draw, whose 64 lanes run one after the other here: a ballot is a loop that counts.
#include "../hostsim_pool/hostsim_pool.cpp"

struct PoolWHost {
    PoolHost pool;
    bool on = false, dirty = true;
    uint32_t ingest_weight = 0, NT = 0;
    uint64_t total = 0, positive = 0, bad_slot = 0, rebuilds = 0;
    std::vector<uint32_t> wt, tile_pos;
    std::vector<uint64_t> tile_sum, tile_pre;
    PoolWHost(uint32_t C, uint32_t Kp, uint8_t n) : pool(C, Kp, n) {}
    uint32_t first() const { return pool.book.live ? pool_first_live(pool.book.written, pool.book.live, pool.M.C) : 0u; }
    void set_weighting(bool enable, uint32_t w) {
        if (!enable) { on = false; wt.clear(); tile_pos.clear(); tile_sum.clear(); tile_pre.clear(); dirty = true; total = positive = bad_slot = rebuilds = 0; return; }
        if (!on) {
            NT = pool_weight_tiles(pool.M.C);
            wt.assign((size_t)NT * POOLW_TILE, w); tile_pos.assign(NT, 0); tile_sum.assign(NT, 0); tile_pre.assign(NT, 0);
            on = true; rebuilds = 0; bad_slot = 0;
        }
        ingest_weight = w; dirty = true;
    }
    int ingest(ExHost* ex, uint64_t* out3) {
        const uint64_t written = pool.book.written;
        uint64_t o3[3];
        const int rc = pool.ingest(ex, o3);
        if (rc) return rc;
        if (out3) { out3[0] = o3[0]; out3[1] = o3[1]; out3[2] = o3[2]; }
        if (on) {
            const uint32_t T = (uint32_t)o3[0], C = pool.M.C, stored = T < C ? T : C;
            for (uint32_t i = 0; i < stored; ++i) wt[pool_stored_slot(written, i, T, C)] = ingest_weight;
        }
        dirty = true;
        return 0;
    }
    // device-pointer semantics (strict = 0): dead slots are skipped and counted; host-pointer semantics (strict = 1): refused before a write
    int set_weights(const uint32_t* slot, const uint32_t* weight, uint32_t count, int strict) {
        if (!on) return -1;
        const uint32_t f = first(), C = pool.M.C; const uint64_t live = pool.book.live;
        if (strict) for (uint32_t i = 0; i < count; ++i) if (!pool_slot_live_from(slot[i], f, live, C)) return -1;
        for (uint32_t i = 0; i < count; ++i) { if (pool_slot_live_from(slot[i], f, live, C)) wt[slot[i]] = 0u; else bad_slot += 1; }
        for (uint32_t i = 0; i < count; ++i) if (pool_slot_live_from(slot[i], f, live, C) && weight[i] > wt[slot[i]]) wt[slot[i]] = weight[i];
        dirty = true;
        return 0;
    }
    void lane_eff(uint32_t t, uint32_t lane, uint32_t e[POOLW_PER_LANE]) const {
        const uint32_t s0 = t * (uint32_t)POOLW_TILE + lane * (uint32_t)POOLW_PER_LANE;
        for (uint32_t q = 0; q < POOLW_PER_LANE; ++q) e[q] = pool_eff(wt[s0 + q], s0 + q, first(), pool.book.live, pool.M.C);
    }
    void rebuild() {
        if (!dirty) return;
        for (uint32_t t = 0; t < NT; ++t) {
            uint64_t sum = 0; uint32_t pos = 0;
            for (uint32_t lane = 0; lane < POOLW_LANES; ++lane) { uint32_t e[POOLW_PER_LANE]; lane_eff(t, lane, e); for (uint32_t q = 0; q < POOLW_PER_LANE; ++q) { sum += e[q]; pos += e[q] != 0u; } }
            tile_sum[t] = sum; tile_pos[t] = pos;
        }
        uint64_t carry = 0, p = 0;
        for (uint32_t t = 0; t < NT; ++t) { tile_pre[t] = carry; carry += tile_sum[t]; p += tile_pos[t]; }
        total = carry; positive = p; rebuilds += 1; dirty = false;
    }
    // k_poolw_draw for one row
    void draw(uint64_t seed, uint64_t step, uint32_t row, uint32_t flags, uint32_t& slot, uint32_t& sym, uint32_t& weight, uint32_t& steps) const {
        uint64_t k;
        pool_wdraw(seed, step, row, total, flags, k, sym);
        uint32_t lo = 0, hi = NT;
        steps = 0;
        while (hi - lo > 1u) {
            uint32_t c = 0;
            for (uint32_t lane = 0; lane < POOLW_LANES; ++lane) { uint32_t idx; if (pool_wsearch_probe(lo, hi, lane, idx) && tile_pre[idx] <= k) ++c; }
            pool_wsearch_narrow(lo, hi, c);
            ++steps;
        }
        const uint64_t kk = k - tile_pre[lo];
        uint64_t excl[POOLW_LANES], run = 0; uint32_t e[POOLW_LANES][POOLW_PER_LANE], c = 0;
        for (uint32_t lane = 0; lane < POOLW_LANES; ++lane) { lane_eff(lo, lane, e[lane]); excl[lane] = run; run += (uint64_t)e[lane][0] + e[lane][1] + e[lane][2] + e[lane][3]; }
        for (uint32_t lane = 0; lane < POOLW_LANES; ++lane) c += excl[lane] <= kk;
        const uint32_t L = c ? c - 1u : 0u;
        const uint32_t j = pool_wpick(e[L][0], e[L][1], e[L][2], e[L][3], kk - excl[L], weight);
        slot = lo * (uint32_t)POOLW_TILE + L * (uint32_t)POOLW_PER_LANE + j;
    }
};

extern "C" {
void* hspw_new(uint32_t C, uint32_t Kp, uint8_t n) { return (C == 0 || Kp == 0 || Kp > 0xFFFFu) ? nullptr : new PoolWHost(C, Kp, n); }
void hspw_free(void* h) { delete (PoolWHost*)h; }
// the PoolHost inside, for the hsp_* calls of this library that do not change the live window (hsp_stats, hsp_gather, hsp_sample, ...)
void* hspw_pool(void* h) { return &((PoolWHost*)h)->pool; }
void hspw_set_weighting(void* h, int enable, uint32_t ingest_weight) { ((PoolWHost*)h)->set_weighting(enable != 0, ingest_weight); }
int hspw_ingest(void* h, void* ex, uint64_t* out3) { return ((PoolWHost*)h)->ingest((ExHost*)ex, out3); }
int hspw_trim(void* h, uint32_t keep) { PoolWHost* p = (PoolWHost*)h; p->dirty = true; return hsp_trim(&p->pool, keep); }
void hspw_clear(void* h) { PoolWHost* p = (PoolWHost*)h; hsp_clear(&p->pool); p->dirty = true; p->total = p->positive = p->bad_slot = p->rebuilds = 0; }
int hspw_set_weights(void* h, const uint32_t* slot, const uint32_t* weight, uint32_t count, int strict) { return ((PoolWHost*)h)->set_weights(slot, weight, count, strict); }
// every slot's stored weight, dead slots too: out[C]
int hspw_raw_weights(void* h, uint32_t* out) { PoolWHost* p = (PoolWHost*)h; if (!p->on) return -1; memcpy(out, p->wt.data(), 4 * (size_t)p->pool.M.C); return 0; }
// tafl_pool_get_weights with device pointers: 0 for a slot that is not live
int hspw_get_weights(void* h, const uint32_t* slot, uint32_t count, uint32_t* out) {
    PoolWHost* p = (PoolWHost*)h;
    if (!p->on) return -1;
    for (uint32_t i = 0; i < count; ++i) out[i] = pool_slot_live_from(slot[i], p->first(), p->pool.book.live, p->pool.M.C) ? p->wt[slot[i]] : 0u;
    return 0;
}
// out8 in the order of tafl_pool_weight_counters (device_bytes: the bytes of the vectors)
void hspw_stats(void* h, uint64_t* out8) {
    PoolWHost* p = (PoolWHost*)h;
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    if (!p->on) return;
    p->rebuild();
    out8[0] = 1; out8[1] = p->ingest_weight; out8[2] = p->total; out8[3] = p->positive; out8[4] = p->bad_slot; out8[5] = p->rebuilds;
    out8[6] = 4 * (uint64_t)p->wt.size() + 20 * (uint64_t)p->NT;
}
// the tile structure after a rebuild: tile_sum[NT], tile_pre[NT]; returns NT
uint32_t hspw_tiles(void* h, uint64_t* tile_sum, uint64_t* tile_pre) {
    PoolWHost* p = (PoolWHost*)h;
    if (!p->on) return 0;
    p->rebuild();
    if (tile_sum) memcpy(tile_sum, p->tile_sum.data(), 8 * (size_t)p->NT);
    if (tile_pre) memcpy(tile_pre, p->tile_pre.data(), 8 * (size_t)p->NT);
    return p->NT;
}
// tafl_pool_sample_weighted, the draw alone: -1 where the call fails with TAFL_ERR_INVALID_ARG, -5 TAFL_ERR_UNSUPPORTED.  out_steps (may be
// NULL): the probe steps of the tile search of each row.
int hspw_draw(void* h, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t count, uint32_t flags, uint32_t* out_slot, uint8_t* out_sym, uint32_t* out_weight,
              uint64_t* out_total, uint32_t* out_steps) {
    PoolWHost* p = (PoolWHost*)h;
    if (flags & ~1u) return -5;
    if (!p->on || (uint64_t)row_base + count > 0xFFFFFFFFull || p->pool.book.live == 0) return -1;
    p->rebuild();
    if (p->total == 0) return -1;
    if (out_total) *out_total = p->total;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t slot, sym, w, steps;
        p->draw(seed, step, row_base + i, flags, slot, sym, w, steps);
        out_slot[i] = slot; out_sym[i] = (uint8_t)sym; out_weight[i] = w;
        if (out_steps) out_steps[i] = steps;
    }
    return 0;
}
uint64_t hspw_mulhi64(uint64_t a, uint64_t b) { return pool_mulhi64(a, b); }
}

#ifdef HSPW_MAIN
// The stand-alone program of the sanitizer target.  Synthetic Brandubh examples as in hostsim_pool's program; a pool of 700 slots (three
// tiles, the last one partial) takes them until the ring wraps, with weighting switched on in between, weights set with duplicates and
// dead slots, a trim, draws in every state, and a pool of one slot.  Prints what it counted.
#include <stdio.h>
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_host.hpp"
int main() {
    tafl_rules r; const uint32_t G = 40;
    if (preset_rules("brandubh", &r)) { printf("no preset\n"); return 1; }
    Consts<2> C; if (make_consts<2, 7>(r, 7, C)) { printf("no consts\n"); return 1; }
    ExHost ex(G, 7, 5, 4);
    ExamplesMem X = ex.mem();
    for (uint32_t g = 0; g < G; ++g) {
        tafl_state st;
        if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st, nullptr)) { printf("bad fen\n"); return 1; }
        DState<2> s; state_from_abi<2>(st, s);
        Ops<2, 7>::random_advance(s, 21, g, 3 * g, C, false);
        for (uint32_t j = 0; j < g % 6u; ++j) {
            const uint32_t m = 1u + (g + j) % 4u;
            example_append<2, 7>(X, g, s, 7, m, 5u * g, j, [&](auto put) { for (uint32_t k = 0; k < m; ++k) put(7u * k + g, k + 1u); });
        }
        for (uint32_t j = 0; j < ex.len[g]; ++j) { ex.z[(size_t)j * G + g] = (g & 1u) ? 1.0f : -1.0f; ex.fin[(size_t)j * G + g] = 1; }
    }
    uint64_t acc = 0, o3[3], s8[8], total = 0;
    const uint32_t count = 2000;
    std::vector<uint32_t> slot(count), w(count), steps(count); std::vector<uint8_t> sym(count);
    for (uint32_t Cp : {700u, 1u}) {
        void* p = hspw_new(Cp, 6, 7);
        if (hspw_draw(p, 1, 2, 0, 4, 1, slot.data(), sym.data(), w.data(), &total, nullptr) != -1) { printf("draw with weighting off\n"); return 1; }
        if (hspw_ingest(p, &ex, o3)) { printf("ingest failed\n"); return 1; }
        hspw_set_weighting(p, 1, 0xFFFFFFFFu);
        for (int i = 0; i < 9; ++i) {
            if (i == 4) hspw_set_weighting(p, 1, 3);
            if (hspw_ingest(p, &ex, o3)) { printf("ingest failed\n"); return 1; }
            if (hspw_draw(p, 5, i, 7, count, 1, slot.data(), sym.data(), w.data(), &total, steps.data())) { printf("draw failed\n"); return 1; }
            for (uint32_t k = 0; k < count; ++k) acc += slot[k] + w[k] + sym[k] + steps[k];
        }
        std::vector<uint32_t> named, given;
        for (uint32_t k = 0; k < 2u * Cp + 5u; ++k) { named.push_back((k * 7u) % (Cp + 3u)); given.push_back(k % 3u ? k * 2654435761u : 0u); }        // (dead slots among them)
        if (hspw_set_weights(p, named.data(), given.data(), (uint32_t)named.size(), 1) != -1) { printf("strict set_weights took a dead slot\n"); return 1; }
        if (hspw_set_weights(p, named.data(), given.data(), (uint32_t)named.size(), 0)) { printf("set_weights failed\n"); return 1; }
        if (hspw_trim(p, 2)) { printf("trim failed\n"); return 1; }
        if (hspw_draw(p, 6, 1, 0xFFFFFFFFu - count, count, 0, slot.data(), sym.data(), w.data(), &total, steps.data())) { printf("draw failed\n"); return 1; }
        for (uint32_t k = 0; k < count; ++k) acc += slot[k] + w[k] + steps[k];
        if (hspw_get_weights(p, named.data(), (uint32_t)named.size(), given.data())) { printf("get_weights failed\n"); return 1; }
        hspw_stats(p, s8);
        printf("C %u: total %llu positive %llu bad_slot %llu rebuilds %llu\n", Cp, (unsigned long long)s8[2], (unsigned long long)s8[3], (unsigned long long)s8[4], (unsigned long long)s8[5]);
        hspw_clear(p);
        if (hspw_draw(p, 1, 2, 0, 4, 1, slot.data(), sym.data(), w.data(), &total, nullptr) != -1) { printf("draw from an empty pool\n"); return 1; }
        hspw_set_weighting(p, 0, 0);
        hspw_free(p);
    }
    printf("checksum %llu\n", (unsigned long long)acc);
    return 0;
}
#endif
