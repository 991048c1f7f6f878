// hostsim_pool_dedup.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  De-duplication of the training pool (include/taflhip.h
// tafl_pool_dedup / _gather_dedup / _weights_from_dedup) on the host, on top of tests/hostsim_pool's PoolHost and the weights of
// tests/hostsim_pool_weights: the per-item functions are the product's (tafl_pool.hpp: pooldd_row_key, pooldd_insert, pooldd_same,
// pooldd_zmean, pooldd_weight), the loops around them restate k_pooldd_key, k_pooldd_insert, k_pooldd_finish, k_pooldd_weights and
// k_pooldd_gather of tafl_pool.hip.  What the kernels leave to the hardware is a parameter here: the size of the table, the order in
// which the rows are inserted, and how many consecutive rows of that order are looked at together for runs of equal keys (a wave).
#include "../hostsim_pool_weights/hostsim_pool_weights.cpp"

struct PoolDDHost {
    PoolWHost w;
    bool valid = false, allocated = false;
    std::vector<uint32_t> rep, mult, ent;
    std::vector<float> zmean;
    std::vector<uint64_t> key;
    std::vector<uint8_t> canon;
    uint64_t res[PDD_WORDS] = {0}, live_at = 0;
    PoolDDHost(uint32_t C, uint32_t Kp, uint8_t n) : w(C, Kp, n) {}
    PoolHost& pool() { return w.pool; }
    void release() { rep.clear(); mult.clear(); ent.clear(); zmean.clear(); key.clear(); canon.clear(); valid = allocated = false; }
    // k_pooldd_key over the live rows
    void keys(uint32_t flags, uint32_t key_bits) {
        const PoolMem& M = pool().M;
        const uint32_t first = w.first();
        for (uint64_t a = 0; a < pool().book.live; ++a) {
            const uint32_t s = (uint32_t)((first + a) % M.C);
            uint32_t c;
            key[s] = pooldd_row_key(M.rows + (size_t)s * M.RW, pool().n, M.BW, (flags & 1u) != 0, key_bits, c);
            canon[s] = (uint8_t)c;
        }
    }
    // tafl_pool_dedup.  table_size 0: the product's; perm (may be NULL): the age ranks in the order of insertion; wave >= 1: the rows of
    // `wave` consecutive positions of that order are inserted run by run (equal keys in neighbouring positions join in one insert).
    int dedup(uint32_t flags, uint32_t key_bits, uint32_t table_size, const uint32_t* perm, uint32_t wave) {
        if ((flags & ~1u) || key_bits > 64u) return -5;
        if (pool().book.live == 0) return -1;
        const PoolMem& M = pool().M;
        const uint32_t live = (uint32_t)pool().book.live, first = w.first(), TS = table_size ? table_size : pooldd_table_size(live);
        if (TS < live || wave == 0) return -1;
        valid = false;
        if (!allocated) { rep.assign(M.C, 0xDEADBEEFu); mult.assign(M.C, 0xDEADBEEFu); ent.assign(M.C, 0xDEADBEEFu); zmean.assign(M.C, -7.0f); key.assign(M.C, 0); canon.assign(M.C, 0xAA); allocated = true; }
        keys(flags, key_bits);
        std::vector<uint64_t> table((pooldd_table_bytes(TS) + 7) / 8, 0);
        const PoolDedupTable T = pooldd_table(table.data(), TS);
        auto slot_of = [&](uint32_t a) { return (uint32_t)(((uint64_t)first + a) % M.C); };
        auto age_at = [&](uint32_t i) { return perm ? perm[i] : i; };
        for (uint32_t i0 = 0; i0 < live; i0 += wave)
            for (uint32_t i = i0; i < live && i < i0 + wave;) {
                const uint64_t k = key[slot_of(age_at(i))];
                uint32_t cnt = 0, wins = 0, losses = 0, newest = 0, j = i;
                for (; j < live && j < i0 + wave && key[slot_of(age_at(j))] == k; ++j) {
                    const float z = pool_row_z(M.rows + (size_t)slot_of(age_at(j)) * M.RW, M.BW);
                    cnt += 1; wins += z == 1.0f; losses += z == -1.0f; newest = age_at(j) > newest ? age_at(j) : newest;
                }
                const uint32_t e = pooldd_insert(T, k, cnt, wins, losses, newest);
                for (; i < j; ++i) ent[slot_of(age_at(i))] = e;
            }
        for (uint64_t& r : res) r = 0;
        for (uint32_t a = 0; a < live; ++a) {                                  // k_pooldd_finish
            const uint32_t s = slot_of(a), e = ent[s], r = slot_of(T.newest[e]), m = T.count[e];
            rep[s] = r; mult[s] = m; zmean[s] = pooldd_zmean(m, T.wins[e], T.losses[e]);
            if (r == s) res[PDD_DISTINCT] += 1;
            else if (!pooldd_same(M.rows + (size_t)s * M.RW, canon[s], M.rows + (size_t)r * M.RW, canon[r], pool().n, M.BW)) res[PDD_COLLISIONS] += 1;
            if (m > res[PDD_LARGEST]) res[PDD_LARGEST] = m;
        }
        live_at = live; valid = true;
        return 0;
    }
    uint64_t bytes() const { return allocated ? 25ull * w.pool.M.C + pooldd_table_bytes(pooldd_table_size(w.pool.M.C)) + 8ull * PDD_WORDS : 0ull; }
};

extern "C" {
void* hspd_new(uint32_t C, uint32_t Kp, uint8_t n) { return (C == 0 || Kp == 0 || Kp > 0xFFFFu) ? nullptr : new PoolDDHost(C, Kp, n); }
void hspd_free(void* h) { delete (PoolDDHost*)h; }
// the PoolWHost and the PoolHost inside, for the hspw_* and hsp_* calls of this library that do not change the live window
void* hspd_wpool(void* h) { return &((PoolDDHost*)h)->w; }
void* hspd_pool(void* h) { return &((PoolDDHost*)h)->w.pool; }
int hspd_ingest(void* h, void* ex, uint64_t* out3) { PoolDDHost* p = (PoolDDHost*)h; p->valid = false; return p->w.ingest((ExHost*)ex, out3); }
int hspd_trim(void* h, uint32_t keep) { PoolDDHost* p = (PoolDDHost*)h; if (keep) p->valid = false; return hspw_trim(&p->w, keep); }
void hspd_clear(void* h) { PoolDDHost* p = (PoolDDHost*)h; p->valid = false; hspw_clear(&p->w); }
void hspd_release(void* h) { ((PoolDDHost*)h)->release(); }
// out5 = live, distinct, largest, collisions, device_bytes
int hspd_dedup(void* h, uint32_t flags, uint32_t key_bits, uint32_t table_size, const uint32_t* perm, uint32_t wave, uint64_t* out5) {
    PoolDDHost* p = (PoolDDHost*)h;
    const int rc = p->dedup(flags, key_bits, table_size, perm, wave);
    if (rc == 0 && out5) { out5[0] = p->live_at; out5[1] = p->res[PDD_DISTINCT]; out5[2] = p->res[PDD_LARGEST]; out5[3] = p->res[PDD_COLLISIONS]; out5[4] = p->bytes(); }
    return rc;
}
// key[C], canon[C] as the last hspd_dedup left them (slots that were not live: whatever they held)
int hspd_keys(void* h, uint64_t* key, uint8_t* canon) {
    PoolDDHost* p = (PoolDDHost*)h;
    if (!p->valid) return -1;
    memcpy(key, p->key.data(), 8 * p->key.size()); memcpy(canon, p->canon.data(), p->canon.size());
    return 0;
}
// tafl_pool_gather_dedup: strict = host pointers (a slot that is not live: -1, nothing written), else zeros for such a slot, counted
int hspd_gather(void* h, const uint32_t* slot, uint32_t count, uint32_t* rep, uint32_t* mult, float* zmean, int strict) {
    PoolDDHost* p = (PoolDDHost*)h;
    if (!p->valid) return -1;
    const uint32_t first = p->w.first(), C = p->pool().M.C; const uint64_t live = p->pool().book.live;
    if (strict) for (uint32_t i = 0; i < count; ++i) if (!pool_slot_live_from(slot[i], first, live, C)) return -1;
    for (uint32_t i = 0; i < count; ++i) {
        const bool ok = pool_slot_live_from(slot[i], first, live, C);
        if (!ok) p->pool().counters[POOL_BAD_SLOT] += 1;
        if (rep) rep[i] = ok ? p->rep[slot[i]] : 0u;
        if (mult) mult[i] = ok ? p->mult[slot[i]] : 0u;
        if (zmean) zmean[i] = ok ? p->zmean[slot[i]] : 0.0f;
    }
    return 0;
}
// tafl_pool_weights_from_dedup
int hspd_weights(void* h, uint32_t scale, uint32_t flags) {
    PoolDDHost* p = (PoolDDHost*)h;
    if ((flags & ~3u) || flags == 3u) return -5;
    if (!p->w.on || !p->valid) return -1;
    const uint32_t first = p->w.first(), C = p->pool().M.C; const uint64_t live = p->pool().book.live;
    for (uint32_t s = 0; s < C; ++s)
        if (pool_slot_live_from(s, first, live, C)) p->w.wt[s] = pooldd_weight(p->w.wt[s], p->mult[s], p->rep[s] == s, scale, flags);
    p->w.dirty = true;
    return 0;
}
float hspd_zmean(uint32_t m, uint32_t wins, uint32_t losses) { return pooldd_zmean(m, wins, losses); }
uint32_t hspd_table_size(uint64_t live) { return pooldd_table_size(live); }
uint32_t hspd_sym_tile(uint32_t sym, uint32_t t, uint32_t n) { return sym_tile(sym, t, n); }
}

#ifdef HSPD_MAIN
// The stand-alone program of the sanitizer target.  Synthetic Brandubh examples as in hostsim_pool's program (lanes 3 * g plies into the
// game, so that neighbouring examples of a lane are copies of one position); a pool of 150 slots takes them until the ring wraps and is
// de-duplicated in every state - empty (refused), partly filled, wrapped, trimmed, cleared - with and without symmetries, with 5-bit keys,
// with the table at exactly `live` entries, in reverse order and in waves of 64, followed by gathers with dead slots and all weight rules.
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
        Ops<2, 7>::random_advance(s, 21, g, g % 4u, C, false);
        for (uint32_t j = 0; j < g % 6u; ++j) {
            const uint32_t m = 1u + (g + j) % 4u;
            example_append<2, 7>(X, g, s, 7, m, 5u * g, j, [&](auto put) { for (uint32_t k = 0; k < m; ++k) put(7u * k + g, k + 1u); });
        }
        const float z = (g % 5u == 0u) ? (float)TAFL_DRAW_VALUE : ((g & 1u) ? 1.0f : -1.0f);
        for (uint32_t j = 0; j < ex.len[g]; ++j) { ex.z[(size_t)j * G + g] = z; ex.fin[(size_t)j * G + g] = 1; }
    }
    uint64_t acc = 0, o3[3], o5[5];
    void* p = hspd_new(150, 6, 7);
    if (hspd_dedup(p, 0, 64, 0, nullptr, 1, o5) != -1) { printf("dedup of an empty pool\n"); return 1; }
    if (hspd_dedup(p, 2, 64, 0, nullptr, 1, o5) != -5 || hspd_dedup(p, 0, 65, 0, nullptr, 1, o5) != -5) { printf("bad cfg accepted\n"); return 1; }
    hspw_set_weighting(hspd_wpool(p), 1, 1000);
    std::vector<uint32_t> all(153), rep(153), mult(153), perm; std::vector<float> zm(153);
    for (uint32_t i = 0; i < 153; ++i) all[i] = i;
    for (int round = 0; round < 4; ++round) {
        if (round == 3) { if (hspd_trim(p, 1)) { printf("trim failed\n"); return 1; } }
        else if (hspd_ingest(p, &ex, o3)) { printf("ingest failed\n"); return 1; }
        if (hspd_gather(p, all.data(), 1, rep.data(), mult.data(), zm.data(), 0) != -1 || hspd_weights(p, 5, 0) != -1) { printf("a stale result was used\n"); return 1; }
        uint64_t s8[8]; hsp_stats(hspd_pool(p), s8);
        const uint32_t live = (uint32_t)s8[1];
        perm.resize(live); for (uint32_t i = 0; i < live; ++i) perm[i] = live - 1u - i;
        for (uint32_t flags = 0; flags < 2; ++flags)
            for (uint32_t bits : {64u, 0u, 5u})
                for (int how = 0; how < 4; ++how) {
                    if (hspd_dedup(p, flags, bits, how == 1 ? live : 0u, how == 2 ? perm.data() : nullptr, how == 3 ? 64u : 1u, o5)) { printf("dedup failed\n"); return 1; }
                    acc += o5[1] * 3u + o5[2] * 5u + o5[3] * 7u;
                }
        printf("round %d: live %llu distinct %llu largest %llu collisions (5 bits, symmetries) %llu\n", round, (unsigned long long)o5[0], (unsigned long long)o5[1], (unsigned long long)o5[2], (unsigned long long)o5[3]);
        if (hspd_gather(p, all.data(), 153, rep.data(), mult.data(), zm.data(), 1) != -1) { printf("strict gather took a dead slot\n"); return 1; }
        if (hspd_gather(p, all.data(), 153, rep.data(), mult.data(), zm.data(), 0)) { printf("gather failed\n"); return 1; }
        for (uint32_t i = 0; i < 153; ++i) acc += rep[i] + mult[i] + (uint64_t)(1000.0f * (zm[i] + 1.0f));
        for (uint32_t wf : {0u, 1u, 2u, 1u}) if (hspd_weights(p, wf == 0 ? 3u : 1000u, wf)) { printf("weights failed\n"); return 1; }
        if (hspd_weights(p, 1, 3) != -5) { printf("both weight flags accepted\n"); return 1; }
        std::vector<uint32_t> wt(150);
        if (hspw_raw_weights(hspd_wpool(p), wt.data())) { printf("no weights\n"); return 1; }
        for (uint32_t v : wt) acc += v;
    }
    hspd_clear(p);
    if (hspd_gather(p, all.data(), 1, rep.data(), mult.data(), zm.data(), 0) != -1 || hspd_dedup(p, 0, 64, 0, nullptr, 1, o5) != -1) { printf("a cleared pool was used\n"); return 1; }
    hspd_release(p);
    acc += (uint64_t)(1e6f * hspd_zmean(3, 1, 1)) + (uint64_t)(1e6f * hspd_zmean(1, 0, 0));
    hspd_free(p);
    printf("checksum %llu\n", (unsigned long long)acc);
    return 0;
}
#endif
