// hostsim_pool.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  The training pool (include/taflhip.h tafl_pool_*) on the host: the
// per-example, per-row and per-draw functions and the bookkeeping are the product's (tafl_pool.hpp), the loops around them restate
// k_pool_count / k_pool_scan / k_pool_copy (one serial pass that counts, one that ranks and stores) and k_pool_rows (one row after the
// other).  The examples come from tests/hostsim's buffer (ExHost, hostsim_common.hpp), filled by hsx_record + hsx_finalize.
#include "../hostsim/hostsim_common.hpp"
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_pool.hpp"

struct PoolHost {
    uint32_t n;
    PoolMem M; PoolBook book;
    uint64_t skipped_open = 0, skipped_overflow = 0;
    unsigned long long counters[POOL_COUNTERS] = {0};
    std::vector<uint32_t> rows;
    // every row is filled with a pattern no ingest writes
    PoolHost(uint32_t C, uint32_t Kp, uint8_t n_) : n(n_) {
        M.C = C; M.Kp = Kp; M.BW = ((uint32_t)n_ * n_ + 3u) / 4u; M.RW = pool_row_words(M.BW, Kp);
        rows.assign((size_t)C * M.RW, 0xDEADBEEFu);
        M.rows = rows.data(); M.counters = counters;
    }
    // tafl_pool_ingest: the count pass, then the ranks in ascending order of e and the rows of the examples that are placed
    int ingest(ExHost* ex, uint64_t* out3) {
        if (ex->n != n || ex->K > M.Kp) return -1;
        const ExamplesMem X = ex->mem();
        const uint32_t E = X.G * X.max_moves, generation = (uint32_t)(book.ingests + 1);
        uint32_t T = 0, open = 0, over = 0, info;
        for (uint32_t e = 0; e < E; ++e) { const uint32_t cls = pool_take(X, e, info); T += cls == POOL_TAKEN; open += cls == POOL_OPEN; over += cls == POOL_OVERFLOW; }
        uint32_t r = 0;
        for (uint32_t e = 0; e < E; ++e) {
            if (pool_take(X, e, info) != POOL_TAKEN) continue;
            uint32_t slot;
            if (pool_place(book.written, r, T, M.C, slot))
                for (uint32_t w = 0; w < M.RW; ++w) M.rows[(size_t)slot * M.RW + w] = pool_row_word(X, e / X.G, e % X.G, info, w, generation);
            ++r;
        }
        book.took(T, M.C); skipped_open += open; skipped_overflow += over;
        if (out3) { out3[0] = T; out3[1] = open; out3[2] = over; }
        return 0;
    }
    // k_pool_rows, one row after the other, with the semantics of device pointers: a slot that is not live gives an all-zero row and counts
    void out_rows(bool draw, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t flags, const uint32_t* slot_in, const uint8_t* sym_in, uint32_t count,
                  uint8_t* boards, uint8_t* sides, float* pi, float* z, uint32_t* out_slot, uint8_t* out_sym) {
        const uint32_t nn = n * n, A = nn * 2u * (n - 1u);
        for (uint32_t i = 0; i < count; ++i) {
            uint32_t slot, s;
            if (draw) pool_draw(seed, step, row_base + i, book.written, book.live, M.C, flags, slot, s);
            else { slot = slot_in[i]; s = sym_in ? (sym_in[i] & 7u) : 0u; }
            const bool ok = draw || pool_slot_live(slot, book.written, book.live, M.C);
            const uint32_t* row = M.rows + (size_t)(ok ? slot : 0u) * M.RW;
            const uint32_t nc = ok ? pool_row_children(row, M.BW) : 0u;
            if (pi) {
                float* dst = pi + (size_t)i * A;
                for (uint32_t a = 0; a < A; ++a) dst[a] = 0.0f;
                for (uint32_t k = 0; k < nc; ++k) { uint32_t a; const float p = pool_out_pi(row, M.BW, k, n, s, a); dst[a] = p; }
            }
            if (boards) for (uint32_t t = 0; t < nn; ++t) { uint32_t dst; const uint8_t v = pool_out_tile(row, t, n, s, dst); boards[(size_t)i * nn + dst] = ok ? v : (uint8_t)0; }
            if (!ok) counters[POOL_BAD_SLOT] += 1;
            if (sides) sides[i] = ok ? pool_row_side(row, M.BW) : (uint8_t)0;
            if (z) z[i] = ok ? pool_row_z(row, M.BW) : 0.0f;
            if (out_slot) out_slot[i] = slot;
            if (out_sym) out_sym[i] = (uint8_t)s;
        }
    }
};

extern "C" {
void* hsp_new(uint32_t C, uint32_t Kp, uint8_t n) { return (C == 0 || Kp == 0 || Kp > 0xFFFFu) ? nullptr : new PoolHost(C, Kp, n); }
void hsp_free(void* h) { delete (PoolHost*)h; }
void hsp_clear(void* h) { PoolHost* p = (PoolHost*)h; p->book.clear(); p->skipped_open = p->skipped_overflow = 0; p->counters[POOL_BAD_SLOT] = 0; }
// `ex`: an ExHost of tests/hostsim (hsx_new); out3 (may be NULL) = taken, skipped open, skipped overflow of this call
int hsp_ingest(void* h, void* ex, uint64_t* out3) { return ((PoolHost*)h)->ingest((ExHost*)ex, out3); }
int hsp_trim(void* h, uint32_t keep) { if (keep == 0) return -1; ((PoolHost*)h)->book.trim(keep); return 0; }
// out8 in the order of tafl_pool_stats, device_bytes = the bytes of the rows
void hsp_stats(void* h, uint64_t* out8) {
    PoolHost* p = (PoolHost*)h;
    out8[0] = p->book.written; out8[1] = p->book.live; out8[2] = p->book.ingests; out8[3] = p->book.oldest_generation();
    out8[4] = p->skipped_open; out8[5] = p->skipped_overflow; out8[6] = p->counters[POOL_BAD_SLOT]; out8[7] = 4 * (uint64_t)p->rows.size();
}
uint32_t hsp_row_words(void* h) { return ((PoolHost*)h)->M.RW; }
// the raw words of every slot, [C * row_words]
void hsp_rows(void* h, uint32_t* out) { PoolHost* p = (PoolHost*)h; memcpy(out, p->rows.data(), 4 * p->rows.size()); }
// tafl_pool_read
int hsp_read(void* h, const uint32_t* slot, uint32_t count, uint32_t* n_children, uint32_t* move_no, uint32_t* generation, uint32_t* actions, uint32_t* visits) {
    PoolHost* p = (PoolHost*)h; const PoolMem& M = p->M;
    for (uint32_t i = 0; i < count; ++i) if (!pool_slot_live(slot[i], p->book.written, p->book.live, M.C)) return -1;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t* row = M.rows + (size_t)slot[i] * M.RW;
        n_children[i] = pool_row_children(row, M.BW); move_no[i] = row[M.BW + PR_MOVE_NO]; generation[i] = row[M.BW + PR_GENERATION];
        for (uint32_t k = 0; k < M.Kp; ++k) { const uint32_t w = row[M.BW + PR_HEAD + k]; actions[(size_t)i * M.Kp + k] = w & 0xFFFFu; visits[(size_t)i * M.Kp + k] = w >> 16; }
    }
    return 0;
}
// pool_draw for the rows row_base .. row_base + count of a pool in the state (written, live, C)
void hsp_draw(uint64_t seed, uint64_t step, uint32_t row_base, uint32_t count, uint32_t flags, uint64_t written, uint64_t live, uint32_t C, uint32_t* out_slot, uint8_t* out_sym) {
    for (uint32_t i = 0; i < count; ++i) { uint32_t slot, sym; pool_draw(seed, step, row_base + i, written, live, C, flags, slot, sym); out_slot[i] = slot; out_sym[i] = (uint8_t)sym; }
}
// tafl_pool_sample: -1 where the call fails with TAFL_ERR_INVALID_ARG, -5 TAFL_ERR_UNSUPPORTED
int hsp_sample(void* h, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t count, uint32_t flags, uint8_t* boards, uint8_t* sides, float* pi, float* z,
               uint32_t* out_slot, uint8_t* out_sym) {
    PoolHost* p = (PoolHost*)h;
    if (flags & ~1u) return -5;
    if ((uint64_t)row_base + count > 0xFFFFFFFFull || p->book.live == 0) return -1;
    p->out_rows(true, seed, step, row_base, flags, nullptr, nullptr, count, boards, sides, pi, z, out_slot, out_sym);
    return 0;
}
// tafl_pool_gather with device pointers: returns the rows whose slot was not live (they are all zero)
uint32_t hsp_gather(void* h, const uint32_t* slot, const uint8_t* sym, uint32_t count, uint8_t* boards, uint8_t* sides, float* pi, float* z) {
    PoolHost* p = (PoolHost*)h;
    const unsigned long long before = p->counters[POOL_BAD_SLOT];
    p->out_rows(false, 0, 0, 0, 0, slot, sym, count, boards, sides, pi, z, nullptr, nullptr);
    return (uint32_t)(p->counters[POOL_BAD_SLOT] - before);
}
}

#ifdef HSP_MAIN
// The stand-alone program of the sanitizer target.  Brandubh positions some random plies into the game are recorded with example_append
// (synthetic visit counts: some lanes overflow K = 4, lanes hold 0..5 examples, a third of the lanes stay open); a pool of 50 rows with
// 6 policy entries takes them three times (the ring wraps, the third time T exceeds what is left), is trimmed, sampled under symmetries
// and gathered under all eight, dead slots included.  Prints what it counted.
#include <stdio.h>
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_host.hpp"
int main() {
    tafl_rules r; const uint32_t G = 40, A = 7 * 7 * 12;
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
            const uint32_t m = 1u + (g + j) % 6u;
            example_append<2, 7>(X, g, s, 7, m, 5u * g, j, [&](auto put) { for (uint32_t k = 0; k < m; ++k) put(7u * k + g, k + 1u); });
        }
        const float z = (g % 3u) ? ((g & 1u) ? 1.0f : -1.0f) : 0.0f;
        for (uint32_t j = 0; j < ex.len[g]; ++j) { ex.z[(size_t)j * G + g] = z; ex.fin[(size_t)j * G + g] = (g % 3u) ? 1 : 0; }
    }
    void* p = hsp_new(50, 6, 7);
    uint64_t o3[3], s8[8], acc = 0;
    for (int i = 0; i < 3; ++i) {
        if (hsp_ingest(p, &ex, o3)) { printf("ingest failed\n"); return 1; }
        hsp_stats(p, s8);
        printf("ingest %d: taken %llu open %llu overflow %llu written %llu live %llu oldest generation %llu\n", i + 1, (unsigned long long)o3[0], (unsigned long long)o3[1],
               (unsigned long long)o3[2], (unsigned long long)s8[0], (unsigned long long)s8[1], (unsigned long long)s8[3]);
    }
    if (hsp_trim(p, 1) || hsp_trim(p, 0) != -1) { printf("trim\n"); return 1; }
    hsp_stats(p, s8);
    const uint32_t count = 300;
    std::vector<uint8_t> boards((size_t)count * 49), sides(count), sym(count); std::vector<float> pi((size_t)count * A), z(count); std::vector<uint32_t> slot(count);
    if (hsp_sample(p, 3, 9, 17, count, 1, boards.data(), sides.data(), pi.data(), z.data(), slot.data(), sym.data())) { printf("sample failed\n"); return 1; }
    for (uint32_t i = 0; i < count; ++i) acc += slot[i] + 64u * sym[i] + boards[(size_t)i * 49 + 24];
    uint32_t bad = 0;
    for (uint32_t k = 0; k < 8; ++k) {
        std::vector<uint32_t> all(50); std::vector<uint8_t> sy(50, (uint8_t)k);
        for (uint32_t i = 0; i < 50; ++i) all[i] = i + (k == 7 ? 1u : 0u);                  // (the last pass names slot 50, which does not exist)
        bad += hsp_gather(p, all.data(), sy.data(), 50, boards.data(), sides.data(), pi.data(), z.data());
        for (uint32_t i = 0; i < 50; ++i) acc += sides[i] + (uint64_t)(1000.0f * pi[(size_t)i * A + (7u * 0u + i % G)]);
    }
    std::vector<uint32_t> nc(1), mv(1), gen(1), ac(6), vi(6);
    if (hsp_read(p, &slot[0], 1, nc.data(), mv.data(), gen.data(), ac.data(), vi.data())) { printf("read failed\n"); return 1; }
    printf("after trim(1): live %llu oldest generation %llu; dead rows gathered %u; row of slot %u: %u children, move %u, generation %u\n", (unsigned long long)s8[1],
           (unsigned long long)s8[3], bad, slot[0], nc[0], mv[0], gen[0]);
    printf("checksum %llu\n", (unsigned long long)acc);
    hsp_free(p);
    return 0;
}
#endif
