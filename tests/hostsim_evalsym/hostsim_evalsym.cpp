// hostsim_evalsym.cpp — TEST HARNESS ONLY (see ../hostsim/hostsim.cpp).  Evaluation under a random board symmetry (include/taflhip.h
// tafl_eval_symmetry) on the host: the product's draw on arbitrary states (Guided::leaf_symmetry) and the lock-step guided search
// (k_gmcts_step_sym or k_gmcts_step / k_gmcts_leaves / k_gmcts_leaf_symmetry) with the setting on or off, one game after the other
// around the product's per-game functions of tafl_guided.hpp.  Everything here is integer or float64 arithmetic in a fixed order:
// comparable bit for bit with the oracle and with the device.
#include "../hostsim/hostsim_common.hpp"
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_host.hpp"

struct SymBase : GuidedCounts {
    virtual ~SymBase() {}
    virtual uint32_t step(const float* priors, const float* values) = 0;
    virtual void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) = 0;
    virtual void leaf_symmetry(uint8_t* out) = 0;
    virtual void root_children(tafl_root_child* out, uint32_t max_children, uint32_t* out_n) = 0;
};
// cfg == NULL: the setting off (GuidedMem::sym stays null, as in every other harness)
template <int NL, int W>
struct SymSession : SymBase {
    using GD = Guided<NL, W>;
    using IO = StateIO<NL>;
    GuidedArena<NL, W> R; std::vector<uint8_t> sym; uint32_t n_sims; double c_puct;
    void latch(const tafl_eval_symmetry* cfg, uint32_t G, uint8_t side) {
        if (!cfg) return;
        sym.assign(G, 0);
        R.M.sym = sym.data(); R.M.sym_seed = cfg->seed; R.M.sym_gid = cfg->game_id_base; R.M.sym_n = side;
    }
    int init(const tafl_rules* r, uint8_t side, const tafl_state* st, uint32_t G, uint32_t sims_, uint32_t edges_per_node, double cp, const tafl_eval_symmetry* cfg) {
        if (R.init(r, side, G, sims_, edges_per_node)) return -1;
        n_sims = sims_; c_puct = cp;
        latch(cfg, G, side);
        for (uint32_t g = 0; g < G; ++g) { DState<NL> s; state_from_abi<NL>(st[g], s); GD::init_game(R.M, g, s); }
        return 0;
    }
    uint32_t step(const float* priors, const float* values) override {
        // k_gmcts_step_sym<NL, W, false> with the setting on, k_gmcts_step<NL, W> with it off
        return R.round(priors, values, *this, [&](uint32_t g, const float* pr, float v, GuidedStats& gs) {
            if (R.M.sym) GD::template step_as<false, false, false, true>(R.M, g, pr, v, R.A, c_puct, n_sims, R.C, gs, nullptr);
            else GD::step(R.M, g, pr, v, R.A, c_puct, n_sims, R.C, gs);
        });
    }
    // k_gmcts_leaves: the arena's rows, a waiting leaf's bytes moved to the tiles its symmetry sends them to
    void leaves(uint8_t* boards, uint8_t* sides, uint8_t* waiting) override {
        R.leaves(boards, sides, waiting);
        if (!R.M.sym) return;
        const uint32_t nn = R.n * R.n;
        std::vector<uint8_t> row(nn);
        for (uint32_t g = 0; g < R.M.G; ++g) {
            if (R.M.kind[g] != 1) continue;
            uint8_t* b = boards + (size_t)g * nn;
            memcpy(row.data(), b, nn);
            for (uint32_t t = 0; t < nn; ++t) b[sym_tile(R.M.sym[g], t, R.n)] = row[t];
        }
    }
    // k_gmcts_leaf_symmetry
    void leaf_symmetry(uint8_t* out) override {
        for (uint32_t g = 0; g < R.M.G; ++g) out[g] = (R.M.sym && R.M.kind[g] == 1) ? R.M.sym[g] : (uint8_t)0;
    }
    void root_children(tafl_root_child* out, uint32_t max_children, uint32_t* out_n) override {
        for (uint32_t g = 0; g < R.M.G; ++g) out_n[g] = GD::root_children(R.M, g, out + (size_t)g * max_children, max_children);
    }
    // the product's draw for G arbitrary states, each as the leaf of game g that starts to wait
    static int draw(uint8_t side, const tafl_state* st, uint32_t G, const tafl_eval_symmetry* cfg, uint8_t* out) {
        GuidedMem M; M.G = G; M.sym = out; M.sym_seed = cfg->seed; M.sym_gid = cfg->game_id_base; M.sym_n = side;
        for (uint32_t g = 0; g < G; ++g) { DState<NL> s; state_from_abi<NL>(st[g], s); GD::leaf_symmetry(M, g, s); }
        return 0;
    }
};

extern "C" {
void* hse_begin(const tafl_rules* r, uint8_t n, uint32_t word_bits, const tafl_state* st, uint32_t G, uint32_t n_sims, uint32_t edges_per_node, double c_puct,
                const tafl_eval_symmetry* cfg) {
    SymBase* s = nullptr; int rc = -2;
    if (word_bits == 64) { auto* p = new SymSession<2, 7>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, cfg); s = p; }
    else if (word_bits == 128) { auto* p = new SymSession<4, 11>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, cfg); s = p; }
    else if (word_bits == 256) { auto* p = new SymSession<8, 15>(); rc = p->init(r, n, st, G, n_sims, edges_per_node, c_puct, cfg); s = p; }
    if (rc) { delete s; return nullptr; }
    return s;
}
void hse_free(void* h) { delete (SymBase*)h; }
uint32_t hse_step(void* h, const float* priors, const float* values) { return ((SymBase*)h)->step(priors, values); }
void hse_leaves(void* h, uint8_t* boards, uint8_t* sides, uint8_t* waiting) { ((SymBase*)h)->leaves(boards, sides, waiting); }
void hse_leaf_symmetry(void* h, uint8_t* out) { ((SymBase*)h)->leaf_symmetry(out); }
void hse_root_children(void* h, tafl_root_child* out, uint32_t max_children, uint32_t* out_n) { ((SymBase*)h)->root_children(out, max_children, out_n); }
// out4 = sims, predicts, terminal hits, faults
void hse_counts(void* h, uint64_t* out4) { SymBase* s = (SymBase*)h; out4[0] = s->sims; out4[1] = s->predicts; out4[2] = s->terminal_hits; out4[3] = s->faults; }
int hse_draw(uint8_t n, uint32_t word_bits, const tafl_state* st, uint32_t G, const tafl_eval_symmetry* cfg, uint8_t* out) {
    switch (word_bits) {
        case 64:  return SymSession<2, 7>::draw(n, st, G, cfg, out);
        case 128: return SymSession<4, 11>::draw(n, st, G, cfg, out);
        case 256: return SymSession<8, 15>::draw(n, st, G, cfg, out);
        default:  return -2;
    }
}
}

#ifdef HSE_MAIN
// the stand-alone program of the sanitizer target: Brandubh start positions, priors that differ per action (so that a wrong permuted
// index matters), a search with the setting off and one with it on; prints a checksum so that nothing is optimised away
#include <stdio.h>
int main() {
    tafl_rules r; tafl_state st[3];
    if (preset_rules("brandubh", &r)) { printf("no preset\n"); return 1; }
    for (int g = 0; g < 3; ++g) if (fen_to_state(preset_board("brandubh"), r.starting_side, 64, &st[g], nullptr)) { printf("bad fen\n"); return 1; }
    const uint32_t A = 7 * 7 * 12;
    std::vector<float> pri((size_t)3 * A), val(3, 0.25f);
    for (size_t i = 0; i < pri.size(); ++i) pri[i] = (float)(1u + (i * 2654435761u) % 97u);
    tafl_eval_symmetry cfg; memset(&cfg, 0, sizeof cfg); cfg.seed = 11; cfg.game_id_base = 40;
    double acc = 0.0;
    for (const tafl_eval_symmetry* c : {(const tafl_eval_symmetry*)nullptr, (const tafl_eval_symmetry*)&cfg}) {
        void* h = hse_begin(&r, 7, 64, st, 3, 24, 128, 1.25, c);
        if (!h) { printf("begin failed\n"); return 1; }
        uint32_t w = hse_step(h, nullptr, nullptr), rounds = 0;
        std::vector<uint8_t> boards(3 * 49), sides(3), waiting(3), sym(3);
        while (w && rounds++ < 200) {
            hse_leaves(h, boards.data(), sides.data(), waiting.data()); hse_leaf_symmetry(h, sym.data());
            for (uint8_t v : boards) acc += v;
            for (uint8_t v : sym) acc += v;
            w = hse_step(h, pri.data(), val.data());
        }
        std::vector<tafl_root_child> kids(3 * 128); uint32_t cnt[3];
        hse_root_children(h, kids.data(), 128, cnt);
        for (int g = 0; g < 3; ++g) for (uint32_t j = 0; j < cnt[g]; ++j) acc += kids[g * 128 + j].q * kids[g * 128 + j].visits;
        hse_free(h);
    }
    uint8_t s3[3];
    if (hse_draw(7, 64, st, 3, &cfg, s3)) return 1;
    printf("checksum %.6f draws %u %u %u\n", acc, s3[0], s3[1], s3[2]);
    return 0;
}
#endif
