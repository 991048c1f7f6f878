// tafl_gmcts_sym.hip — the guided rounds under a random board symmetry per leaf evaluation (include/taflhip.h tafl_eval_symmetry, DESIGN.md
// section 22): the SYM instantiations of Guided::step_as / selfplay_step_as / selfplay_reopen (tafl_guided.hpp) as kernels of their own,
// so that the kernels of tafl_gmcts.hip stay as they are, in a translation unit of its own, so that the two compile side by side.
// tafl_gmcts_step and gselfplay_launch (tafl_gmcts.hip) come here when the open search or run latched the setting.
#include "tafl_internal.hpp"

// k_gmcts_step, without and with root noise (nz is read by the NOISE instantiations alone; nz.gid holds the game id base)
template <int NL, int W, bool NOISE>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gmcts_step_sym(Consts<NL> C, GuidedMem M, const float* priors, const float* values, uint32_t A, double c_puct,
                                                               uint32_t n_sims, unsigned long long* stats, RootNoise nz) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    nz.gid += g;
    Guided<NL, W>::template step_as<NOISE, false, false, true>(M, g, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct, n_sims, C, gs,
                                                                 NOISE ? &nz : nullptr);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// the rounds of a guided self-play run: FAMILY names the kernel of tafl_gmcts.hip it stands for - k_gselfplay_step / _episodes (plain),
// _capped, _forced (through the capped path), _solver (through both) - and every argument is read by the instantiations that kernel
// reads it in
enum { SYM_PLAIN = 0, SYM_CAPPED, SYM_FORCED, SYM_SOLVER };
template <int NL, int W, int FAMILY, bool NOISE, bool EPISODES>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_sym(Consts<NL> C, GuidedMem M, Quad* soa, const float* priors, const float* values, uint32_t A, double c_puct,
                                                              uint32_t n_sims, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats, RootNoise nz, PlayoutCap pc,
                                                              ForcedPlayouts fp, SolverCfg sv) {
    constexpr bool CAP = FAMILY >= SYM_CAPPED, FORCED = FAMILY >= SYM_FORCED, SOLVER = FAMILY == SYM_SOLVER;
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    GuidedStats gs; gs.sims = gs.predicts = gs.terminal_hits = gs.faults = gs.depth = 0;
    Guided<NL, W>::template selfplay_step_as<NOISE, EPISODES, CAP, FORCED, SOLVER, true>(M, g, soa, priors ? priors + (size_t)g * A : nullptr, values ? values[g] : 0.f, A, c_puct,
                                                                                         n_sims, sp, rec, C, gs, NOISE ? &nz : nullptr, EPISODES ? &ep : nullptr,
                                                                                         CAP ? &pc : nullptr, FORCED ? &fp : nullptr, SOLVER ? &sv : nullptr);
    gstats_flush(gs, M.kind[g] == 1, stats);
}
// k_gselfplay_reopen: the new episode's root draws its symmetry as it starts to wait
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_gselfplay_reopen_sym(GuidedMem M, Quad* soa, GSelfPlay sp, GEpisodes ep, SelfPlayRec rec, unsigned long long* stats) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= M.G) return;
    if (Guided<NL, W>::template selfplay_reopen<true>(M, g, soa, sp, ep, rec)) atomicAdd(&stats[GS_WAITING], 1ull);
}

int gsym_launch_step(tafl_batch* b, const float* priors, const float* values, uint32_t A, double c_puct, uint32_t n_sims, unsigned long long* stats) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    if (b->g_noise_on) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_step_sym<t.NL, t.W, true>), c, n, t.CC, b->gmem, priors, values, A, c_puct, n_sims, stats, b->g_noise); });
    else dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gmcts_step_sym<t.NL, t.W, false>), c, n, t.CC, b->gmem, priors, values, A, c_puct, n_sims, stats, RootNoise{}); });
    return TAFL_OK;
}

template <int FAMILY>
static void gsym_selfplay_family(tafl_batch* b, const float* dp, const float* dv, uint32_t A, unsigned long long* st) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    const bool nz = b->g_noise_on, ep = b->gsp_episodes;
#define TAFL_SYM_ROUND(NZ, EP) dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_sym<t.NL, t.W, FAMILY, NZ, EP>), c, n, t.CC, b->gmem, b->soa, dp, dv, A, b->gsp_cpuct, b->gsp_sims, b->gsp, b->gsp_ep, b->gsp_rec, st, b->g_noise, b->gsp_cap, b->gsp_forced, b->gsp_solver); })
    if (ep) { if (nz) TAFL_SYM_ROUND(true, true); else TAFL_SYM_ROUND(false, true); }
    else { if (nz) TAFL_SYM_ROUND(true, false); else TAFL_SYM_ROUND(false, false); }
#undef TAFL_SYM_ROUND
}
// the choice of gselfplay_launch: the solver's rounds whatever else is set, then the forced ones, then the capped ones, then the plain ones;
// an episodes run closes and reopens after its round
int gsym_launch_selfplay(tafl_batch* b, const float* dp, const float* dv, uint32_t A, unsigned long long* st) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    if (b->gsp_solver_on) gsym_selfplay_family<SYM_SOLVER>(b, dp, dv, A, st);
    else if (b->gsp_forced_on) gsym_selfplay_family<SYM_FORCED>(b, dp, dv, A, st);
    else if (b->gsp_cap_on) gsym_selfplay_family<SYM_CAPPED>(b, dp, dv, A, st);
    else gsym_selfplay_family<SYM_PLAIN>(b, dp, dv, A, st);
    HIPCHK(hipGetLastError());
    if (b->gsp_episodes) {
        dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_gselfplay_reopen_sym<t.NL, t.W>), c, n, b->gmem, b->soa, b->gsp, b->gsp_ep, b->gsp_rec, st); });
        HIPCHK(hipGetLastError());
    }
    return TAFL_OK;
}
