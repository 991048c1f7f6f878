// tafl_internal.hpp — what tafl_core.hip, tafl_mcts.hip, tafl_gmcts.hip and tafl_examples.hip share: the host objects behind the C-ABI of
// include/taflhip.h, the owner of device memory (DevBuf), error reporting, the kernel dispatcher, the device helpers of more than one file.
//
// Execution shape: ONE GAME PER LANE, 64-lane workgroups (one wavefront), so that a 65 536-game
// batch is 1 024 waves = one wave per SIMD on the 256 CUs x 4 SIMDs of an MI355X.  Whole game
// states live in VGPRs for the duration of a kernel (a random playout never touches HBM between its
// first load and its final 1-byte result).  Batch states are quad-plane SoA in HBM (16 B per lane per
// load, 1 KiB per wave instruction); tree nodes are 64-B records (DESIGN.md "Data layout in HBM").
// No CPU fallback exists: every compute entry point launches kernels or fails.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <algorithm>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "tafl_host.hpp"
#include "tafl_ops.hpp"
#include "tafl_guided.hpp"

using namespace tafl;

// nothing declared here is an export of the library: only the extern "C" API of include/taflhip.h is
#pragma GCC visibility push(hidden)

// --------------------------------------------------------------------------------------------------
// device code shared by the kernels of more than one file
// --------------------------------------------------------------------------------------------------
#define TAFL_BLOCK 64
#ifndef TAFL_KATTR
#define TAFL_KATTR
#endif
// minimum waves per SIMD the playout kernels are compiled for (a bound for the register allocator; the preset 11x11 kernel needs 104
// VGPRs and runs four, which is what the pipeline fills: DESIGN.md section 6)
#ifndef TAFL_ROLLOUT_WAVES
#define TAFL_ROLLOUT_WAVES 2
#endif
#define TAFL_MCTS_MAX_SLOTS 8        /* playout slots per game (the pending leaf + up to 7 predicted ones) */
static_assert(TAFL_MCTS_MAX_SLOTS == tafl::kMctsMaxSlots, "slot bound of tafl_ops.hpp");
#define TAFL_MCTS_MAX_PARTS 8         /* partitions of a batch that run the two-kernel pipeline on their own streams */
#define TAFL_MCTS_TRACE_ROUNDS 4096   /* rounds of a search whose work counts are kept for tafl_mcts_round_trace */
#define TAFL_MCTS_UNDO_CAP 16        /* undo records per game and prediction pass (edges and headers each), in LDS: 16 x 14 words x 64 lanes = 56 KiB per tree wave */
#define TAFL_MCTS_UNDO_CAP_FUSED 5   /* the fused kernel predicts one simulation (two slots) and runs eight waves per CU: 17.5 KiB per wave */
#define TAFL_UNDO_LDS_BYTES(cap) ((size_t)(cap) * (tafl::kUndoEWords + tafl::kUndoHWords) * TAFL_BLOCK * sizeof(uint32_t))

// For PRESET != 0 every geometry / rule mask is a compile-time literal (no SMEM loads, no SGPR pressure) and rule
// branches that the preset never takes are pruned; PRESET == 0 uses the run-time Consts passed as a kernel argument.
#define TAFL_PICK_CONSTS(C, Carg)                                                   \
    constexpr Consts<NL> C##_ct = preset_consts<NL, W, PRESET>();                   \
    const Consts<NL>& C = (PRESET != PRESET_NONE) ? C##_ct : (Carg)

// The index policy of a playout kernel (tafl_tables.hpp): the bit_at table in LDS, filled by the whole workgroup, for the preset kernels
// of the layouts that keep one; the computed code for every other instantiation (run-time rules, dense 13x13).  Call it before any lane
// of the workgroup leaves the kernel.
template <int NL, int W, int PRESET>
__device__ __forceinline__ auto playout_tables() {
    if constexpr (PRESET == PRESET_NONE || !playout_bit_table<NL>()) return IdxComputed<NL>();
    else {
        using L = IdxTables<NL>;
        __shared__ typename L::Row mem[L::ROWS];
        L::fill(mem, threadIdx.x, blockDim.x);
        __syncthreads();
        L lut; lut.base = mem;
        return lut;
    }
}

// game g of the batch (quad-plane SoA in the reference layout <NLS, WS>) in the layout <NL, W> the kernel works in: the same, or the dense
// 13-column layout of the 13x13 preset (restride, tafl_core.hpp)
template <int NLS, int WS, int NL, int W>
__device__ __forceinline__ void load_batch_state(const Quad* soa, uint32_t n, uint32_t g, uint32_t side_len, DState<NL>& st) {
    if constexpr (NLS == NL && WS == W) StateIO<NL>::load_soa(soa, n, g, st);
    else { DState<NLS> t; StateIO<NLS>::load_soa(soa, n, g, t); restride<NLS, WS, NL, W>(t, side_len, st); }
}

// the play of tafl_mcts_advance / tafl_gmcts_advance on the batch state (layout <NL, W>): do_play (logic.rs:827-834) of a dense action
// index, exactly tafl_step; returns true when the play was made
template <int NL, int W>
__device__ __forceinline__ bool advance_play(const Consts<NL>& C, DState<NL>& st, uint32_t a, uint32_t A, tafl_play& p, tafl_effects& e) {
    using O = Ops<NL, W>;
    O::caps_to_effects(bz<NL>(), 0, e);
    p.from_row = p.from_col = p.axis = 0; p.disp = 0;
    if (a == TAFL_ACTION_NONE || TAFL_F_STATUS(st.flags) != TAFL_STATUS_ONGOING) { O::status_to_effects(st, TAFL_PLAY_GAME_OVER, e); return false; }
    if (a >= A) { O::status_to_effects(st, TAFL_PLAY_OUT_OF_BOUNDS, e); return false; }
    const tafl_play pl = O::to_play(O::move_of_action(a, C));
    DState<NL> s2 = st;
    O::step(s2, pl, C, &e);
    if (e.code != TAFL_PLAY_OK) return false;
    st = s2; p = pl;
    return true;
}
template <int NL>
__device__ __forceinline__ bool same_state(const Quad* rec, const DState<NL>& st) {
    uint32_t v[StateIO<NL>::WORDS]; StateIO<NL>::pack(st, v);
    bool same = true;
    TAFL_UNROLL for (int q = 0; q < StateIO<NL>::QUADS; ++q) {
        const Quad t = rec[q];
        same = same && t.x == v[4 * q] && t.y == v[4 * q + 1] && t.z == v[4 * q + 2] && t.w == v[4 * q + 3];
    }
    return same;
}

// probs of src/mcts.py:43-53 for any temperature.
//   temp > 0 : counts ** (1 / temp) (float64 pow of the device math library; exactly the count for temp == 1), summed in ascending action
//              order like Python's sum(), then divided (mcts.py:50-52).
//   temp == 0: one-hot on one of the maxima (mcts.py:44-48).  The reference draws it with the process-global np.random.choice; here it is
//              the first maximum (tie_seed == 0) or the floor(r * ties / 2^32)-th one in ascending action order with r = the taflmix32 word keyed by
//              (tie_seed, global game id): reproducible and independent of the sharding.
__device__ __forceinline__ uint32_t tie_pick(uint64_t tie_seed, uint64_t game_id, uint32_t ties) {
    const uint64_t gk = Engine<2, 7>::game_key(tie_seed, game_id);
    const uint32_t h = Engine<2, 7>::fmix32((uint32_t)gk ^ Engine<2, 7>::fmix32((uint32_t)(gk >> 32) + 0x7A1E5EEDu));
    return Engine<2, 7>::mulhi(h, ties);
}
__device__ __forceinline__ double temp_weight(uint32_t n, double inv_temp) { return inv_temp == 1.0 ? (double)n : pow((double)n, inv_temp); }

// --------------------------------------------------------------------------------------------------
// host objects
// --------------------------------------------------------------------------------------------------
int fail(int code, const std::string& msg);       // sets the per-thread message of tafl_last_error() and returns `code`
// for the translation units of the library that do not include this header (tafl_replay.cpp): same per-thread message
int tafl_fail_(int code, const char* msg);
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(TAFL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

enum { KC_MOVEGEN = 0, KC_STEP, KC_ROLLOUT, KC_MCTS_TREE, KC_MCTS_ROLLOUT, KC_COUNT };

struct TimedSpan { hipEvent_t a, b; int cls; };

struct tafl_ctx {
    tafl_rules rules;
    uint32_t n, word_bits, nl, w;
    int device;
    hipStream_t stream;
    bool own_stream;
    Consts<2> c2; Consts<4> c4; Consts<8> c8;
    Consts<6> c6;                    // the same rules in the dense 13-column layout (dense13: 256-bit words, side_len <= 13)
    bool dense13;
    int preset;                      // PRESET_* detected at ctx_create: selects kernels with compile-time constants
    uint32_t live_batches = 0;       // batches created on this context and not yet destroyed (tafl_ctx_destroy refuses while > 0)
    uint32_t rollout_capacity = 0;   // playouts k_mcts_rollout holds on the device at once (occupancy x CUs x 64 lanes); 0 = not asked yet
    bool timing = false;
    std::vector<TimedSpan> spans;
    double acc_ms[KC_COUNT] = {}; uint64_t acc_n[KC_COUNT] = {};
    // the same spans as intervals on one clock (milliseconds since `t_ref`, recorded by tafl_timing_reset): launches of a class that
    // overlap on different streams are counted once by tafl_timing_get_union
    hipEvent_t t_ref; bool has_ref = false;
    std::vector<std::pair<float, float>> ivals[KC_COUNT];
};

// The one owner of a piece of device memory: freed when its owner (a batch, an examples object) is deleted, never copied.  The kernels'
// argument structs (MctsMem, GuidedMem, ExamplesMem) hold plain pointers INTO these buffers (as<T>() / bind()).
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }      // (std::swap of two arenas)
    ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return -1; }
        cap = bytes; return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
    template <class T> void bind(T*& field) const { field = static_cast<T*>(p); }       // a pointer of an argument struct follows its buffer
};
#define NEED(buf, bytes) do { if ((buf).ensure(bytes)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed"); } while (0)
// Outputs.  STAGED: where a kernel writes the output `out` of `count` elements: through the caller's own pointer if that is a device
// pointer (or null: not asked for), otherwise into the staging buffer `buf`, from where COPY_OUT brings it to the host pointer.
// COPY_OUT: `count` elements from device memory to the host pointer `out` if there is one (asynchronous: the caller synchronises).
#define STAGED(dst, buf, out, count, out_is_device) do { dst = (out); if ((out) && !(out_is_device)) { NEED(buf, sizeof(*(out)) * (size_t)(count)); dst = static_cast<decltype(dst)>((buf).p); } } while (0)
#define COPY_OUT(out, src, count, s) do { if (out) HIPCHK(hipMemcpyAsync((out), (src), sizeof(*(out)) * (size_t)(count), hipMemcpyDeviceToHost, (s))); } while (0)

// a search in flight on a batch: tafl_mcts_run_async enqueues the whole plan, tafl_mcts_wait joins it (and runs the stragglers' rounds)
struct SearchPart { uint32_t g0, g1, cap, grid_tree, grid_roll; hipStream_t s; uint32_t* wl; uint32_t* wc; };
struct SearchPlan {
    bool active, fused;
    tafl_mcts_params p; uint64_t base;
    MctsMem M;
    uint32_t parts, slots, planned, probe_every, next_round, max_rounds;
    unsigned long long ctrl0[4];     // initial control words (CT_*): source of an asynchronous copy
    SelfPlay selfplay;               // n_moves != 0: a self-play run (tafl_selfplay_run)
    bool recording; SelfPlayRec rec; // a recording run (tafl_selfplay_record): k_mcts_tree_selfplay_rec
    SearchPart P[TAFL_MCTS_MAX_PARTS];
};

struct tafl_batch {
    tafl_ctx* ctx = nullptr;
    uint32_t n = 0;
    // searches run on streams of the BATCH (created on first use), forked from the context's stream when the search is enqueued and joined
    // by tafl_mcts_wait: two batches of one context search side by side
    hipStream_t sstream[TAFL_MCTS_MAX_PARTS];
    hipEvent_t ev_fork[TAFL_MCTS_MAX_PARTS], ev_start, ev_half;
    uint32_t n_sstreams = 0;
    bool half_recorded = false;      // ev_half sits in the stream of the search in flight (half of its planned rounds are enqueued before it)
    SearchPlan plan = {};
    DevBuf ctrl;
    DevBuf states; Quad* soa = nullptr;      // quad-plane SoA: [QUADS][n]
    DevBuf plays, effects, counts, masks, codes, ranks, results, out_plays, u8out, plies;
    // MCTS
    MctsMem mem = {}; bool has_mem = false; uint32_t reserved_sims = 0;
    DevBuf node_state, hdr, edges, node_top, edge_top, leaf, kind, fault, stats, children, children_n, visits;
    DevBuf best_plays, best_visits, enc, policy;
    DevBuf work, work_count, trace, sim_base, sp_moves_done, sp_start_round, sp_plays;
    uint32_t trace_rounds = 0;       // rounds of the last two-kernel search recorded in `trace` (requested / run playouts per round)
    DevBuf sim_next, spec_state, spec_meta, spec_value, spec_kind, spec_reason, spec_plies, spec_ref, spec_cls, spec_pend, spec_bias;
#ifdef TAFL_EXPERIMENT_SPEC_K
    uint32_t spec_k = TAFL_EXPERIMENT_SPEC_K;      // measurement builds only
#else
    uint32_t spec_k = TAFL_MCTS_MAX_SLOTS;         // playout slots per game that exist
#endif
    bool ran = false;
    bool stats_ok = false;           // the counters of the last finished search / self-play run can be read (a self-play run leaves no tree: ran = false)
    // guided MCTS (external evaluator)
    GuidedMem gmem = {}; bool g_has = false; uint32_t g_max_sims = 0;
    DevBuf g_node_state, g_hdr, g_pedge, g_edges, g_node_top, g_edge_top, g_leaf, g_kind, g_fault, g_sims, g_stats, g_priors, g_values, g_boards, g_sides, g_wait;
    // guided self-play at each game's own pace (tafl_gselfplay_*): the run open on the guided arena; gsp_first: tafl_gselfplay_begin has run
    // the first round and the first tafl_gselfplay_step reports it; gsp_has: the buffers hold the plays of a run (tafl_gselfplay_end)
    bool gsp_active = false, gsp_first = false, gsp_has = false;
    GSelfPlay gsp = {}; SelfPlayRec gsp_rec = {}; uint32_t gsp_sims = 0; double gsp_cpuct = 0.0;
    ExampleStatsMem gsp_stats = {};  // the run records into an examples object with search statistics (cq != nullptr): k_gselfplay_record_stats follows every round
    // ... and value targets (ep_end != nullptr): k_gselfplay_mark_boundary follows the recorder, reading the object's open_from
    ExampleTargetsMem gsp_targets = {}; const uint32_t* gsp_open_from = nullptr;
    struct tafl_examples* gsp_targets_ex = nullptr;      // that object: every round of the run marks its targets stale
    DevBuf gsp_moves_done, gsp_plays;
    // an episodes run (tafl_gselfplay_begin_episodes): per lane the episode number and the move count at which it began, the openings
    // (quad-plane SoA like the batch states) and the four result counters; gsp_episodes: the run that is open, or was last, is one
    bool gsp_episodes = false; GEpisodes gsp_ep = {};
    DevBuf gsp_episode, gsp_ep_start, gsp_openings, gsp_ep_counters;
    // a match run (tafl_gmatch_begin): gm_on: the run that is open, or was last, is one; gm_leaves: tafl_gmatch_leaves has run since the
    // last step, gm_count holds its counts and gm_row_of every lane's row; the lanes of the two compact batches [2][n], the partition's
    // workgroup counts, its two totals, the tally [2][4]
    bool gm_on = false, gm_leaves = false; GMatch gm = {}; uint32_t gm_count[2] = {0, 0};
    DevBuf gm_row_of, gm_lanes, gm_blocks, gm_counts, gm_games;
    // Dirichlet noise at the root (tafl_gmcts_set_root_noise): the setting, and what the open search or run latched at its begin
    bool noise_set = false, g_noise_on = false;
    tafl_root_noise noise_cfg = {}; RootNoise g_noise = {};
    // evaluation under a random board symmetry (tafl_gmcts_set_eval_symmetry): the setting; what the open search or run latched at its
    // begin is gmem.sym (null: off) with its seed and game id base, over one byte per game
    bool evalsym_set = false;
    tafl_eval_symmetry evalsym_cfg = {};
    DevBuf g_sym;
    // playout cap randomization (tafl_gselfplay_set_playout_cap): the setting, and what the guided self-play run that is open, or was last,
    // latched at its begin (gsp_cap_on: it is a capped run; its two class counters)
    bool cap_set = false, gsp_cap_on = false;
    tafl_playout_cap cap_cfg = {}; PlayoutCap gsp_cap = {};
    DevBuf gsp_cap_counters;
    // forced playouts and policy target pruning (tafl_gselfplay_set_forced_playouts): the setting, and what that run latched (gsp_forced_on:
    // its rounds are the forced ones; its four counters)
    bool forced_set = false, gsp_forced_on = false;
    tafl_forced_playouts forced_cfg = {}; ForcedPlayouts gsp_forced = {};
    DevBuf gsp_forced_counters;
    // exact win/loss proofs (tafl_gselfplay_set_solver): the setting, and what that run latched (gsp_solver_on: its rounds are the solver
    // ones; its eight counters)
    bool solver_set = false, gsp_solver_on = false;
    SolverCfg gsp_solver = {};
    DevBuf gsp_solver_counters;
    // subtree reuse (TAFL_MCTS_FLAG_KEEP_TREE): the arena holds trees rooted at the current batch states (*_tree_live); the second edge
    // arena and the id map of a re-root; a small read-back buffer
    bool tree_live = false, g_tree_live = false;
    DevBuf edges_alt, idmap, g_edges_alt, g_idmap, small;
};

// training examples
struct tafl_examples {
    tafl_ctx* ctx;
    uint32_t n_games, max_moves, max_children;
    uint32_t flags = 0;              // TAFL_EXAMPLES_* of tafl_examples_create_ex
    ExamplesMem mem;
    ExampleStatsMem smem = {};       // TAFL_EXAMPLES_SEARCH_STATS: the arrays beside pol (all null without the flag)
    DevBuf len, boards, info, played, move_no, pol, z, fin, counters;
    DevBuf cq, cp, seen, g_s;        // g_s: staging of the second scalar of a host-pointer tafl_examples_gather_stats
    // TAFL_EXAMPLES_VALUE_TARGETS: the three arrays (all null without the flag), the four result counters, the staging of the second byte
    // of a host-pointer tafl_examples_gather_targets; vt_valid: a result of tafl_examples_value_targets stands
    ExampleTargetsMem tmem = {};
    DevBuf ep_end, vt, kind, vt_res, g_k;
    bool vt_valid = false;
    DevBuf open_from;                // [n_games] first example of game g whose result is still open: 0 unless an episodes run has moved it
    DevBuf g_index, g_sym, g_boards, g_sides, g_pi, g_z, g_fin;      // staging of a gather with host pointers
    size_t device_bytes = 0;         // sum of the capacities above: every allocation goes through need()
    int need(DevBuf& d, size_t bytes) { device_bytes -= d.cap; const int rc = d.ensure(bytes); device_bytes += d.cap; return rc; }
};

static inline int quads_of(const tafl_ctx* c) { return (2 * (int)c->nl + 8) / 4; }
static inline uint32_t grid_of(uint32_t n) { return (n + TAFL_BLOCK - 1) / TAFL_BLOCK; }
// the launch of most kernels: one game per lane, on the context's stream
#define LAUNCH_PER_GAME(kernel, c, n, ...) hipLaunchKernelGGL(kernel, dim3(grid_of(n)), dim3(TAFL_BLOCK), 0, (c)->stream, __VA_ARGS__)
// the common end of an entry point: the context's stream has run dry, so the copies to host memory have arrived
static inline int sync_ok(tafl_ctx* c) { HIPCHK(hipStreamSynchronize(c->stream)); return TAFL_OK; }

// ---- the dispatcher: from the context's run-time geometry to the kernels' template arguments ---------------------------------------------
// dispatch<LAYOUT, PRESETS>(ctx, f) calls the generic lambda f with one tag t: t.NL, t.W the layout the kernel works in, t.NLS, t.WS the
// layout of the batch states, t.PRESET, and t.CC the matching Consts<NL>.  LAYOUT BATCH: the batch layout (the reference's words: 2 x 7,
// 4 x 11, 8 x 15).  ARENA: the kernels that work on the search arena (and the playouts); it differs for the 13x13 preset only, which is
// searched in the dense 13-column layout (6 limbs instead of the reference's 8).  PRESETS: for the hot kernels that also exist specialised
// on a compile-time preset (t.PRESET = the context's preset; otherwise always PRESET_NONE).  A call site instantiates its kernel for
// exactly the tags of its <LAYOUT, PRESETS>: the pair decides which instantiations exist.
template <int NL_, int W_, int NLS_, int WS_, int PRESET_>
struct KernelTag { static constexpr int NL = NL_, W = W_, NLS = NLS_, WS = WS_, PRESET = PRESET_; const Consts<NL_>& CC; };
enum DispatchLayout { BATCH, ARENA };
template <int PRESET, bool PRESETS, int NL, int W, class F>
static inline void dispatch_preset(const tafl_ctx* c, const Consts<NL>& CC, F& f) {
    if constexpr (PRESETS) { if (c->preset == PRESET) { f(KernelTag<NL, W, NL, W, PRESET>{CC}); return; } }
    f(KernelTag<NL, W, NL, W, PRESET_NONE>{CC});
}
template <DispatchLayout LAYOUT, bool PRESETS, class F>
static inline void dispatch(const tafl_ctx* c, F f) {
    if (c->nl == 2) dispatch_preset<PRESET_BRANDUBH7, PRESETS, 2, 7>(c, c->c2, f);
    else if (c->nl == 4) dispatch_preset<PRESET_COPENHAGEN11, PRESETS, 4, 11>(c, c->c4, f);
    else if constexpr (LAYOUT == ARENA) {
        if (c->preset == PRESET_COPENHAGEN13) f(KernelTag<6, 13, 8, 15, PRESETS ? PRESET_COPENHAGEN13 : PRESET_NONE>{c->c6});
        else f(KernelTag<8, 15, 8, 15, PRESET_NONE>{c->c8});
    } else dispatch_preset<PRESET_COPENHAGEN13, PRESETS, 8, 15>(c, c->c8, f);
}
template <int NLS> static const Consts<NLS>& batch_consts(const tafl_ctx* c) {
    if constexpr (NLS == 2) return c->c2; else if constexpr (NLS == 4) return c->c4; else return c->c8;
}

struct SpanGuard {
    tafl_ctx* c; int idx;
    hipStream_t st;
    SpanGuard(tafl_ctx* ctx, int cls, hipStream_t on = nullptr) : c(ctx), idx(-1), st(on ? on : ctx->stream) {
        if (!c->timing) return;
        TimedSpan s; s.cls = cls;
        if (hipEventCreate(&s.a) != hipSuccess) return;
        if (hipEventCreate(&s.b) != hipSuccess) { (void)hipEventDestroy(s.a); return; }
        (void)hipEventRecord(s.a, st);
        c->spans.push_back(s); idx = (int)c->spans.size() - 1;
    }
    ~SpanGuard() { if (idx >= 0) (void)hipEventRecord(c->spans[idx].b, st); }
};

// ---- what crosses the files (tafl_mcts.hip defines it) -------------------------------------------------------------------------------
// a search in flight is joined before its batch is written, grown, re-rooted or read (tafl_mcts_wait; TAFL_OK when there is none)
static inline int join_search(tafl_batch* b) { return b->plan.active ? tafl_mcts_wait(b) : TAFL_OK; }
// tafl_mcts_run_async and its kin; n_moves != 0: a self-play run, with `rec` a recording one
int mcts_begin(tafl_batch* b, const tafl_mcts_params* p, uint64_t game_id_base, tafl_batch* after, uint32_t n_moves = 0, const SelfPlayRec* rec = nullptr);
// the common end of tafl_selfplay_run / tafl_selfplay_record: joins the run that mcts_begin returned `rc` for and hands out its plays
int selfplay_finish(tafl_batch* b, int rc, uint32_t n_moves, tafl_play* out_plays);
// the largest retained tree of the batch: out[0] = nodes, out[1] = edges (a 8-byte read-back)
int arena_max(tafl_batch* b, const uint32_t* node_top, const uint32_t* edge_top, uint32_t out[2]);
// One array of a search arena and the pointer of the kernels' argument struct that must follow it: node-major [node][game] with `elem`
// bytes per node and game, or the edge arena [game * edge_cap + e] with `elem` bytes per edge.
struct ArenaArray {
    DevBuf* buf; size_t elem; void* field; void (*follow_)(void* field, void* p);
    template <class T> ArenaArray(DevBuf& d, size_t elem_bytes, T*& ptr)
        : buf(&d), elem(elem_bytes), field(&ptr), follow_([](void* f, void* p) { *static_cast<T**>(f) = static_cast<T*>(p); }) {}
    void follow() const { follow_(field, buf->p); }
};
// an arena grown, with its contents kept, to `nodes` nodes and `edges` edges per game (no-op for a capacity it already has)
int arena_grow(tafl_batch* b, std::initializer_list<ArenaArray> node_arrays, uint32_t& node_cap, unsigned long long nodes,
               const ArenaArray& edge_array, DevBuf& edges_alt, uint32_t& edge_cap, unsigned long long edges);

// play + re-root (TAFL_MCTS_FLAG_KEEP_TREE), the body of tafl_mcts_advance and tafl_gmcts_advance (`name`): `launch` runs the arena's
// advance kernel, which writes every game's edges into the second edge arena; that one then becomes the arena, and `rerooted` lets the
// arena's pointer follow and sets the *_tree_live flags.  A 4-byte read-back reports kept roots whose state differs from the batch state
// (an internal error; those games get fresh roots).
template <class Launch, class Rerooted>
static int tree_advance(tafl_batch* b, const char* name, DevBuf& edges, DevBuf& edges_alt, DevBuf& idmap, uint32_t node_cap, const uint32_t* actions,
                        tafl_play* out_plays, tafl_effects* out_effects, Launch launch, Rerooted rerooted) {
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    NEED(edges_alt, edges.cap); NEED(idmap, (size_t)node_cap * n * sizeof(uint32_t)); NEED(b->small, 64);
    if (actions) { NEED(b->ranks, sizeof(uint32_t) * n); HIPCHK(hipMemcpyAsync(b->ranks.p, actions, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream)); }
    tafl_play* dplays; tafl_effects* deff;
    STAGED(dplays, b->best_plays, out_plays, n, 0);
    STAGED(deff, b->effects, out_effects, n, 0);
    uint32_t* bad = b->small.as<uint32_t>() + 2;
    HIPCHK(hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
    launch(actions ? b->ranks.as<const uint32_t>() : nullptr, tafl_action_size(c), dplays, deff, bad);
    HIPCHK(hipGetLastError());
    std::swap(edges, edges_alt);
    rerooted();
    uint32_t h_bad = 0;
    HIPCHK(hipMemcpyAsync(&h_bad, bad, sizeof h_bad, hipMemcpyDeviceToHost, c->stream));
    COPY_OUT(out_plays, dplays, n, c->stream);
    COPY_OUT(out_effects, deff, n, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h_bad) return fail(TAFL_ERR_HIP, std::string(name) + ": a kept root differs from its new batch state (internal error; those games got fresh roots)");
    return TAFL_OK;
}

// ---- guided rounds: what tafl_gmcts.hip and tafl_gmcts_sym.hip share -------------------------------------------------------------------
enum { GS_SIMS = 0, GS_PREDICTS, GS_TERMINAL, GS_FAULTS, GS_DEPTH, GS_WAITING, GS_COUNT };
// what one lane's round adds to the counters of a step kernel
static __device__ __forceinline__ void gstats_flush(const GuidedStats& gs, bool waiting, unsigned long long* stats) {
    if (gs.sims) atomicAdd(&stats[GS_SIMS], (unsigned long long)gs.sims);
    if (gs.predicts) atomicAdd(&stats[GS_PREDICTS], (unsigned long long)gs.predicts);
    if (gs.terminal_hits) atomicAdd(&stats[GS_TERMINAL], (unsigned long long)gs.terminal_hits);
    if (gs.faults) atomicAdd(&stats[GS_FAULTS], (unsigned long long)gs.faults);
    if (gs.depth) atomicAdd(&stats[GS_DEPTH], (unsigned long long)gs.depth);
    if (waiting) atomicAdd(&stats[GS_WAITING], 1ull);
}
// the rounds of a search or run that latched tafl_eval_symmetry (b->gmem.sym != nullptr): the SYM instantiations, in a translation unit
// of their own (tafl_gmcts_sym.hip).  They take what tafl_gmcts_step / gselfplay_launch give their kernels and launch on the same stream.
int gsym_launch_step(tafl_batch* b, const float* priors, const float* values, uint32_t A, double c_puct, uint32_t n_sims, unsigned long long* stats);
int gsym_launch_selfplay(tafl_batch* b, const float* priors, const float* values, uint32_t A, unsigned long long* stats);

#pragma GCC visibility pop
