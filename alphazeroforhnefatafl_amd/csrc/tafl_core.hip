// tafl_core.hip — context and batch lifecycle, FEN, upload / download, timing, and the streamed entry points of include/taflhip.h
// (movegen, validate, step, rollout, random advance, board encoding) with their kernels.
#include "tafl_internal.hpp"

// ---- kernels ----------------------------------------------------------------------------------------
#ifdef TAFL_PROF
// profiling builds only (never the product library): totals of the TAFL_PROF_* section timers
extern "C" __device__ unsigned long long tafl_prof_acc[4096 * 32] = {};
extern "C" int tafl_prof_read(unsigned long long* out, int reset) {
    static unsigned long long h[4096 * 32];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(tafl_prof_acc), sizeof h) != hipSuccess) return -1;
    for (int k = 0; k < 32; ++k) { out[k] = 0; for (int w = 0; w < 4096; ++w) out[k] += h[w * 32 + k]; }
    if (reset) { memset(h, 0, sizeof h); if (hipMemcpyToSymbol(HIP_SYMBOL(tafl_prof_acc), h, sizeof h) != hipSuccess) return -1; }
    return 0;
}
#endif

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_fill(Quad* soa, uint32_t n, DState<NL> st) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g < n) StateIO<NL>::store_soa(soa, n, g, st);
}

// counts only: one game per lane
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_movegen(Consts<NL> C, const Quad* soa, uint32_t n, uint32_t* counts) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
    counts[g] = Ops<NL, W>::movegen(st, C, nullptr);
}

// counts + dense action masks.  A workgroup serves 64 games with ONE WAVE PER BOARD LINE (lane = game, wave i = row i and column i:
// Ops::movegen_line), so the line index is wave-uniform (every bit position a scalar, no divergence between the lines) and the state loads
// stay coalesced (quad-plane SoA: 1 KiB per wave instruction; the waves of a workgroup read the same 4 KiB, from L2 after the first).
// The masks are assembled in LDS (ds_or, odd row stride: no bank conflicts) and streamed out as one contiguous block per workgroup
// (64 x mask_words uint32, fully coalesced).
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK * 15) void k_movegen_masks(Consts<NL> C, const Quad* soa, uint32_t n, uint32_t* counts, uint32_t* masks, uint32_t mw) {
    extern __shared__ uint32_t lds_masks[];                      // [TAFL_BLOCK][mw | 1] masks, then [TAFL_BLOCK] counts
    const uint32_t ldw = mw | 1u, lane = threadIdx.x & 63u, line = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lines = blockDim.x >> 6;     // lines == C.n
    const uint32_t g0 = blockIdx.x * TAFL_BLOCK, g = g0 + lane;
    uint32_t* lds_cnt = lds_masks + TAFL_BLOCK * ldw;
    for (uint32_t i = threadIdx.x; i < TAFL_BLOCK * (ldw + 1u); i += blockDim.x) lds_masks[i] = 0;
    __syncthreads();
    if (g < n) {
        DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
        const uint32_t c = Ops<NL, W>::movegen_line(st, line, C, lds_masks + (size_t)lane * ldw);
        if (c) atomicAdd(&lds_cnt[lane], c);
    }
    __syncthreads();
    if (line == 0 && g < n && counts) counts[g] = lds_cnt[lane];
    const uint32_t games = (n - g0) < TAFL_BLOCK ? (n - g0) : TAFL_BLOCK;
    uint32_t* dst = masks + (size_t)g0 * mw;
    for (uint32_t gi = line; gi < games; gi += lines)                                        // one game per wave and pass: 304 contiguous bytes
        for (uint32_t w = lane; w < mw; w += TAFL_BLOCK) dst[(size_t)gi * mw + w] = lds_masks[(size_t)gi * ldw + w];
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_validate(Consts<NL> C, const Quad* soa, uint32_t n, const tafl_play* plays, uint8_t* codes) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
    codes[g] = (uint8_t)Ops<NL, W>::validate(st, plays[g], C);
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_step(Consts<NL> C, Quad* soa, uint32_t n, const tafl_play* plays, tafl_effects* eff) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
    tafl_effects e;
    Ops<NL, W>::step(st, plays[g], C, &e);
    StateIO<NL>::store_soa(soa, n, g, st);
    if (eff) eff[g] = e;
}

// game i plays its (rank mod count)-th legal play in canonical order, in two launches:
//   k_select_kth  the dense legal mask is built in LDS by one wave per board line as in k_movegen_masks; every wave then counts the plays in
//                 its share of the mask words, and the first wave (lane = game) walks the partial counts to the chunk that holds the k-th
//                 set bit and finds it there: the chosen dense action index per game (4 B) and the number of plays
//   k_step_action do_valid_play of that action, one game per lane (k_step without the validation): a workgroup of one wave per 64 games,
//                 so that as many games are being applied at once as the device has SIMDs (inside the line-wave workgroup only one wave in
//                 eleven would do this, the longest dependent chain of the call)
// The streamed step of a 256-bit batch whose board has at most 13 columns: the play is validated on the reference's 15-column words (the
// error code of an off-board play depends on that layout, Engine::validate) and applied in the dense 13-column layout of the 13x13 search
// (restride, tafl_core.hpp): six limbs instead of eight keep do_valid_play in registers (k_step<8, 15> carried 720 B of scratch per lane).
template <bool VALIDATE>
__device__ __forceinline__ void step_dense13(const Consts<8>& C, const Consts<6>& Cd, DState<8>& st, tafl_play play, uint32_t action, uint32_t total, tafl_play& pl, tafl_effects& e) {
    using O8 = Ops<8, 15>; using E6 = Engine<6, 13>;
    O8::caps_to_effects(bz<8>(), 0, e);
    pl.from_row = pl.from_col = pl.axis = 0; pl.disp = 0;
    Move m; m.from = m.to = m.dir = m.dist = 0;
    int code;
    if constexpr (VALIDATE) code = Engine<8, 15>::validate(st, play, st.flags & TAFL_F_SIDE, C, &m);
    else {
        if (total == 0) code = TAFL_F_STATUS(st.flags) != TAFL_STATUS_ONGOING ? TAFL_PLAY_GAME_OVER : TAFL_PLAY_NO_PIECE;
        else if (action != O8::NO_ACTION) { m = O8::move_of_action(action, C); pl = O8::to_play(m); code = TAFL_PLAY_OK; }
        else code = TAFL_PLAY_NO_PIECE;
    }
    if (code == TAFL_PLAY_OK) {
        DState<6> d; restride<8, 15, 6, 13>(st, C.n, d);
        Move md = m; md.from = restride_sq<15, 13>(m.from); md.to = restride_sq<15, 13>(m.to);
        StepOut<6> so; Moves<6> nx;
        E6::apply(d, md, Cd, &so, nx);
        restride<6, 13, 8, 15>(d, C.n, st);
        Bits<8> caps = bz<8>(); restride_rows<6, 13, 8, 15>(so.captures, C.n, caps);
        O8::caps_to_effects(caps, so.n_captures, e);
    }
    O8::status_to_effects(st, code, e);
}
__global__ __launch_bounds__(TAFL_BLOCK) void k_step_dense13(Consts<8> C, Consts<6> Cd, Quad* soa, uint32_t n, const tafl_play* plays, tafl_effects* eff) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<8> st; StateIO<8>::load_soa(soa, n, g, st);
    tafl_effects e; tafl_play pl;
    step_dense13<true>(C, Cd, st, plays[g], 0u, 0u, pl, e);
    StateIO<8>::store_soa(soa, n, g, st);
    if (eff) eff[g] = e;
}
__global__ __launch_bounds__(TAFL_BLOCK) void k_step_action_dense13(Consts<8> C, Consts<6> Cd, Quad* soa, uint32_t n, const uint32_t* actions, const uint32_t* totals, tafl_play* out_plays, tafl_effects* eff) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<8> st; StateIO<8>::load_soa(soa, n, g, st);
    tafl_effects e; tafl_play pl; tafl_play none; none.from_row = none.from_col = none.axis = 0; none.disp = 0;
    step_dense13<false>(C, Cd, st, none, actions[g], totals[g], pl, e);
    StateIO<8>::store_soa(soa, n, g, st);
    if (eff) eff[g] = e;
    if (out_plays) out_plays[g] = pl;
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK * 15) void k_select_kth(Consts<NL> C, const Quad* soa, uint32_t n, const uint32_t* ranks, uint32_t* actions, uint32_t* totals, uint32_t mw) {
    extern __shared__ uint32_t lds_masks[];                      // [TAFL_BLOCK][mw | 1] masks, [TAFL_BLOCK] counts, [TAFL_BLOCK][16] partial counts
    const uint32_t ldw = mw | 1u, lane = threadIdx.x & 63u, line = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lines = blockDim.x >> 6;
    const uint32_t g = blockIdx.x * TAFL_BLOCK + lane;
    uint32_t* lds_cnt = lds_masks + TAFL_BLOCK * ldw;
    uint32_t* lds_part = lds_cnt + TAFL_BLOCK;                    // [lane * 17 + line]
    for (uint32_t i = threadIdx.x; i < TAFL_BLOCK * (ldw + 1u); i += blockDim.x) lds_masks[i] = 0;
    __syncthreads();
    if (g < n) {
        DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
        const uint32_t c = Ops<NL, W>::movegen_line(st, line, C, lds_masks + (size_t)lane * ldw);
        if (c) atomicAdd(&lds_cnt[lane], c);
    }
    __syncthreads();
    const uint32_t chunk = (mw + lines - 1u) / lines, w0 = line * chunk, w1 = (w0 + chunk) < mw ? (w0 + chunk) : mw;
    {
        uint32_t pc = 0;
        for (uint32_t w = w0; w < w1; ++w) pc += (uint32_t)__builtin_popcount(lds_masks[(size_t)lane * ldw + w]);
        lds_part[lane * 17u + line] = pc;
    }
    __syncthreads();
    if (line != 0 || g >= n) return;
    const uint32_t total = lds_cnt[lane];
    uint32_t action = Ops<NL, W>::NO_ACTION;
    if (total) {
        uint32_t k = ranks[g] % total, j = 0; bool found = false;
        for (uint32_t q = 0; q < lines; ++q) { const uint32_t pc = lds_part[lane * 17u + q]; if (!found) { if (k < pc) { j = q; found = true; } else k -= pc; } }
        if (found) { const uint32_t a0 = j * chunk, a1 = (a0 + chunk) < mw ? (a0 + chunk) : mw; action = Ops<NL, W>::kth_set_bit(lds_masks + (size_t)lane * ldw, a0, a1, k); }
    }
    actions[g] = action; totals[g] = total;
}
template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_step_action(Consts<NL> C, Quad* soa, uint32_t n, const uint32_t* actions, const uint32_t* totals, tafl_play* out_plays, tafl_effects* eff) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
    tafl_effects e; tafl_play p;
    Ops<NL, W>::step_action(st, actions[g], totals[g], C, &p, &e);
    StateIO<NL>::store_soa(soa, n, g, st);
    if (eff) eff[g] = e;
    if (out_plays) out_plays[g] = p;
}

template <int NL, int W>
__global__ __launch_bounds__(TAFL_BLOCK) void k_side_can_play(Consts<NL> C, const Quad* soa, uint32_t n, uint32_t side, uint8_t* out) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
    out[g] = Ops<NL, W>::side_can_play(st, side, C) ? 1 : 0;
}

template <int NLS, int WS, int NL, int W, int PRESET>
__global__ TAFL_KATTR __launch_bounds__(TAFL_BLOCK) void k_rollout(Consts<NL> Carg, const Quad* soa, uint32_t n, uint64_t seed, uint32_t sim, uint32_t max_plies,
                                                        uint64_t base, tafl_rollout_result* out) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    TAFL_PICK_CONSTS(C, Carg);
    const auto lut = playout_tables<NL, W, PRESET>();            // filled by the whole workgroup: before any lane leaves
    if (g >= n) return;
    DState<NL> st; load_batch_state<NLS, WS, NL, W>(soa, n, g, C.n, st);
    tafl_rollout_result r;
    Ops<NL, W>::rollout(st, seed, base + g, sim, max_plies, C, r, false, lut, KernelPlayout());
    out[g] = r;
}

template <int NL, int W, int PRESET>
__global__ __launch_bounds__(TAFL_BLOCK) void k_random_advance(Consts<NL> Carg, Quad* soa, uint32_t n, uint64_t seed, const uint32_t* plies, uint64_t base) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= n) return;
    TAFL_PICK_CONSTS(C, Carg);
    DState<NL> st; StateIO<NL>::load_soa(soa, n, g, st);
    Ops<NL, W>::random_advance(st, seed, base + g, plies[g], C);
    StateIO<NL>::store_soa(soa, n, g, st);
}

template <int NL, int W>
__global__ __launch_bounds__(256) void k_encode_boards(Consts<NL> C, const Quad* soa, uint32_t n_games, uint8_t* out) {
    const uint32_t nn = C.n * C.n;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n_games * nn) return;
    const uint32_t g = (uint32_t)(i / nn), t = (uint32_t)(i % nn), r = t / C.n, c = t % C.n, bit = r * (uint32_t)W + c;
    const uint32_t wa = bit >> 5, wd = (uint32_t)NL + (bit >> 5);         // absolute state words: att[NL], def[NL], rep[4], meta[4]
    const Quad qa = soa[(size_t)(wa >> 2) * n_games + g], qd = soa[(size_t)(wd >> 2) * n_games + g];
    const uint32_t la = wa & 3, ld = wd & 3;
    const uint32_t aw = la == 0 ? qa.x : la == 1 ? qa.y : la == 2 ? qa.z : qa.w;
    const uint32_t dw = ld == 0 ? qd.x : ld == 1 ? qd.y : ld == 2 ? qd.z : qd.w;
    const Quad meta = soa[(size_t)(2 * NL + 4) / 4 * n_games + g];
    out[i] = (uint8_t)board_value((aw >> (bit & 31)) & 1u, (dw >> (bit & 31)) & 1u, r, c, C.n, meta.w);
}

// ---- errors, timing spans ----------------------------------------------------------------------------
static thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int tafl_fail_(int code, const char* msg) { return fail(code, msg ? msg : ""); }

static void drain_spans(tafl_ctx* c) {
    for (auto& s : c->spans) {
        (void)hipEventSynchronize(s.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
            c->acc_ms[s.cls] += ms; c->acc_n[s.cls] += 1;
            float t0 = 0.f;
            if (c->has_ref && hipEventElapsedTime(&t0, c->t_ref, s.a) == hipSuccess) c->ivals[s.cls].push_back(std::make_pair(t0, t0 + ms));
        }
        (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b);
    }
    c->spans.clear();
}

// every write to the batch states joins a search in flight first (the search reads them, and its tree must not be dropped under it) and
// drops the retained trees (TAFL_MCTS_FLAG_KEEP_TREE): they belong to the states before the write
static int batch_write(tafl_batch* b) {
    if (const int rc = join_search(b)) return rc;
    b->tree_live = false; b->g_tree_live = false;
    b->gsp_active = false;                                   // (and close a guided self-play run: it plays on from the states it wrote)
    return TAFL_OK;
}

// ---- C-ABI ------------------------------------------------------------------------------------------
extern "C" {

const char* tafl_last_error(void) { return g_err.c_str(); }
int tafl_abi_version(void) { return TAFLHIP_ABI_VERSION; }
int tafl_preset_rules(const char* name, tafl_rules* out) {
    if (!name || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    if (preset_rules(name, out)) return fail(TAFL_ERR_INVALID_ARG, std::string("unknown ruleset preset: ") + name);
    return TAFL_OK;
}
const char* tafl_preset_board(const char* name) { return preset_board(name); }

int tafl_ctx_create(const tafl_rules* rules, uint8_t side_len, uint32_t word_bits, int device, void* stream, tafl_ctx** out) {
    if (!rules || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    int l64, rw;
    if (word_params(word_bits, &l64, &rw)) return fail(TAFL_ERR_INVALID_ARG, "word_bits must be 64, 128 or 256");
    if (side_len < 3 || (int)side_len > rw || side_len > 15) return fail(TAFL_ERR_INVALID_ARG, "side_len does not fit the board word");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(TAFL_ERR_NO_DEVICE, "no HIP device visible: taflhip has no CPU path");
    if (device < 0 || device >= ndev) return fail(TAFL_ERR_INVALID_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    tafl_ctx* c = new (std::nothrow) tafl_ctx();
    if (!c) return fail(TAFL_ERR_OOM, "out of host memory");
    c->rules = *rules; c->n = side_len; c->word_bits = word_bits; c->nl = (uint32_t)l64 * 2; c->w = (uint32_t)rw; c->device = device;
    c->preset = detect_preset(*rules, side_len, word_bits);
    int rc = 0;
    if (c->nl == 2) rc = make_consts<2, 7>(*rules, side_len, c->c2);
    else if (c->nl == 4) rc = make_consts<4, 11>(*rules, side_len, c->c4);
    else rc = make_consts<8, 15>(*rules, side_len, c->c8);
    c->dense13 = c->nl == 8 && side_len <= 13;      // the 13-column layout holds the board: streamed steps and the 13x13 preset's searches use it
    if (!rc && c->dense13) rc = make_consts<6, 13>(*rules, side_len, c->c6);
    if (rc) { delete c; return fail(TAFL_ERR_INVALID_ARG, "bad rules / geometry"); }
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else { if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return fail(TAFL_ERR_HIP, "hipStreamCreate failed"); } c->own_stream = true; }
    *out = c;
    return TAFL_OK;
}

int tafl_ctx_destroy(tafl_ctx* c) {
    if (!c) return TAFL_OK;
    if (c->live_batches != 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_ctx_destroy: batches of this context are still alive (destroy them first)");
    (void)hipSetDevice(c->device);
    drain_spans(c);
    if (c->has_ref) (void)hipEventDestroy(c->t_ref);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return TAFL_OK;
}

void* tafl_ctx_stream(tafl_ctx* c) { return c ? (void*)c->stream : nullptr; }

uint32_t tafl_action_size(const tafl_ctx* c) { return c ? c->n * c->n * 2u * (c->n - 1) : 0; }
uint32_t tafl_action_mask_words(const tafl_ctx* c) { return (tafl_action_size(c) + 31) / 32; }
int tafl_action_encode(const tafl_ctx* c, tafl_play p, uint32_t* action) {
    if (!c || !action) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    const uint32_t dist = (uint32_t)(p.disp < 0 ? -(int)p.disp : (int)p.disp), r = p.from_row, cc = p.from_col, m = c->n - 1;
    if (r >= c->n || cc >= c->n || dist == 0) return fail(TAFL_ERR_INVALID_ARG, "play outside the action space");
    const bool vert = p.axis == TAFL_AXIS_VERTICAL;
    const uint32_t room = vert ? (p.disp > 0 ? m - r : r) : (p.disp > 0 ? m - cc : cc);
    if (dist > room) return fail(TAFL_ERR_INVALID_ARG, "play outside the action space");
    const uint32_t slot = vert ? (p.disp > 0 ? dist - 1 : (m - r) + dist - 1) : (p.disp > 0 ? m + dist - 1 : m + (m - cc) + dist - 1);
    *action = (r * c->n + cc) * 2u * m + slot;
    return TAFL_OK;
}
int tafl_action_decode(const tafl_ctx* c, uint32_t a, tafl_play* play) {
    if (!c || !play || a >= tafl_action_size(c)) return fail(TAFL_ERR_INVALID_ARG, "action out of range");
    const uint32_t m = c->n - 1, per = 2u * m, sq = a / per, slot = a % per, r = sq / c->n, cc = sq % c->n;
    play->from_row = (uint8_t)r; play->from_col = (uint8_t)cc;
    if (slot < m - r) { play->axis = TAFL_AXIS_VERTICAL; play->disp = (int8_t)(slot + 1); }
    else if (slot < m) { play->axis = TAFL_AXIS_VERTICAL; play->disp = (int8_t)(-(int)(slot - (m - r) + 1)); }
    else if (slot < m + (m - cc)) { play->axis = TAFL_AXIS_HORIZONTAL; play->disp = (int8_t)(slot - m + 1); }
    else { play->axis = TAFL_AXIS_HORIZONTAL; play->disp = (int8_t)(-(int)(slot - m - (m - cc) + 1)); }
    return TAFL_OK;
}

int tafl_state_from_fen(const tafl_ctx* c, const char* fen, uint8_t side, tafl_state* out) {
    if (!c || !fen || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    std::string err;
    if (fen_to_state(fen, side, c->word_bits, out, &err)) return fail(TAFL_ERR_PARSE, err);
    if (out->side_len != c->n) return fail(TAFL_ERR_PARSE, "FEN side length differs from the context's side_len");
    return TAFL_OK;
}

// BoardState::to_fen for one ABI state (host only).  Returns the length written (without the terminating NUL).
int tafl_state_to_fen(const tafl_state* st, uint32_t word_bits, char* out, uint32_t cap) {
    if (!st || !out || cap == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_state_to_fen: null argument");
    std::string f;
    if (state_to_fen(st, word_bits, &f)) return fail(TAFL_ERR_INVALID_ARG, "tafl_state_to_fen: bad word size / side length");
    if (f.size() + 1 > cap) return fail(TAFL_ERR_CAPACITY, "tafl_state_to_fen: buffer too small");
    memcpy(out, f.c_str(), f.size() + 1);
    return (int)f.size();
}

int tafl_batch_create(tafl_ctx* c, uint32_t n, tafl_batch** out) {
    if (!c || !out || n == 0) return fail(TAFL_ERR_INVALID_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    tafl_batch* b = new (std::nothrow) tafl_batch();
    if (!b) return fail(TAFL_ERR_OOM, "out of host memory");
    b->ctx = c; b->n = n;
    const size_t bytes = (size_t)quads_of(c) * n * sizeof(Quad);
    if (b->states.ensure(bytes)) { delete b; return fail(TAFL_ERR_OOM, "hipMalloc(batch states) failed"); }
    b->states.bind(b->soa);
    if (hipMemsetAsync(b->soa, 0, bytes, c->stream) != hipSuccess) { delete b; return fail(TAFL_ERR_HIP, "hipMemsetAsync failed"); }
    c->live_batches += 1;
    *out = b;
    return TAFL_OK;
}

int tafl_batch_destroy(tafl_batch* b) {
    if (!b) return TAFL_OK;
    if (b->ctx->live_batches > 0) b->ctx->live_batches -= 1;
    (void)hipSetDevice(b->ctx->device);
    for (uint32_t k = 0; k < b->n_sstreams; ++k) {           // a search in flight is abandoned: let its launches drain, then free
        (void)hipStreamSynchronize(b->sstream[k]); (void)hipStreamDestroy(b->sstream[k]); (void)hipEventDestroy(b->ev_fork[k]);
    }
    if (b->n_sstreams) { (void)hipEventDestroy(b->ev_start); (void)hipEventDestroy(b->ev_half); }
    (void)hipStreamSynchronize(b->ctx->stream);
    delete b;                                                // every DevBuf of the batch frees its memory
    return TAFL_OK;
}

uint32_t tafl_batch_size(const tafl_batch* b) { return b ? b->n : 0; }

int tafl_sync(tafl_ctx* c) {
    if (!c) return fail(TAFL_ERR_INVALID_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    return sync_ok(c);
}

int tafl_batch_reset_fen(tafl_batch* b, const char* fen, uint8_t side) {
    if (!b || !fen) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx;
    tafl_state st;
    int rc = tafl_state_from_fen(c, fen, side, &st);
    if (rc) return rc;
    if ((rc = batch_write(b)) != TAFL_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    dispatch<BATCH, false>(c, [&](auto t) {
        DState<t.NL> ds; state_from_abi<t.NL>(st, ds);
        LAUNCH_PER_GAME((k_fill<t.NL, t.W>), c, b->n, b->soa, b->n, ds); });
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}

int tafl_batch_upload(tafl_batch* b, const tafl_state* states, uint32_t first, uint32_t count) {
    if (!b || !states || count == 0 || first > b->n || count > b->n - first) return fail(TAFL_ERR_INVALID_ARG, "bad range");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int Q = quads_of(c);
    for (uint32_t i = 0; i < count; ++i)
        if (states[i].side_len != c->n) return fail(TAFL_ERR_INVALID_ARG, "state.side_len differs from the context's side_len");
    if (const int rc = batch_write(b)) return rc;
    std::vector<Quad> stage((size_t)Q * count);
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t v[24];
        dispatch<BATCH, false>(c, [&](auto t) { DState<t.NL> ds; state_from_abi<t.NL>(states[i], ds); StateIO<t.NL>::pack(ds, v); });
        for (int q = 0; q < Q; ++q) { Quad t; t.x = v[4 * q]; t.y = v[4 * q + 1]; t.z = v[4 * q + 2]; t.w = v[4 * q + 3]; stage[(size_t)q * count + i] = t; }
    }
    for (int q = 0; q < Q; ++q)
        HIPCHK(hipMemcpyAsync(b->soa + (size_t)q * b->n + first, stage.data() + (size_t)q * count, sizeof(Quad) * count, hipMemcpyHostToDevice, c->stream));
    return sync_ok(c);
}

int tafl_batch_download(tafl_batch* b, tafl_state* states, uint32_t first, uint32_t count) {
    if (!b || !states || count == 0 || first > b->n || count > b->n - first) return fail(TAFL_ERR_INVALID_ARG, "bad range");
    tafl_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int Q = quads_of(c);
    std::vector<Quad> stage((size_t)Q * count);
    for (int q = 0; q < Q; ++q)
        HIPCHK(hipMemcpyAsync(stage.data() + (size_t)q * count, b->soa + (size_t)q * b->n + first, sizeof(Quad) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t v[24];
        for (int q = 0; q < Q; ++q) { const Quad t = stage[(size_t)q * count + i]; v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w; }
        dispatch<BATCH, false>(c, [&](auto t) { DState<t.NL> ds; StateIO<t.NL>::unpack(v, ds); state_to_abi<t.NL>(ds, (uint8_t)c->n, states[i]); });
    }
    return TAFL_OK;
}

// ---- hot path --------------------------------------------------------------------------------------
int tafl_movegen(tafl_batch* b, uint32_t* out_counts, uint32_t* out_masks) {
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "null batch");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n, mw = tafl_action_mask_words(c);
    HIPCHK(hipSetDevice(c->device));
    NEED(b->counts, sizeof(uint32_t) * n);
    uint32_t* dmasks;
    STAGED(dmasks, b->masks, out_masks, (size_t)n * mw, 0);
    {
        SpanGuard sg(c, KC_MOVEGEN);
        dispatch<BATCH, false>(c, [&](auto t) {
            if (dmasks) hipLaunchKernelGGL((k_movegen_masks<t.NL, t.W>), dim3(grid_of(n)), dim3(TAFL_BLOCK * c->n), TAFL_BLOCK * ((mw | 1u) + 1u) * sizeof(uint32_t), c->stream,
                                           t.CC, b->soa, n, b->counts.as<uint32_t>(), dmasks, mw);
            else LAUNCH_PER_GAME((k_movegen<t.NL, t.W>), c, n, t.CC, b->soa, n, b->counts.as<uint32_t>()); });
    }
    HIPCHK(hipGetLastError());
    COPY_OUT(out_counts, b->counts.p, n, c->stream);
    COPY_OUT(out_masks, dmasks, (size_t)n * mw, c->stream);
    return sync_ok(c);
}

int tafl_validate(tafl_batch* b, const tafl_play* plays, uint8_t* out_codes) {
    if (!b || !plays || !out_codes) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->plays, sizeof(tafl_play) * n); NEED(b->codes, n);
    HIPCHK(hipMemcpyAsync(b->plays.p, plays, sizeof(tafl_play) * n, hipMemcpyHostToDevice, c->stream));
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_validate<t.NL, t.W>), c, n, t.CC, b->soa, n, b->plays.as<const tafl_play>(), b->codes.as<uint8_t>()); });
    HIPCHK(hipGetLastError());
    COPY_OUT(out_codes, b->codes.p, n, c->stream);
    return sync_ok(c);
}

int tafl_step(tafl_batch* b, const tafl_play* plays, tafl_effects* out_effects) {
    if (!b || !plays) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    if (const int rc = batch_write(b)) return rc;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->plays, sizeof(tafl_play) * n);
    tafl_effects* deff;
    STAGED(deff, b->effects, out_effects, n, 0);
    HIPCHK(hipMemcpyAsync(b->plays.p, plays, sizeof(tafl_play) * n, hipMemcpyHostToDevice, c->stream));
    {
        SpanGuard sg(c, KC_STEP);
        if (c->dense13) LAUNCH_PER_GAME(k_step_dense13, c, n, c->c8, c->c6, b->soa, n, b->plays.as<const tafl_play>(), deff);
        else dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_step<t.NL, t.W>), c, n, t.CC, b->soa, n, b->plays.as<const tafl_play>(), deff); });
    }
    HIPCHK(hipGetLastError());
    COPY_OUT(out_effects, deff, n, c->stream);
    return sync_ok(c);
}

int tafl_step_kth(tafl_batch* b, const uint32_t* ranks, tafl_play* out_plays, tafl_effects* out_effects) {
    if (!b || !ranks) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    if (const int rc = batch_write(b)) return rc;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->ranks, sizeof(uint32_t) * n); NEED(b->counts, sizeof(uint32_t) * 2 * (size_t)n);      // counts: chosen action and number of plays per game
    tafl_play* dplays; tafl_effects* deff;
    STAGED(dplays, b->out_plays, out_plays, n, 0);
    STAGED(deff, b->effects, out_effects, n, 0);
    HIPCHK(hipMemcpyAsync(b->ranks.p, ranks, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
    {
        SpanGuard sg(c, KC_STEP);
        const uint32_t mw = tafl_action_mask_words(c);
        uint32_t* actions = b->counts.as<uint32_t>(); uint32_t* totals = actions + n;
        dispatch<BATCH, false>(c, [&](auto t) {
            hipLaunchKernelGGL((k_select_kth<t.NL, t.W>), dim3(grid_of(n)), dim3(TAFL_BLOCK * c->n), TAFL_BLOCK * ((mw | 1u) + 1u + 17u) * sizeof(uint32_t), c->stream,
                               t.CC, b->soa, n, b->ranks.as<const uint32_t>(), actions, totals, mw); });
        if (c->dense13) LAUNCH_PER_GAME(k_step_action_dense13, c, n, c->c8, c->c6, b->soa, n, (const uint32_t*)actions, (const uint32_t*)totals, dplays, deff);
        else dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_step_action<t.NL, t.W>), c, n, t.CC, b->soa, n, (const uint32_t*)actions, (const uint32_t*)totals, dplays, deff); });
    }
    HIPCHK(hipGetLastError());
    COPY_OUT(out_plays, dplays, n, c->stream);
    COPY_OUT(out_effects, deff, n, c->stream);
    return sync_ok(c);
}

int tafl_side_can_play(tafl_batch* b, uint8_t side, uint8_t* out) {
    if (!b || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->u8out, n);
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_side_can_play<t.NL, t.W>), c, n, t.CC, b->soa, n, side ? 1u : 0u, b->u8out.as<uint8_t>()); });
    HIPCHK(hipGetLastError());
    COPY_OUT(out, b->u8out.p, n, c->stream);
    return sync_ok(c);
}

int tafl_rollout(tafl_batch* b, uint64_t seed, uint32_t sim, uint32_t max_plies, uint64_t game_id_base, tafl_rollout_result* out) {
    if (!b || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->results, sizeof(tafl_rollout_result) * n);
    {
        SpanGuard sg(c, KC_ROLLOUT);
        dispatch<ARENA, true>(c, [&](auto t) { LAUNCH_PER_GAME((k_rollout<t.NLS, t.WS, t.NL, t.W, t.PRESET>), c, n, t.CC, b->soa, n, seed, sim, max_plies, game_id_base, b->results.as<tafl_rollout_result>()); });
    }
    HIPCHK(hipGetLastError());
    COPY_OUT(out, b->results.p, n, c->stream);
    return sync_ok(c);
}

int tafl_random_advance(tafl_batch* b, uint64_t seed, const uint32_t* plies, uint64_t game_id_base) {
    if (!b || !plies) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n;
    if (const int rc = batch_write(b)) return rc;
    HIPCHK(hipSetDevice(c->device));
    NEED(b->plies, sizeof(uint32_t) * n);
    HIPCHK(hipMemcpyAsync(b->plies.p, plies, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
    dispatch<BATCH, true>(c, [&](auto t) { LAUNCH_PER_GAME((k_random_advance<t.NL, t.W, t.PRESET>), c, n, t.CC, b->soa, n, seed, b->plies.as<const uint32_t>(), game_id_base); });
    HIPCHK(hipGetLastError());
    return sync_ok(c);
}

// ---- training-tensor writers: outputs may be HOST or DEVICE pointers --------------------
int tafl_encode_boards(tafl_batch* b, uint8_t* out, int out_is_device) {
    if (!b || !out) return fail(TAFL_ERR_INVALID_ARG, "null argument");
    tafl_ctx* c = b->ctx; const uint32_t n = b->n; const size_t total = (size_t)n * c->n * c->n;
    HIPCHK(hipSetDevice(c->device));
    uint8_t* dst;
    STAGED(dst, b->enc, out, total, out_is_device);
    dispatch<BATCH, false>(c, [&](auto t) { hipLaunchKernelGGL((k_encode_boards<t.NL, t.W>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, t.CC, b->soa, n, dst); });
    HIPCHK(hipGetLastError());
    if (!out_is_device) COPY_OUT(out, dst, total, c->stream);
    return sync_ok(c);
}

// ---- timing ---------------------------------------------------------------------------------------------
int tafl_timing_enable(tafl_ctx* c, int enable) { if (!c) return fail(TAFL_ERR_INVALID_ARG, "null ctx"); c->timing = enable != 0; return TAFL_OK; }
int tafl_timing_reset(tafl_ctx* c) {
    if (!c) return fail(TAFL_ERR_INVALID_ARG, "null ctx");
    (void)hipSetDevice(c->device);
    drain_spans(c);
    for (int i = 0; i < KC_COUNT; ++i) { c->acc_ms[i] = 0; c->acc_n[i] = 0; c->ivals[i].clear(); }
    if (!c->has_ref) { if (hipEventCreate(&c->t_ref) != hipSuccess) return fail(TAFL_ERR_HIP, "hipEventCreate failed"); c->has_ref = true; }
    HIPCHK(hipEventRecord(c->t_ref, c->stream));
    HIPCHK(hipEventSynchronize(c->t_ref));
    return TAFL_OK;
}
// wall-clock time during which AT LEAST ONE launch of the class was running (union of the spans' intervals), and the sum of the spans:
// sum / union = how many launches of the class were in flight on average (partitions on their own streams overlap)
int tafl_timing_get_union(tafl_ctx* c, int cls, double* union_ms, double* sum_ms) {
    if (!c || cls < 0 || cls >= KC_COUNT) return fail(TAFL_ERR_INVALID_ARG, "bad kernel class");
    (void)hipSetDevice(c->device);
    drain_spans(c);
    std::vector<std::pair<float, float>> v = c->ivals[cls];
    std::sort(v.begin(), v.end());
    double u = 0.0, s = 0.0; float lo = 0.f, hi = -1.f;
    for (const auto& iv : v) {
        s += (double)iv.second - (double)iv.first;
        if (hi < lo) { lo = iv.first; hi = iv.second; }
        else if (iv.first <= hi) { if (iv.second > hi) hi = iv.second; }
        else { u += (double)hi - (double)lo; lo = iv.first; hi = iv.second; }
    }
    if (hi >= lo) u += (double)hi - (double)lo;
    if (union_ms) *union_ms = u;
    if (sum_ms) *sum_ms = s;
    return TAFL_OK;
}
int tafl_timing_get(tafl_ctx* c, int cls, double* total_ms, uint64_t* launches) {
    if (!c || cls < 0 || cls >= KC_COUNT) return fail(TAFL_ERR_INVALID_ARG, "bad kernel class");
    (void)hipSetDevice(c->device);
    drain_spans(c);
    if (total_ms) *total_ms = c->acc_ms[cls];
    if (launches) *launches = c->acc_n[cls];
    return TAFL_OK;
}

}  // extern "C"
