// tafl_examples.hip — training examples recorded on the device: k_examples_*, tafl_examples_* and tafl_selfplay_record.
#include "tafl_internal.hpp"

// z and the final mark of every recorded example whose result is open (all of them, unless an episodes run has closed some), from the
// CURRENT status of its game in the batch (tafl_examples_finalize): one lane per game
template <int NL>
__global__ __launch_bounds__(TAFL_BLOCK) void k_examples_finalize(const Quad* soa, ExamplesMem X, const uint32_t* open_from) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    if (g >= X.G) return;
    const uint32_t flags = soa[(size_t)((2 * NL + 4) / 4) * X.G + g].w;
    examples_settle(X, g, open_from[g], flags);
}

// Minibatch rows (tafl_examples_gather): row i = example index[i] under symmetry sym[i].  The dense policy row (4 * action_size bytes, at
// most K words non-zero) is built in LDS and streamed out with full-width stores: the row in LDS is all zero between two examples (every
// thread clears the words it has just read), so an example costs the scatter of its <= K entries, two barriers and the stream.  One
// workgroup serves examples blockIdx.x, blockIdx.x + gridDim.x, ...  VEC: `pi` is 16-byte aligned (action_size is a multiple of 4).
template <bool VEC>
__global__ __launch_bounds__(256) void k_examples_gather(ExamplesMem X, const uint32_t* index, const uint8_t* sym, uint32_t count, uint32_t n, uint32_t A,
                                                         uint8_t* boards, uint8_t* sides, float* pi, float* z, uint8_t* fin) {
    extern __shared__ __align__(16) float lds_row[];                          // [A]
    for (uint32_t v = threadIdx.x; v < A; v += 256) lds_row[v] = 0.0f;
    __syncthreads();
    const uint32_t nn = n * n;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t e = index[i], g = e % X.G, j = e / X.G;
        const bool ok = j < X.max_moves && j < X.len[g];          // (block-uniform)
        const uint32_t s = sym ? (sym[i] & 7u) : 0u;
        const uint32_t info = ok ? X.info[e] : 0u, nc = info & 0xFFFFu;
        if (pi && threadIdx.x < nc) {
            const double N = (double)(X.played[e] >> 16);          // sum of the Nsa, noted when the example was recorded
            for (uint32_t k = threadIdx.x; k < nc; k += 256) {
                const uint32_t w = X.pol[((size_t)j * X.K + k) * X.G + g], a = w & 0xFFFFu;
                lds_row[s ? sym_action(s, a, n) : a] = (float)((double)(w >> 16) / N);
            }
        }
        if (boards && threadIdx.x < nn) {
            const uint32_t t = threadIdx.x;
            const uint32_t w = ok ? X.boards[((size_t)j * X.BW + (t >> 2)) * X.G + g] : 0u;
            boards[(size_t)i * nn + (s ? sym_tile(s, t, n) : t)] = (uint8_t)(w >> (8u * (t & 3u)));
        }
        if (threadIdx.x == 0) {
            if (!ok) atomicAdd(&X.counters[EX_BAD_INDEX], 1ull);
            if (sides) sides[i] = (uint8_t)((info >> 16) & 0xFFu);
            if (z) z[i] = ok ? X.z[e] : 0.0f;
            if (fin) fin[i] = ok ? X.fin[e] : (uint8_t)0;
        }
        if (pi) {
            __syncthreads();
            if constexpr (VEC) {
                float4* dst = reinterpret_cast<float4*>(pi + (size_t)i * A); float4* src = reinterpret_cast<float4*>(lds_row);
                for (uint32_t v = threadIdx.x; v < A / 4u; v += 256) { dst[v] = src[v]; src[v] = make_float4(0.f, 0.f, 0.f, 0.f); }
            } else {
                float* dst = pi + (size_t)i * A;
                for (uint32_t v = threadIdx.x; v < A; v += 256) { dst[v] = lds_row[v]; lds_row[v] = 0.0f; }
            }
            __syncthreads();
        }
    }
}

// The two scalars of tafl_examples_gather_stats, one lane per row: value[i], surprise[i] of example index[i] (example_search_stats); an
// index that names no example gives zeros and is counted
__global__ __launch_bounds__(256) void k_examples_gather_stats(ExamplesMem X, ExampleStatsMem S, const uint32_t* index, uint32_t count, float* value, float* surprise) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t e = index[i], g = e % X.G, j = e / X.G;
    const bool ok = j < X.max_moves && j < X.len[g];
    float v = 0.0f, s = 0.0f;
    if (ok) example_search_stats(X, S, j, g, X.info[e], v, s);
    else atomicAdd(&X.counters[EX_BAD_INDEX], 1ull);
    if (value) value[i] = v;
    if (surprise) surprise[i] = s;
}

// tafl_examples_value_targets, pass 1: one lane per entry of the per-example arrays (consecutive g: a wave's loads of info, pol and cq
// coalesce), the search value and the participation bit staged in vt and kind
__global__ __launch_bounds__(256) void k_examples_vt_stage(ExamplesMem X, ExampleStatsMem S, ExampleTargetsMem T, uint32_t E) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (e < E) vt_stage(X, S, T, (uint32_t)e);
}
// pass 2: one lane per game walks its examples backward (entries j * G + g: a wave's accesses coalesce), the whole wave as far as its
// longest lane so that the four counters go through ballots; one flush per wave
__global__ __launch_bounds__(TAFL_BLOCK) void k_examples_vt_chain(ExamplesMem X, ExampleTargetsMem T, double lambda, uint32_t settle, unsigned long long* res) {
    const uint32_t g = blockIdx.x * TAFL_BLOCK + threadIdx.x;
    const uint32_t len = g < X.G ? (X.len[g] < X.max_moves ? X.len[g] : X.max_moves) : 0u;
    uint32_t top = len;
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)top, d, 64); top = o > top ? o : top; }
    VtChain c; c.A = 0.0; c.L = 1.0; c.u_last = 0.0; c.u_next = 0.0; c.mv_next = 0u; c.have = 0u; c.closed = 0u;
    uint32_t n[VT_COUNTERS] = {0u, 0u, 0u, 0u};
    for (uint32_t j = top; j-- > 0u;) {
        const uint32_t ev = j < len ? vt_step(X, T, j, g, lambda, settle != 0u, c) : 0u;
        n[VT_ROWS] += (uint32_t)__popcll(__ballot(ev & VT_EV_ROW));
        n[VT_CLOSED] += (uint32_t)__popcll(__ballot(ev & VT_EV_CLOSED));
        n[VT_UNFINISHED] += (uint32_t)__popcll(__ballot(ev & VT_EV_UNFINISHED));
        n[VT_SETTLED] += (uint32_t)__popcll(__ballot(ev & VT_EV_SETTLED));
    }
    if (threadIdx.x == 0)
        for (uint32_t k = 0; k < VT_COUNTERS; ++k) if (n[k]) atomicAdd(&res[k], (unsigned long long)n[k]);
}
// tafl_examples_gather_targets, one lane per row: an index that names no example gives zeros and is counted
__global__ __launch_bounds__(256) void k_examples_gather_targets(ExamplesMem X, ExampleTargetsMem T, const uint32_t* index, uint32_t count, float* target, uint8_t* kind, uint8_t* ep_end) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t e = index[i], g = e % X.G, j = e / X.G;
    const bool ok = j < X.max_moves && j < X.len[g];
    if (!ok) atomicAdd(&X.counters[EX_BAD_INDEX], 1ull);
    if (target) target[i] = ok ? T.vt[e] : 0.0f;
    if (kind) kind[i] = ok ? T.kind[e] : (uint8_t)0;
    if (ep_end) ep_end[i] = ok ? T.ep_end[e] : (uint8_t)0;
}

#define EXCHK(ex, name) do { if (!(ex)) return fail(TAFL_ERR_INVALID_ARG, name ": null examples object"); HIPCHK(hipSetDevice((ex)->ctx->device)); } while (0)

extern "C" {

int tafl_examples_create(tafl_ctx* c, uint32_t n_games, uint32_t max_moves, uint32_t max_children, tafl_examples** out) {
    return tafl_examples_create_ex(c, n_games, max_moves, max_children, 0u, out);
}
int tafl_examples_create_ex(tafl_ctx* c, uint32_t n_games, uint32_t max_moves, uint32_t max_children, uint32_t flags, tafl_examples** out) {
    if (flags & ~(uint32_t)(TAFL_EXAMPLES_SEARCH_STATS | TAFL_EXAMPLES_VALUE_TARGETS)) return fail(TAFL_ERR_UNSUPPORTED, "tafl_examples_create_ex: unknown flag bits");
    if ((flags & TAFL_EXAMPLES_VALUE_TARGETS) && !(flags & TAFL_EXAMPLES_SEARCH_STATS))
        return fail(TAFL_ERR_UNSUPPORTED, "tafl_examples_create_ex: TAFL_EXAMPLES_VALUE_TARGETS needs TAFL_EXAMPLES_SEARCH_STATS");
    if (!c || !out || n_games == 0 || max_moves == 0 || max_children == 0 || max_children > 0xFFFFu)
        return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_create: bad argument (n_games, max_moves >= 1, max_children in 1..65535)");
    if ((unsigned long long)n_games * max_moves > 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_create: n_games * max_moves exceeds 32 bits");
    HIPCHK(hipSetDevice(c->device));
    tafl_examples* x = new (std::nothrow) tafl_examples();
    if (!x) return fail(TAFL_ERR_OOM, "out of host memory");
    c->live_batches += 1;                                    // (the context outlives its examples objects as it outlives its batches)
    x->ctx = c; x->n_games = n_games; x->max_moves = max_moves; x->max_children = max_children; x->flags = flags;
    const size_t E = (size_t)n_games * max_moves, BW = ((size_t)c->n * c->n + 3) / 4;
    if (x->need(x->len, 4 * (size_t)n_games) || x->need(x->boards, 4 * E * BW) || x->need(x->info, 4 * E) || x->need(x->played, 4 * E) || x->need(x->move_no, 4 * E) ||
        x->need(x->pol, 4 * E * max_children) || x->need(x->z, 4 * E) || x->need(x->fin, E) || x->need(x->counters, 8 * EX_COUNTERS) ||
        x->need(x->open_from, 4 * (size_t)n_games) ||
        ((flags & TAFL_EXAMPLES_SEARCH_STATS) && (x->need(x->cq, 4 * E * max_children) || x->need(x->cp, 4 * E * max_children) || x->need(x->seen, 4 * (size_t)n_games))) ||
        ((flags & TAFL_EXAMPLES_VALUE_TARGETS) && (x->need(x->ep_end, E) || x->need(x->vt, 4 * E) || x->need(x->kind, E) || x->need(x->vt_res, 8 * VT_COUNTERS)))) {
        tafl_examples_destroy(x);
        return fail(TAFL_ERR_OOM, "hipMalloc failed (tafl_examples_create)");
    }
    ExamplesMem& M = x->mem;
    x->len.bind(M.len); x->boards.bind(M.boards); x->info.bind(M.info); x->played.bind(M.played); x->move_no.bind(M.move_no);
    x->pol.bind(M.pol); x->z.bind(M.z); x->fin.bind(M.fin); x->counters.bind(M.counters);
    if (flags & TAFL_EXAMPLES_SEARCH_STATS) { x->cq.bind(x->smem.cq); x->cp.bind(x->smem.cp); x->seen.bind(x->smem.seen); }
    if (flags & TAFL_EXAMPLES_VALUE_TARGETS) { x->ep_end.bind(x->tmem.ep_end); x->vt.bind(x->tmem.vt); x->kind.bind(x->tmem.kind); }
    M.G = n_games; M.max_moves = max_moves; M.K = max_children; M.BW = (uint32_t)BW;
    const int rc = tafl_examples_clear(x);
    if (rc) { tafl_examples_destroy(x); return rc; }
    *out = x;
    return TAFL_OK;
}
int tafl_examples_destroy(tafl_examples* x) {
    if (!x) return TAFL_OK;
    (void)hipSetDevice(x->ctx->device);
    (void)hipStreamSynchronize(x->ctx->stream);
    x->ctx->live_batches -= 1;
    delete x;                                                // every DevBuf of the object frees its memory
    return TAFL_OK;
}
int tafl_examples_clear(tafl_examples* x) {
    EXCHK(x, "tafl_examples_clear");
    hipStream_t s = x->ctx->stream;
    HIPCHK(hipMemsetAsync(x->len.p, 0, 4 * (size_t)x->n_games, s));
    HIPCHK(hipMemsetAsync(x->counters.p, 0, 8 * EX_COUNTERS, s));
    HIPCHK(hipMemsetAsync(x->open_from.p, 0, 4 * (size_t)x->n_games, s));
    if (x->seen.p) HIPCHK(hipMemsetAsync(x->seen.p, 0, 4 * (size_t)x->n_games, s));
    if (x->ep_end.p) {                                       // no boundary is known any more; vt and kind never hold anything but zeros or a result
        const size_t E = (size_t)x->n_games * x->max_moves;
        HIPCHK(hipMemsetAsync(x->ep_end.p, 0, E, s)); HIPCHK(hipMemsetAsync(x->vt.p, 0, 4 * E, s)); HIPCHK(hipMemsetAsync(x->kind.p, 0, E, s));
    }
    x->vt_valid = false;
    return sync_ok(x->ctx);
}
int tafl_examples_counts(tafl_examples* x, uint32_t* out_len, uint64_t* out_total) {
    EXCHK(x, "tafl_examples_counts");
    hipStream_t s = x->ctx->stream;
    std::vector<uint32_t> h(x->n_games);
    COPY_OUT(h.data(), x->len.p, x->n_games, s);
    HIPCHK(hipStreamSynchronize(s));
    uint64_t tot = 0;
    for (uint32_t g = 0; g < x->n_games; ++g) { tot += h[g]; if (out_len) out_len[g] = h[g]; }
    if (out_total) *out_total = tot;
    return TAFL_OK;
}
int tafl_examples_get_stats(tafl_examples* x, tafl_examples_stats* out) {
    EXCHK(x, "tafl_examples_get_stats");
    if (!out) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_get_stats: null argument");
    hipStream_t s = x->ctx->stream;
    unsigned long long h[EX_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, x->counters.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->dropped = h[EX_DROPPED]; out->overflowed = h[EX_OVERFLOWED]; out->bad_index = h[EX_BAD_INDEX];
    out->device_bytes = x->device_bytes;                     // (the staging of host-pointer gathers included)
    return TAFL_OK;
}

// tafl_selfplay_run with the play of the opening moves drawn from the visit counts and every move's training example left in `ex`
int tafl_selfplay_record(tafl_batch* b, const tafl_mcts_params* p, const tafl_selfplay_opts* o, uint32_t n_moves, uint64_t game_id_base, tafl_examples* ex, tafl_play* out_plays) {
    if (!p || !o || n_moves == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_record: bad argument");
    if (o->flags != 0 || o->_reserved[0] != 0 || o->_reserved[1] != 0 || o->_reserved[2] != 0) return fail(TAFL_ERR_UNSUPPORTED, "tafl_selfplay_opts: flags and reserved words must be 0");
    if (p->flags & TAFL_MCTS_FLAG_KEEP_TREE) return fail(TAFL_ERR_UNSUPPORTED, "tafl_selfplay_record: TAFL_MCTS_FLAG_KEEP_TREE is not supported (no re-root inside a self-play run)");
    if ((unsigned long long)n_moves * p->n_sims + p->sim_offset > 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_record: sim_offset + n_moves * n_sims exceeds 32 bits");
    if ((unsigned long long)o->move_base + n_moves > 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_record: move_base + n_moves exceeds 32 bits");
    if (p->n_sims > 0xFFFFu) return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_record: n_sims must be below 65536 (Nsa is stored in 16 bits)");
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_record: null batch");
    if (ex && (ex->n_games != b->n || ex->ctx->device != b->ctx->device || ex->ctx->n != b->ctx->n))
        return fail(TAFL_ERR_INVALID_ARG, "tafl_selfplay_record: the examples object was created for another batch size, board or device");
    if (ex && (ex->flags & TAFL_EXAMPLES_SEARCH_STATS)) return fail(TAFL_ERR_UNSUPPORTED, "tafl_selfplay_record: the examples object carries search statistics (TAFL_EXAMPLES_SEARCH_STATS), which a rollout-mode search has none of");
    SelfPlayRec rec{};
    if (ex) rec.ex = ex->mem;
    rec.sample_seed = o->sample_seed; rec.game_id_base = game_id_base; rec.temp_moves = o->temp_moves; rec.move_base = o->move_base;
    if (ex) { HIPCHK(hipSetDevice(ex->ctx->device)); HIPCHK(hipStreamSynchronize(ex->ctx->stream)); }      // (clears and gathers of another context's stream)
    return selfplay_finish(b, mcts_begin(b, p, game_id_base, nullptr, n_moves, &rec), n_moves, out_plays);
}

int tafl_examples_finalize(tafl_examples* x, tafl_batch* b) {
    EXCHK(x, "tafl_examples_finalize");
    if (!b) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_finalize: null batch");
    if (b->n != x->n_games || b->ctx->device != x->ctx->device) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_finalize: the batch has another size or device");
    if (const int rc = join_search(b)) return rc;
    tafl_ctx* c = b->ctx;
    if (c != x->ctx) HIPCHK(hipStreamSynchronize(x->ctx->stream));
    x->vt_valid = false;                                     // (z and final of the open tail change: the targets are stale)
    dispatch<BATCH, false>(c, [&](auto t) { LAUNCH_PER_GAME((k_examples_finalize<t.NL>), c, b->n, b->soa, x->mem, x->open_from.as<const uint32_t>()); });
    HIPCHK(hipGetLastError());
    return sync_ok(c);
}

// the sparse form of examples, for hosts that store or inspect them: host pointers, any output may be NULL
int tafl_examples_read(tafl_examples* x, const uint32_t* index, uint32_t count, uint32_t* n_children, uint8_t* overflow, uint32_t* played, uint32_t* move_no,
                       uint32_t* actions, uint32_t* visits) {
    EXCHK(x, "tafl_examples_read");
    if (!index && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_read: null index");
    hipStream_t s = x->ctx->stream;
    const size_t K = x->max_children, G = x->n_games;
    // the arrays are example-major in j: only the prefix up to the highest j asked for is copied
    size_t jmax = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const size_t j = index[i] / G;
        if (j >= x->max_moves) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_read: index " + std::to_string(index[i]) + " (row " + std::to_string(i) + ") names no recorded example");
        if (j > jmax) jmax = j;
    }
    const size_t E = count ? (jmax + 1) * G : 0;
    std::vector<uint32_t> len(G), info(E), pl(E), mv(E), pol((actions || visits) ? E * K : 0);
    if (count == 0) return TAFL_OK;
    COPY_OUT(len.data(), x->len.p, G, s);
    COPY_OUT(info.data(), x->info.p, E, s);
    COPY_OUT(pl.data(), x->played.p, E, s);
    COPY_OUT(mv.data(), x->move_no.p, E, s);
    if (!pol.empty()) COPY_OUT(pol.data(), x->pol.p, E * K, s);
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < count; ++i) {
        const size_t e = index[i], g = e % G, j = e / G;
        if (j >= x->max_moves || j >= len[g]) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_read: index " + std::to_string(index[i]) + " (row " + std::to_string(i) + ") names no recorded example");
        const uint32_t nc = info[e] & 0xFFFFu;
        if (n_children) n_children[i] = nc;
        if (overflow) overflow[i] = (info[e] & kExOverflow) ? 1 : 0;
        if (played) played[i] = pl[e] & 0xFFFFu;
        if (move_no) move_no[i] = mv[e];
        for (size_t k = 0; k < K && !pol.empty(); ++k) {
            const uint32_t w = k < nc ? pol[(j * K + k) * G + g] : 0u;
            if (actions) actions[(size_t)i * K + k] = w & 0xFFFFu;
            if (visits) visits[(size_t)i * K + k] = w >> 16;
        }
    }
    return TAFL_OK;
}

// Qsa and Ps of the stored children (TAFL_EXAMPLES_SEARCH_STATS), the slow path beside tafl_examples_read: host pointers, [count * K]
int tafl_examples_read_stats(tafl_examples* x, const uint32_t* index, uint32_t count, float* q, float* prior) {
    EXCHK(x, "tafl_examples_read_stats");
    if (!(x->flags & TAFL_EXAMPLES_SEARCH_STATS)) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_read_stats: the object was created without TAFL_EXAMPLES_SEARCH_STATS");
    if (!index && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_read_stats: null index");
    if (count == 0) return TAFL_OK;
    hipStream_t s = x->ctx->stream;
    const size_t K = x->max_children, G = x->n_games;
    size_t jmax = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const size_t j = index[i] / G;
        if (j >= x->max_moves) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_read_stats: index " + std::to_string(index[i]) + " (row " + std::to_string(i) + ") names no recorded example");
        if (j > jmax) jmax = j;
    }
    const size_t E = (jmax + 1) * G;
    std::vector<uint32_t> len(G), info(E); std::vector<float> hq(q ? E * K : 0), hp(prior ? E * K : 0);
    COPY_OUT(len.data(), x->len.p, G, s);
    COPY_OUT(info.data(), x->info.p, E, s);
    if (q) COPY_OUT(hq.data(), x->cq.p, E * K, s);
    if (prior) COPY_OUT(hp.data(), x->cp.p, E * K, s);
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < count; ++i) {
        const size_t e = index[i], g = e % G, j = e / G;
        if (j >= len[g]) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_read_stats: index " + std::to_string(index[i]) + " (row " + std::to_string(i) + ") names no recorded example");
        const uint32_t nc = example_stored_children(x->mem, info[e]);
        for (size_t k = 0; k < K; ++k) {
            if (q) q[(size_t)i * K + k] = k < nc ? hq[(j * K + k) * G + g] : 0.0f;
            if (prior) prior[(size_t)i * K + k] = k < nc ? hp[(j * K + k) * G + g] : 0.0f;
        }
    }
    return TAFL_OK;
}

static int examples_gather_launch(tafl_examples* x, const uint32_t* index, const uint8_t* sym, uint32_t count, uint8_t* boards, uint8_t* sides, float* pi, float* z, uint8_t* fin) {
    tafl_ctx* c = x->ctx;
    const uint32_t A = c->n * c->n * 2u * (c->n - 1u);
    const uint32_t grid = count < 8192u ? count : 8192u;
    if (((uintptr_t)pi & 15u) == 0)
        hipLaunchKernelGGL((k_examples_gather<true>), dim3(grid), dim3(256), A * sizeof(float), c->stream, x->mem, index, sym, count, c->n, A, boards, sides, pi, z, fin);
    else
        hipLaunchKernelGGL((k_examples_gather<false>), dim3(grid), dim3(256), A * sizeof(float), c->stream, x->mem, index, sym, count, c->n, A, boards, sides, pi, z, fin);
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}
#define EXNEED(buf, bytes) do { if (x->need(buf, bytes)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed"); } while (0)
int tafl_examples_gather(tafl_examples* x, const uint32_t* index, const uint8_t* sym, uint32_t count, uint8_t* boards, uint8_t* sides, float* pi, float* z, uint8_t* final_, int ptrs_are_device) {
    EXCHK(x, "tafl_examples_gather");
    if (!index && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather: null index");
    if (count == 0) return TAFL_OK;
    tafl_ctx* c = x->ctx; hipStream_t s = c->stream;
    if (ptrs_are_device) return examples_gather_launch(x, index, sym, count, boards, sides, pi, z, final_);       // (asynchronous on the context's stream, like the other device writers)
    // host pointers: every index is checked first, then the rows are gathered into device staging and copied out, a chunk at a time
    {
        std::vector<uint32_t> len(x->n_games);
        COPY_OUT(len.data(), x->len.p, x->n_games, s);
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t g = index[i] % x->n_games, j = index[i] / x->n_games;
            if (j >= x->max_moves || j >= len[g]) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather: index " + std::to_string(index[i]) + " (row " + std::to_string(i) + ") names no recorded example");
            if (sym && sym[i] > 7) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather: sym must be in 0..7");
        }
    }
    const size_t A = (size_t)c->n * c->n * 2u * (c->n - 1u), nn = (size_t)c->n * c->n;
    const uint32_t chunk = count < 8192u ? count : 8192u;       // (staging for what is asked for: a one-row gather holds one row)
    EXNEED(x->g_index, 4 * (size_t)chunk); EXNEED(x->g_sym, chunk); EXNEED(x->g_sides, chunk); EXNEED(x->g_z, 4 * (size_t)chunk); EXNEED(x->g_fin, chunk);
    if (boards) EXNEED(x->g_boards, nn * chunk);
    if (pi) EXNEED(x->g_pi, 4 * A * chunk);
    for (uint32_t i0 = 0; i0 < count; i0 += chunk) {
        const uint32_t k = count - i0 < chunk ? count - i0 : chunk;
        HIPCHK(hipMemcpyAsync(x->g_index.p, index + i0, 4 * (size_t)k, hipMemcpyHostToDevice, s));
        if (sym) HIPCHK(hipMemcpyAsync(x->g_sym.p, sym + i0, k, hipMemcpyHostToDevice, s));
        const int rc = examples_gather_launch(x, x->g_index.as<const uint32_t>(), sym ? x->g_sym.as<const uint8_t>() : nullptr, k, boards ? x->g_boards.as<uint8_t>() : nullptr,
                                              sides ? x->g_sides.as<uint8_t>() : nullptr, pi ? x->g_pi.as<float>() : nullptr, z ? x->g_z.as<float>() : nullptr, final_ ? x->g_fin.as<uint8_t>() : nullptr);
        if (rc) return rc;
        if (boards) COPY_OUT(boards + (size_t)i0 * nn, x->g_boards.p, nn * k, s);
        if (sides) COPY_OUT(sides + i0, x->g_sides.p, k, s);
        if (pi) COPY_OUT(pi + (size_t)i0 * A, x->g_pi.p, A * k, s);
        if (z) COPY_OUT(z + i0, x->g_z.p, k, s);
        if (final_) COPY_OUT(final_ + i0, x->g_fin.p, k, s);
        HIPCHK(hipStreamSynchronize(s));
    }
    return TAFL_OK;
}

// value and surprise per row (example_search_stats): with device pointers one asynchronous launch, a bad index gives zeros and is counted
int tafl_examples_gather_stats(tafl_examples* x, const uint32_t* index, uint32_t count, float* value, float* surprise, int ptrs_are_device) {
    EXCHK(x, "tafl_examples_gather_stats");
    if (!(x->flags & TAFL_EXAMPLES_SEARCH_STATS)) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather_stats: the object was created without TAFL_EXAMPLES_SEARCH_STATS");
    if (!index && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather_stats: null index");
    if (count == 0) return TAFL_OK;
    hipStream_t s = x->ctx->stream;
    const uint32_t grid = (uint32_t)(((unsigned long long)count + 255u) / 256u);
    if (ptrs_are_device) {
        hipLaunchKernelGGL(k_examples_gather_stats, dim3(grid), dim3(256), 0, s, x->mem, x->smem, index, count, value, surprise);
        HIPCHK(hipGetLastError());
        return TAFL_OK;
    }
    {
        std::vector<uint32_t> len(x->n_games);
        COPY_OUT(len.data(), x->len.p, x->n_games, s);
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t g = index[i] % x->n_games, j = index[i] / x->n_games;
            if (j >= x->max_moves || j >= len[g]) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather_stats: index " + std::to_string(index[i]) + " (row " + std::to_string(i) + ") names no recorded example");
        }
    }
    EXNEED(x->g_index, 4 * (size_t)count); EXNEED(x->g_z, 4 * (size_t)count); EXNEED(x->g_s, 4 * (size_t)count);
    HIPCHK(hipMemcpyAsync(x->g_index.p, index, 4 * (size_t)count, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_examples_gather_stats, dim3(grid), dim3(256), 0, s, x->mem, x->smem, x->g_index.as<const uint32_t>(), count, x->g_z.as<float>(), x->g_s.as<float>());
    HIPCHK(hipGetLastError());
    COPY_OUT(value, x->g_z.p, count, s);
    COPY_OUT(surprise, x->g_s.p, count, s);
    HIPCHK(hipStreamSynchronize(s));
    return TAFL_OK;
}

// the two passes of the value targets (include/taflhip.h): asynchronous up to the 32-byte read-back of the counters
int tafl_examples_value_targets(tafl_examples* x, const tafl_value_targets_cfg* cfg, tafl_value_targets_result* out) {
    EXCHK(x, "tafl_examples_value_targets");
    if (!cfg) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_value_targets: null argument");
    if (!(x->flags & TAFL_EXAMPLES_VALUE_TARGETS)) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_value_targets: the object was created without TAFL_EXAMPLES_VALUE_TARGETS");
    if (!(cfg->lambda >= 0.0 && cfg->lambda <= 1.0)) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_value_targets: lambda must be in [0, 1]");
    if (cfg->flags & ~(uint32_t)TAFL_VT_SETTLE_UNFINISHED) return fail(TAFL_ERR_UNSUPPORTED, "tafl_examples_value_targets: unknown flag bits");
    for (uint32_t r : cfg->_reserved) if (r) return fail(TAFL_ERR_UNSUPPORTED, "tafl_examples_value_targets: reserved words must be 0");
    hipStream_t s = x->ctx->stream;
    const uint32_t E = x->n_games * x->max_moves;
    unsigned long long* res = x->vt_res.as<unsigned long long>();
    x->vt_valid = false;
    HIPCHK(hipMemsetAsync(res, 0, 8 * VT_COUNTERS, s));
    hipLaunchKernelGGL(k_examples_vt_stage, dim3((uint32_t)(((unsigned long long)E + 255u) / 256u)), dim3(256), 0, s, x->mem, x->smem, x->tmem, E);
    hipLaunchKernelGGL(k_examples_vt_chain, dim3(grid_of(x->n_games)), dim3(TAFL_BLOCK), 0, s, x->mem, x->tmem, cfg->lambda, cfg->flags & (uint32_t)TAFL_VT_SETTLE_UNFINISHED, res);
    HIPCHK(hipGetLastError());
    unsigned long long h[VT_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    x->vt_valid = true;
    if (out) { out->episodes_closed = h[VT_CLOSED]; out->episodes_unfinished = h[VT_UNFINISHED]; out->rows_with_target = h[VT_ROWS]; out->rows_settled = h[VT_SETTLED]; }
    return TAFL_OK;
}

// vt, kind and ep_end per row: with device pointers one asynchronous launch, a bad index gives zeros and is counted
int tafl_examples_gather_targets(tafl_examples* x, const uint32_t* index, uint32_t count, float* target, uint8_t* kind, uint8_t* ep_end, int ptrs_are_device) {
    EXCHK(x, "tafl_examples_gather_targets");
    if (!(x->flags & TAFL_EXAMPLES_VALUE_TARGETS)) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather_targets: the object was created without TAFL_EXAMPLES_VALUE_TARGETS");
    if ((target || kind) && !x->vt_valid) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather_targets: the targets are stale (tafl_examples_value_targets has not run since the last clear, finalize or run)");
    if (!index && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather_targets: null index");
    if (count == 0) return TAFL_OK;
    hipStream_t s = x->ctx->stream;
    const uint32_t grid = (uint32_t)(((unsigned long long)count + 255u) / 256u);
    if (ptrs_are_device) {
        hipLaunchKernelGGL(k_examples_gather_targets, dim3(grid), dim3(256), 0, s, x->mem, x->tmem, index, count, target, kind, ep_end);
        HIPCHK(hipGetLastError());
        return TAFL_OK;
    }
    {
        std::vector<uint32_t> len(x->n_games);
        COPY_OUT(len.data(), x->len.p, x->n_games, s);
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t g = index[i] % x->n_games, j = index[i] / x->n_games;
            if (j >= x->max_moves || j >= len[g]) return fail(TAFL_ERR_INVALID_ARG, "tafl_examples_gather_targets: index " + std::to_string(index[i]) + " (row " + std::to_string(i) + ") names no recorded example");
        }
    }
    EXNEED(x->g_index, 4 * (size_t)count); EXNEED(x->g_z, 4 * (size_t)count); EXNEED(x->g_fin, count); EXNEED(x->g_k, count);
    HIPCHK(hipMemcpyAsync(x->g_index.p, index, 4 * (size_t)count, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_examples_gather_targets, dim3(grid), dim3(256), 0, s, x->mem, x->tmem, x->g_index.as<const uint32_t>(), count, target ? x->g_z.as<float>() : nullptr,
                       kind ? x->g_fin.as<uint8_t>() : nullptr, ep_end ? x->g_k.as<uint8_t>() : nullptr);
    HIPCHK(hipGetLastError());
    COPY_OUT(target, x->g_z.p, count, s);
    COPY_OUT(kind, x->g_fin.p, count, s);
    COPY_OUT(ep_end, x->g_k.p, count, s);
    HIPCHK(hipStreamSynchronize(s));
    return TAFL_OK;
}

}  // extern "C"
