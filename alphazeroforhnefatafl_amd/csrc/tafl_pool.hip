// tafl_pool.hip — the training pool on the device: k_pool_*, tafl_pool_*.
#include "tafl_internal.hpp"
#include "tafl_pool.hpp"

#define POOL_TILE 256            /* examples per workgroup of the ingest kernels: one thread each, in the order of the per-example arrays */
#define POOL_CHUNK 32            /* words of a row that pass through LDS at a time */
#define POOL_LDS_STRIDE 33       /* words between two examples in LDS: odd, so that 32 lanes storing one word each of 32 examples hit 32 banks,
                                    and 32 lanes reading the 8 quads of 4 examples do too (bank = (example + word) mod 32) */

// The flags of the tile's examples and where a taken one stands among the tile's taken ones: ballot and popcount in the wave, the four
// wave totals through LDS.  Returns the example's class (pool_take); lr = its rank in the tile, nt = the tile's taken examples.
__device__ __forceinline__ uint32_t pool_tile_flags(const ExamplesMem& X, uint32_t E, uint32_t* wave_tot, uint32_t& info, uint32_t& e, uint32_t& lr, uint32_t& nt) {
    const unsigned long long e64 = (unsigned long long)blockIdx.x * POOL_TILE + threadIdx.x;
    e = (uint32_t)e64;
    const uint32_t cls = e64 < E ? pool_take(X, e, info) : (uint32_t)POOL_NONE;
    const unsigned long long m = __ballot(cls == POOL_TAKEN);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    lr = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    nt = 0;
    for (uint32_t w = 0; w < POOL_TILE / 64; ++w) { const uint32_t c = wave_tot[w]; if (w < wave) lr += c; nt += c; }
    return cls;
}

// Ingest, pass 1: per tile the number of examples taken, skipped as open and skipped for overflow
__global__ __launch_bounds__(POOL_TILE) void k_pool_count(ExamplesMem X, uint32_t E, uint32_t* blk_taken, uint32_t* blk_open, uint32_t* blk_over) {
    __shared__ uint32_t wave_tot[POOL_TILE / 64], skipped[2];
    if (threadIdx.x < 2) skipped[threadIdx.x] = 0;
    uint32_t info, e, lr, nt;
    const uint32_t cls = pool_tile_flags(X, E, wave_tot, info, e, lr, nt);        // (its barrier also publishes the zeroes)
    const unsigned long long mo = __ballot(cls == POOL_OPEN), mv = __ballot(cls == POOL_OVERFLOW);
    if ((threadIdx.x & 63u) == 0) { atomicAdd(&skipped[0], (uint32_t)__popcll(mo)); atomicAdd(&skipped[1], (uint32_t)__popcll(mv)); }
    __syncthreads();
    if (threadIdx.x == 0) { blk_taken[blockIdx.x] = nt; blk_open[blockIdx.x] = skipped[0]; blk_over[blockIdx.x] = skipped[1]; }
}

// Ingest, pass 2: the exclusive prefix of the tiles' taken counts, by one workgroup that walks them POOL_TILE at a time with a carry (no
// width limit), and the three totals res = { T, skipped open, skipped overflow }
__global__ __launch_bounds__(POOL_TILE) void k_pool_scan(const uint32_t* blk_taken, const uint32_t* blk_open, const uint32_t* blk_over, uint32_t nb, uint32_t* prefix,
                                                         unsigned long long* res) {
    __shared__ uint32_t wave_tot[POOL_TILE / 64];
    __shared__ unsigned long long sums[2];
    if (threadIdx.x < 2) sums[threadIdx.x] = 0;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    unsigned long long open = 0, over = 0;
    for (uint32_t c0 = 0; c0 < nb; c0 += POOL_TILE) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t v = i < nb ? blk_taken[i] : 0u;
        if (i < nb) { open += blk_open[i]; over += blk_over[i]; }
        uint32_t incl = v;
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < POOL_TILE / 64; ++w) { const uint32_t c = wave_tot[w]; if (w < wave) before += c; total += c; }
        if (i < nb) prefix[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    atomicAdd(&sums[0], open); atomicAdd(&sums[1], over);
    __syncthreads();
    if (threadIdx.x == 0) { res[0] = carry; res[1] = sums[0]; res[2] = sums[1]; }
}

// Ingest, pass 3: the rows.  The examples' arrays are column-major (word w of example (j, g) at [(j * BW + w) * G + g]), so a wave reads
// one word of 64 consecutive examples per load; a row is contiguous, and the tile's taken examples have consecutive ranks, hence
// consecutive slots: the tile's rows are one contiguous piece of the pool (two where the ring wraps).  POOL_CHUNK words of every taken
// example go through LDS - example-major there - and leave as 16-byte stores, eight consecutive lanes per 128-byte piece of a row.
__global__ __launch_bounds__(POOL_TILE) void k_pool_copy(ExamplesMem X, uint32_t E, PoolMem P, const uint32_t* prefix, const unsigned long long* res,
                                                         unsigned long long written, uint32_t generation) {
    __shared__ uint32_t wave_tot[POOL_TILE / 64];
    __shared__ uint32_t tile[POOL_TILE * POOL_LDS_STRIDE];
    uint32_t info, e, lr, nt;
    const bool taken = pool_tile_flags(X, E, wave_tot, info, e, lr, nt) == POOL_TAKEN;
    if (nt == 0) return;                                                        // (block-uniform)
    const uint32_t T = (uint32_t)res[0], base = prefix[blockIdx.x], g = e % X.G, j = e / X.G;
    const uint32_t slot0 = (uint32_t)((written + base) % P.C);
    uint4* rows = reinterpret_cast<uint4*>(P.rows);
    for (uint32_t w0 = 0; w0 < P.RW; w0 += POOL_CHUNK) {
        const uint32_t cw = P.RW - w0 < POOL_CHUNK ? P.RW - w0 : POOL_CHUNK, qpr = cw / 4u;       // (RW is a multiple of 4)
        if (taken)
            for (uint32_t u0 = 0; u0 < cw; u0 += 4) {
                uint32_t v[4];
                TAFL_UNROLL for (uint32_t u = 0; u < 4; ++u) v[u] = pool_row_word(X, j, g, info, w0 + u0 + u, generation);
                TAFL_UNROLL for (uint32_t u = 0; u < 4; ++u) tile[lr * POOL_LDS_STRIDE + u0 + u] = v[u];
            }
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < nt * qpr; q += POOL_TILE) {
            const uint32_t row = q / qpr, wq = q % qpr;
            uint32_t slot;
            if (!pool_place(written, base + row, T, P.C, slot)) continue;
            unsigned long long s = (unsigned long long)slot0 + row;            // (the same slot, without a 64-bit division per quad)
            if (s >= P.C) s %= P.C;
            const uint32_t* src = tile + row * POOL_LDS_STRIDE + 4u * wq;
            rows[((size_t)s * P.RW + w0) / 4u + wq] = make_uint4(src[0], src[1], src[2], src[3]);
        }
        __syncthreads();
    }
}

// Ingest, the pass of a pool that carries search statistics (tafl_pool_set_search_stats): one lane per example in the order of the
// per-example arrays, so that a wave reads consecutive g; the rank comes from the prefix k_pool_copy used, through pool_tile_flags, and the
// two scalars of a stored example (example_search_stats, the functions of tafl_examples_gather_stats) go to its slot.  What the copy
// skips - the ranks below T - min(T, C) - is skipped here.
__global__ __launch_bounds__(POOL_TILE) void k_pool_ingest_stats(ExamplesMem X, ExampleStatsMem S, uint32_t E, const uint32_t* prefix, const unsigned long long* res,
                                                                 unsigned long long written, uint32_t C, float* value, float* surprise) {
    __shared__ uint32_t wave_tot[POOL_TILE / 64];
    uint32_t info, e, lr, nt;
    const bool taken = pool_tile_flags(X, E, wave_tot, info, e, lr, nt) == POOL_TAKEN;
    if (!taken) return;
    const uint32_t T = (uint32_t)res[0], rank = prefix[blockIdx.x] + lr, first = T - (T < C ? T : C);
    if (rank < first) return;
    float v, s;
    example_search_stats(X, S, e / X.G, e % X.G, info, v, s);
    const uint32_t slot = pool_stored_slot(written, rank - first, T, C);
    value[slot] = v; surprise[slot] = s;
}
// Ingest, the pass of a pool that carries value targets (tafl_pool_set_value_targets): the rank and the placement of k_pool_ingest_stats,
// vt and kind of a stored example copied to its slot
__global__ __launch_bounds__(POOL_TILE) void k_pool_ingest_targets(ExamplesMem X, ExampleTargetsMem T, uint32_t E, const uint32_t* prefix, const unsigned long long* res,
                                                                   unsigned long long written, uint32_t C, float* vt, uint8_t* kind) {
    __shared__ uint32_t wave_tot[POOL_TILE / 64];
    uint32_t info, e, lr, nt;
    const bool taken = pool_tile_flags(X, E, wave_tot, info, e, lr, nt) == POOL_TAKEN;
    if (!taken) return;
    const uint32_t Tn = (uint32_t)res[0], rank = prefix[blockIdx.x] + lr, first = Tn - (Tn < C ? Tn : C);
    if (rank < first) return;
    const uint32_t slot = pool_stored_slot(written, rank - first, Tn, C);
    vt[slot] = T.vt[e]; kind[slot] = T.kind[e];
}
// tafl_pool_gather_targets: zeros for a slot that is not live, counted
__global__ __launch_bounds__(256) void k_pool_gather_targets(const float* tv, const uint8_t* tk, unsigned long long* counters, const uint32_t* slot, uint32_t count, uint32_t first,
                                                             unsigned long long live, uint32_t C, float* target, uint8_t* kind) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = slot[i];
        const bool ok = pool_slot_live_from(s, first, live, C);
        if (!ok) atomicAdd(&counters[POOL_BAD_SLOT], 1ull);
        if (target) target[i] = ok ? tv[s] : 0.0f;
        if (kind) kind[i] = ok ? tk[s] : (uint8_t)0;
    }
}
// tafl_pool_gather_stats: zeros for a slot that is not live, counted
__global__ __launch_bounds__(256) void k_pool_gather_stats(const float* sv, const float* ss, unsigned long long* counters, const uint32_t* slot, uint32_t count, uint32_t first,
                                                           unsigned long long live, uint32_t C, float* value, float* surprise) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = slot[i];
        const bool ok = pool_slot_live_from(s, first, live, C);
        if (!ok) atomicAdd(&counters[POOL_BAD_SLOT], 1ull);
        if (value) value[i] = ok ? sv[s] : 0.0f;
        if (surprise) surprise[i] = ok ? ss[s] : 0.0f;
    }
}
// tafl_pool_weights_from_surprise: every live slot whose row has the generation (0: every live slot) is ASSIGNED pool_surprise_weight
__global__ __launch_bounds__(256) void k_poolw_from_surprise(uint32_t* wt, const float* ss, const uint32_t* rows, uint32_t RW, uint32_t gen_word, uint32_t first, unsigned long long live,
                                                             uint32_t C, uint32_t base, uint32_t generation, double per_nat) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < C; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = (uint32_t)i;
        if (!pool_slot_live_from(s, first, live, C)) continue;
        if (generation != 0u && rows[(size_t)s * RW + gen_word] != generation) continue;
        wt[s] = pool_surprise_weight(ss[s], base, per_nat);
    }
}

// Minibatch rows (tafl_pool_sample: DRAW, tafl_pool_gather: slot_in / sym_in): row i = the row of a slot under a symmetry, in the shape
// of k_examples_gather - the dense policy row is built in LDS, which is all zero between two rows, and streamed out with full-width
// stores - reading one contiguous row.  One workgroup serves rows blockIdx.x, blockIdx.x + gridDim.x, ...
template <bool DRAW, bool VEC>
__global__ __launch_bounds__(256) void k_pool_rows(PoolMem P, unsigned long long written, unsigned long long live, unsigned long long seed, unsigned long long step,
                                                   uint32_t row_base, uint32_t flags, const uint32_t* slot_in, const uint8_t* sym_in, uint32_t count, uint32_t n, uint32_t A,
                                                   uint8_t* boards, uint8_t* sides, float* pi, float* z, uint32_t* out_slot, uint8_t* out_sym) {
    extern __shared__ __align__(16) float lds_row[];                          // [A]
    for (uint32_t v = threadIdx.x; v < A; v += 256) lds_row[v] = 0.0f;
    __syncthreads();
    const uint32_t nn = n * n;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        uint32_t slot, s;                                                       // (block-uniform)
        if constexpr (DRAW) pool_draw(seed, step, row_base + i, written, live, P.C, flags, slot, s);
        else { slot = slot_in[i]; s = sym_in ? (sym_in[i] & 7u) : 0u; }
        const bool ok = DRAW || pool_slot_live(slot, written, live, P.C);
        const uint32_t* row = P.rows + (size_t)(ok ? slot : 0u) * P.RW;
        const uint32_t nc = ok ? pool_row_children(row, P.BW) : 0u;
        if (pi) for (uint32_t k = threadIdx.x; k < nc; k += 256) { uint32_t a; const float p = pool_out_pi(row, P.BW, k, n, s, a); lds_row[a] = p; }
        if (boards && threadIdx.x < nn) {
            uint32_t dst; const uint8_t v = pool_out_tile(row, threadIdx.x, n, s, dst);
            boards[(size_t)i * nn + dst] = ok ? v : (uint8_t)0;
        }
        if (threadIdx.x == 0) {
            if (!ok) atomicAdd(&P.counters[POOL_BAD_SLOT], 1ull);
            if (sides) sides[i] = ok ? pool_row_side(row, P.BW) : (uint8_t)0;
            if (z) z[i] = ok ? pool_row_z(row, P.BW) : 0.0f;
            if (out_slot) out_slot[i] = slot;
            if (out_sym) out_sym[i] = (uint8_t)s;
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

// ---- weighted sampling: per-slot weights, the tiles' prefix sums, the draw (tafl_pool.hpp: PoolWeights) ---------------------------------
// every slot of [0, n) receives v (tafl_pool_set_weighting, off -> on; the padding beyond C too, it is never live)
__global__ __launch_bounds__(256) void k_poolw_fill(uint32_t* wt, unsigned long long n, uint32_t v) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) wt[i] = v;
}
// Ingest, pass 4 (weighting on): the rows this ingest stored receive v.  res[0] = T as k_pool_scan left it.
__global__ __launch_bounds__(256) void k_poolw_ingest(uint32_t* wt, const unsigned long long* res, unsigned long long written, uint32_t C, uint32_t v) {
    const uint32_t T = (uint32_t)res[0], stored = T < C ? T : C;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < stored; i += (unsigned long long)gridDim.x * 256) wt[pool_stored_slot(written, (uint32_t)i, T, C)] = v;
}
// tafl_pool_set_weights, pass 1: 0 into every live slot named (a slot that is not live is skipped and counted, here only)
__global__ __launch_bounds__(256) void k_poolw_zero(PoolWeights W, const uint32_t* slot, uint32_t count, uint32_t first, unsigned long long live, uint32_t C) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = slot[i];
        if (pool_slot_live_from(s, first, live, C)) W.wt[s] = 0u;
        else atomicAdd(&W.res[PW_BAD_SLOT], 1ull);
    }
}
// pass 2: the maximum of the weights given for a slot, whatever the order
__global__ __launch_bounds__(256) void k_poolw_max(PoolWeights W, const uint32_t* slot, const uint32_t* weight, uint32_t count, uint32_t first, unsigned long long live, uint32_t C) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = slot[i];
        if (pool_slot_live_from(s, first, live, C)) atomicMax(&W.wt[s], weight[i]);
    }
}
// tafl_pool_get_weights: 0 for a slot that is not live
__global__ __launch_bounds__(256) void k_poolw_get(PoolWeights W, const uint32_t* slot, uint32_t count, uint32_t first, unsigned long long live, uint32_t C, uint32_t* out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = slot[i];
        out[i] = pool_slot_live_from(s, first, live, C) ? W.wt[s] : 0u;
    }
}
// a lane's four consecutive slots 4 * lane .. 4 * lane + 3 of tile t (one 16-byte load), the weights of the dead ones masked away
__device__ __forceinline__ void poolw_lane_eff(const PoolWeights& W, uint32_t t, uint32_t lane, uint32_t first, unsigned long long live, uint32_t C, uint32_t e[POOLW_PER_LANE]) {
    const uint4 v = reinterpret_cast<const uint4*>(W.wt)[(size_t)t * POOLW_LANES + lane];
    const uint32_t s0 = t * (uint32_t)POOLW_TILE + lane * (uint32_t)POOLW_PER_LANE;
    e[0] = pool_eff(v.x, s0, first, live, C); e[1] = pool_eff(v.y, s0 + 1u, first, live, C);
    e[2] = pool_eff(v.z, s0 + 2u, first, live, C); e[3] = pool_eff(v.w, s0 + 3u, first, live, C);
}
// Rebuild, pass 1: one wave per tile of 256 slots (four tiles per workgroup): the tile's sum of eff and its count of positive live slots
__global__ __launch_bounds__(256) void k_poolw_tiles(PoolWeights W, uint32_t first, unsigned long long live, uint32_t C) {
    const uint32_t lane = threadIdx.x & 63u, t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= W.NT) return;                                                     // (wave-uniform)
    uint32_t e[POOLW_PER_LANE];
    poolw_lane_eff(W, t, lane, first, live, C, e);
    unsigned long long sum = (unsigned long long)e[0] + e[1] + e[2] + e[3];
    uint32_t pos = (e[0] != 0u) + (e[1] != 0u) + (e[2] != 0u) + (e[3] != 0u);
    for (uint32_t d = 32; d; d >>= 1) { sum += __shfl_xor(sum, d, 64); pos += __shfl_xor(pos, d, 64); }
    if (lane == 0) { W.tile_sum[t] = sum; W.tile_pos[t] = pos; }
}
// Rebuild, pass 2: the exclusive prefix of the tiles' sums in 64 bits, by one workgroup that walks them 256 at a time with a carry as
// k_pool_scan does (no width limit), and res = { total, positive live slots }
__global__ __launch_bounds__(256) void k_poolw_scan(PoolWeights W) {
    __shared__ unsigned long long wave_tot[4], pos_tot[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = 0, positive = 0;
    for (uint32_t c0 = 0; c0 < W.NT; c0 += 256) {
        const uint32_t i = c0 + threadIdx.x;
        const unsigned long long v = i < W.NT ? W.tile_sum[i] : 0ull;
        unsigned long long pos = i < W.NT ? W.tile_pos[i] : 0ull;
        unsigned long long incl = v;
        for (uint32_t d = 1; d < 64; d <<= 1) { const unsigned long long u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
        for (uint32_t d = 32; d; d >>= 1) pos += __shfl_xor(pos, d, 64);
        if (lane == 63) { wave_tot[wave] = incl; pos_tot[wave] = pos; }
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (uint32_t w = 0; w < 4; ++w) { const unsigned long long c = wave_tot[w]; if (w < wave) before += c; total += c; positive += pos_tot[w]; }
        if (i < W.NT) W.tile_pre[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) { W.res[PW_TOTAL] = carry; W.res[PW_POSITIVE] = positive; }
}
// The weighted draw, one wave per row: the tile by pool_wsearch_* (64 prefixes per load, a ballot per step), then inside the tile a
// wave scan of the lanes' sums of four weights, a ballot for the lane and pool_wpick for the slot.  total > 0.
__global__ __launch_bounds__(256) void k_poolw_draw(PoolWeights W, uint32_t first, unsigned long long live, uint32_t C, unsigned long long seed, unsigned long long step,
                                                    uint32_t row_base, uint32_t flags, uint32_t count, unsigned long long total, uint32_t* out_slot, uint8_t* out_sym,
                                                    uint32_t* out_weight) {
    const uint32_t lane = threadIdx.x & 63u;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6); i < count; i += (unsigned long long)gridDim.x * 4u) {      // (wave-uniform)
        uint64_t k; uint32_t sym;
        pool_wdraw(seed, step, row_base + (uint32_t)i, total, flags, k, sym);
        uint32_t lo = 0, hi = W.NT;
        while (hi - lo > 1u) {
            uint32_t idx;
            const bool in = pool_wsearch_probe(lo, hi, lane, idx);
            const bool le = in && W.tile_pre[idx] <= k;
            pool_wsearch_narrow(lo, hi, (uint32_t)__popcll(__ballot(le)));
        }
        uint32_t e[POOLW_PER_LANE];
        poolw_lane_eff(W, lo, lane, first, live, C, e);
        const unsigned long long sum = (unsigned long long)e[0] + e[1] + e[2] + e[3], kk = k - W.tile_pre[lo];
        unsigned long long incl = sum;
        for (uint32_t d = 1; d < 64; d <<= 1) { const unsigned long long u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
        const unsigned long long excl = incl - sum;
        const uint32_t c = (uint32_t)__popcll(__ballot(excl <= kk)), L = c ? c - 1u : 0u;      // (excl ascends over the lanes, lane 0 holds 0)
        if (lane == L) {
            uint32_t w;
            const uint32_t j = pool_wpick(e[0], e[1], e[2], e[3], kk - excl, w);
            out_slot[i] = lo * (uint32_t)POOLW_TILE + L * (uint32_t)POOLW_PER_LANE + j;
            out_sym[i] = (uint8_t)sym;
            out_weight[i] = w;
        }
    }
}

// ---- de-duplication: the key of every live row, the groups in a hash table, the per-slot outputs (tafl_pool.hpp: pooldd_*) -----------------
#ifndef TAFL_POOLDD_AGGREGATE
#define TAFL_POOLDD_AGGREGATE 1      /* how k_pooldd_insert joins equal keys inside a wave: 1 runs of neighbouring lanes; the measurement compares with
                                        0 (every lane inserts its own row) and 2 (a loop over the wave's distinct keys, one leader each) */
#endif
// the slot of the live row of age rank a (first = the slot of rank 0)
__device__ __forceinline__ uint32_t pooldd_slot(uint32_t first, unsigned long long a, uint32_t C) { const unsigned long long s = first + a; return (uint32_t)(s >= C ? s - C : s); }
// Pass 1: key[s] and canon[s] of every live row.  A workgroup stages the board words and the info word of POOLDD_ROWS rows of consecutive
// age ranks - consecutive slots, contiguous memory but for the ring's end - in LDS with 16-byte loads, Q quads per row; eight lanes per
// row fold one symmetry each with byte reads from LDS and take the minimum (hash, symmetry) across the eight.  Without symmetries only
// the first lane of the eight folds.
__global__ __launch_bounds__(256) void k_pooldd_key(PoolMem P, uint32_t first, uint32_t live, uint32_t n, uint32_t Q, uint32_t symmetries, uint32_t key_bits,
                                                    unsigned long long* key, uint8_t* canon) {
    extern __shared__ __align__(16) uint32_t dd_rows[];                       // [POOLDD_ROWS][4 * Q]
    const uint32_t sub = threadIdx.x & 7u, lr = threadIdx.x >> 3, qpr = P.RW / 4u;
    const uint4* rows = reinterpret_cast<const uint4*>(P.rows);
    for (unsigned long long a0 = (unsigned long long)blockIdx.x * POOLDD_ROWS; a0 < live; a0 += (unsigned long long)gridDim.x * POOLDD_ROWS) {      // (block-uniform)
        const uint32_t nr = live - a0 < POOLDD_ROWS ? (uint32_t)(live - a0) : (uint32_t)POOLDD_ROWS;
        for (uint32_t q = threadIdx.x; q < nr * Q; q += 256) {
            const uint32_t row = q / Q, wq = q % Q;
            reinterpret_cast<uint4*>(dd_rows)[q] = rows[(size_t)pooldd_slot(first, a0 + row, P.C) * qpr + wq];
        }
        __syncthreads();
        if (lr < nr) {                                                          // (the eight lanes of a row together)
            const uint32_t* row = dd_rows + lr * 4u * Q;
            unsigned long long h = ~0ull; uint32_t c = sub;
            if (sub == 0u || symmetries) h = pooldd_hash(reinterpret_cast<const uint8_t*>(row), sub, n, P.BW, pool_row_side(row, P.BW));
            if (symmetries)
                for (uint32_t d = 1; d < 8u; d <<= 1) {
                    const unsigned long long oh = __shfl_xor(h, d, 8); const uint32_t oc = __shfl_xor(c, d, 8);
                    if (oh < h || (oh == h && oc < c)) { h = oh; c = oc; }
                }
            if (sub == 0u) { const uint32_t s = pooldd_slot(first, a0 + lr, P.C); key[s] = pooldd_key(h, key_bits); canon[s] = (uint8_t)c; }
        }
        __syncthreads();
    }
}
// Pass 2: one lane per live row, in the order of the age ranks, joins its key's entry (pooldd_insert) and stores the entry's index.  An
// ingest stores the examples e = j * G + g in ascending order, so the copies of a position reached by neighbouring games at the same move
// - the start position above all - sit in neighbouring slots: a run of equal keys in neighbouring lanes is inserted once, by its first
// lane, with the run's counts (ballots and popcounts, no loop), and rows without such a neighbour go on in parallel as they would alone.
template <int AGG>
__global__ __launch_bounds__(256) void k_pooldd_insert(PoolMem P, PoolDedupTable T, uint32_t first, uint32_t live, const unsigned long long* key, uint32_t* ent) {
    const uint32_t lane = threadIdx.x & 63u;
    for (unsigned long long a0 = (unsigned long long)blockIdx.x * 256 + (threadIdx.x - lane); a0 < live; a0 += (unsigned long long)gridDim.x * 256) {     // (wave-uniform)
        const unsigned long long a = a0 + lane;
        const bool in = a < live;
        uint32_t s = 0; unsigned long long k = 0; float z = 0.0f;
        if (in) { s = pooldd_slot(first, a, P.C); k = key[s]; z = pool_row_z(P.rows + (size_t)s * P.RW, P.BW); }
        const bool won = z == 1.0f, lost = z == -1.0f;
        uint32_t pos = 0;
        if constexpr (AGG == 2) {
            unsigned long long todo = __ballot(in);
            while (todo) {                                                      // (wave-uniform: one turn per distinct key of the wave)
                const int leader = __ffsll((long long)todo) - 1;
                const unsigned long long lk = __shfl(k, leader, 64);
                const bool same = in && k == lk;
                const unsigned long long m = __ballot(same), mw = __ballot(same && won), ml = __ballot(same && lost);
                uint32_t e = 0;
                if (lane == (uint32_t)leader)
                    e = pooldd_insert(T, lk, (uint32_t)__popcll(m), (uint32_t)__popcll(mw), (uint32_t)__popcll(ml), (uint32_t)a0 + 63u - (uint32_t)__clzll((long long)m));
                e = __shfl(e, leader, 64);
                if (same) pos = e;
                todo &= ~m;
            }
        } else if constexpr (AGG == 1) {
            const unsigned long long prev = __shfl_up(k, 1, 64);
            const bool head = in && (lane == 0u || k != prev);                  // (the lanes that are in are the first ones of the wave)
            const unsigned long long heads = __ballot(head), inm = __ballot(in), mw = __ballot(in && won), ml = __ballot(in && lost);
            uint32_t e = 0;
            if (head) {
                const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
                const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;
                const unsigned long long run = (end == 64u ? ~0ull : (1ull << end) - 1ull) & (~0ull << lane) & inm;
                e = pooldd_insert(T, k, (uint32_t)__popcll(run), (uint32_t)__popcll(run & mw), (uint32_t)__popcll(run & ml), (uint32_t)a0 + 63u - (uint32_t)__clzll((long long)run));
            }
            const unsigned long long upto = heads & ((2ull << lane) - 1ull);    // (lane 63: 2 << 63 wraps to 0, the mask is all ones)
            const uint32_t hl = upto ? 63u - (uint32_t)__clzll((long long)upto) : 0u;
            pos = __shfl(e, hl, 64);
        } else if (in) pos = pooldd_insert(T, k, 1u, won ? 1u : 0u, lost ? 1u : 0u, (uint32_t)a);
        if (in) ent[s] = pos;
    }
}
// Pass 3: one lane per live row reads its entry: rep, mult and zmean of its slot; a row that is not its group's representative compares
// its side and canonical image with the representative's.  A wave counts distinct and collisions by
// ballot and keeps its largest mult over all its turns, and flushes once at its end.
__global__ __launch_bounds__(256) void k_pooldd_finish(PoolMem P, PoolDedupTable T, uint32_t first, uint32_t live, uint32_t n, const uint32_t* ent, const uint8_t* canon,
                                                       uint32_t* rep, uint32_t* mult, float* zmean, unsigned long long* res) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t nd = 0, nc = 0, largest = 0;                                       // of this wave, over all its turns
    for (unsigned long long a0 = (unsigned long long)blockIdx.x * 256 + (threadIdx.x - lane); a0 < live; a0 += (unsigned long long)gridDim.x * 256) {     // (wave-uniform)
        const unsigned long long a = a0 + lane;
        bool is_rep = false, differs = false;
        uint32_t m = 0;
        if (a < live) {
            const uint32_t s = pooldd_slot(first, a, P.C), e = ent[s], r = pooldd_slot(first, T.newest[e], P.C);
            m = T.count[e];
            rep[s] = r; mult[s] = m; zmean[s] = pooldd_zmean(m, T.wins[e], T.losses[e]);
            is_rep = r == s;
            if (!is_rep) differs = !pooldd_same(P.rows + (size_t)s * P.RW, canon[s], P.rows + (size_t)r * P.RW, canon[r], n, P.BW);
        }
        nd += (uint32_t)__popcll(__ballot(is_rep)); nc += (uint32_t)__popcll(__ballot(differs));
        largest = m > largest ? m : largest;
    }
    for (uint32_t d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(largest, d, 64); largest = o > largest ? o : largest; }
    if (lane == 0u) {                                                           // (at most 8 192 waves: the grid is capped)
        if (nd) atomicAdd(&res[PDD_DISTINCT], (unsigned long long)nd);
        if (nc) atomicAdd(&res[PDD_COLLISIONS], (unsigned long long)nc);
        if (largest) atomicMax(&res[PDD_LARGEST], (unsigned long long)largest);
    }
}
// tafl_pool_weights_from_dedup: every live slot is ASSIGNED pooldd_weight
__global__ __launch_bounds__(256) void k_pooldd_weights(uint32_t* wt, const uint32_t* rep, const uint32_t* mult, uint32_t first, unsigned long long live, uint32_t C, uint32_t scale,
                                                        uint32_t flags) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < C; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = (uint32_t)i;
        if (!pool_slot_live_from(s, first, live, C)) continue;
        wt[s] = pooldd_weight(wt[s], mult[s], rep[s] == s, scale, flags);
    }
}
// tafl_pool_gather_dedup: zeros for a slot that is not live, counted
__global__ __launch_bounds__(256) void k_pooldd_gather(const uint32_t* drep, const uint32_t* dmult, const float* dz, unsigned long long* counters, const uint32_t* slot, uint32_t count,
                                                       uint32_t first, unsigned long long live, uint32_t C, uint32_t* rep, uint32_t* mult, float* zmean) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * 256) {
        const uint32_t s = slot[i];
        const bool ok = pool_slot_live_from(s, first, live, C);
        if (!ok) atomicAdd(&counters[POOL_BAD_SLOT], 1ull);
        if (rep) rep[i] = ok ? drep[s] : 0u;
        if (mult) mult[i] = ok ? dmult[s] : 0u;
        if (zmean) zmean[i] = ok ? dz[s] : 0.0f;
    }
}

struct tafl_pool {
    tafl_ctx* ctx;
    PoolMem mem;
    PoolBook book;                       // written, live, ingests and the rows per generation
    uint64_t skipped_open = 0, skipped_overflow = 0;
    DevBuf rows, counters, blk, res;
    DevBuf g_slot, g_sym, g_boards, g_sides, g_pi, g_z;      // staging of calls with host pointers
    size_t device_bytes = 0;
    int need(DevBuf& d, size_t bytes) { device_bytes -= d.cap; const int rc = d.ensure(bytes); device_bytes += d.cap; return rc; }
    // weighted sampling (off: no buffer of it exists)
    bool weighting = false, dirty = true;
    uint32_t ingest_weight = 0;
    uint64_t total = 0, positive = 0, rebuilds = 0;          // total, positive: as of the last rebuild
    PoolWeights wmem{};
    DevBuf wt, wtiles, wres, w_slot, w_sym, w_weight;        // w_*: the draw and its staging
    size_t weight_bytes = 0;
    int wneed(DevBuf& d, size_t bytes) { const size_t before = d.cap; const int rc = need(d, bytes); weight_bytes += d.cap - before; return rc; }
    void wfree() {
        for (DevBuf* d : {&wt, &wtiles, &wres, &w_slot, &w_sym, &w_weight}) { device_bytes -= d->cap; d->release(); }
        weight_bytes = 0; weighting = false; wmem = PoolWeights{};
    }
    // search statistics per row (tafl_pool_set_search_stats; off: no buffer of it exists): value and surprise of the row in slot s
    bool search_stats = false;
    DevBuf s_value, s_surprise, g_s;     // g_s: staging of the second scalar of a host-pointer tafl_pool_gather_stats
    // value targets per row (tafl_pool_set_value_targets; off: no buffer of it exists): vt and kind of the row in slot s
    bool value_targets = false;
    DevBuf t_vt, t_kind, g_k;            // g_k: staging of the kinds of a host-pointer tafl_pool_gather_targets
    // de-duplication (tafl_pool_dedup; before the first call and after tafl_pool_dedup(pool, NULL, ..): no buffer of it exists)
    bool dd_valid = false;               // a result stands: no ingest, trim or clear since the last tafl_pool_dedup
    DevBuf dd_rep, dd_mult, dd_zmean, dd_canon, dd_key, dd_ent, dd_table, dd_res, dd_stage;     // dd_stage: slot, rep, mult, zmean of a host-pointer gather
    size_t dedup_bytes = 0;
    int ddneed(DevBuf& d, size_t bytes) { const size_t before = d.cap; const int rc = need(d, bytes); dedup_bytes += d.cap - before; return rc; }
    void ddfree() {
        for (DevBuf* d : {&dd_rep, &dd_mult, &dd_zmean, &dd_canon, &dd_key, &dd_ent, &dd_table, &dd_res, &dd_stage}) { device_bytes -= d->cap; d->release(); }
        dedup_bytes = 0; dd_valid = false;
    }
    uint32_t first_live() const { return book.live ? pool_first_live(book.written, book.live, mem.C) : 0u; }
};

#define POOLCHK(p, name) do { if (!(p)) return fail(TAFL_ERR_INVALID_ARG, name ": null pool"); HIPCHK(hipSetDevice((p)->ctx->device)); } while (0)
#define POOLNEED(buf, bytes) do { if (p->need(buf, bytes)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed"); } while (0)

// one launch of k_pool_rows on the context's stream; every pointer is a device pointer
static int pool_rows_launch(tafl_pool* p, bool draw, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t flags, const uint32_t* slot, const uint8_t* sym, uint32_t count,
                            uint8_t* boards, uint8_t* sides, float* pi, float* z, uint32_t* out_slot, uint8_t* out_sym) {
    tafl_ctx* c = p->ctx;
    const uint32_t A = c->n * c->n * 2u * (c->n - 1u);
    const uint32_t grid = count < 8192u ? count : 8192u;
    const bool vec = ((uintptr_t)pi & 15u) == 0;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), A * sizeof(float), c->stream, p->mem, (unsigned long long)p->book.written, (unsigned long long)p->book.live,
                           (unsigned long long)seed, (unsigned long long)step, row_base, flags, slot, sym, count, c->n, A, boards, sides, pi, z, out_slot, out_sym);
    };
    if (draw) { if (vec) go(k_pool_rows<true, true>); else go(k_pool_rows<true, false>); }
    else { if (vec) go(k_pool_rows<false, true>); else go(k_pool_rows<false, false>); }
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}
// tafl_pool_sample (draw) and tafl_pool_gather: with host pointers the rows are written into device staging and copied out, a chunk at a time
static int pool_rows(tafl_pool* p, bool draw, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t flags, const uint32_t* slot, const uint8_t* sym, uint32_t count,
                     uint8_t* boards, uint8_t* sides, float* pi, float* z, uint32_t* out_slot, uint8_t* out_sym, int ptrs_are_device) {
    if (ptrs_are_device) return pool_rows_launch(p, draw, seed, step, row_base, flags, slot, sym, count, boards, sides, pi, z, out_slot, out_sym);
    tafl_ctx* c = p->ctx; hipStream_t s = c->stream;
    const size_t A = (size_t)c->n * c->n * 2u * (c->n - 1u), nn = (size_t)c->n * c->n;
    const uint32_t chunk = count < 8192u ? count : 8192u;
    POOLNEED(p->g_slot, 4 * (size_t)chunk); POOLNEED(p->g_sym, chunk); POOLNEED(p->g_sides, chunk); POOLNEED(p->g_z, 4 * (size_t)chunk);
    if (boards) POOLNEED(p->g_boards, nn * chunk);
    if (pi) POOLNEED(p->g_pi, 4 * A * chunk);
    for (uint32_t i0 = 0; i0 < count; i0 += chunk) {
        const uint32_t k = count - i0 < chunk ? count - i0 : chunk;
        if (!draw) {
            HIPCHK(hipMemcpyAsync(p->g_slot.p, slot + i0, 4 * (size_t)k, hipMemcpyHostToDevice, s));
            if (sym) HIPCHK(hipMemcpyAsync(p->g_sym.p, sym + i0, k, hipMemcpyHostToDevice, s));
        }
        const int rc = pool_rows_launch(p, draw, seed, step, row_base + i0, flags, p->g_slot.as<const uint32_t>(), (!draw && sym) ? p->g_sym.as<const uint8_t>() : nullptr, k,
                                        boards ? p->g_boards.as<uint8_t>() : nullptr, sides ? p->g_sides.as<uint8_t>() : nullptr, pi ? p->g_pi.as<float>() : nullptr,
                                        z ? p->g_z.as<float>() : nullptr, (draw && out_slot) ? p->g_slot.as<uint32_t>() : nullptr, (draw && out_sym) ? p->g_sym.as<uint8_t>() : nullptr);
        if (rc) return rc;
        if (boards) COPY_OUT(boards + (size_t)i0 * nn, p->g_boards.p, nn * k, s);
        if (sides) COPY_OUT(sides + i0, p->g_sides.p, k, s);
        if (pi) COPY_OUT(pi + (size_t)i0 * A, p->g_pi.p, A * k, s);
        if (z) COPY_OUT(z + i0, p->g_z.p, k, s);
        if (draw && out_slot) COPY_OUT(out_slot + i0, p->g_slot.p, k, s);
        if (draw && out_sym) COPY_OUT(out_sym + i0, p->g_sym.p, k, s);
        HIPCHK(hipStreamSynchronize(s));
    }
    return TAFL_OK;
}

extern "C" {

int tafl_pool_create(tafl_ctx* c, uint32_t capacity, uint32_t max_children, tafl_pool** out) {
    if (!c || !out || capacity == 0 || max_children == 0 || max_children > 0xFFFFu)
        return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_create: bad argument (capacity >= 1, max_children in 1..65535)");
    HIPCHK(hipSetDevice(c->device));
    tafl_pool* p = new (std::nothrow) tafl_pool();
    if (!p) return fail(TAFL_ERR_OOM, "out of host memory");
    c->live_batches += 1;                                    // (the context outlives its pools as it outlives its batches)
    p->ctx = c;
    PoolMem& M = p->mem;
    M.C = capacity; M.Kp = max_children; M.BW = (c->n * c->n + 3u) / 4u; M.RW = pool_row_words(M.BW, M.Kp);
    if (p->need(p->rows, 4 * (size_t)capacity * M.RW) || p->need(p->counters, 8 * POOL_COUNTERS) || p->need(p->res, 8 * 3)) {
        tafl_pool_destroy(p);
        return fail(TAFL_ERR_OOM, "hipMalloc failed (tafl_pool_create)");
    }
    p->rows.bind(M.rows); p->counters.bind(M.counters);
    const int rc = tafl_pool_clear(p);
    if (rc) { tafl_pool_destroy(p); return rc; }
    *out = p;
    return TAFL_OK;
}
int tafl_pool_destroy(tafl_pool* p) {
    if (!p) return TAFL_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    p->ctx->live_batches -= 1;
    delete p;
    return TAFL_OK;
}
int tafl_pool_clear(tafl_pool* p) {
    POOLCHK(p, "tafl_pool_clear");
    HIPCHK(hipMemsetAsync(p->counters.p, 0, 8 * POOL_COUNTERS, p->ctx->stream));
    if (p->weighting) HIPCHK(hipMemsetAsync(p->wres.p, 0, 8 * PW_WORDS, p->ctx->stream));
    p->book.clear(); p->skipped_open = p->skipped_overflow = 0;
    p->dd_valid = false;
    p->dirty = true; p->total = p->positive = p->rebuilds = 0;          // (the setting of the weighting and the stored weights stay)
    return sync_ok(p->ctx);
}
int tafl_pool_get_stats(tafl_pool* p, tafl_pool_stats* out) {
    POOLCHK(p, "tafl_pool_get_stats");
    if (!out) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_get_stats: null argument");
    unsigned long long h[POOL_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, p->counters.p, sizeof h, hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    memset(out, 0, sizeof *out);
    out->written = p->book.written; out->live = p->book.live; out->ingests = p->book.ingests; out->oldest_generation = p->book.oldest_generation();
    out->skipped_open = p->skipped_open; out->skipped_overflow = p->skipped_overflow; out->bad_slot = h[POOL_BAD_SLOT];
    out->device_bytes = p->device_bytes;
    return TAFL_OK;
}

int tafl_pool_ingest(tafl_pool* p, tafl_examples* ex, tafl_pool_ingest_result* out) {
    POOLCHK(p, "tafl_pool_ingest");
    if (!ex) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_ingest: null examples object");
    if (ex->ctx != p->ctx) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_ingest: the examples object belongs to another context (board size or device)");
    if (ex->max_children > p->mem.Kp) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_ingest: the examples hold more policy entries (max_children) than a row of the pool");
    if (p->book.ingests >= 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_ingest: the generation exceeds 32 bits");
    if (p->search_stats && !(ex->flags & TAFL_EXAMPLES_SEARCH_STATS))
        return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_ingest: the pool carries search statistics, the examples object was created without TAFL_EXAMPLES_SEARCH_STATS");
    if (p->value_targets && !((ex->flags & TAFL_EXAMPLES_VALUE_TARGETS) && ex->vt_valid))
        return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_ingest: the pool carries value targets, the examples object was created without TAFL_EXAMPLES_VALUE_TARGETS or its targets are stale");
    tafl_ctx* c = p->ctx; hipStream_t s = c->stream;
    p->dd_valid = false;
    const uint32_t E = ex->n_games * ex->max_moves, nb = (uint32_t)(((unsigned long long)E + POOL_TILE - 1) / POOL_TILE);       // (E fits 32 bits: tafl_examples_create)
    POOLNEED(p->blk, 16 * (size_t)nb);
    uint32_t* taken = p->blk.as<uint32_t>(); uint32_t* open = taken + nb; uint32_t* over = open + nb; uint32_t* prefix = over + nb;
    unsigned long long* res = p->res.as<unsigned long long>();
    const uint32_t generation = (uint32_t)(p->book.ingests + 1);
    hipLaunchKernelGGL(k_pool_count, dim3(nb), dim3(POOL_TILE), 0, s, ex->mem, E, taken, open, over);
    hipLaunchKernelGGL(k_pool_scan, dim3(1), dim3(POOL_TILE), 0, s, (const uint32_t*)taken, (const uint32_t*)open, (const uint32_t*)over, nb, prefix, res);
    hipLaunchKernelGGL(k_pool_copy, dim3(nb), dim3(POOL_TILE), 0, s, ex->mem, E, p->mem, (const uint32_t*)prefix, (const unsigned long long*)res,
                       (unsigned long long)p->book.written, generation);
    if (p->search_stats)
        hipLaunchKernelGGL(k_pool_ingest_stats, dim3(nb), dim3(POOL_TILE), 0, s, ex->mem, ex->smem, E, (const uint32_t*)prefix, (const unsigned long long*)res,
                           (unsigned long long)p->book.written, p->mem.C, p->s_value.as<float>(), p->s_surprise.as<float>());
    if (p->value_targets)
        hipLaunchKernelGGL(k_pool_ingest_targets, dim3(nb), dim3(POOL_TILE), 0, s, ex->mem, ex->tmem, E, (const uint32_t*)prefix, (const unsigned long long*)res,
                           (unsigned long long)p->book.written, p->mem.C, p->t_vt.as<float>(), p->t_kind.as<uint8_t>());
    if (p->weighting) {
        const uint32_t most = E < p->mem.C ? E : p->mem.C, grid = std::min<uint32_t>((most + 255u) / 256u, 2048u);       // (T <= E rows at most)
        if (grid) hipLaunchKernelGGL(k_poolw_ingest, dim3(grid), dim3(256), 0, s, p->wmem.wt, (const unsigned long long*)res, (unsigned long long)p->book.written, p->mem.C, p->ingest_weight);
        p->dirty = true;
    }
    HIPCHK(hipGetLastError());
    unsigned long long h[3];
    HIPCHK(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    p->book.took(h[0], p->mem.C); p->skipped_open += h[1]; p->skipped_overflow += h[2];
    if (out) { out->taken = h[0]; out->skipped_open = h[1]; out->skipped_overflow = h[2]; out->_reserved = 0; }
    return TAFL_OK;
}

int tafl_pool_trim(tafl_pool* p, uint32_t keep_generations) {
    POOLCHK(p, "tafl_pool_trim");
    if (keep_generations == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_trim: keep_generations must be at least 1");
    p->book.trim(keep_generations);
    p->dirty = true; p->dd_valid = false;
    return TAFL_OK;
}

int tafl_pool_sample(tafl_pool* p, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t count, uint32_t flags, uint8_t* boards, uint8_t* sides, float* pi, float* z,
                     uint32_t* out_slot, uint8_t* out_sym, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_sample");
    if (flags & ~(uint32_t)TAFL_POOL_SAMPLE_SYM) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_sample: unknown flag bits");
    if ((unsigned long long)row_base + count > 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_sample: row_base + count exceeds 32 bits");
    if (p->book.live == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_sample: the pool holds no live row");
    if (count == 0) return TAFL_OK;
    return pool_rows(p, true, seed, step, row_base, flags, nullptr, nullptr, count, boards, sides, pi, z, out_slot, out_sym, ptrs_are_device);
}

int tafl_pool_gather(tafl_pool* p, const uint32_t* slot, const uint8_t* sym, uint32_t count, uint8_t* boards, uint8_t* sides, float* pi, float* z, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_gather");
    if (!slot && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather: null slot");
    if (count == 0) return TAFL_OK;
    if (!ptrs_are_device)
        for (uint32_t i = 0; i < count; ++i) {
            if (!pool_slot_live(slot[i], p->book.written, p->book.live, p->mem.C)) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather: slot " + std::to_string(slot[i]) + " (row " + std::to_string(i) + ") is not live");
            if (sym && sym[i] > 7) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather: sym must be in 0..7");
        }
    return pool_rows(p, false, 0, 0, 0, 0, slot, sym, count, boards, sides, pi, z, nullptr, nullptr, ptrs_are_device);
}

// the sparse form of rows, for hosts that store or inspect them: one copy of the span of rows between the lowest and the highest slot asked for
int tafl_pool_read(tafl_pool* p, const uint32_t* slot, uint32_t count, uint32_t* n_children, uint32_t* move_no, uint32_t* generation, uint32_t* actions, uint32_t* visits) {
    POOLCHK(p, "tafl_pool_read");
    if (!slot && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_read: null slot");
    if (count == 0) return TAFL_OK;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t i = 0; i < count; ++i) {
        if (!pool_slot_live(slot[i], p->book.written, p->book.live, p->mem.C)) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_read: slot " + std::to_string(slot[i]) + " (row " + std::to_string(i) + ") is not live");
        lo = std::min(lo, slot[i]); hi = std::max(hi, slot[i]);
    }
    const size_t RW = p->mem.RW, Kp = p->mem.Kp, BW = p->mem.BW;
    std::vector<uint32_t> h(((size_t)hi - lo + 1) * RW);
    HIPCHK(hipMemcpyAsync(h.data(), p->mem.rows + (size_t)lo * RW, 4 * h.size(), hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t* row = h.data() + ((size_t)slot[i] - lo) * RW;
        if (n_children) n_children[i] = pool_row_children(row, (uint32_t)BW);
        if (move_no) move_no[i] = row[BW + PR_MOVE_NO];
        if (generation) generation[i] = row[BW + PR_GENERATION];
        for (size_t k = 0; k < Kp; ++k) {
            const uint32_t w = row[BW + PR_HEAD + k];
            if (actions) actions[(size_t)i * Kp + k] = w & 0xFFFFu;
            if (visits) visits[(size_t)i * Kp + k] = w >> 16;
        }
    }
    return TAFL_OK;
}

}  // extern "C"

// ---- weighted sampling ---------------------------------------------------------------------------------------------------------------------
static uint32_t poolw_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>((items + 255u) / 256u, 2048u); }
// the tiles' sums and prefixes follow the weights and the live window again; total and positive come back (16 bytes)
static int poolw_rebuild(tafl_pool* p) {
    if (!p->dirty) return TAFL_OK;
    hipStream_t s = p->ctx->stream;
    const uint32_t first = p->first_live();
    hipLaunchKernelGGL(k_poolw_tiles, dim3((p->wmem.NT + 3u) / 4u), dim3(256), 0, s, p->wmem, first, (unsigned long long)p->book.live, p->mem.C);
    hipLaunchKernelGGL(k_poolw_scan, dim3(1), dim3(256), 0, s, p->wmem);
    HIPCHK(hipGetLastError());
    unsigned long long h[2];
    HIPCHK(hipMemcpyAsync(h, p->wres.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    p->total = h[PW_TOTAL]; p->positive = h[PW_POSITIVE]; p->rebuilds += 1; p->dirty = false;
    return TAFL_OK;
}
// the slots (and weights) of a call in device memory: the caller's own arrays, or copies of the host's in the weighting's staging
static int poolw_stage_in(tafl_pool* p, const uint32_t*& slot, const uint32_t*& weight, uint32_t count, int ptrs_are_device, const char* name) {
    if (ptrs_are_device) return TAFL_OK;
    for (uint32_t i = 0; i < count; ++i)
        if (!pool_slot_live(slot[i], p->book.written, p->book.live, p->mem.C)) return fail(TAFL_ERR_INVALID_ARG, std::string(name) + ": slot " + std::to_string(slot[i]) + " (entry " + std::to_string(i) + ") is not live");
    if (p->wneed(p->w_slot, 4 * (size_t)count)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed");
    HIPCHK(hipMemcpyAsync(p->w_slot.p, slot, 4 * (size_t)count, hipMemcpyHostToDevice, p->ctx->stream));
    slot = p->w_slot.as<const uint32_t>();
    if (weight) {
        if (p->wneed(p->w_weight, 4 * (size_t)count)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed");
        HIPCHK(hipMemcpyAsync(p->w_weight.p, weight, 4 * (size_t)count, hipMemcpyHostToDevice, p->ctx->stream));
        weight = p->w_weight.as<const uint32_t>();
    }
    return TAFL_OK;
}

extern "C" {

int tafl_pool_set_weighting(tafl_pool* p, const tafl_pool_weights* w) {
    POOLCHK(p, "tafl_pool_set_weighting");
    hipStream_t s = p->ctx->stream;
    if (!w) {
        HIPCHK(hipStreamSynchronize(s));
        p->wfree(); p->dirty = true; p->total = p->positive = p->rebuilds = 0;
        return TAFL_OK;
    }
    if (w->flags) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_set_weighting: flags must be 0");
    for (uint32_t r : w->_reserved) if (r) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_set_weighting: reserved words must be 0");
    if (!p->weighting) {
        const uint32_t NT = pool_weight_tiles(p->mem.C);
        const size_t slots = (size_t)NT * POOLW_TILE;
        // tile_sum, tile_pre (8 bytes each), then tile_pos (4 bytes) per tile
        if (p->wneed(p->wt, 4 * slots) || p->wneed(p->wtiles, 20 * (size_t)NT) || p->wneed(p->wres, 8 * PW_WORDS)) {
            p->wfree();
            return fail(TAFL_ERR_OOM, "hipMalloc failed (tafl_pool_set_weighting)");
        }
        PoolWeights& W = p->wmem;
        W.NT = NT; p->wt.bind(W.wt); p->wres.bind(W.res);
        W.tile_sum = p->wtiles.as<unsigned long long>(); W.tile_pre = W.tile_sum + NT; W.tile_pos = reinterpret_cast<uint32_t*>(W.tile_pre + NT);
        HIPCHK(hipMemsetAsync(p->wres.p, 0, 8 * PW_WORDS, s));
        hipLaunchKernelGGL(k_poolw_fill, dim3(poolw_grid(slots)), dim3(256), 0, s, W.wt, (unsigned long long)slots, w->ingest_weight);
        HIPCHK(hipGetLastError());
        p->weighting = true; p->rebuilds = 0;
    }
    p->ingest_weight = w->ingest_weight;
    p->dirty = true;
    return sync_ok(p->ctx);
}

int tafl_pool_set_weights(tafl_pool* p, const uint32_t* slot, const uint32_t* weight, uint32_t count, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_set_weights");
    if (!p->weighting) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_set_weights: weighting is off (tafl_pool_set_weighting)");
    if ((!slot || !weight) && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_set_weights: null argument");
    if (count == 0) return TAFL_OK;
    const int rc = poolw_stage_in(p, slot, weight, count, ptrs_are_device, "tafl_pool_set_weights");
    if (rc) return rc;
    hipStream_t s = p->ctx->stream;
    const uint32_t first = p->first_live(), grid = poolw_grid(count);
    hipLaunchKernelGGL(k_poolw_zero, dim3(grid), dim3(256), 0, s, p->wmem, slot, count, first, (unsigned long long)p->book.live, p->mem.C);
    hipLaunchKernelGGL(k_poolw_max, dim3(grid), dim3(256), 0, s, p->wmem, slot, weight, count, first, (unsigned long long)p->book.live, p->mem.C);
    HIPCHK(hipGetLastError());
    p->dirty = true;
    if (!ptrs_are_device) HIPCHK(hipStreamSynchronize(s));
    return TAFL_OK;
}

int tafl_pool_get_weights(tafl_pool* p, const uint32_t* slot, uint32_t count, uint32_t* weight, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_get_weights");
    if (!p->weighting) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_get_weights: weighting is off (tafl_pool_set_weighting)");
    if ((!slot || !weight) && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_get_weights: null argument");
    if (count == 0) return TAFL_OK;
    const uint32_t* none = nullptr;
    const int rc = poolw_stage_in(p, slot, none, count, ptrs_are_device, "tafl_pool_get_weights");
    if (rc) return rc;
    hipStream_t s = p->ctx->stream;
    uint32_t* out = weight;
    if (!ptrs_are_device) { if (p->wneed(p->w_weight, 4 * (size_t)count)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed"); out = p->w_weight.as<uint32_t>(); }
    hipLaunchKernelGGL(k_poolw_get, dim3(poolw_grid(count)), dim3(256), 0, s, p->wmem, slot, count, p->first_live(), (unsigned long long)p->book.live, p->mem.C, out);
    HIPCHK(hipGetLastError());
    if (!ptrs_are_device) { COPY_OUT(weight, out, count, s); HIPCHK(hipStreamSynchronize(s)); }
    return TAFL_OK;
}

int tafl_pool_sample_weighted(tafl_pool* p, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t count, uint32_t flags, uint8_t* boards, uint8_t* sides, float* pi, float* z,
                              uint32_t* out_slot, uint8_t* out_sym, uint32_t* out_weight, uint64_t* out_total, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_sample_weighted");
    if (flags & ~(uint32_t)TAFL_POOL_SAMPLE_SYM) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_sample_weighted: unknown flag bits");
    if (!p->weighting) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_sample_weighted: weighting is off (tafl_pool_set_weighting)");
    if ((unsigned long long)row_base + count > 0xFFFFFFFFull) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_sample_weighted: row_base + count exceeds 32 bits");
    if (p->book.live == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_sample_weighted: the pool holds no live row");
    int rc = poolw_rebuild(p);
    if (rc) return rc;
    if (p->total == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_sample_weighted: every live row has weight 0");
    tafl_ctx* c = p->ctx; hipStream_t s = c->stream;
    if (out_total) {                                         // (one uint64, also with device pointers)
        if (ptrs_are_device) HIPCHK(hipMemcpyAsync(out_total, p->wres.as<unsigned long long>() + PW_TOTAL, 8, hipMemcpyDeviceToDevice, s));
        else *out_total = p->total;
    }
    if (count == 0) return TAFL_OK;
    const uint32_t first = p->first_live();
    auto draw = [&](uint32_t base, uint32_t k, uint32_t* d_slot, uint8_t* d_sym, uint32_t* d_weight) {
        const uint32_t grid = std::min<uint32_t>((k + 3u) / 4u, 4096u);
        hipLaunchKernelGGL(k_poolw_draw, dim3(grid), dim3(256), 0, s, p->wmem, first, (unsigned long long)p->book.live, p->mem.C, (unsigned long long)seed, (unsigned long long)step,
                           base, flags, k, (unsigned long long)p->total, d_slot, d_sym, d_weight);
    };
    // the draw needs somewhere to write: what the caller did not ask for goes to the weighting's staging
    const uint32_t chunk = ptrs_are_device ? count : (count < 8192u ? count : 8192u);
    uint32_t* d_slot = out_slot; uint8_t* d_sym = out_sym; uint32_t* d_weight = out_weight;
    if (!ptrs_are_device || !out_slot) { if (p->wneed(p->w_slot, 4 * (size_t)chunk)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed"); d_slot = p->w_slot.as<uint32_t>(); }
    if (!ptrs_are_device || !out_sym) { if (p->wneed(p->w_sym, chunk)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed"); d_sym = p->w_sym.as<uint8_t>(); }
    if (!ptrs_are_device || !out_weight) { if (p->wneed(p->w_weight, 4 * (size_t)chunk)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed"); d_weight = p->w_weight.as<uint32_t>(); }
    if (ptrs_are_device) {
        draw(row_base, count, d_slot, d_sym, d_weight);
        HIPCHK(hipGetLastError());
        return pool_rows_launch(p, false, 0, 0, 0, 0, d_slot, d_sym, count, boards, sides, pi, z, nullptr, nullptr);
    }
    const size_t A = (size_t)c->n * c->n * 2u * (c->n - 1u), nn = (size_t)c->n * c->n;
    POOLNEED(p->g_sides, chunk); POOLNEED(p->g_z, 4 * (size_t)chunk);
    if (boards) POOLNEED(p->g_boards, nn * chunk);
    if (pi) POOLNEED(p->g_pi, 4 * A * chunk);
    for (uint32_t i0 = 0; i0 < count; i0 += chunk) {
        const uint32_t k = count - i0 < chunk ? count - i0 : chunk;
        draw(row_base + i0, k, d_slot, d_sym, d_weight);
        HIPCHK(hipGetLastError());
        rc = pool_rows_launch(p, false, 0, 0, 0, 0, d_slot, d_sym, k, boards ? p->g_boards.as<uint8_t>() : nullptr, sides ? p->g_sides.as<uint8_t>() : nullptr,
                              pi ? p->g_pi.as<float>() : nullptr, z ? p->g_z.as<float>() : nullptr, nullptr, nullptr);
        if (rc) return rc;
        if (boards) COPY_OUT(boards + (size_t)i0 * nn, p->g_boards.p, nn * k, s);
        if (sides) COPY_OUT(sides + i0, p->g_sides.p, k, s);
        if (pi) COPY_OUT(pi + (size_t)i0 * A, p->g_pi.p, A * k, s);
        if (z) COPY_OUT(z + i0, p->g_z.p, k, s);
        if (out_slot) COPY_OUT(out_slot + i0, d_slot, k, s);
        if (out_sym) COPY_OUT(out_sym + i0, d_sym, k, s);
        if (out_weight) COPY_OUT(out_weight + i0, d_weight, k, s);
        HIPCHK(hipStreamSynchronize(s));
    }
    return TAFL_OK;
}

int tafl_pool_set_search_stats(tafl_pool* p, int on) {
    POOLCHK(p, "tafl_pool_set_search_stats");
    if (p->book.live != 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_set_search_stats: the pool holds live rows (the setting changes only while live == 0)");
    hipStream_t s = p->ctx->stream;
    if (!on) {
        HIPCHK(hipStreamSynchronize(s));
        for (DevBuf* d : {&p->s_value, &p->s_surprise, &p->g_s, &p->t_vt, &p->t_kind, &p->g_k}) { p->device_bytes -= d->cap; d->release(); }
        p->search_stats = false; p->value_targets = false;      // (value targets need the statistics)
        return TAFL_OK;
    }
    if (p->search_stats) return TAFL_OK;
    if (p->need(p->s_value, 4 * (size_t)p->mem.C) || p->need(p->s_surprise, 4 * (size_t)p->mem.C)) {
        for (DevBuf* d : {&p->s_value, &p->s_surprise}) { p->device_bytes -= d->cap; d->release(); }
        return fail(TAFL_ERR_OOM, "hipMalloc failed (tafl_pool_set_search_stats)");
    }
    HIPCHK(hipMemsetAsync(p->s_value.p, 0, 4 * (size_t)p->mem.C, s));
    HIPCHK(hipMemsetAsync(p->s_surprise.p, 0, 4 * (size_t)p->mem.C, s));
    p->search_stats = true;
    return sync_ok(p->ctx);
}

int tafl_pool_gather_stats(tafl_pool* p, const uint32_t* slot, uint32_t count, float* value, float* surprise, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_gather_stats");
    if (!p->search_stats) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_stats: search statistics are off (tafl_pool_set_search_stats)");
    if (!slot && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_stats: null slot");
    if (count == 0) return TAFL_OK;
    hipStream_t s = p->ctx->stream;
    float* dv = value; float* ds = surprise;
    if (!ptrs_are_device) {
        for (uint32_t i = 0; i < count; ++i)
            if (!pool_slot_live(slot[i], p->book.written, p->book.live, p->mem.C)) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_stats: slot " + std::to_string(slot[i]) + " (row " + std::to_string(i) + ") is not live");
        POOLNEED(p->g_slot, 4 * (size_t)count); POOLNEED(p->g_z, 4 * (size_t)count); POOLNEED(p->g_s, 4 * (size_t)count);
        HIPCHK(hipMemcpyAsync(p->g_slot.p, slot, 4 * (size_t)count, hipMemcpyHostToDevice, s));
        slot = p->g_slot.as<const uint32_t>(); dv = p->g_z.as<float>(); ds = p->g_s.as<float>();
    }
    hipLaunchKernelGGL(k_pool_gather_stats, dim3(poolw_grid(count)), dim3(256), 0, s, p->s_value.as<const float>(), p->s_surprise.as<const float>(), p->mem.counters, slot, count,
                       p->first_live(), (unsigned long long)p->book.live, p->mem.C, dv, ds);
    HIPCHK(hipGetLastError());
    if (!ptrs_are_device) { COPY_OUT(value, dv, count, s); COPY_OUT(surprise, ds, count, s); HIPCHK(hipStreamSynchronize(s)); }
    return TAFL_OK;
}

int tafl_pool_set_value_targets(tafl_pool* p, int on) {
    POOLCHK(p, "tafl_pool_set_value_targets");
    if (p->book.live != 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_set_value_targets: the pool holds live rows (the setting changes only while live == 0)");
    hipStream_t s = p->ctx->stream;
    if (!on) {
        HIPCHK(hipStreamSynchronize(s));
        for (DevBuf* d : {&p->t_vt, &p->t_kind, &p->g_k}) { p->device_bytes -= d->cap; d->release(); }
        p->value_targets = false;
        return TAFL_OK;
    }
    if (!p->search_stats) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_set_value_targets: search statistics are off (tafl_pool_set_search_stats)");
    if (p->value_targets) return TAFL_OK;
    if (p->need(p->t_vt, 4 * (size_t)p->mem.C) || p->need(p->t_kind, (size_t)p->mem.C)) {
        for (DevBuf* d : {&p->t_vt, &p->t_kind}) { p->device_bytes -= d->cap; d->release(); }
        return fail(TAFL_ERR_OOM, "hipMalloc failed (tafl_pool_set_value_targets)");
    }
    HIPCHK(hipMemsetAsync(p->t_vt.p, 0, 4 * (size_t)p->mem.C, s));
    HIPCHK(hipMemsetAsync(p->t_kind.p, 0, (size_t)p->mem.C, s));
    p->value_targets = true;
    return sync_ok(p->ctx);
}

int tafl_pool_gather_targets(tafl_pool* p, const uint32_t* slot, uint32_t count, float* target, uint8_t* kind, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_gather_targets");
    if (!p->value_targets) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_targets: value targets are off (tafl_pool_set_value_targets)");
    if (!slot && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_targets: null slot");
    if (count == 0) return TAFL_OK;
    hipStream_t s = p->ctx->stream;
    float* dt = target; uint8_t* dk = kind;
    if (!ptrs_are_device) {
        for (uint32_t i = 0; i < count; ++i)
            if (!pool_slot_live(slot[i], p->book.written, p->book.live, p->mem.C)) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_targets: slot " + std::to_string(slot[i]) + " (row " + std::to_string(i) + ") is not live");
        POOLNEED(p->g_slot, 4 * (size_t)count); POOLNEED(p->g_z, 4 * (size_t)count); POOLNEED(p->g_k, count);
        HIPCHK(hipMemcpyAsync(p->g_slot.p, slot, 4 * (size_t)count, hipMemcpyHostToDevice, s));
        slot = p->g_slot.as<const uint32_t>(); dt = target ? p->g_z.as<float>() : nullptr; dk = kind ? p->g_k.as<uint8_t>() : nullptr;
    }
    hipLaunchKernelGGL(k_pool_gather_targets, dim3(poolw_grid(count)), dim3(256), 0, s, p->t_vt.as<const float>(), p->t_kind.as<const uint8_t>(), p->mem.counters, slot, count,
                       p->first_live(), (unsigned long long)p->book.live, p->mem.C, dt, dk);
    HIPCHK(hipGetLastError());
    if (!ptrs_are_device) { COPY_OUT(target, dt, count, s); COPY_OUT(kind, dk, count, s); HIPCHK(hipStreamSynchronize(s)); }
    return TAFL_OK;
}

int tafl_pool_weights_from_surprise(tafl_pool* p, const tafl_pool_surprise_weights* cfg) {
    POOLCHK(p, "tafl_pool_weights_from_surprise");
    if (!cfg) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_weights_from_surprise: null argument");
    if (!p->weighting || !p->search_stats) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_weights_from_surprise: needs weighting (tafl_pool_set_weighting) and search statistics (tafl_pool_set_search_stats) on");
    if (!(cfg->per_nat >= 0.0)) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_weights_from_surprise: per_nat must be a number >= 0");
    if (cfg->flags) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_weights_from_surprise: flags must be 0");
    for (uint32_t r : cfg->_reserved) if (r) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_weights_from_surprise: reserved words must be 0");
    p->dirty = true;
    if (p->book.live == 0) return TAFL_OK;
    hipLaunchKernelGGL(k_poolw_from_surprise, dim3(poolw_grid(p->mem.C)), dim3(256), 0, p->ctx->stream, p->wmem.wt, p->s_surprise.as<const float>(), (const uint32_t*)p->mem.rows, p->mem.RW,
                       p->mem.BW + (uint32_t)PR_GENERATION, p->first_live(), (unsigned long long)p->book.live, p->mem.C, cfg->base, cfg->generation, cfg->per_nat);
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}

int tafl_pool_dedup(tafl_pool* p, const tafl_pool_dedup_cfg* cfg, tafl_pool_dedup_result* out) {
    POOLCHK(p, "tafl_pool_dedup");
    tafl_ctx* c = p->ctx; hipStream_t s = c->stream;
    if (!cfg) {
        HIPCHK(hipStreamSynchronize(s));
        p->ddfree();
        if (out) memset(out, 0, sizeof *out);
        return TAFL_OK;
    }
    if (cfg->flags & ~(uint32_t)TAFL_POOL_DEDUP_SYMMETRIES) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_dedup: unknown flag bits");
    if (cfg->key_bits > 64u) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_dedup: key_bits must be in 0..64");
    for (uint32_t r : cfg->_reserved) if (r) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_dedup: reserved words must be 0");
    if (p->book.live == 0) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_dedup: the pool holds no live row");
    if ((uint64_t)p->mem.C > (1ull << 30)) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_dedup: pools of more than 2^30 rows are not supported");
    p->dd_valid = false;
    const size_t C = p->mem.C;
    const uint32_t live = (uint32_t)p->book.live, first = p->first_live(), TS = pooldd_table_size(live);
    if (p->ddneed(p->dd_rep, 4 * C) || p->ddneed(p->dd_mult, 4 * C) || p->ddneed(p->dd_zmean, 4 * C) || p->ddneed(p->dd_canon, C) || p->ddneed(p->dd_key, 8 * C) ||
        p->ddneed(p->dd_ent, 4 * C) || p->ddneed(p->dd_table, pooldd_table_bytes(pooldd_table_size(C))) || p->ddneed(p->dd_res, 8 * PDD_WORDS)) {
        p->ddfree();
        return fail(TAFL_ERR_OOM, "hipMalloc failed (tafl_pool_dedup)");
    }
    const PoolDedupTable T = pooldd_table(p->dd_table.p, TS);
    unsigned long long* res = p->dd_res.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(p->dd_table.p, 0, pooldd_table_bytes(TS), s));
    HIPCHK(hipMemsetAsync(res, 0, 8 * PDD_WORDS, s));
    const uint32_t Q = (p->mem.BW + 1u + 3u) / 4u;                             // the board words and the info word, in quads
    const uint32_t kgrid = std::min<uint32_t>((live + POOLDD_ROWS - 1u) / POOLDD_ROWS, 16384u), grid = poolw_grid(live);
    hipLaunchKernelGGL(k_pooldd_key, dim3(kgrid), dim3(256), (size_t)POOLDD_ROWS * 16u * Q, s, p->mem, first, live, c->n, Q, cfg->flags & (uint32_t)TAFL_POOL_DEDUP_SYMMETRIES,
                       cfg->key_bits, p->dd_key.as<unsigned long long>(), p->dd_canon.as<uint8_t>());
    hipLaunchKernelGGL(k_pooldd_insert<TAFL_POOLDD_AGGREGATE>, dim3(grid), dim3(256), 0, s, p->mem, T, first, live, p->dd_key.as<const unsigned long long>(), p->dd_ent.as<uint32_t>());
    hipLaunchKernelGGL(k_pooldd_finish, dim3(grid), dim3(256), 0, s, p->mem, T, first, live, c->n, p->dd_ent.as<const uint32_t>(), p->dd_canon.as<const uint8_t>(),
                       p->dd_rep.as<uint32_t>(), p->dd_mult.as<uint32_t>(), p->dd_zmean.as<float>(), res);
    HIPCHK(hipGetLastError());
    unsigned long long h[PDD_WORDS];
    HIPCHK(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    p->dd_valid = true;
    if (out) {
        memset(out, 0, sizeof *out);
        out->live = live; out->distinct = h[PDD_DISTINCT]; out->largest = h[PDD_LARGEST]; out->collisions = h[PDD_COLLISIONS]; out->device_bytes = p->dedup_bytes;
    }
    return TAFL_OK;
}

int tafl_pool_gather_dedup(tafl_pool* p, const uint32_t* slot, uint32_t count, uint32_t* rep, uint32_t* mult, float* zmean, int ptrs_are_device) {
    POOLCHK(p, "tafl_pool_gather_dedup");
    if (!p->dd_valid) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_dedup: no de-duplication result stands (tafl_pool_dedup after the last ingest, trim or clear)");
    if (!slot && count) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_dedup: null slot");
    if (count == 0) return TAFL_OK;
    hipStream_t s = p->ctx->stream;
    uint32_t* dr = rep; uint32_t* dm = mult; float* dz = zmean;
    if (!ptrs_are_device) {
        for (uint32_t i = 0; i < count; ++i)
            if (!pool_slot_live(slot[i], p->book.written, p->book.live, p->mem.C)) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_gather_dedup: slot " + std::to_string(slot[i]) + " (row " + std::to_string(i) + ") is not live");
        if (p->ddneed(p->dd_stage, 16 * (size_t)count)) return fail(TAFL_ERR_OOM, "hipMalloc(workspace) failed");
        uint32_t* st = p->dd_stage.as<uint32_t>();
        HIPCHK(hipMemcpyAsync(st, slot, 4 * (size_t)count, hipMemcpyHostToDevice, s));
        slot = st; dr = st + count; dm = dr + count; dz = reinterpret_cast<float*>(dm + count);
    }
    hipLaunchKernelGGL(k_pooldd_gather, dim3(poolw_grid(count)), dim3(256), 0, s, p->dd_rep.as<const uint32_t>(), p->dd_mult.as<const uint32_t>(), p->dd_zmean.as<const float>(),
                       p->mem.counters, slot, count, p->first_live(), (unsigned long long)p->book.live, p->mem.C, dr, dm, dz);
    HIPCHK(hipGetLastError());
    if (!ptrs_are_device) { COPY_OUT(rep, dr, count, s); COPY_OUT(mult, dm, count, s); COPY_OUT(zmean, dz, count, s); HIPCHK(hipStreamSynchronize(s)); }
    return TAFL_OK;
}

int tafl_pool_weights_from_dedup(tafl_pool* p, const tafl_pool_dedup_weights* cfg) {
    POOLCHK(p, "tafl_pool_weights_from_dedup");
    if (!cfg) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_weights_from_dedup: null argument");
    if (cfg->flags & ~(uint32_t)(TAFL_POOL_DEDUP_DIVIDE | TAFL_POOL_DEDUP_REPRESENTATIVES)) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_weights_from_dedup: unknown flag bits");
    if (cfg->flags == (uint32_t)(TAFL_POOL_DEDUP_DIVIDE | TAFL_POOL_DEDUP_REPRESENTATIVES))
        return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_weights_from_dedup: TAFL_POOL_DEDUP_DIVIDE and TAFL_POOL_DEDUP_REPRESENTATIVES exclude each other");
    for (uint32_t r : cfg->_reserved) if (r) return fail(TAFL_ERR_UNSUPPORTED, "tafl_pool_weights_from_dedup: reserved words must be 0");
    if (!p->weighting) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_weights_from_dedup: weighting is off (tafl_pool_set_weighting)");
    if (!p->dd_valid) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_weights_from_dedup: no de-duplication result stands (tafl_pool_dedup after the last ingest, trim or clear)");
    p->dirty = true;
    hipLaunchKernelGGL(k_pooldd_weights, dim3(poolw_grid(p->mem.C)), dim3(256), 0, p->ctx->stream, p->wmem.wt, p->dd_rep.as<const uint32_t>(), p->dd_mult.as<const uint32_t>(), p->first_live(),
                       (unsigned long long)p->book.live, p->mem.C, cfg->scale, cfg->flags);
    HIPCHK(hipGetLastError());
    return TAFL_OK;
}

int tafl_pool_weight_stats(tafl_pool* p, tafl_pool_weight_counters* out) {
    POOLCHK(p, "tafl_pool_weight_stats");
    if (!out) return fail(TAFL_ERR_INVALID_ARG, "tafl_pool_weight_stats: null argument");
    memset(out, 0, sizeof *out);
    if (!p->weighting) return TAFL_OK;
    const int rc = poolw_rebuild(p);
    if (rc) return rc;
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, p->wres.as<unsigned long long>() + PW_BAD_SLOT, 8, hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    out->enabled = 1; out->ingest_weight = p->ingest_weight; out->total_weight = p->total; out->positive = p->positive; out->bad_slot = bad;
    out->rebuilds = p->rebuilds; out->device_bytes = p->weight_bytes;
    return TAFL_OK;
}

}  // extern "C"
