// tafl_tables.hpp — how the playout ply turns a run-time tile index into its one-bit mask: a policy.
//
// Bits<NL> lives in registers and cannot be indexed dynamically, so bit_at<NL>(idx) is lowered to a 64-bit shift, compares and a select
// chain: VALU instructions of the slow class that are no game logic, in a kernel whose limit is VALU issue and whose LDS pipe is idle
// (DESIGN.md section 4.2).  It is a pure function of an index below NL*32, so a playout kernel may read it from a small per-workgroup
// table in LDS instead: one row of NL limbs per index, one ds_read_b128 (NL = 4) / ds_read_b64 (NL = 2) per lookup.
//
//   IdxComputed<NL>   today's computed code: the default of every function that takes the policy; every kernel but the preset playout
//                     kernels, and every host build, uses it
//   IdxTables<NL>     the table, filled cooperatively at kernel entry by fill() from bit_at itself, so that an entry IS the computed
//                     value (tests/hostsim_tables compares every entry)
//
// Only indices that are run-time values go through the policy (the move's origin and destination in both layouts); call sites whose
// index is a literal after inlining (king_specials, the rule masks of a preset) and the rare loops keep calling bit_at.
// The same mechanism was measured for below<NL>, for (row, col, T index) packed in a word and for the 64-bit field of the constant
// hostile sets: none of them paid (profiles/r04_tables), so they stay computed.
#pragma once
#include <type_traits>
#include "tafl_bits.hpp"

namespace tafl {

template <int NL>
struct IdxComputed {
    TAFL_HD Bits<NL> bit(uint32_t i) const { return bit_at<NL>(i); }
};

struct alignas(16) LutQuad { uint32_t x, y, z, w; };
struct alignas(8) LutPair { uint32_t x, y; };

template <int NL>
struct IdxTables {
    static_assert(NL == 2 || NL % 4 == 0, "a row is read as one 8-byte word or as 16-byte words");
    static constexpr uint32_t N = NL * 32u;                 // every index the layout admits
    static constexpr uint32_t BYTES = N * NL * 4u;
    using Row = typename std::conditional<NL == 2, LutPair, LutQuad>::type;
    static constexpr uint32_t ROWS = BYTES / sizeof(Row);   // the workgroup's array: Row[ROWS]

    const Row* base;

    // entries tid, tid + nthreads, ... ; the caller synchronises the workgroup afterwards
    static TAFL_HD void fill(Row* mem, uint32_t tid, uint32_t nthreads) {
        for (uint32_t i = tid; i < N; i += nthreads) {
            const Bits<NL> v = bit_at<NL>(i);
            if constexpr (NL == 2) { Row r; r.x = v.w[0]; r.y = v.w[1]; mem[i] = r; }
            else { TAFL_UNROLL for (int k = 0; k < NL / 4; ++k) { Row r; r.x = v.w[4 * k]; r.y = v.w[4 * k + 1]; r.z = v.w[4 * k + 2]; r.w = v.w[4 * k + 3]; mem[i * (NL / 4) + k] = r; } }
        }
    }
    TAFL_HD Bits<NL> bit(uint32_t i) const {                // i < N
        Bits<NL> o;
        if constexpr (NL == 2) { const Row r = base[i]; o.w[0] = r.x; o.w[1] = r.y; }
        else { TAFL_UNROLL for (int k = 0; k < NL / 4; ++k) { const Row r = base[i * (NL / 4) + k]; o.w[4 * k] = r.x; o.w[4 * k + 1] = r.y; o.w[4 * k + 2] = r.z; o.w[4 * k + 3] = r.w; } }
        return o;
    }
};

// the layouts whose preset playout kernels keep the table (budget and measurements: DESIGN.md section 4.2): 11x11 in four limbs (2 KiB)
// and 7x7 in two (512 B).  The dense 13x13 layout <6, 13> stays computed: its table (4.5 KiB) does not fit beside the tree phase.
template <int NL> constexpr bool playout_bit_table() { return NL == 4 || NL == 2; }

}  // namespace tafl
