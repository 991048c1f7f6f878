// hostsim_tables.cpp — the LDS index table of the playout kernels (tafl_tables.hpp) on the host: IdxTables::fill() writes a plain buffer
// with several "threads" in turn, as the workgroup does, and every entry is handed out next to the value IdxComputed gives for the same
// index.  tests/test_hostsim_tables.py compares them.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../alphazeroforhnefatafl_amd/csrc/tafl_core.hpp"

using namespace tafl;

namespace {
// out_table / out_computed: NL words each.  Returns NL, 0 for an index outside the layout.
template <int NL>
uint32_t entry(uint32_t idx, uint32_t nthreads, uint32_t* out_table, uint32_t* out_computed) {
    using L = IdxTables<NL>;
    if (idx >= L::N || nthreads == 0u) return 0u;
    std::vector<typename L::Row> mem(L::ROWS);
    memset(mem.data(), 0xA5, L::BYTES);
    for (uint32_t t = 0; t < nthreads; ++t) L::fill(mem.data(), t, nthreads);
    L lut; lut.base = mem.data();
    const Bits<NL> a = lut.bit(idx), b = IdxComputed<NL>().bit(idx);
    memcpy(out_table, a.w, sizeof a.w); memcpy(out_computed, b.w, sizeof b.w);
    return NL;
}
}  // namespace

extern "C" {
// limbs: 4 (11x11, 128-bit words), 2 (7x7, 64-bit words), 8 (256-bit words; no kernel keeps this one)
uint32_t hst_entries(uint32_t limbs) { return limbs == 4 ? IdxTables<4>::N : limbs == 2 ? IdxTables<2>::N : limbs == 8 ? IdxTables<8>::N : 0u; }
uint32_t hst_bytes(uint32_t limbs) { return limbs == 4 ? IdxTables<4>::BYTES : limbs == 2 ? IdxTables<2>::BYTES : limbs == 8 ? IdxTables<8>::BYTES : 0u; }
int hst_kept(uint32_t limbs) { return limbs == 2 ? playout_bit_table<2>() : limbs == 4 ? playout_bit_table<4>() : limbs == 6 ? playout_bit_table<6>() : limbs == 8 ? playout_bit_table<8>() : 0; }
uint32_t hst_entry(uint32_t limbs, uint32_t idx, uint32_t nthreads, uint32_t* out_table, uint32_t* out_computed) {
    if (limbs == 4) return entry<4>(idx, nthreads, out_table, out_computed);
    if (limbs == 2) return entry<2>(idx, nthreads, out_table, out_computed);
    if (limbs == 8) return entry<8>(idx, nthreads, out_table, out_computed);
    return 0u;
}
}
