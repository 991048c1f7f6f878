"""The bit_at table of the playout kernels (alphazeroforhnefatafl_amd/csrc/tafl_tables.hpp) on the host: tests/hostsim_tables fills it with
the fill function the kernels call and reads it back through the table policy; every entry must EQUAL what the computed policy gives for
the same index, for every index the layout admits, and both must equal the definition written out here in Python.  (The issue that
brought the table also asked for below<NL>, (row, col, T index) and the hostile-special fields; those tables did not pay on the device
and were removed again, profiles/r04_tables, so there is nothing of theirs to compare.)"""
import ctypes as C
import os
import subprocess

import pytest

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_tables")
_LIB = None
LIMBS = {"11x11_4_limbs": 4, "7x7_2_limbs": 2, "256_bit_8_limbs": 8}


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_tables.so"))
        u32, P = C.c_uint32, C.POINTER
        L.hst_entries.restype = u32; L.hst_entries.argtypes = [u32]
        L.hst_bytes.restype = u32; L.hst_bytes.argtypes = [u32]
        L.hst_kept.restype = C.c_int; L.hst_kept.argtypes = [u32]
        L.hst_entry.restype = u32; L.hst_entry.argtypes = [u32, u32, u32, P(u32), P(u32)]
        _LIB = L
    return _LIB


def entry(limbs, idx, nthreads=64):
    a, b = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
    n = lib().hst_entry(limbs, idx, nthreads, a, b)
    assert n == limbs, (limbs, idx)
    return list(a[:n]), list(b[:n])


def words(v, n):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


@pytest.mark.parametrize("name", list(LIMBS))
def test_every_entry_equals_the_computed_helper(name):
    limbs = LIMBS[name]
    n = lib().hst_entries(limbs)
    assert n == 32 * limbs                       # 0 .. 127 for <4, 11>, the full range for the others
    for idx in range(n):
        got, want = entry(limbs, idx)
        assert got == want, (name, idx, got, want)
        assert got == words(1 << idx, limbs), (name, idx, got)
    assert lib().hst_entry(limbs, n, 64, (C.c_uint32 * 8)(), (C.c_uint32 * 8)()) == 0      # one past the layout: refused


@pytest.mark.parametrize("nthreads", [1, 7, 64, 256])
def test_fill_is_the_same_for_any_workgroup_size(nthreads):
    for limbs in (2, 4):
        for idx in (0, 1, 31, 32, 63, 32 * limbs - 1):
            got, want = entry(limbs, idx, nthreads)
            assert got == want == words(1 << idx, limbs)


def test_table_sizes_fit_the_budget():
    """LDS is handed out in 1 280-byte granules; beside the two tree workgroups of a CU (57 344 B of undo log each) the
    16 one-wave playout workgroups of the 11x11 kernel have two granules each; the fused 7x7 kernel runs eight workgroups per CU with
    17 920 B of undo log each.  The dense 13x13 layout keeps no table (six limbs: 4.5 KiB would not fit beside 12 workgroups)."""
    gran, lds = 1280, 160 * 1024
    up = lambda b: -(-b // gran) * gran
    assert lib().hst_kept(4) and lib().hst_kept(2) and not lib().hst_kept(6) and not lib().hst_kept(8)
    assert lib().hst_bytes(4) == 2048 and lib().hst_bytes(2) == 512
    assert 2 * up(57344) + 16 * up(lib().hst_bytes(4)) <= lds
    assert 8 * up(17920 + lib().hst_bytes(2)) <= lds
    assert 2 * up(57344) + 12 * up(192 * 24) > lds
