"""The training pool (include/taflhip.h tafl_pool_*), CPU only: the product's tafl_pool.hpp (take predicate, row
store, placement, draw, row writer, bookkeeping) compiled for the host (tests/hostsim_pool) against the Python / numpy restatements of
tests/pool_util.py.  Every comparison is exact.  The examples come from the host harness's recording run (hsx_record + hsx_finalize) on
Brandubh; the same comparisons run against the real kernels in tests/test_gpu_pool.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams
from oracle import oracle as orc
from tests import examples_util as xu
from tests import parity_util as pu
from tests import pool_util as qu

N = 7
G, MOVES, K, SIMS = 64, 24, 6, 8          # K below S: roots with more than six visited children overflow
WORKLOAD_ADVANCE_SEED = 3


@functools.lru_cache(maxsize=None)
def workload():
    """Two recorded and finalized examples buffers (A, B: the same start positions, other seeds) with their tables, and an empty one.
    The games are pre-advanced by (i * 5) % 30 random plies: some end inside the run, some are over before it."""
    rules, fen, wb = pu.CONFIGS["brandubh7"]
    lg = orc.GameLogic(rules, N)
    out = []
    for seed, sample_seed in ((8, 11), (9, 12)):
        states = pu.start_states(orc, fen, rules.starting_side, wb, G)
        plies = (C.c_uint32 * G)(*[(i * 5) % 30 for i in range(G)])
        orc.batch_random_advance(lg, states, G, wb, WORKLOAD_ADVANCE_SEED, plies, 0)
        hx = xu.HostExamples(rules, N, wb, G, MOVES, K)
        hx.record(states, TaflMctsParams(SIMS, 64, 1.0, seed, 0, 0), MOVES, 0, sample_seed, 4)
        hx.finalize(states)
        out += [hx, qu.host_table(hx)]
    empty = xu.HostExamples(rules, N, wb, G, MOVES, K)
    return tuple(out) + (empty, qu.host_table(empty))


def _check(pool, model, where):
    """The harness's pool against the model: the counters, every live row through read and gather under mixed symmetries, and the slots
    that are not live rejected."""
    st = pool.stats()
    for k, v in model.stats().items():
        assert st[k] == v, (where, k, st[k], v)
    slots = model.live_slots()
    assert len(set(slots)) == len(slots) == model.live
    if slots:
        sym = [(3 * i + s) % 8 for i, s in enumerate(slots)]
        rc, got_read = pool.read(slots)
        assert rc == 0
        got_gather, bad = pool.gather(slots, sym)
        assert bad == 0
        qu.check_rows(model, slots, sym, got_read, got_gather, where)
    dead = sorted(set(range(model.C)) - set(slots))
    for s in dead[:3] + [model.C]:
        assert pool.read([s])[0] == -1, (where, s)


def test_workload_meets_the_coverage_floors():
    """Asserted on the restatement alone: per ingest at least 50 taken examples, 5 skipped as open, 5 skipped for overflow, 5 lanes with
    len < max_moves and one lane without an example."""
    _, ta, _, tb, _, te = workload()
    qu.assert_floors(ta, "A")
    qu.assert_floors(tb, "B")
    assert qu.coverage(te)["taken"] == 0 and qu.coverage(te)["empty_lanes"] == G


@pytest.mark.parametrize("Kp", [K, K + 3])
def test_ingest_into_a_pool_with_room(Kp):
    """C > T, with rows as wide as the examples and wider (the policy words beyond the examples' max_children are zero)."""
    hx, ta, *_ = workload()
    T = qu.coverage(ta)["taken"]
    pool, model = qu.HostPool(T + 7, Kp, N), qu.PoolModel(T + 7, Kp, N)
    assert pool.ingest(hx) == model.ingest(ta) == (T, qu.coverage(ta)["open"], qu.coverage(ta)["overflow"])
    _check(pool, model, Kp)
    assert model.live == T and model.oldest_generation() == 1
    # the slots no ingest reached still hold the harness's fill pattern
    assert (pool.raw()[T:] == 0xDEADBEEF).all() and not (pool.raw()[:T, :4] == 0xDEADBEEF).all()
    assert pool.raw().shape[1] % 4 == 0


def test_ingest_larger_than_the_pool_keeps_the_newest_rows():
    """C < T in one call: only the examples of rank >= T - C are stored, in the slots rank mod C; C == T fills the ring exactly."""
    hx, ta, *_ = workload()
    T = qu.coverage(ta)["taken"]
    for Cp in (T - 13, T, 1):
        pool, model = qu.HostPool(Cp, K, N), qu.PoolModel(Cp, K, N)
        assert pool.ingest(hx)[0] == model.ingest(ta)[0] == T
        _check(pool, model, Cp)
        assert model.live == Cp and pool.stats()["written"] == T


def test_two_ingests_cross_the_end_of_the_ring_and_an_empty_one_counts():
    hx, ta, hy, tb, he, te = workload()
    Ta, Tb = qu.coverage(ta)["taken"], qu.coverage(tb)["taken"]
    Cp = Ta + Tb // 2
    pool, model = qu.HostPool(Cp, K + 1, N), qu.PoolModel(Cp, K + 1, N)
    assert pool.ingest(hx) == model.ingest(ta)
    _check(pool, model, "first")
    assert pool.ingest(hy) == model.ingest(tb)
    _check(pool, model, "second")
    assert model.written > Cp and model.oldest_generation() == 1 and sorted(model.live_slots()) == list(range(Cp))
    # T = 0 is a generation: nothing moves but the count of ingests
    before = pool.raw().copy()
    assert pool.ingest(he) == model.ingest(te) == (0, 0, 0)
    _check(pool, model, "empty")
    assert np.array_equal(pool.raw(), before) and pool.stats()["ingests"] == 3
    # ingesting the same object twice takes its examples twice
    assert pool.ingest(hy) == model.ingest(tb)
    _check(pool, model, "again")
    pool.clear(); model.clear()
    _check(pool, model, "cleared")
    assert pool.stats()["live"] == 0 and pool.sample(1, 1, 1)[0] == -1


def test_trim_across_three_generations():
    """live and oldest_generation after trims, with generation 1 partly fallen out of the ring before the first trim."""
    hx, ta, hy, tb, he, te = workload()
    Ta, Tb = qu.coverage(ta)["taken"], qu.coverage(tb)["taken"]
    Cp = Ta // 2 + Tb + Ta - 5                       # after A, B, A: generation 1 has Ta // 2 - 5 rows left
    pool, model = qu.HostPool(Cp, K, N), qu.PoolModel(Cp, K, N)
    for hz, tz in ((hx, ta), (hy, tb), (hx, ta)):
        assert pool.ingest(hz) == model.ingest(tz)
    assert pool.trim(0) == -1
    assert pool.trim(5) == 0 and pool.trim(3) == 0                  # nothing to remove
    model.trim(5); model.trim(3)
    _check(pool, model, "keep 3")
    assert model.live == Cp and model.oldest_generation() == 1
    assert pool.trim(2) == 0
    model.trim(2)
    _check(pool, model, "keep 2")
    assert model.live == Tb + Ta and model.oldest_generation() == 2
    assert pool.ingest(he) == model.ingest(te)                      # generation 4 is empty: keeping two generations now keeps 3 and 4
    assert pool.trim(2) == 0
    model.trim(2)
    _check(pool, model, "keep 2 of 4")
    assert model.live == Ta and model.oldest_generation() == 3
    assert pool.ingest(hy) == model.ingest(tb)                      # the pool fills up again behind a trimmed prefix
    _check(pool, model, "refill")
    assert model.live == Ta + Tb
    assert pool.trim(1) == 0
    model.trim(1)
    _check(pool, model, "keep 1")
    assert model.live == Tb and model.oldest_generation() == 5


STATES = [(57, 57, 100), (1000, 64, 64), (300, 41, 128), (2 ** 40 + 12345, 2 ** 31 + 7, 2 ** 32 - 1)]      # (written, live, C): not wrapped, wrapped, trimmed, wide


@pytest.mark.parametrize("written,live,Cp", STATES)
def test_draw_is_the_stated_function(written, live, Cp):
    """10 000 rows against the restatement; the ranks' calls with row_base = k * count reproduce the single call; every a < live."""
    seed, step, count = 0x1234567890ABCDEF, 77, 10000
    slot, sym = qu.host_draw(seed, step, 5, count, 1, written, live, Cp)
    want_slot, want_sym, a = qu.draw_many(seed, step, 5, count, written, live, Cp)
    assert np.array_equal(slot, want_slot) and np.array_equal(sym, want_sym)
    assert a.min() >= 0 and a.max() < live
    assert set(np.unique(sym)) == set(range(8))
    if live >= 41:
        assert len(np.unique(a)) >= 41 or live > 10000           # every age rank of a small window is drawn
    parts = [qu.host_draw(seed, step, 5 + k * 2500, 2500, 1, written, live, Cp) for k in range(4)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), slot) and np.array_equal(np.concatenate([p[1] for p in parts]), sym)
    s0, y0 = qu.host_draw(seed, step, 5, 100, 0, written, live, Cp)
    assert np.array_equal(s0, slot[:100]) and not y0.any()        # without TAFL_POOL_SAMPLE_SYM: the same slots, sym = 0
    assert not np.array_equal(qu.host_draw(seed, step + 1, 5, 100, 1, written, live, Cp)[0], slot[:100])


def test_gather_rows_equal_the_examples_gather_under_all_symmetries():
    """A row holds the bytes hsx_gather (k_examples_gather restated) writes for the source example under the same symmetry."""
    hx, ta, *_ = workload()
    T = qu.coverage(ta)["taken"]
    pool, model = qu.HostPool(T - 9, K + 2, N), qu.PoolModel(T - 9, K + 2, N)
    pool.ingest(hx); model.ingest(ta)
    slots = model.live_slots()
    src = model.source(slots)
    for k in range(8):
        got, bad = pool.gather(slots, [k] * len(slots))
        (boards, sides, pi, z, _fin), bad_src = hx.gather(src, [k] * len(slots))
        assert bad == 0 and bad_src == 0
        for name, a, b in zip(("boards", "sides", "pi", "z"), got, (boards, sides, pi, z)):
            assert a.tobytes() == b.tobytes(), (k, name)
        assert (z != 0).all()                                      # every taken example is final
    ident, _ = pool.gather(slots)
    assert ident[0].tobytes() == pool.gather(slots, [0] * len(slots))[0][0].tobytes()


def test_sample_rows_are_the_gather_of_the_draw_and_dead_slots_give_zero_rows():
    hx, ta, hy, tb, *_ = workload()
    Ta = qu.coverage(ta)["taken"]
    pool, model = qu.HostPool(Ta + 20, K, N), qu.PoolModel(Ta + 20, K, N)
    assert pool.sample(4, 1, 2)[0] == -1                           # live == 0
    pool.ingest(hx); model.ingest(ta)
    pool.ingest(hy); model.ingest(tb)
    pool.trim(1); model.trim(1)
    st = pool.stats()
    rc, rows, slot, sym = pool.sample(257, 9, 4, row_base=1000)
    assert rc == 0
    want_slot, want_sym, _ = qu.draw_many(9, 4, 1000, 257, st["written"], st["live"], pool.C)
    assert np.array_equal(slot, want_slot) and np.array_equal(sym, want_sym)
    assert set(int(s) for s in slot) <= set(model.live_slots())
    again, bad = pool.gather(slot, sym)
    assert bad == 0
    for a, b, c in zip(rows, again, model.expect_gather(slot, sym)):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert pool.sample(1, 9, 4, flags=2)[0] == -5 and pool.sample(2, 9, 4, row_base=0xFFFFFFFF)[0] == -1
    dead = sorted(set(range(pool.C)) - set(model.live_slots()))
    assert dead
    mixed = [model.live_slots()[0], dead[0], pool.C, model.live_slots()[-1]]
    got, bad = pool.gather(mixed, [1, 2, 3, 12])                   # (sym is taken modulo 8)
    assert bad == 2 and pool.stats()["bad_slot"] == 2
    for a in got:
        assert not a[1].any() and not a[2].any()
    want = model.expect_gather([mixed[0], mixed[3]], [1, 4])
    for a, w in zip(got, want):
        assert a[0].tobytes() == w[0].tobytes() and a[3].tobytes() == w[1].tobytes()
