"""Search statistics per training row (include/taflhip.h "search value and policy surprise") on the host harness
(tests/hostsim_search_stats: the product's record_stats after every round of tests/hostsim_solver's sessions, example_search_stats for
the scalars) against the Python twins (tests/search_stats_util.py): Copenhagen 11 x 11 / u128, 65 lanes at 0 .. 39 plies, S = 24, K = 64.
cq, cp and value bit for bit, surprise within 2^-23 |want| + 1e-10.  CPU only."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import noise_util as nu
from tests import search_stats_util as ssu

G, S, K = 65, 24, 64


@functools.lru_cache(maxsize=None)
def shape():
    return ssu.shape(orc, "copenhagen11", G)


def settings(mode):
    return dict(ssu.MODES[mode])


@functools.lru_cache(maxsize=None)
def expectation(mode):
    rules, n, wb, lg, states, salts, _over = shape()
    return ssu.twin_run(orc, lg, states, wb, salts, nu.HostSide(rules, n, wb), S, **settings(mode))


@functools.lru_cache(maxsize=None)
def harness(mode, stats=True):
    rules, n, wb, _lg, states, salts, over = shape()
    return ssu.host_run(rules, n, wb, states, salts, S, K, stats=stats, over=over, **settings(mode))


@pytest.mark.parametrize("mode", list(ssu.MODES))
def test_the_expectation_meets_the_coverage_floors(mode):
    """Asserted on the twin alone: half of the examples have two or more stored children, one has a value whose sign differs from its
    later z, the surprise is positive in half."""
    ssu.assert_floors(expectation(mode), shape()[6], mode)


@pytest.mark.parametrize("mode", list(ssu.MODES))
def test_a_run_records_what_the_twin_holds(mode):
    got = harness(mode)
    assert got.dropped == 0 and got.overflowed == 0
    ssu.assert_rows(got, expectation(mode), mode)
    if mode == "episodes":
        assert all(eps >= 1 for eps in got.counters[5]), "every lane reopens"
    if mode == "cap_forced":
        assert got.counters[2][0] == sum(got.lens) and got.counters[2][1] > 0, "only full moves carry rows"


@pytest.mark.parametrize("mode", list(ssu.MODES))
def test_the_recorder_changes_nothing_else(mode):
    on, off = harness(mode), harness(mode, False)
    assert on.plays == off.plays and on.states == off.states and on.moves == off.moves
    assert on.examples == off.examples and on.counters == off.counters and on.lens == off.lens
    assert (on.dropped, on.overflowed) == (off.dropped, off.overflowed)


def test_overflowed_and_dropped_examples_store_nothing():
    """K = 4 and room for two examples per lane: an overflowed example holds the pattern and its scalars are 0; what fits equals the twin."""
    rules, n, wb, _lg, states, salts, over = shape()
    got = ssu.host_run(rules, n, wb, states, salts, S, 4, over=over, max_moves=2)
    want = expectation("plain")
    assert got.overflowed > 0 and got.dropped > 0
    pattern = np.uint32(0x7FC0BEEF)
    seen_fit = 0
    for g in range(G):
        assert got.lens[g] <= 2
        for j in range(got.lens[g]):
            w = want[g][j]
            if got.over_flags[(g, j)]:
                assert len(w.visits) > 4
                assert (got.raw_q[j, :, g].view(np.uint32) == pattern).all() and (got.raw_p[j, :, g].view(np.uint32) == pattern).all()
                assert got.value[(g, j)] == 0 and got.surprise[(g, j)] == 0
            else:
                seen_fit += 1
                assert got.rows[g][j].key() == w.key() and np.float32(got.value[(g, j)]).tobytes() == w.value().tobytes()
                assert (got.raw_q[j, len(w.visits):, g].view(np.uint32) == pattern).all()
        for j in range(got.lens[g], 2):
            assert (got.raw_q[j, :, g].view(np.uint32) == pattern).all()
    assert seen_fit > 0


def test_indices_that_name_no_example_give_zeros_and_are_counted():
    bad, count, zeros = harness("plain").bad
    assert bad == count and zeros


# ---- the pool carries the two scalars ------------------------------------------------------------------------------------------------------
from tests import pool_weights_util as pwu  # noqa: E402

POOL_MOVES, POOL_C = 5, 300


@functools.lru_cache(maxsize=None)
def pool_want(moves=POOL_MOVES):
    rules, n, wb, lg, states, salts, _over = shape()
    return ssu.twin_run(orc, lg, states, wb, salts, None, S, n_moves=moves)


@functools.lru_cache(maxsize=None)
def pool_examples(moves=POOL_MOVES):
    rules, n, wb, _lg, states, salts, over = shape()
    return ssu.host_examples_run(rules, n, wb, states, salts, S, K, over, moves)


def filled(weight=7):
    """A pool of 300 slots with the statistics and the weighting on after the ingest of the 325 examples of a five-move run (25 ranks
    dropped) and of the 65 of a one-move run (the ring wraps: 235 rows of generation 1 and 65 of generation 2 live), and its expectation."""
    n = shape()[1]
    pool, want = ssu.HostStatsPool(POOL_C, K, n), ssu.PoolExpectation(POOL_C)
    assert pool.set_search_stats(True) == 0
    pool.set_weighting(weight); want.model.set_weighting(weight)
    for moves in (POOL_MOVES, 1):
        rc, taken = pool.ingest(pool_examples(moves))
        assert rc == 0 and taken == want.ingest(pool_want(moves)) == G * moves
    return pool, want


def test_the_pool_holds_the_scalars_of_its_rows():
    pool, want = filled()
    assert pool.stats()["live"] == POOL_C == want.win.live
    slots = want.win.live_slots()
    bad, v, s = pool.gather_stats(slots, True)
    assert bad == 0
    want.check(slots, v, s, "two ingests")
    assert pool.trim(1) == 0
    want.win.trim(1)
    live = want.win.live_slots()
    assert 0 < len(live) < POOL_C and pool.stats()["live"] == len(live)
    bad, v, s = pool.gather_stats(live, True)
    assert bad == 0
    want.check(live, v, s, "after the trim")
    dead = [x for x in range(POOL_C) if x not in set(live)][:3] + [POOL_C, 2 ** 32 - 1]
    assert pool.gather_stats(dead, True)[0] == -1                      # host pointers: refused
    before = pool.stats()["bad_slot"]
    bad, v, s = pool.gather_stats(dead + live[:2], False)
    assert bad == len(dead) and pool.stats()["bad_slot"] == before + len(dead) and not v[:len(dead)].any() and not s[:len(dead)].any()
    want.check(live[:2], v[len(dead):], s[len(dead):], "beside dead slots")


def test_weights_from_surprise():
    pool, want = filled()
    pool.trim(2); want.win.trim(2)
    live = want.win.live_slots()
    _bad, _v, read = pool.gather_stats(list(range(POOL_C)), False)
    for base, per_nat, gen in ((3, 1000.0, 2), (11, 12345.678, 0), (5, 0.0, 1), (2 ** 32 - 16, 1e300, 2), (0, float("inf"), 0)):
        assert pool.weights_from_surprise(base, per_nat, gen) == 0
        want.weights_from_surprise(read, base, per_nat, gen)
        got = pool.raw_weights()
        assert [int(got[x]) for x in range(POOL_C)] == want.model.wt, (base, per_nat, gen)
    assert max(want.model.wt) == pwu.MAXW
    pool.trim(1); want.win.trim(1)
    dead_before = {x: want.model.wt[x] for x in range(POOL_C) if x not in set(want.win.live_slots())}
    assert pool.weights_from_surprise(9, 10.0) == 0
    want.weights_from_surprise(read, 9, 10.0)
    got = pool.raw_weights()
    assert all(int(got[x]) == w for x, w in dead_before.items()) and [int(w) for w in got] == want.model.wt      # dead slots untouched
    sl, sy, wt, total = pool.draw(500, 3, 9)
    ms, my, mw, mt, _ks = want.model.draw_many(3, 9, 0, 500)
    assert total == mt and sl.tobytes() == ms.tobytes() and sy.tobytes() == my.tobytes() and wt.tobytes() == mw.tobytes()


def test_what_the_pool_refuses():
    n = shape()[1]
    pool = ssu.HostStatsPool(POOL_C, K, n)
    assert pool.weights_from_surprise(1, 1.0) == -1                      # neither setting on
    assert pool.gather_stats([0], False)[0] == -1
    assert pool.ingest(pool_examples(), with_stats=False)[0] == 0        # off: an object without the arrays is taken
    assert pool.set_search_stats(True) == -1                             # live rows
    pool.clear()
    assert pool.set_search_stats(True) == 0
    assert pool.ingest(pool_examples(), with_stats=False)[0] == -1 and pool.stats()["live"] == 0
    assert pool.weights_from_surprise(1, 1.0) == -1                      # weighting off
    pool.set_weighting(1)
    assert pool.weights_from_surprise(1, 1.0) == 0
    assert pool.weights_from_surprise(1, -0.5) == -1 and pool.weights_from_surprise(1, float("nan")) == -1
    assert pool.weights_from_surprise(1, 1.0, flags=1) == -5 and all(pool.weights_from_surprise(1, 1.0, reserved=i) == -5 for i in range(3))
    assert pool.ingest(pool_examples())[0] == 0
    pool.clear()
    assert pool.set_search_stats(False) == 0 and pool.gather_stats([0], False)[0] == -1
