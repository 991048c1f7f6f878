"""Value targets from search values (include/taflhip.h "value targets") on the host harness
(tests/hostsim_value_targets: the product's vt_mark_boundary after every round of tests/hostsim_search_stats' sessions, vt_stage and
vt_step for the targets) against the Python twins (tests/value_targets_util.py): Brandubh 7 x 7 / u64, 65 lanes at (7 g) mod 60 plies,
S = 16, a lane budget of 20.  vt, kind, ep_end, settled z and final and the counters bit for bit.  CPU only."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import noise_util as nu
from tests import search_stats_util as ssu
from tests import value_targets_util as vtu

G, K = vtu.G, vtu.K
LAMBDAS = (0.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def shape():
    return ssu.shape(orc, "brandubh7", G, vtu.MODULUS)


@functools.lru_cache(maxsize=None)
def expectation(mode):
    rules, n, wb, lg, states, salts, _over = shape()
    return vtu.twin(orc, lg, states, wb, salts, nu.HostSide(rules, n, wb), **vtu.MODES[mode])


def recorded(mode, targets_on=True, K_=K, max_moves=vtu.BUDGET):
    rules, n, wb, _lg, states, salts, _over = shape()
    ex = vtu.HostExamples(n, G, max_moves, K_)
    ex.run(rules, wb, states, salts, targets_on=targets_on, **vtu.MODES[mode])
    return ex


@functools.lru_cache(maxsize=None)
def harness(mode):
    return recorded(mode)


def test_the_expectation_meets_the_conditions():
    """Asserted on the twins alone, over the runs of this file."""
    tot = {}
    for mode in vtu.MODES:
        c = vtu.coverage(expectation(mode))
        print(mode, c)
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
    assert tot["closed"] >= 20 and tot["cut"] >= 10 and tot["tails"] >= 10 and tot["three"] >= 10 and tot["gaps"] >= 20 and tot["quiet"] >= 5 and tot["empty"] >= 1
    assert tot["flips"] >= 1, tot


@pytest.mark.parametrize("mode", list(vtu.MODES))
def test_boundaries_and_targets_equal_the_twin(mode):
    ex, want = harness(mode), expectation(mode)
    lens, dropped, overflowed = ex.lens()
    assert dropped == 0 and overflowed == 0
    rows, _plain = ex.rows()
    vtu.assert_recorded(rows, want, mode)
    index = vtu.index_of(lens, G)
    rc, _t, _k, ee = ex.gather_targets(index, want=(False, False, True))
    assert rc == 0 and [int(x) for x in ee] == [want.lanes[e % G][e // G].ep_end for e in index], "boundaries can be read before any target exists"
    for lam in LAMBDAS:
        exp = vtu.targets(want, lam)
        rc, o4 = ex.value_targets(lam)
        assert rc == 0 and o4 == (exp.closed, exp.unfinished, exp.rows, 0), (mode, lam, o4)
        rc, t, kd, ee = ex.gather_targets(index)
        assert rc == 0
        vtu.assert_targets(index, G, t, kd, ee, want, exp, (mode, lam))
        if lam == 1.0:                                            # the two identities
            for i, e in enumerate(index):
                en = want.lanes[e % G][e // G]
                if kd[i] == 1:
                    assert np.float32(t[i]).tobytes() == np.float32(en.z).tobytes()
                elif kd[i] == 2:
                    ep = [x for x in vtu.episodes_of(want.lanes[e % G], len(want.lanes[e % G])) if e // G in x][0]
                    last = want.lanes[e % G][[j for j in ep if sum(want.lanes[e % G][j].row.visits) > 0][-1]].row
                    sign = 1.0 if last.side == en.row.side else -1.0
                    assert np.float32(t[i]).tobytes() == np.float32(sign * float(last.value())).tobytes()


@pytest.mark.parametrize("mode", list(vtu.MODES))
def test_the_recorder_changes_nothing_else(mode):
    on, off = harness(mode).rows()[1], recorded(mode, targets_on=False).rows()[1]
    assert on == off and len(on) > 0


def test_the_recorder_changes_nothing_else_in_the_two_other_runs():
    """K = 4 with room for two examples, and a plain run continued with move_base: every parent array equal to the run without the flag."""
    rules, n, wb, _lg, states, salts, _over = shape()
    assert recorded("episodes", K_=4, max_moves=2).rows()[1] == recorded("episodes", targets_on=False, K_=4, max_moves=2).rows()[1]
    got = []
    for on in (True, False):
        ex = vtu.HostExamples(n, G, 6, K)
        ex.run(rules, wb, states, salts, n_moves=3, targets_on=on)
        ex.run(rules, wb, states, salts, n_moves=3, move_base=3, base=vtu.BASE + 5000, targets_on=on)
        got.append(ex.rows()[1])
    assert got[0] == got[1] and len(got[0]) > 3 * G


def test_settling_unfinished_episodes_and_a_finalize_after_it():
    rules, n, wb, _lg, _states, _salts, over = shape()
    ex, want = recorded("cut"), expectation("cut")
    lens, _d, _o = ex.lens()
    index = vtu.index_of(lens, G)
    exp = vtu.targets(want, 0.5, settle=True)
    rc, o4 = ex.value_targets(0.5, settle=True)
    assert rc == 0 and o4 == (exp.closed, exp.unfinished, exp.rows, exp.settled) and exp.settled > 0
    rc, t, kd, ee = ex.gather_targets(index)
    rows, _p = ex.rows()
    z, fin = [rows[e % G][e // G][1] for e in index], [rows[e % G][e // G][2] for e in index]
    vtu.assert_targets(index, G, t, kd, ee, want, exp, "settled", z, fin)
    rc, again = ex.value_targets(0.5, settle=True)               # settled rows stay unfinished: the call can be repeated
    assert rc == 0 and again == o4
    # a pool without the setting now takes every row with a policy: skipped_open falls to 0
    pool = vtu.HostPool(4096, K, n)
    rc, o3 = pool.ingest(ex)
    assert rc == 0 and o3 == (exp.rows, 0, 0)
    # finalize rewrites the open tail and marks the result stale
    ex.finalize(over)
    assert not ex.valid() and ex.gather_targets(index)[0] == -1
    import copy
    want2 = copy.deepcopy(want)
    for g, lane in enumerate(want2.lanes):                       # what the settlement left in the cut episodes stands
        for j, en in enumerate(lane):
            en.z, en.fin = float(exp.z[(g, j)]), exp.fin[(g, j)]
    vtu.finalize(want2, over)
    exp2 = vtu.targets(want2, 0.5)
    rc, o4 = ex.value_targets(0.5)
    assert rc == 0 and o4 == (exp2.closed, exp2.unfinished, exp2.rows, 0)
    rc, t, kd, ee = ex.gather_targets(index)
    vtu.assert_targets(index, G, t, kd, ee, want2, exp2, "after finalize")


def test_a_plain_run_continued_with_move_base_is_one_episode():
    rules, n, wb, lg, states, salts, _over = shape()
    ex = vtu.HostExamples(n, G, 6, K)
    want = vtu.twin(orc, lg, states, wb, salts, None, n_moves=3)
    ex.run(rules, wb, states, salts, n_moves=3)
    # the second run starts where the first ended: its states are the twin's, reached by replaying the recorded plays
    import ctypes as C
    from alphazeroforhnefatafl_amd import abi
    nxt = []
    for g in range(G):
        st = orc.GameState.from_abi(states[g], wb)
        for en in want.lanes[g]:
            _c, st, _e = lg.do_play(abi.action_decode(n, en.row.played), st)
        nxt.append(st.to_abi())
    nxt = (abi.TaflState * G)(*nxt)
    want = vtu.twin(orc, lg, nxt, wb, salts, None, n_moves=3, move_base=3, into=want)
    ex.run(rules, wb, nxt, salts, n_moves=3, move_base=3)
    assert not ex.valid()
    lens, _d, _o = ex.lens()
    index = vtu.index_of(lens, G)
    vtu.assert_recorded(ex.rows()[0], want, "two runs")
    exp = vtu.targets(want, 0.5)
    assert exp.closed == 0 and exp.unfinished == sum(1 for lane in want.lanes if lane)
    rc, o4 = ex.value_targets(0.5)
    assert rc == 0 and o4 == (0, exp.unfinished, exp.rows, 0)
    rc, t, kd, ee = ex.gather_targets(index)
    assert rc == 0 and not ee.any()
    vtu.assert_targets(index, G, t, kd, ee, want, exp, "two runs")


def test_examples_without_a_policy_take_no_part():
    """K = 4 and room for two examples per lane: an overflowed example has vt = 0, kind = 0 and the chain passes over it."""
    rules, n, wb, _lg, states, salts, _over = shape()
    ex, want = recorded("episodes", K_=4, max_moves=2), expectation("episodes")
    lens, dropped, overflowed = ex.lens()
    assert dropped > 0 and overflowed > 0 and max(lens) == 2
    index = vtu.index_of(lens, G)
    exp = vtu.targets(want, 0.5, Kmax=4, max_moves=2)
    rc, o4 = ex.value_targets(0.5)
    assert rc == 0 and o4 == (exp.closed, exp.unfinished, exp.rows, 0) and exp.rows < len(index)
    rc, t, kd, _ee = ex.gather_targets(index)
    vtu.assert_targets(index, G, t, kd, None, want, exp, "K = 4")
    inside = [g for g in range(G) if lens[g] == 2 and exp.kind[(g, 0)] == 0 and exp.kind[(g, 1)] != 0 and not want.lanes[g][0].ep_end]
    assert inside, "an example without a policy inside an episode"


def test_staleness_and_refusals():
    rules, n, wb, _lg, states, salts, over = shape()
    ex = recorded("episodes")
    lens, _d, _o = ex.lens()
    index = vtu.index_of(lens, G)
    assert not ex.valid() and ex.gather_targets(index)[0] == -1
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        assert ex.value_targets(lam)[0] == -1
    assert ex.value_targets(0.5, flags=2)[0] == -5 and all(ex.value_targets(0.5, reserved=i)[0] == -5 for i in range(5))
    assert not ex.valid()
    assert ex.value_targets(0.5)[0] == 0 and ex.valid()
    bad = [G * vtu.BUDGET, 0xFFFFFFFF] + [j * G + g for g in range(G) for j in range(lens[g], vtu.BUDGET)][:3]
    assert ex.gather_targets(bad + index[:2])[0] == -1                       # host pointers: refused
    rc, t, kd, ee = ex.gather_targets(bad + index[:2], strict=False)
    assert rc == len(bad) and not t[:len(bad)].any() and not kd[:len(bad)].any() and not ee[:len(bad)].any()
    ex.finalize(over)
    assert not ex.valid()
    assert ex.value_targets(0.5)[0] == 0 and ex.valid()
    ex.run(rules, wb, states, salts, n_moves=1)                              # run begin
    assert not ex.valid()
    assert ex.value_targets(0.5)[0] == 0 and ex.valid()
    ex.clear()
    assert not ex.valid() and ex.lens()[0] == [0] * G


# ---- the pool carries vt and kind ------------------------------------------------------------------------------------------------------------
def test_the_pool_holds_the_targets_of_its_rows():
    rules, n, wb, _lg, _states, _salts, _over = shape()
    ex, want = recorded("cut"), expectation("cut")
    pool, model = vtu.HostPool(300, K, n), vtu.PoolModel(300)
    assert pool.set_value_targets(True) == -1                                # needs the statistics
    assert pool.set_search_stats(True) == 0 and pool.set_value_targets(True) == 0
    assert pool.ingest(ex)[0] == -1 and pool.ingest(ex, with_targets=False)[0] == -1      # stale; an object without the flag
    exp = vtu.targets(want, 0.5)
    assert ex.value_targets(0.5)[0] == 0
    order = vtu.taken_order(want, exp)
    rc, o3 = pool.ingest(ex)
    assert rc == 0 and o3[0] == len(order) == model.ingest([(exp.vt[x], exp.kind[x]) for x in order]) and o3[1] > 0
    open_before = o3[1]
    exp = vtu.targets(want, 0.9, settle=True)                                # settled: nothing stays open, 300 slots drop ranks and wrap
    assert ex.value_targets(0.9, settle=True)[0] == 0
    order = vtu.taken_order(want, exp)
    rc, o3 = pool.ingest(ex)
    assert rc == 0 and o3 == (len(order), 0, 0) and len(order) > 300 and open_before == len(order) - model.gens[0]
    model.ingest([(exp.vt[x], exp.kind[x]) for x in order])
    slots = model.live_slots()
    assert len(slots) == 300 == pool.stats()["live"]
    bad, t, kd = pool.gather_targets(slots)
    assert bad == 0 and set(int(x) for x in kd) == {1, 2}
    model.check(slots, t, kd, "past the wrap")
    exp1 = vtu.targets(want, 1.0)
    assert ex.value_targets(1.0)[0] == 0
    order = [x for x in vtu.taken_order(want, exp)]                          # (z and final stay settled)
    rc, o3 = pool.ingest(ex)
    assert rc == 0 and o3[0] == len(order)
    # after the settlement the rows of cut episodes are final = 2: kind stays 2, vt at lambda = 1 is the last value
    exp1s = vtu.targets(want, 1.0, settle=True)
    model.ingest([(exp1s.vt[x], exp1s.kind[x]) for x in order])
    assert pool.trim(1) == 0
    model.trim(1)
    live = model.live_slots()
    bad, t, kd = pool.gather_targets(live)
    assert bad == 0
    model.check(live, t, kd, "after the trim")
    dead = [300, 2 ** 32 - 1]
    assert pool.gather_targets(dead)[0] == -1
    before = pool.stats()["bad_slot"]
    bad, t, kd = pool.gather_targets(dead + live[:2], strict=False)
    assert bad == 2 and pool.stats()["bad_slot"] == before + 2 and not t[:2].any() and not kd[:2].any()
    assert pool.set_value_targets(False) == -1                               # live rows
    pool.clear()
    assert pool.set_search_stats(False) == 0 and pool.gather_targets([0])[0] == -1      # the statistics off take the targets with them
