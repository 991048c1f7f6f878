"""Playout cap randomization in guided self-play (include/taflhip.h tafl_playout_cap) on the host harness
(tests/hostsim_caps: selfplay_step_capped and selfplay_reopen compiled for the CPU): 72 lanes, S = 16, fast_sims = 4, a quarter of the
moves full, temp_moves = 4, on the three preset layouts, against a chain of one-move oracle runs, against the per-move composition of two
uncapped one-move harness runs, at the two extremes, in two shards, and the invariants of the counters.  Every comparison is exact.
CPU only."""
import functools

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlayoutCap, TaflState
from oracle import oracle as orc
from tests import episodes_util as epu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import playout_cap_util as pcu

G, S, FAST = pcu.G, pcu.S, pcu.FAST
LAYOUTS = list(pcu.SHAPES)


def _run(cfg, episodes, cap, noise=None, states=None, salts=None, base=pcu.IDS, stride=G, S_=S, ex="new"):
    rules, n, wb, _lg, st, sa, _over, _S, budget = pcu.shape(orc, cfg)
    states, salts = st if states is None else states, sa if salts is None else salts
    if ex == "new":
        ex = pcu.HostExamples(n, len(states), budget, S_)
    got = pcu.host_capped(rules, n, wb, states, S_, salts, budget, cap, ex, episodes=episodes, base=base, stride=stride if episodes else 0, noise=noise)
    assert not any(got.faults) and got.stat_faults == 0
    if ex is not None:
        assert ex.counts()[1] == {"dropped": 0, "overflowed": 0}
    return got, ex


@functools.lru_cache(maxsize=None)
def capped(cfg, episodes, noisy=False):
    return _run(cfg, episodes, pcu.cap_of(cfg), nu.noise_cfg() if noisy else None)[0]


@functools.lru_cache(maxsize=None)
def composed(cfg, episodes, noisy=False):
    rules, n, wb, _lg, states, salts, over, _S, budget = pcu.shape(orc, cfg)
    route = pcu.host_route(rules, n, wb, salts, FAST, nu.noise_cfg() if noisy else None)
    return pcu.composition(route, states, over, budget, pcu.CAP_SEED[cfg], pcu.FULL_PER, episodes, base=pcu.IDS, stride=G)


def test_the_shapes_are_those_of_the_gpu_episodes_tests():
    from tests import test_gpu_episodes as tge
    assert pcu.SHAPES == tge.SHAPES and pcu.G == tge.G
    assert (pcu.S, pcu.FAST, pcu.FULL_PER, pcu.TEMP) == (16, 4, 16384, 4)


@pytest.mark.parametrize("cfg", LAYOUTS)
def test_the_inputs_meet_the_conditions(cfg):
    """Asserted on the expectation (the composition), for the plain and the episodes run."""
    states = pcu.shape(orc, cfg)[4]
    for episodes in (False, True):
        want = composed(cfg, episodes)
        total = sum(want.moves)
        print(cfg, "episodes" if episodes else "plain", "moves", total, "full", want.full, "fast", want.fast, "episodes", sum(want.episodes), "closed sizes", sorted(want.closed))
        assert want.full + want.fast == total and 5 * want.full >= total and 5 * want.fast >= total
        after_full = sum(any(a and not b for a, b in zip(c, c[1:])) for c in want.classes)
        after_fast = sum(any(b and not a for a, b in zip(c, c[1:])) for c in want.classes)
        assert after_full >= 18 and after_fast >= 18, (after_full, after_fast)
        # a drawn play (M < temp_moves) of each class: in a plain run M = m, in an episodes run the first moves of a lane are episode 0's
        drawn = [c[m] for g, c in enumerate(want.classes) for m in range(min(len(c), pcu.TEMP)) if states[g].status == abi.ONGOING]
        assert any(drawn) and not all(drawn)
    want = composed(cfg, True)
    assert any(want.open_at_budget)
    if cfg == "brandubh7":
        assert 0 in want.closed and any(c >= 2 for c in want.closed), sorted(want.closed)


@pytest.mark.parametrize("cfg", LAYOUTS)
def test_ten_spot_lanes_equal_a_chain_of_one_move_oracle_runs(cfg):
    _rules, _n, wb, lg, states, salts, _over, _S, budget = pcu.shape(orc, cfg)
    ongoing = [g for g in range(G) if states[g].status == abi.ONGOING]
    spots = [g for g in (0, 1, 63, 64, 65, 70, 71, 30, 31, 32, 2, 3, 4, 5, 6) if g in ongoing][:10]
    assert len(spots) == 10
    want = pcu.oracle_chain(orc, lg, wb, states, salts, budget, pcu.CAP_SEED[cfg], pcu.FULL_PER, FAST, spots, base=pcu.IDS)
    got = capped(cfg, False)
    assert any(True in want.classes[g] and False in want.classes[g] for g in spots)
    for g in spots:
        assert got.plays[g] == want.plays[g], (cfg, "plays", g)
        assert got.states[g] == want.states[g], (cfg, "state", g)
        assert got.examples[g] == want.examples[g], (cfg, "examples", g)
        assert got.moves[g] == want.moves[g], (cfg, "moves", g)


@pytest.mark.parametrize("cfg", LAYOUTS)
def test_the_plain_capped_run_equals_the_composition(cfg):
    got, want = capped(cfg, False), composed(cfg, False)
    pcu.assert_equal(got, want, (cfg, "plain"))
    assert got.cap_stats == (want.full, want.fast)


@pytest.mark.parametrize("cfg", LAYOUTS)
def test_the_noisy_episodes_capped_run_equals_the_composition(cfg):
    """The full route runs with root noise, the fast route without."""
    got, want = capped(cfg, True, True), composed(cfg, True, True)
    pcu.assert_equal(got, want, (cfg, "episodes, noise"))
    assert got.cap_stats == (want.full, want.fast) and got.open_from == want.open_from
    quiet = composed(cfg, True)
    assert quiet.plays != want.plays                                  # (the noise changes the run)


@pytest.mark.parametrize("cfg", LAYOUTS)
def test_every_move_full_equals_the_uncapped_run(cfg):
    """full_per_65536 = 65536: everything the uncapped run of tests/hostsim_episodes leaves, noise, z and open_from included; and the
    plain run against tests/hostsim."""
    rules, n, wb, _lg, states, salts, _over, _S, budget = pcu.shape(orc, cfg)
    ncfg = nu.noise_cfg()
    got, ex = _run(cfg, True, pcu.cap_of(cfg, 65536), ncfg)
    wex = epu.HostExamples(n, G, budget, S)
    want, faults, _ = epu.host_episodes(rules, n, wb, states, S, pcu.CPUCT, salts, budget, pcu.SSEED, pcu.TEMP, wex, base=pcu.IDS, stride=G, noise=ncfg)
    assert not any(faults)
    epu.assert_same(got, want, (cfg, "all full"))
    assert ex.counts() == wex.counts() and got.moves == [len(p) for p in want.plays]
    assert got.cap_stats == (sum(got.moves), 0) and sum(want.episodes) > 0
    got, ex = _run(cfg, False, pcu.cap_of(cfg, 65536))
    pex = gsu.HostExamples(n, G, budget, S)
    run, faults, _ = gsu.host_run(rules, n, wb, states, S, pcu.CPUCT, salts, budget, pcu.SSEED, pcu.TEMP, ex=pex, base=pcu.IDS)
    assert not any(faults) and got.sims == run.sims
    run.examples = pex.all()[0]
    assert sum(len(col) for col in run.examples) == sum(run.moves) > 0
    gsu.assert_same_run(_as_run(got, budget), run, [[f for f, _z, _fin in col] for col in got.examples], where=(cfg, "all full, plain"))


def _as_run(lanes, budget):
    run = gsu.Run(len(lanes.states), budget)
    run.plays = [[lanes.plays[g][m] if m < len(lanes.plays[g]) else (0, 0, 0, 0) for g in range(len(lanes.states))] for m in range(budget)]
    run.states, run.moves, run.sims = lanes.states, lanes.moves, lanes.sims
    return run


@pytest.mark.parametrize("cfg", LAYOUTS)
def test_every_move_fast_equals_the_uncapped_run_at_fast_sims_that_records_nothing(cfg):
    """full_per_65536 = 0 with noise latched: the uncapped run at n_sims = fast_sims without noise and with ex = NULL; the examples object
    is untouched."""
    rules, n, wb, _lg, states, salts, _over, _S, budget = pcu.shape(orc, cfg)
    got, ex = _run(cfg, True, pcu.cap_of(cfg, 0), nu.noise_cfg())
    want, faults, _ = epu.host_episodes(rules, n, wb, states, FAST, pcu.CPUCT, salts, budget, pcu.SSEED, pcu.TEMP, None, base=pcu.IDS, stride=G)
    assert not any(faults)
    epu.assert_same(got, want, (cfg, "all fast"))
    assert got.moves == [len(p) for p in want.plays] and got.cap_stats == (0, sum(got.moves))
    assert ex.counts() == ([0] * G, {"dropped": 0, "overflowed": 0}, [0] * G)
    got, ex = _run(cfg, False, pcu.cap_of(cfg, 0))
    run, faults, _ = gsu.host_run(rules, n, wb, states, FAST, pcu.CPUCT, salts, budget, pcu.SSEED, pcu.TEMP, ex=None, base=pcu.IDS)
    assert not any(faults) and got.sims == run.sims
    run.examples = [[] for _ in range(G)]
    gsu.assert_same_run(_as_run(got, budget), run, got.examples, where=(cfg, "all fast, plain"))
    assert ex.counts()[0] == [0] * G


@pytest.mark.parametrize("episodes", [False, True])
def test_two_shards_equal_the_whole(episodes):
    """Lanes [0, 36) and [36, 72) with game_id_base offset (and id_stride = 72): the class is a function of the game id, not of the lane."""
    cfg = "brandubh7"
    states, salts = pcu.shape(orc, cfg)[4], pcu.shape(orc, cfg)[5]
    whole = capped(cfg, episodes)
    half, total, caps = G // 2, [0, 0, 0, 0], [0, 0]
    for first in (0, half):
        part, _ex = _run(cfg, episodes, pcu.cap_of(cfg), states=(TaflState * half)(*[states[first + g] for g in range(half)]), salts=salts[first:first + half],
                         base=pcu.IDS + first, stride=G)
        for g in range(half):
            assert part.plays[g] == whole.plays[first + g] and part.states[g] == whole.states[first + g], (first, g)
            assert part.examples[g] == whole.examples[first + g] and part.episodes[g] == whole.episodes[first + g], (first, g)
        total = [a + b for a, b in zip(total, part.counters)]
        caps = [a + b for a, b in zip(caps, part.cap_stats)]
    assert total == list(whole.counters) and tuple(caps) == whole.cap_stats


@pytest.mark.parametrize("cfg", LAYOUTS)
@pytest.mark.parametrize("episodes", [False, True])
def test_invariants_of_the_counters(cfg, episodes):
    got = capped(cfg, episodes)
    full, fast = got.cap_stats
    assert full + fast == sum(got.moves) and full > 0 and fast > 0
    assert sum(len(col) for col in got.examples) == full               # (nothing was dropped: _run)
    assert got.sims == S * full + FAST * fast                         # (no faults: _run)


def test_what_the_harness_refuses():
    """The checks of tafl_gselfplay_set_playout_cap and of the begin, restated beside the harness."""
    L = pcu.hlib()
    import ctypes as C

    def check(fast, full_per, flags=0, reserved=None, sims=S):
        cap = TaflPlayoutCap(0, fast, full_per, flags)
        if reserved is not None:
            cap._reserved[reserved] = 1
        return L.hsc_cap_check(C.byref(cap), sims)
    assert check(4, 16384) == 0 and check(2, 0) == 0 and check(16, 65536) == 0
    assert check(1, 16384) == -1 and check(65536, 16384, sims=65535) == -1 and check(4, 65537) == -1 and check(17, 16384) == -1
    assert check(4, 16384, flags=1) == -5 and all(check(4, 16384, reserved=i) == -5 for i in range(3))
