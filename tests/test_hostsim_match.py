"""Match play (include/taflhip.h tafl_gmatch_*) on the host harness (tests/hostsim_match: match_owner,
selfplay_step_episodes given the compact row pointer, match_tally and selfplay_reopen compiled for the CPU, the partition as the
obvious sequential loop) against the oracle match loop (tests/match_util.oracle_match), and the ABI of the four entry points.  CPU only."""
import ctypes as C
import functools
import os

import pytest

from alphazeroforhnefatafl_amd import _lib, abi
from alphazeroforhnefatafl_amd.abi import TaflState
from oracle import oracle as orc
from tests import episodes_util as epu
from tests import match_util as mu
from tests import rare_workloads as rw

G, S, BUDGET = mu.G0, mu.S0, mu.BUDGET


def setup():
    return epu.setup(orc, "brandubh7", G, mu.MODULUS)


@functools.lru_cache(maxsize=None)
def want(swap=0, episode_moves=0):
    """The oracle route of the base setting."""
    _rules, _n, wb, lg, states, _salts, _over = setup()
    return mu.oracle_match(orc, lg, wb, states, states, S, mu.CPUCT, mu.SALT, BUDGET, mu.SSEED, mu.TEMP, mu.IDS, G, episode_moves, swap)


@functools.lru_cache(maxsize=None)
def got(swap=0, episode_moves=0):
    rules, n, wb, _lg, states, _salts, _over = setup()
    ex = mu.HostExamples(n, G, BUDGET, S)
    out, games, faults, rounds = mu.host_match(rules, n, wb, states, S, mu.CPUCT, mu.SALT, BUDGET, mu.SSEED, mu.TEMP, ex, base=mu.IDS, stride=G, episode_moves=episode_moves,
                                               swap=swap)
    assert not any(faults) and out.stat_faults == 0
    return out, games, ex


def test_the_base_setting_fills_every_cell():
    """On the oracle route: every (seat, winner) cell holds two games or more, two lanes close two episodes or more, two lanes are over
    at the start; and the tally is the one the setting was chosen for."""
    states = setup()[4]
    lanes, games = want()
    print("games", games, "episodes", lanes.episodes)
    assert all(games[a][r] >= 2 for a in range(2) for r in range(2))
    assert sum(e >= 2 for e in lanes.episodes) >= 2
    assert sum(states[g].status != abi.ONGOING for g in range(G)) == 2
    assert games == [[3, 2, 0, 0], [4, 3, 0, 0]] and want(1)[1] == [[3, 3, 0, 0], [2, 5, 0, 0]]
    assert games == mu.games_from_lanes(lanes, mu.IDS, 0)


@pytest.mark.parametrize("swap", [0, 1])
def test_the_match_equals_the_oracle_match_loop(swap):
    out, games, ex = got(swap)
    lanes, wgames = want(swap)
    epu.assert_same(out, lanes, ("oracle route", swap))
    assert games == wgames
    _lens, ct, open_from = ex.counts()
    assert ct == {"dropped": 0, "overflowed": 0} and open_from == lanes.open_from
    # the column sums are the episode counters
    assert [games[0][r] + games[1][r] for r in range(4)] == list(out.counters) == list(lanes.counters)
    assert sum(out.counters) == sum(out.episodes)


def test_swap_changes_the_match():
    assert want(0)[0].plays != want(1)[0].plays


def test_an_episode_cap_fills_the_cut_cells():
    lanes, wgames = want(0, 5)
    assert wgames[0][3] > 0 and wgames[1][3] > 0 and any(lanes.capped)
    out, games, ex = got(0, 5)
    epu.assert_same(out, lanes, "episode_moves = 5")
    assert games == wgames and [games[0][r] + games[1][r] for r in range(4)] == list(out.counters)
    assert ex.counts()[2] == lanes.open_from


def test_two_shards_equal_the_whole():
    rules, n, wb, _lg, states, _salts, _over = setup()
    whole, games, _ex = got(0)
    half = G // 2
    total = [[0] * 4, [0] * 4]
    for first in (0, half):
        sub = (TaflState * half)(*[states[first + g] for g in range(half)])
        ex = mu.HostExamples(n, half, BUDGET, S)
        part, pg, faults, _ = mu.host_match(rules, n, wb, sub, S, mu.CPUCT, mu.SALT, BUDGET, mu.SSEED, mu.TEMP, ex, base=mu.IDS + first, stride=G)
        assert not any(faults)
        for g in range(half):
            assert part.plays[g] == whole.plays[first + g] and part.states[g] == whole.states[first + g], (first, g)
            assert part.examples[g] == whole.examples[first + g] and part.episodes[g] == whole.episodes[first + g], (first, g)
        total = [[a + b for a, b in zip(total[e], pg[e])] for e in range(2)]
    assert total == games


def test_a_larger_board_from_positions_where_games_end():
    """Copenhagen 11x11, a few lanes of the rare-rule workload: positions from which the guided run ends the game within its moves, and
    some where it does not."""
    name = "copenhagen11"
    cfg = rw.CONFIGS[name]
    w, _, _ = rw.mcts_workload(name)
    plain = rw.gselfplay_expectation(name)
    ending = [g for g in range(w.G) if TaflState.from_buffer_copy(plain.states[g]).status != abi.ONGOING and plain.moves[g] >= 1][:4]
    going = [g for g in range(w.G) if TaflState.from_buffer_copy(plain.states[g]).status == abi.ONGOING][:2]
    pick = ending + going
    assert len(ending) == 4 and len(going) == 2
    states = (TaflState * len(pick))(*[w.states[g] for g in pick])
    lg = orc.GameLogic(cfg.rules, cfg.n)
    S_, budget = rw.guided_sims(name), 6
    lanes, wgames = mu.oracle_match(orc, lg, cfg.wb, states, states, S_, mu.CPUCT, mu.SALT, budget, mu.SSEED, 2, 500, 0, 0, 1)
    print(name, "games", wgames, "episodes", lanes.episodes)
    assert sum(e >= 1 for e in lanes.episodes) >= 2 and sum(wgames[0]) >= 1 and sum(wgames[1]) >= 1
    ex = mu.HostExamples(cfg.n, len(pick), budget, S_)
    out, games, faults, _ = mu.host_match(cfg.rules, cfg.n, cfg.wb, states, S_, mu.CPUCT, mu.SALT, budget, mu.SSEED, 2, ex, base=500, swap=1)
    assert not any(faults)
    epu.assert_same(out, lanes, name)
    assert games == wgames


def test_abi_of_the_match_entry_points():
    assert C.sizeof(abi.TaflMatchOpts) == 32 == abi.EXPECTED_SIZES["tafl_match_opts"]
    assert C.sizeof(abi.TaflMatchStats) == 128 == abi.EXPECTED_SIZES["tafl_match_stats"]
    assert C.sizeof(abi.TaflMatchIo) == 8 * C.sizeof(C.c_void_p) + 8
    assert abi.TaflMatchStats.games.offset == 0 and abi.TaflMatchStats._reserved.offset == 64 and abi.TaflMatchIo.cap.offset == 8 * C.sizeof(C.c_void_p)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "taflhip.h")).read()
    assert "} tafl_match_opts;             /* 32 bytes */" in hdr and "} tafl_match_stats;            /* 128 bytes */" in hdr
    L = C.CDLL(_lib.LIB_PATH)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in ("tafl_gmatch_begin", "tafl_gmatch_leaves", "tafl_gmatch_step", "tafl_gmatch_get_stats"):
        assert hasattr(L, name) and name in bound, name
