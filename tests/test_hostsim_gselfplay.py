"""Guided self-play at each game's own pace (include/taflhip.h tafl_gselfplay_*): the product's per-game code
(tafl_guided.hpp Guided::selfplay_step, compiled for the host in tests/hostsim) against the oracle loop - orc.GameLogic.gmcts,
then examples_util.pick_rule with examples_util.sample_word, then the oracle's do_play - per game and move.  The evaluator is
tests/stub_net.stub_predict with a per-game salt.  Every comparison is exact.  CPU only."""
import ctypes as C
import random

import pytest

from alphazeroforhnefatafl_amd import abi
from oracle import oracle as orc
from tests import examples_util as eu
from tests import gselfplay_util as gsu
from tests import parity_util as pu

CPUCT, SEED = 1.25, 5
#            G   S  n_moves temp_moves  start positions: game i advanced by (7 i) mod this many random plies (0: the start position)
SETTINGS = {"brandubh7": (24, 24, 8, 4, 60), "copenhagen11": (6, 16, 3, 2, 36), "tablut9": (8, 16, 4, 4, 0), "copenhagen13": (4, 12, 2, 1, 0)}
_CACHE = {}


def setting(cfg):
    """(rules, n, wb, states, salts, the oracle loop's Run) of a setting, computed once and never modified."""
    if cfg not in _CACHE:
        G, S, n_moves, temp_moves, modulus = SETTINGS[cfg]
        rules, fen, wb = pu.CONFIGS[cfg]
        n = abi.fen_side_len(fen)
        lg = orc.GameLogic(rules, n)
        states = gsu.start_states(orc, lg, rules, fen, wb, G, modulus)
        salts = [(3 * g + 1) % 256 for g in range(G)]
        _CACHE[cfg] = (rules, n, wb, states, salts, gsu.oracle_run(orc, lg, states, wb, S, CPUCT, salts, n_moves, SEED, temp_moves))
    return _CACHE[cfg]


@pytest.mark.parametrize("cfg", list(SETTINGS))
def test_run_matches_the_oracle_loop(cfg):
    G, S, n_moves, temp_moves, _ = SETTINGS[cfg]
    rules, n, wb, states, salts, want = setting(cfg)
    if cfg == "brandubh7":                       # the three fates of a game, on the oracle route
        over0, ended, going = gsu.fates(states, want)
        assert over0 and ended and going, (over0, ended, going)
        drawn = [e for row in want.examples for e in row if e[5] < temp_moves]      # fields: board, side, actions, visits, played, move_no
        assert any(e[4] != e[2][e[3].index(max(e[3]))] for e in drawn), "no drawn play differs from the most visited one"
    ex = gsu.HostExamples(n, G, n_moves, S)
    got, faults, _rounds = gsu.host_run(rules, n, wb, states, S, CPUCT, salts, n_moves, SEED, temp_moves, ex)
    examples, overflow = ex.all()
    gsu.assert_same_run(got, want, examples, where=cfg)
    assert got.sims == want.sims and not any(faults) and got.stat_faults == 0
    lens, counters = ex.counts()
    assert lens == want.moves and counters == {"dropped": 0, "overflowed": 0, "bad_index": 0} and not any(any(o) for o in overflow)


def test_edge_pick_is_the_pick_rule_over_the_visited_edges():
    """Guided::selfplay_pick over an edge block with unvisited edges in between == pick_rule over the visited ones, at every boundary
    ceil(j * 2^32 / N) of r and one below it, and on random words."""
    L = gsu.hlib()
    rng = random.Random(11)
    vectors = [[0, 3, 0, 0, 1, 2, 0], [5], [0, 0, 7], [1, 0, 1, 0, 1, 0], [0, 65535, 1, 0, 65535]]
    vectors += [[rng.choice([0, 0, rng.randint(1, 1000)]) for _ in range(rng.randint(1, 200))] + [rng.randint(1, 9)] for _ in range(20)]
    for vis in vectors:
        N, m = sum(vis), len(vis)
        seen = [i for i, v in enumerate(vis) if v]
        rs = {0, eu.M32}
        for j in (range(1, N) if N <= 4096 else rng.sample(range(1, N), 4096)):
            b = -((-j << 32) // N)
            rs.update((b, b - 1))
        rs.update(rng.getrandbits(32) for _ in range(256))
        rs = sorted(r for r in rs if 0 <= r <= eu.M32)
        arr, out = (C.c_uint32 * len(rs))(*rs), (C.c_uint32 * len(rs))()
        L.hsg_pick_many((C.c_uint32 * m)(*vis), m, arr, len(rs), out)
        dense = [v for v in vis if v]
        assert list(out) == [seen[eu.pick_rule(dense, r)] for r in rs], vis
    assert [L.hsg_rand(9, g, mv) for g in (0, 1, 1 << 40) for mv in (0, 7)] == [eu.sample_word(9, g, mv) for g in (0, 1, 1 << 40) for mv in (0, 7)]


def test_an_episode_in_two_runs_equals_one_run():
    G, S, n_moves, temp_moves, _ = SETTINGS["brandubh7"]
    rules, n, wb, states, salts, want = setting("brandubh7")
    first = 3
    ex = gsu.HostExamples(n, G, n_moves, S)
    a, _, _ = gsu.host_run(rules, n, wb, states, S, CPUCT, salts, first, SEED, temp_moves, ex)
    b, _, _ = gsu.host_run(rules, n, wb, a.abi_states, S, CPUCT, salts, n_moves - first, SEED, temp_moves, ex, move_base=first)
    both = gsu.Run(G, n_moves)
    both.plays, both.states, both.moves = a.plays + b.plays, b.states, [x + y for x, y in zip(a.moves, b.moves)]
    gsu.assert_same_run(both, want, ex.all()[0], where="two runs")
    assert a.sims + b.sims == want.sims


def test_capacity_is_bookkeeping():
    """max_moves below the moves made counts `dropped`, max_children = 2 counts `overflowed` (n_children = 0): plays and states as before."""
    G, S, n_moves, temp_moves, _ = SETTINGS["brandubh7"]
    rules, n, wb, states, salts, want = setting("brandubh7")
    ex = gsu.HostExamples(n, G, 2, S)
    got, faults, _ = gsu.host_run(rules, n, wb, states, S, CPUCT, salts, n_moves, SEED, temp_moves, ex)
    examples, _ = ex.all()
    lens, counters = ex.counts()
    assert lens == [min(m, 2) for m in want.moves] and counters["dropped"] == sum(max(m - 2, 0) for m in want.moves) > 0
    trimmed = gsu.Run(G, n_moves)
    trimmed.plays, trimmed.states, trimmed.moves, trimmed.examples = want.plays, want.states, want.moves, [e[:2] for e in want.examples]
    gsu.assert_same_run(got, trimmed, examples, where="max_moves")
    assert got.stat_faults == 0 and not any(faults)

    ex = gsu.HostExamples(n, G, n_moves, 2)
    got, faults, _ = gsu.host_run(rules, n, wb, states, S, CPUCT, salts, n_moves, SEED, temp_moves, ex)
    examples, overflow = ex.all()
    wide = sum(len(e[2]) > 2 for row in want.examples for e in row)
    assert wide > 0 and ex.counts()[1]["overflowed"] == wide and ex.counts()[1]["dropped"] == 0
    narrow = gsu.Run(G, n_moves)
    narrow.plays, narrow.states, narrow.moves = want.plays, want.states, want.moves
    narrow.examples = [[e if len(e[2]) <= 2 else (e[0], e[1], [], [], e[4], e[5]) for e in row] for row in want.examples]
    gsu.assert_same_run(got, narrow, examples, where="max_children")
    assert [[int(len(e[2]) > 2) for e in row] for row in want.examples] == overflow
    assert got.stat_faults == 0 and not any(faults)


def test_one_simulation_plays_and_records_nothing():
    G, _S, n_moves, temp_moves, _ = SETTINGS["brandubh7"]
    rules, n, wb, states, salts, _ = setting("brandubh7")
    ex = gsu.HostExamples(n, G, n_moves, 4)
    got, faults, rounds = gsu.host_run(rules, n, wb, states, 1, CPUCT, salts, n_moves, SEED, temp_moves, ex)
    live = sum(states[g].status == abi.ONGOING for g in range(G))
    assert got.moves == [0] * G and got.states == [bytes(states[g]) for g in range(G)] and all(p == (0, 0, 0, 0) for row in got.plays for p in row)
    assert ex.counts() == ([0] * G, {"dropped": 0, "overflowed": 0, "bad_index": 0})
    assert got.sims == live and rounds == 1 and not any(faults)


def test_a_game_that_outgrows_its_arena_faults_alone():
    """edges_per_node = 30 is below the legal plays of Brandubh's opening positions (40 at the start) and above those of its endgames:
    the games that outgrow (n_sims + 1) * 30 edges fault once each and stop before the move they were searching; every other game
    equals the run with room for all."""
    G, S, n_moves, temp_moves, _ = SETTINGS["brandubh7"]
    rules, n, wb, states, salts, want = setting("brandubh7")
    ex = gsu.HostExamples(n, G, n_moves, S)
    got, faults, _ = gsu.host_run(rules, n, wb, states, S, CPUCT, salts, n_moves, SEED, temp_moves, ex, edges_per_node=30)
    examples, _ = ex.all()
    bad = [g for g in range(G) if faults[g]]
    good = [g for g in range(G) if not faults[g]]
    assert bad and len(good) > sum(states[g].status != abi.ONGOING for g in range(G)), (bad, good)
    assert got.stat_faults == len(bad)
    gsu.assert_same_run(got, want, examples, games=good, where="fault")
    for g in bad:                                # the moves before the fault stand
        k = got.moves[g]
        assert k < want.moves[g] and [row[g] for row in got.plays[:k]] == [row[g] for row in want.plays[:k]], g
        assert all(row[g] == (0, 0, 0, 0) for row in got.plays[k:]) and examples[g] == want.examples[g][:k], g
