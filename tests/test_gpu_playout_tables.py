"""The playout kernels with their bit_at table in LDS (tafl_tables.hpp; k_rollout, k_mcts_rollout and, on 7x7, k_mcts_fused) against the CPU
oracle, on playouts that are PROVEN, on the oracle alone, to move from and to every tile of the board and to capture with the
destination in the highest limb that holds tiles: every row of the table is read, in both layouts.

Per configuration 512 games from the start position, game i advanced by i mod 64 seeded random plies, playouts capped at 128 plies;
value, status, reason, winner and plies of every game must equal the oracle's.  The three presets read the table (Copenhagen 13x13
works in the dense six-limb layout, which keeps the computed code); koch7_u128 is the run-time-rules kernel, computed as before.
Coverage (tests/tables_util.py, seeds recorded there): a corner is never an origin - only the king may stand on one and the game ends
when he does - every other tile is, and every tile, corners included, is a destination."""
import ctypes as C

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflState
from oracle import oracle as orc
from tests import parity_util as pu
from tests import rare_workloads as rw
from tests import tables_util as tu

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        cfg = rw.CONFIGS[name]
        _ENGINES[name] = rw.GpuEngine(cfg.rules, cfg.n, cfg.wb)
    return _ENGINES[name]


@pytest.mark.parametrize("name", list(tu.SEEDS))
def test_oracle_playouts_meet_the_coverage_condition(name):
    never_from, never_to, capture_in_top_limb = tu.coverage(name)
    assert never_from == [] and never_to == [] and capture_in_top_limb, (name, never_from, never_to, capture_in_top_limb)


@pytest.mark.parametrize("name", list(tu.SEEDS))
def test_rollouts_equal_the_oracle(name):
    states, want = tu.workload(name)
    got, after = _engine(name).rollout(pu.clone_states(states, tu.G), tu.G, tu.SEEDS[name][1], tu.SIM, tu.CAP, tu.BASE)
    assert pu.states_equal(after, states, tu.G)                       # a rollout leaves the batch as it was
    bad = [(g, rw.result_tuple(got[g]), want[g]) for g in range(tu.G) if rw.result_tuple(got[g]) != want[g]]
    assert not bad, (name, len(bad), bad[:4])
    assert max(w[4] for w in want) == tu.CAP and min(w[4] for w in want) < tu.CAP      # capped and decided playouts both occur


def test_mcts_pipelines_agree_and_equal_the_oracle():
    """256 games on 11x11, S = 16, cap 64: the default pipeline and one playout slot per game give the same root children and the same
    number of playout plies; four games equal the oracle's search."""
    name, G, S, cap, seed = "copenhagen11", 256, 16, 64, 29
    cfg = rw.CONFIGS[name]
    states = pu.clone_states(tu.workload(name)[0], G)
    runs = []
    for flags in (0, abi.mcts_tune(0, 1)):
        kids, cnt, stats, _ = _engine(name).mcts(pu.clone_states(states, G), G, TaflMctsParams(S, cap, 1.0, seed, 0, flags), tu.BASE, 64)
        runs.append((pu.children_view(kids, cnt, G, 64), stats))
    (rec_a, cnt_a), st_a = runs[0]
    (rec_b, cnt_b), st_b = runs[1]
    assert pu.first_children_diff(rec_a, cnt_a, rec_b, cnt_b) == -1
    assert st_a.rollout_plies == st_b.rollout_plies and st_a.rollout_plies > 0
    assert st_a.faults == 0 and st_b.faults == 0
    spots = (0, 63, 64, 255)
    lg = orc.GameLogic(cfg.rules, cfg.n)
    want = pu.oracle_children_parallel(orc, lg, cfg.wb, TaflMctsParams(S, cap, 1.0, seed, 0, 0), [(g, states[g], tu.BASE + g) for g in spots], 64)
    for g in spots:
        assert pu.children_of(rec_a, cnt_a, g) == want[g], g
        assert pu.children_of(rec_b, cnt_b, g) == want[g], g
