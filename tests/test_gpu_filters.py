"""The playout ply's exact pre-filters on the device (far-tile filter of the king capture, the two-stage exit-fort candidate test, the
enclosure filter): tafl_rollout and a short tafl_mcts_run on 512 / 128 games drawn from the inputs of tests/filters_util.py
(crafted rare-rule positions, ringed kings, kings on every edge between flanking defenders, the start position), game by game against the
CPU oracle - the Copenhagen 11x11 and Brandubh 7x7 preset kernels and one run-time-rules instantiation (Copenhagen with a weak king, under
which the far-tile filter is in force and king captures are frequent).  Playout caps 64 and 512; searches of 16 simulations, the default
pipeline and the one-slot, one-partition route both against the oracle, hence equal.

What the oracle gives (won playouts by reason, cap 64 / cap 512; searches: terminal hits and playouts ended by king capture, exit fort,
enclosure); the floors below are half of the cap-64 figures, rounded up:
  copenhagen11:  king captured 2 / 4, exit fort 33 / 34, enclosed 8 / 8;   265 terminal hits; 11, 31, 7
  brandubh7:     king captured 49 / 78, enclosed 24 / 24;                  429; 201, -, 12
  weak_armed11:  king captured 20 / 73, exit fort 33 / 34, enclosed 8 / 8; 327; 77, 31, 7
(a strong Copenhagen king falls to four attackers only: the far-tile filter is pinned there by the adjacencies, of which every playout
has many, and under the weak king by the captures as well)"""
import functools

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams
from oracle import oracle as orc
from tests import parity_util as pu
from tests import rare_workloads as rw
from tests import filters_util as hf

pytestmark = pytest.mark.gpu

NAMES = ("copenhagen11", "brandubh7", "weak_armed11")      # preset 4 x 11, preset 2 x 7, run-time rules on 4 x 11
G_ROLLOUT, G_MCTS = 512, 128
SEED, BASE, SIMS, MCTS_CAP, CPUCT, WIDTH = 2, 100, 16, 64, 1.0, 256
CAPS = (64, 512)
FLOORS = {"copenhagen11": {abi.KING_CAPTURED: 1, abi.EXIT_FORT: 17, abi.ENCLOSED: 4},
          "brandubh7": {abi.KING_CAPTURED: 25, abi.ENCLOSED: 12},
          "weak_armed11": {abi.KING_CAPTURED: 10, abi.EXIT_FORT: 17, abi.ENCLOSED: 4}}
_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        cfg = hf.CONFIGS[name]
        _ENGINES[name] = rw.GpuEngine(cfg.rules, cfg.n, cfg.wb)
    return _ENGINES[name]


@functools.lru_cache(maxsize=None)
def _games(name, count):
    """`count` games of the inputs of the host test whose side to move has a legal play: the same number from every kind, spread evenly
    over the kind, the remainder from the ringed kings."""
    cfg = hf.CONFIGS[name]
    states, G, _, spans = hf.workload(name)
    counts, _ = orc.batch_movegen(orc.GameLogic(cfg.rules, cfg.n), states, G, cfg.wb, want_masks=False)
    share, picked = count // len(spans), []
    for kind, (first, end) in spans.items():
        live = [g for g in range(first, end) if counts[g] > 0]
        k = share + (count - share * len(spans) if kind == "king" else 0)
        picked += [live[(i * (len(live) - 1)) // (k - 1)] for i in range(k)]
    assert len(picked) == count and len(set(picked)) >= count - 64, (name, len(picked), len(set(picked)))      # (the start position repeats)
    return pu.states_array([states[g] for g in picked]), count


@functools.lru_cache(maxsize=None)
def _rollout_want(name, cap):
    cfg = hf.CONFIGS[name]
    states, G = _games(name, G_ROLLOUT)
    return rw._oracle_rollouts(cfg, orc.GameLogic(cfg.rules, cfg.n), states, G, (SEED,), cap, BASE)


@functools.lru_cache(maxsize=None)
def _mcts_want(name):
    cfg = hf.CONFIGS[name]
    states, G = _games(name, G_MCTS)
    return rw.oracle_mcts(orc.GameLogic(cfg.rules, cfg.n), states, G, cfg.wb, TaflMctsParams(SIMS, MCTS_CAP, CPUCT, SEED, 0, 0), BASE, WIDTH)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", NAMES)
def test_rollouts_equal_the_oracle(name, cap):
    cfg = hf.CONFIGS[name]
    states, G = _games(name, G_ROLLOUT)
    want = _rollout_want(name, cap)
    hist = rw.win_reason_hist(want)
    print(name, cap, {abi.WIN_REASON_NAMES[k]: v for k, v in hist.items()})
    for reason, floor in FLOORS[name].items():
        assert hist[reason] >= floor, (name, cap, abi.WIN_REASON_NAMES[reason], hist[reason], floor)
    rw._compare_rollouts(_engine(name), cfg, states, G, want, cap, BASE, f"{name} rollout, cap {cap}")


@pytest.mark.parametrize("name", NAMES)
def test_searches_equal_the_oracle_on_both_routes(name):
    cfg = hf.CONFIGS[name]
    states, G = _games(name, G_MCTS)
    ok, on, ostats = _mcts_want(name)
    print(name, "terminal hits", ostats.terminal_hits)
    assert ostats.faults == 0 and ostats.terminal_hits >= 100, (name, ostats.faults, ostats.terminal_hits)
    orec, ocnt = pu.children_view(ok, on, G, WIDTH)
    for label, flags in (("default", 0), ("one slot, one partition", abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 1, 1))):
        tag = f"{name} mcts ({label})"
        gk, gn, gstats, after = _engine(name).mcts(states, G, TaflMctsParams(SIMS, MCTS_CAP, CPUCT, SEED, 0, flags), BASE, WIDTH)
        grec, gcnt = pu.children_view(gk, gn, G, WIDTH)
        g = pu.first_children_diff(orec, ocnt, grec, gcnt)
        assert g < 0, f"{tag}: root children of game {g}\n{pu.describe_state(states[g], cfg.wb)}\noracle {pu.children_of(orec, ocnt, g)}\n" \
                      f"engine {pu.children_of(grec, gcnt, g)}"
        for f in rw.STAT_FIELDS:
            assert getattr(ostats, f) == getattr(gstats, f), (tag, f, getattr(ostats, f), getattr(gstats, f))
        assert list(ostats.reason_hist) == list(gstats.reason_hist), (tag, list(ostats.reason_hist), list(gstats.reason_hist))
        assert pu.states_equal(states, after, G), f"{tag}: a search must not modify the batch"
