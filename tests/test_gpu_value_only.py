"""The value-only playout on the device: k_rollout and the playout kernels of both search pipelines run the fast playout with the
repetition tracker on packed records beside the state (tafl_core.hpp: ValueOnly).  The inputs are those of
tests/test_hostsim_value_only.py (tests/value_only_util.py: shuffles cut at every ply, with crafted trackers, put together so that the
oracle ends at least 32 playouts per ruleset by repetition), as batches of 641, 65 and 1 games - a partial last wave, a lone lane -
through tafl_rollout with cap 80 on the 11x11 and 7x7 presets and a run-time twin (Tablut 9x9, where repetition draws), and as one search
of S = 16 over 513 games per pipeline; everything is compared with the CPU oracle."""
import pytest

from tests import parity_util as pu
from tests import rare_workloads as rw
from tests import value_only_util as vu

pytestmark = pytest.mark.gpu

NAMES = ("copenhagen11", "brandubh7", "tablut9")
_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        cfg = vu.CONFIGS[name]
        _ENGINES[name] = rw.GpuEngine(cfg.rules, cfg.n, cfg.wb)
    return _ENGINES[name]


@pytest.mark.parametrize("name", NAMES)
def test_rollouts_from_crafted_trackers(name):
    cfg = vu.CONFIGS[name]
    got = vu.repetition_endings(name, vu.GPU_CAP)
    assert got >= vu.FLOOR, (name, got)
    for count, (states, G, want) in vu.expectations(name, vu.GPU_CAP).items():
        rw._compare_rollouts(_engine(name), cfg, states, G, want, vu.GPU_CAP, vu.BASE, f"{name} rollout of {count}")


@pytest.mark.parametrize("name", NAMES)
def test_search_from_crafted_trackers(name):
    cfg = vu.CONFIGS[name]
    engine = _engine(name)
    states, (ok, on, ostats) = vu.mcts_expectation(name)
    G, width = vu.MCTS_G, rw.MCTS_WIDTH
    orec, ocnt = pu.children_view(ok, on, G, width)
    for label, flags in engine.pipelines:
        tag = f"gpu {name} mcts ({label})"
        gk, gn, gstats, after = engine.mcts(states, G, vu.mcts_params(flags), rw.MCTS_BASE, width)
        grec, gcnt = pu.children_view(gk, gn, G, width)
        g = pu.first_children_diff(orec, ocnt, grec, gcnt)
        assert g < 0, f"{tag}: root children of game {g}\n{pu.describe_state(states[g], cfg.wb)}\n" \
                      f"oracle {pu.children_of(orec, ocnt, g)}\nengine {pu.children_of(grec, gcnt, g)}"
        for f in rw.STAT_FIELDS:
            assert getattr(ostats, f) == getattr(gstats, f), (tag, f, getattr(ostats, f), getattr(gstats, f))
        assert list(ostats.reason_hist) == list(gstats.reason_hist), (tag, list(ostats.reason_hist), list(gstats.reason_hist))
        assert pu.states_equal(states, after, G), f"{tag}: a search must not modify the batch"
