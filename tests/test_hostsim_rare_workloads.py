"""The rare-rule workloads of tests/rare_workloads.py against host-sim (the device code compiled for the host, run-time Consts): proves
the workloads, the oracle's expectations and the comparison code before they meet the device, and holds the coverage conditions on the
oracle's results alone.  Host-sim never compiles the preset instantiations; tests/test_gpu_rare_rollouts.py runs the same code against
the library.  CPU only."""
import pytest

from alphazeroforhnefatafl_amd import abi
from tests import rare_workloads as rw

ALL = rw.PRESETS + rw.TWINS


def _engine(name):
    cfg = rw.CONFIGS[name]
    return rw.HostSimEngine(cfg.rules, cfg.n, cfg.wb)


@pytest.mark.parametrize("name", rw.PRESETS)
def test_the_floors_are_at_least_half_of_what_the_oracle_gives(name):
    """A floor that the workload clears many times over would let most of the coverage erode unnoticed."""
    hist = rw.check_rollout_coverage(name)
    for reason, floor in rw.ROLLOUT_FLOORS[name].items():
        assert 2 * floor >= hist[reason], (name, abi.WIN_REASON_NAMES[reason], hist[reason], floor)
    w = rw.rollout_workload(name)
    assert w.G % 64 == 1 and w.G > 64 * 4


@pytest.mark.parametrize("name", ALL)
def test_rollouts_from_crafted_positions(name):
    rw.check_rollout_coverage(name)
    rw.compare_rollouts(_engine(name), name)


@pytest.mark.parametrize("name", ALL)
def test_in_place_playouts_from_crafted_positions(name):
    rw.compare_advance(_engine(name), name)


@pytest.mark.parametrize("n,wb", [(11, 128), (13, 256)])
def test_shieldwall_hint_many_seeds(n, wb):
    rw.compare_hint(rw.HostSimEngine, n, wb)


@pytest.mark.parametrize("name", ALL)
def test_mcts_from_crafted_positions(name):
    stats = rw.check_mcts_coverage(name)
    assert stats.faults == 0, name
    rw.compare_mcts(_engine(name), name)
