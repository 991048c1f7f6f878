"""The rare-rule workloads of tests/rare_workloads.py against host-sim (the device code compiled for the host, run-time Consts): proves
the workloads, the oracle's expectations and the comparison code before they meet the device, and holds the coverage conditions on the
oracle's results alone.  Host-sim never compiles the preset instantiations; tests/test_gpu_rare_rollouts.py and
tests/test_gpu_rare_runs.py run the same code against the library.  CPU only."""
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


# ---- checks e .. h: the runs (self-play, recording, guided search, guided self-play) from the crafted mix ------------------------------

@pytest.mark.parametrize("name", ALL)
def test_the_run_floors_are_at_least_half_of_what_the_oracle_gives(name):
    for temp_moves, floors in ((0, rw.RUN_FLOORS[name]), (rw.run_moves(name), rw.RUN_FLOORS_SAMPLED[name])):
        hist, later = rw.check_run_coverage(name, temp_moves)
        for key, floor in floors.items():
            assert 2 * floor >= (later if key == "later" else hist[key]), (name, temp_moves, key, floor)
    hist, later = rw.check_gselfplay_coverage(name)
    for key, floor in rw.GSELFPLAY_FLOORS[name].items():
        assert 2 * floor >= (later if key == "later" else hist[key]), (name, "guided", key, floor)
    assert 2 * rw.GUIDED_HIT_FLOORS[name] >= rw.check_guided_coverage(name)[2]
    for kind, want in (("mcts", rw.advance_expectation_mcts(name)), ("guided", rw.advance_expectation_guided(name))):
        rare, multi = rw.check_advance_coverage(name, kind, want)
        assert 2 * rw.ADVANCE_FLOORS[name][kind][0] >= rare and 2 * rw.ADVANCE_FLOORS[name][kind][1] >= multi, (name, kind, rare, multi)


@pytest.mark.parametrize("name", ALL)
def test_selfplay_run_from_crafted_positions(name):
    rw.check_run_coverage(name, 0)
    rw.compare_selfplay(_engine(name), name)


@pytest.mark.parametrize("name", ALL)
def test_recording_run_from_crafted_positions(name):
    rw.check_run_coverage(name, 0)
    rw.check_run_coverage(name, rw.run_moves(name))
    rw.compare_record(_engine(name), name)


@pytest.mark.parametrize("name", ALL)
def test_guided_search_from_crafted_positions(name):
    rw.check_guided_coverage(name)
    rw.compare_guided(_engine(name), name)


@pytest.mark.parametrize("name", ALL)
def test_guided_selfplay_from_crafted_positions(name):
    rw.check_gselfplay_coverage(name)
    rw.compare_gselfplay(_engine(name), name)
