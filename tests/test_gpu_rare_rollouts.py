"""The preset instantiations of the playout kernels (k_rollout, k_random_advance, k_mcts_rollout, k_mcts_tree, k_mcts_fused with literal
masks and folded rule branches) on rare-rule positions, bit for bit against the CPU oracle, next to their run-time twins.

Host-sim compiles the device code with run-time Consts only, and playouts from reachable positions end by ply cap, escape or capture
almost always, so this file is what pins the enclosure filter and flood, the exit-fort edge-line filter, the shieldwall window
pre-filter, king_specials, the no-plays / all-captured outcomes and the 15 -> 13 column restride of the presets on the device.  The
workloads, expectations and comparisons are those of tests/rare_workloads.py, proven on the CPU by test_hostsim_rare_workloads.py.
A preset that fails while its twin passes is a folding error; both failing is the engine's.

What the oracle gives for these inputs (the floors of rare_workloads.py were set against it), won games by reason over both seeds:
  copenhagen11 / copenhagen11_u256 (641 games): escaped 302, exit fort 31, all captured 21, no plays 16, enclosed 14, king captured 8
  copenhagen13 (641): escaped 223, exit fort 38, enclosed 19, all captured 14, no plays 10, king captured 6
  brandubh7 (513): escaped 464, king captured 124, all captured 66, enclosed 39, no plays 20, repetition 1
  koch7_u128 (513): escaped 475, king captured 105, all captured 60, enclosed 39, no plays 20, repetition 1
  tablut9 (641): escaped 916, king captured 77, all captured 31
and for the searches, terminal_hits / playouts ended by exit fort, all captured, enclosed, no plays:
  copenhagen11 (96 games, S = 48): 1 133 / 34, 19, 9, 2      copenhagen13 (64, S = 32): 458 / 12, 10, 3, 0
  brandubh7 (71 of 72, S = 48): 1 368 / 0, 146, 9, 3         tablut9 (96): 704 / 0, 67, 0, 0      koch7_u128 (71 of 72): 1 333 / 0, 134, 9, 3
Wall time on one MI355X, oracle included: the whole file 4.1 s; rollouts 1.9 s for the first configuration (it opens the device), 0.03 to
0.16 s for the others; in-place playouts at most 0.03 s; shieldwall hint 0.10 s (11x11) and 0.28 s (13x13); searches 0.05 to 0.23 s."""
import pytest

from tests import rare_workloads as rw

pytestmark = pytest.mark.gpu

ALL = rw.PRESETS + rw.TWINS
_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        cfg = rw.CONFIGS[name]
        _ENGINES[name] = rw.GpuEngine(cfg.rules, cfg.n, cfg.wb)
    return _ENGINES[name]


@pytest.mark.parametrize("name", ALL)
def test_rollouts_from_crafted_positions(name):
    rw.check_rollout_coverage(name)
    rw.compare_rollouts(_engine(name), name)


@pytest.mark.parametrize("name", ALL)
def test_in_place_playouts_from_crafted_positions(name):
    rw.compare_advance(_engine(name), name)


@pytest.mark.parametrize("n,wb", [(11, 128), (13, 256)])
def test_shieldwall_hint_many_seeds(n, wb):
    rw.compare_hint(rw.GpuEngine, n, wb)


@pytest.mark.parametrize("name", ALL)
def test_mcts_from_crafted_positions(name):
    stats = rw.check_mcts_coverage(name)
    assert stats.faults == 0, name
    rw.compare_mcts(_engine(name), name)
