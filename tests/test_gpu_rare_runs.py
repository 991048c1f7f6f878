"""The code that makes a move and goes on, on rare-rule positions, on the device: the preset instantiations of k_mcts_tree_selfplay and
k_mcts_tree_selfplay_rec (Ops::selfplay_advance_impl with literal-folded constants, on 13x13 between the two restrides 8x15 <-> 6x13),
k_examples_finalize and the gather for games that a recording run itself ended, k_gmcts_step / k_gselfplay_step / k_gmcts_leaves
(Guided::step's term, Guided::selfplay_step's stop on the child's status), and k_mcts_advance / k_gmcts_advance onto children that are
terminal by a rare rule - each bit for bit against the CPU oracle, on the three presets and their run-time twins.

Host-sim compiles the run-time form only and has no advance entry point, and from reachable positions a Copenhagen game never ends by
enclosure, exit fort, no plays or all captured; the workloads (the crafted mix of check d), expectations, comparisons and coverage floors
are those of tests/rare_workloads.py (checks e .. i), proven on the CPU by tests/test_hostsim_rare_workloads.py.  A preset that fails while
its twin passes is a folding error (or the restride, the LDS frames, the dispatcher); both failing is the engine's.

What the oracle gives for these inputs (games ended inside the run by win reason; "later": ended after two moves or more):
  self-play / recording with temp_moves 0 (S = 48, 4 moves; 13x13: S = 32, 3 moves; cap 80, seed 2, base 7):
    copenhagen11 / copenhagen11_u256 (96 games): enclosed 10, all captured 7, exit fort 7, no plays 4, king captured 3, escaped 3; later 7
    copenhagen13 (64): exit fort 7, enclosed 4, all captured 4, escaped 2, king captured 1, no plays 1; later 3
    brandubh7 (71 of 72): king captured 12, all captured 10, enclosed 8, no plays 7, escaped 4; later 10
    tablut9 (96): all captured 13, escaped 10, king captured 7; later 12      koch7_u128 (71): king captured 11, enclosed 9, all captured 9,
    no plays 7, escaped 3; later 8
  recording with temp_moves = n_moves, sample seed 11 (non-argmax picks 155 of 305, 90 of 162, 75 of 196 game-moves):
    copenhagen11: enclosed 10, exit fort 8, all captured 7, escaped 2, no plays 1, king captured 1; later 5
    copenhagen13: exit fort 6, enclosed 4, all captured 3, escaped 2, king captured 1, no plays 1; later 3
    brandubh7: king captured 12, enclosed 8, all captured 7, no plays 6, escaped 2; later 10
  guided search (S = 32, 24 on 13x13; c_puct 1.25), sims / predicts / terminal hits: copenhagen11 3 072 / 2 505 / 567, copenhagen13
    1 536 / 1 230 / 306, brandubh7 2 272 / 1 675 / 597, tablut9 3 072 / 2 680 / 392, koch7_u128 2 272 / 1 677 / 595
  guided self-play (3 moves, 4 on 7x7; temp_moves 2): copenhagen11 enclosed 8, exit fort 7, escaped 4, no plays 2, king captured 1, all
    captured 1; copenhagen13 exit fort 7, all captured 4, enclosed 3, no plays 1, escaped 1; brandubh7 enclosed 9, escaped 6, all captured 6,
    no plays 4, king captured 1
  advance: first-maximum children terminal by a rare rule 25 / 15 / 22 after the playout search (two multi-captures on 11x11, one of four
    pieces) and 19 / 15 / 15 after the guided search; search, advance and keep-search run under the default tuning (the fused kernel on
    64-bit boards) and under mcts_tune(TWO_KERNEL, slots=1), and the kept children must be the same

Wall time on one MI355X, the oracle's runs included (they are computed once per process and shared), in the order copenhagen11,
copenhagen13, brandubh7, copenhagen11_u256, tablut9, koch7_u128; the whole file 21 s:
  self-play run       2.34 (it opens the device), 0.36, 0.29, 0.74, 0.32, 0.21 s
  recording run       0.71, 0.38, 0.23, 0.80, 0.48, 0.28 s
  guided search       0.94, 0.65, 0.32, 0.69, 0.69, 0.21 s
  guided self-play    1.57, 1.26, 0.49, 1.30, 0.99, 0.35 s
  advance             0.76, 0.53, 0.33, 0.82, 0.60, 0.35 s"""
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


@pytest.mark.parametrize("name", ALL)
def test_advance_onto_rare_terminal_children(name):
    rw.check_mcts_coverage(name)
    rw.compare_advance_onto_children(_engine(name), name)
