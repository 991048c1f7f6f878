"""The C-ABI and Python surface of exact win/loss proofs in guided self-play (include/taflhip.h tafl_solver): struct sizes, exports,
defaults, and null arguments (the library's own refusals on a GPU in tests/test_gpu_solver.py).  No GPU."""
import ctypes as C

import pytest

from alphazeroforhnefatafl_amd import abi


def test_struct_sizes_and_layout():
    assert C.sizeof(abi.TaflSolver) == 32 == abi.EXPECTED_SIZES["tafl_solver"]
    assert C.sizeof(abi.TaflSolverStats) == 64 == abi.EXPECTED_SIZES["tafl_solver_stats"]
    T, U = abi.TaflSolver, abi.TaflSolverStats
    assert (T.flags.offset, T._reserved.offset) == (0, 4)
    names = ("root_won", "root_lost", "skipped_sims", "nodes_won", "nodes_lost", "pruned_visits", "pruned_children", "moves")
    assert [getattr(U, name).offset for name in names] == [8 * i for i in range(8)]


def test_the_two_symbols_are_exported_and_the_abi_version_stays():
    from alphazeroforhnefatafl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("tafl_gselfplay_set_solver", "tafl_gselfplay_solver_stats"):
        assert hasattr(L, name), name
        assert name in {s for s, _, _ in _lib.SYMBOLS}
    assert abi.ABI_VERSION == 1 and L.tafl_abi_version() == 1


def test_null_arguments_are_refused():
    from alphazeroforhnefatafl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.tafl_gselfplay_set_solver.argtypes = [C.c_void_p, C.POINTER(abi.TaflSolver)]
    L.tafl_gselfplay_solver_stats.argtypes = [C.c_void_p, C.POINTER(abi.TaflSolverStats)]
    cfg, st = abi.TaflSolver(0), abi.TaflSolverStats()
    assert L.tafl_gselfplay_set_solver(None, C.byref(cfg)) == -1 and L.tafl_gselfplay_set_solver(None, None) == -1
    assert L.tafl_gselfplay_solver_stats(None, C.byref(st)) == -1 and L.tafl_gselfplay_solver_stats(None, None) == -1


def test_the_python_defaults_leave_it_off():
    from alphazeroforhnefatafl_amd.mcts import MCTSArgs
    assert MCTSArgs().solver is False


def test_play_match_refuses_the_setting():
    from alphazeroforhnefatafl_amd.mcts import MCTSArgs
    from alphazeroforhnefatafl_amd.selfplay import play_match
    with pytest.raises(ValueError):
        play_match(None, (None, None), MCTSArgs(solver=True), 4)
