"""The C-ABI and Python surface of the random board symmetry per leaf evaluation (include/taflhip.h tafl_eval_symmetry): struct size,
declarations, exports, the MCTSArgs plumbing and null arguments (the library's own refusals on a GPU in tests/test_gpu_eval_symmetry.py).
No GPU."""
import ctypes as C
import os

import pytest

from alphazeroforhnefatafl_amd import abi

SYMBOLS = ("tafl_gmcts_set_eval_symmetry", "tafl_gmcts_leaf_symmetry")


def test_struct_size_and_layout():
    T = abi.TaflEvalSymmetry
    assert C.sizeof(T) == 32 == abi.EXPECTED_SIZES["tafl_eval_symmetry"]
    assert (T.seed.offset, T.game_id_base.offset, T.flags.offset, T._reserved.offset) == (0, 8, 16, 20)


def test_the_symbols_are_declared_exported_and_the_abi_version_stays():
    from alphazeroforhnefatafl_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "taflhip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert f"int {name}(tafl_batch* b" in header, name
        assert hasattr(L, name), name
        assert name in {s for s, _, _ in _lib.SYMBOLS}
    assert "} tafl_eval_symmetry;" in header and "0x53594D4D45545259" in header
    assert abi.ABI_VERSION == 1 and L.tafl_abi_version() == 1


def test_null_arguments_are_refused():
    from alphazeroforhnefatafl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.tafl_gmcts_set_eval_symmetry.argtypes = [C.c_void_p, C.POINTER(abi.TaflEvalSymmetry)]
    L.tafl_gmcts_leaf_symmetry.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    cfg, out = abi.TaflEvalSymmetry(1, 0, 0), (C.c_uint8 * 4)()
    assert L.tafl_gmcts_set_eval_symmetry(None, C.byref(cfg)) == -1 and L.tafl_gmcts_set_eval_symmetry(None, None) == -1
    assert L.tafl_gmcts_leaf_symmetry(None, C.cast(out, C.c_void_p), 0) == -1


class _Recorder:
    """Stands in for a GameBatch: records the eval-symmetry calls."""

    def __init__(self):
        self.calls = []

    def set_eval_symmetry(self, seed, game_id_base=0):
        self.calls.append(("set", seed, game_id_base))

    def clear_eval_symmetry(self):
        self.calls.append(("clear",))


def test_the_args_plumbing():
    import alphazeroforhnefatafl_amd as pkg
    from alphazeroforhnefatafl_amd.engine import GameBatch
    from alphazeroforhnefatafl_amd.mcts import MCTSArgs, apply_eval_symmetry
    assert MCTSArgs().evalSymmetry is False and MCTSArgs().symmetrySeed == 0
    assert pkg.apply_eval_symmetry is apply_eval_symmetry and "apply_eval_symmetry" in pkg.__all__
    for name in ("set_eval_symmetry", "clear_eval_symmetry", "gmcts_leaf_symmetry"):
        assert callable(getattr(GameBatch, name)), name
    r = _Recorder()
    apply_eval_symmetry(r, MCTSArgs())
    apply_eval_symmetry(r, MCTSArgs(evalSymmetry=True, symmetrySeed=77, game_id_base=5))
    assert r.calls == [("clear",), ("set", 77, 5)]


def test_play_match_refuses_the_setting():
    from alphazeroforhnefatafl_amd.mcts import MCTSArgs
    from alphazeroforhnefatafl_amd.selfplay import play_match
    with pytest.raises(ValueError):
        play_match(None, (None, None), MCTSArgs(evalSymmetry=True), 4)
