"""The C-ABI and Python surface of forced playouts with policy target pruning (include/taflhip.h tafl_forced_playouts): struct sizes,
exports, defaults, and what the setting refuses (the check restated beside the host harness; the library's own on a GPU in
tests/test_gpu_forced_playouts.py).  No GPU."""
import ctypes as C

import pytest

from alphazeroforhnefatafl_amd import abi


def test_struct_sizes_and_layout():
    assert C.sizeof(abi.TaflForcedPlayouts) == 32 == abi.EXPECTED_SIZES["tafl_forced_playouts"]
    assert C.sizeof(abi.TaflForcedPlayoutsStats) == 32 == abi.EXPECTED_SIZES["tafl_forced_playouts_stats"]
    T, U = abi.TaflForcedPlayouts, abi.TaflForcedPlayoutsStats
    assert (T.k.offset, T.flags.offset, T._reserved.offset) == (0, 8, 12)
    assert (U.forced_sims.offset, U.pruned_visits.offset, U.pruned_children.offset, U.full_moves.offset) == (0, 8, 16, 24)


def test_the_two_symbols_are_exported_and_the_abi_version_stays():
    from alphazeroforhnefatafl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("tafl_gselfplay_set_forced_playouts", "tafl_gselfplay_forced_playouts_stats"):
        assert hasattr(L, name), name
        assert name in {s for s, _, _ in _lib.SYMBOLS}
    assert abi.ABI_VERSION == 1 and L.tafl_abi_version() == 1


def test_a_null_batch_is_refused():
    from alphazeroforhnefatafl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.tafl_gselfplay_set_forced_playouts.argtypes = [C.c_void_p, C.POINTER(abi.TaflForcedPlayouts)]
    L.tafl_gselfplay_forced_playouts_stats.argtypes = [C.c_void_p, C.POINTER(abi.TaflForcedPlayoutsStats)]
    cfg, st = abi.TaflForcedPlayouts(2.0, 0), abi.TaflForcedPlayoutsStats()
    assert L.tafl_gselfplay_set_forced_playouts(None, C.byref(cfg)) == -1
    assert L.tafl_gselfplay_forced_playouts_stats(None, C.byref(st)) == -1


@pytest.mark.parametrize("k", [0.0, -2.0, float("nan"), float("inf"), -float("inf"), 64.0000001, 1e300])
def test_a_k_outside_its_range_is_an_invalid_argument(k):
    from tests import forced_util as fu
    assert fu.hlib().hsf_forced_check(C.byref(abi.TaflForcedPlayouts(k, 0))) == -1


def test_flags_and_reserved_words_are_unsupported_and_the_range_is_closed_at_64():
    from tests import forced_util as fu
    L = fu.hlib()
    assert L.hsf_forced_check(C.byref(abi.TaflForcedPlayouts(64.0, 0))) == 0 and L.hsf_forced_check(C.byref(abi.TaflForcedPlayouts(2.0 ** -40, 0))) == 0
    assert L.hsf_forced_check(C.byref(abi.TaflForcedPlayouts(2.0, 1))) == -5
    for i in range(5):
        cfg = abi.TaflForcedPlayouts(2.0, 0)
        cfg._reserved[i] = 1
        assert L.hsf_forced_check(C.byref(cfg)) == -5


def test_the_python_defaults_leave_it_off():
    from alphazeroforhnefatafl_amd.mcts import MCTSArgs
    assert MCTSArgs().forcedPlayoutsK == 0.0


def test_play_match_refuses_the_setting():
    from alphazeroforhnefatafl_amd.mcts import MCTSArgs
    from alphazeroforhnefatafl_amd.selfplay import play_match
    with pytest.raises(ValueError):
        play_match(None, (None, None), MCTSArgs(forcedPlayoutsK=2.0), 4)
