"""The C-ABI and Python surface of playout cap randomization (include/taflhip.h tafl_playout_cap): struct sizes, exports, the class rule
of mcts.playout_cap_is_full against the RNG words restated in tests/examples_util.py, the defaults.  No GPU."""
import ctypes as C

from alphazeroforhnefatafl_amd import abi
from tests import examples_util as eu

KEY = 0x504C41594F555443


def test_struct_sizes_and_layout():
    assert C.sizeof(abi.TaflPlayoutCap) == 32 == abi.EXPECTED_SIZES["tafl_playout_cap"]
    assert C.sizeof(abi.TaflPlayoutCapStats) == 32 == abi.EXPECTED_SIZES["tafl_playout_cap_stats"]
    T = abi.TaflPlayoutCap
    assert (T.seed.offset, T.fast_sims.offset, T.full_per_65536.offset, T.flags.offset, T._reserved.offset) == (0, 8, 12, 16, 20)
    assert (abi.TaflPlayoutCapStats.full_moves.offset, abi.TaflPlayoutCapStats.fast_moves.offset) == (0, 8)


def test_the_two_symbols_are_exported_and_the_abi_version_stays():
    from alphazeroforhnefatafl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("tafl_gselfplay_set_playout_cap", "tafl_gselfplay_playout_cap_stats"):
        assert hasattr(L, name), name
        assert name in {s for s, _, _ in _lib.SYMBOLS}
    assert abi.ABI_VERSION == 1 and L.tafl_abi_version() == 1


def test_playout_cap_is_full_agrees_with_the_restated_words():
    from alphazeroforhnefatafl_amd.mcts import playout_cap_is_full
    seeds = (0, 1, 3, 0xD1CE, 2 ** 32 + 5, 2 ** 64 - 1)
    gids = (0, 1, 71, 1000, 1072, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40 + 3, 2 ** 63 + 11, 2 ** 64 - 1)
    moves = (0, 1, 2, 3, 4, 19, 255, 2 ** 31, 2 ** 32 - 1)
    seen = set()
    for seed in seeds:
        for gid in gids:
            for M in moves:
                w = eu.ply_rand(eu.sim_key(eu.game_key(seed, gid) ^ KEY, M), 0)
                for per in (0, 1, 16384, 32768, 65535, 65536):
                    want = (w >> 16) < per
                    assert playout_cap_is_full(seed, gid, M, per) == want, (seed, gid, M, per)
                    seen.add(want)
                assert not playout_cap_is_full(seed, gid, M, 0) and playout_cap_is_full(seed, gid, M, 65536)
    assert seen == {True, False}
    # ids that differ only above 2^32 are different games
    assert len({eu.ply_rand(eu.sim_key(eu.game_key(3, gid) ^ KEY, 0), 0) for gid in (7, 2 ** 32 + 7, 2 ** 33 + 7)}) == 3
    # about a quarter of the moves are full at 16384 (a binomial of 4096 draws: 1024 +- 5 sigma)
    full = sum(playout_cap_is_full(3, gid, M, 16384) for gid in range(256) for M in range(16))
    assert abs(full - 1024) < 5 * 27.8, full


def test_the_class_stream_differs_from_the_sample_stream_for_equal_seeds():
    same = sum(eu.ply_rand(eu.sim_key(eu.game_key(5, gid) ^ KEY, M), 0) == eu.sample_word(5, gid, M) for gid in range(64) for M in range(8))
    assert same == 0


def test_the_harness_computes_the_same_class():
    """cap_is_full of tafl_guided.hpp, compiled for the host."""
    from tests import playout_cap_util as pcu
    L = pcu.hlib()
    for seed in (0, 3, 2 ** 64 - 1):
        for gid in (0, 1000, 2 ** 32 + 7, 2 ** 63 + 11):
            for M in (0, 3, 19, 2 ** 32 - 1):
                for per in (0, 16384, 65536):
                    assert bool(L.hsc_is_full(seed, per, gid, M)) == pcu.is_full(seed, gid, M, per), (seed, gid, M, per)


def test_defaults_leave_the_cap_off():
    from alphazeroforhnefatafl_amd import MCTSArgs
    from alphazeroforhnefatafl_amd.engine import full_per_65536
    a = MCTSArgs()
    assert (a.fastSims, a.fullMoveProb, a.capSeed) == (0, 1.0, 0)
    assert full_per_65536(0.25) == 16384 and full_per_65536(1.0) == 65536 and full_per_65536(0.0) == 0


def test_play_match_refuses_a_cap_before_it_touches_the_batch():
    import pytest
    from alphazeroforhnefatafl_amd import MCTSArgs
    from alphazeroforhnefatafl_amd.selfplay import play_match
    with pytest.raises(ValueError):
        play_match(None, (None, None), MCTSArgs(numMCTSSims=16, fastSims=4, fullMoveProb=0.25), 4)
