"""Calls that arrive while an asynchronous search is in flight (tafl_mcts_run_async without tafl_mcts_wait): every writer of the batch
states and tafl_mcts_reserve must join the search by itself, so that the order {run_async; call} gives what {run; call} gives.
Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflState
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

SIMS, CAP, SEED, CPUCT, WIDTH = 40, 160, 4, 1.0, 128
STAT_FIELDS = ("sims", "rollouts", "rollout_plies", "tree_depth_sum", "children_scanned", "terminal_hits", "faults")


def _logic():
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    rules, _fen, wb = pu.CONFIGS["copenhagen11"]
    return BatchedGameLogic(rules, 11, wb, device=0)


def _midgame_pair(lg, G):
    """Two batches with the same mixed mid-game positions (game i advanced by (3 i mod 48) seeded random plies)."""
    _rules, fen, _wb = pu.CONFIGS["copenhagen11"]
    a = lg.new_batch(G, fen)
    a.random_advance(1, (C.c_uint32 * G)(*[(i * 3) % 48 for i in range(G)]), 0)
    states = a.download()
    t = lg.new_batch(G)
    t.upload(states)
    return a, t, states


def _stats_tuple(st):
    return tuple(int(getattr(st, f)) for f in STAT_FIELDS) + (tuple(int(x) for x in st.reason_hist),)


def _assert_children_equal(a, t, G, what, nonempty=True):
    ra, ca = pu.children_view(*a.mcts_root_children(WIDTH), G, WIDTH)
    rt, ct = pu.children_view(*t.mcts_root_children(WIDTH), G, WIDTH)
    g = pu.first_children_diff(ra, ca, rt, ct)
    assert g < 0, f"{what}: root children of game {g} differ: {pu.children_of(ra, ca, g)} != {pu.children_of(rt, ct, g)}"
    assert not nonempty or int(ct.sum()) > G                   # (the comparison is not one of empty lists)


def test_reserve_joins_a_search_in_flight_and_keeps_its_tree():
    """tafl_mcts_reserve with a larger max_sims between tafl_mcts_run_async and tafl_mcts_wait grows the arena: it has to join the search
    first (the plan holds the old pointers and tafl_mcts_wait still issues straggler rounds on them), and the finished tree has to move
    into the larger arena, because the readers stay valid after a reserve.  16 384 mid-game games (two partitions on two streams),
    S = 40 then reserve(400); the children are read without an explicit wait and must equal the synchronous search's."""
    G = 16384
    lg = _logic()
    a, t, states = _midgame_pair(lg, G)
    t.mcts_run(SIMS, CPUCT, SEED, CAP, game_id_base=0)
    a.mcts_run_async(SIMS, CPUCT, SEED, CAP, game_id_base=0)
    a.mcts_reserve(400)
    _assert_children_equal(a, t, G, "run_async; reserve(400)")
    assert _stats_tuple(a.mcts_stats()) == _stats_tuple(t.mcts_stats())
    sa = a.mcts_stats()
    assert sa.sims == G * SIMS and sa.faults == 0
    # the grown arena is a working arena: a longer search on it equals the twin's (whose arena grows inside tafl_mcts_run)
    a.mcts_run(3 * SIMS, CPUCT, SEED, CAP, game_id_base=0)
    t.mcts_run(3 * SIMS, CPUCT, SEED, CAP, game_id_base=0)
    _assert_children_equal(a, t, G, "search after the reserve")
    # a reserve that follows a FINISHED search keeps its tree readable too
    t.mcts_reserve(800)
    _assert_children_equal(a, t, G, "reserve(800) after a finished search")
    assert pu.states_equal(states, a.download(), G)
    a.close(); t.close(); lg.close()


def _kth_ranks(G):
    return (C.c_uint32 * G)(*[(i * 2654435761) & 0x3FFFFFFF for i in range(G)])


def _call_do_play(b, G, ctx):
    eff = b.do_play(ctx["plays"])
    return bytes(eff)


def _call_do_kth_play(b, G, ctx):
    plays, eff = b.do_kth_play(_kth_ranks(G))
    return bytes(plays) + bytes(eff)


def _call_upload(b, G, ctx):
    b.upload(ctx["other_states"], first=G // 4, count=G // 2)       # a range that spans both partitions
    return b""


def _call_reset_fen(b, G, ctx):
    b.reset_fen(abi.boards.COPENHAGEN, abi.DEFENDER)
    return b""


def _call_random_advance(b, G, ctx):
    b.random_advance(9, (C.c_uint32 * G)(*[i % 5 for i in range(G)]), 77)
    return b""


def _call_mcts_play_best(b, G, ctx):
    plays, eff = b.mcts_play_best()
    return bytes(plays) + bytes(eff)


def _call_mcts_advance(b, G, ctx):
    plays, eff = b.mcts_advance(None)
    return bytes(plays) + bytes(eff)


# name -> (call, the root children of the search stay readable after it: include/taflhip.h - tafl_mcts_play_best gives the tree up,
# tafl_mcts_advance reports the kept root, the plain writers leave the last search's results alone)
WRITERS = {"do_play": (_call_do_play, True), "do_kth_play": (_call_do_kth_play, True), "upload": (_call_upload, True),
           "reset_fen": (_call_reset_fen, True), "random_advance": (_call_random_advance, True),
           "mcts_play_best": (_call_mcts_play_best, False), "mcts_advance": (_call_mcts_advance, True)}


@pytest.mark.parametrize("writer", list(WRITERS))
def test_writers_join_a_search_in_flight(writer):
    """{tafl_mcts_run_async; writer} without tafl_mcts_wait == {tafl_mcts_run; writer} on a twin batch: the states after the call, what
    the call returned, the statistics of the search and (where they stay readable) its root children.  8 192 games: two partitions on
    two streams, and a search that is still running when the writer arrives."""
    G = 8192
    call, children_readable = WRITERS[writer]
    lg = _logic()
    a, t, states = _midgame_pair(lg, G)
    # a legal play per game for do_play (the kth legal play of a scratch copy), other positions for upload
    scratch = lg.new_batch(G)
    scratch.upload(states)
    plays, _ = scratch.do_kth_play(_kth_ranks(G))
    ctx = {"plays": (TaflPlay * G).from_buffer_copy(bytes(plays)), "other_states": (TaflState * (G // 2)).from_buffer_copy(
        bytes(scratch.download(G // 4, G // 2)))}
    scratch.close()
    t.mcts_run(SIMS, CPUCT, SEED, CAP, game_id_base=0)
    want_ret = call(t, G, ctx)
    a.mcts_run_async(SIMS, CPUCT, SEED, CAP, game_id_base=0)
    got_ret = call(a, G, ctx)                                        # no mcts_wait: the call has to join by itself
    assert got_ret == want_ret, writer
    fa, ft = a.download(), t.download()
    assert pu.states_equal(fa, ft, G), (writer, pu.first_state_diff(fa, ft, G))
    assert not pu.states_equal(fa, states, G)                        # the call did write
    sa, st = a.mcts_stats(), t.mcts_stats()
    assert _stats_tuple(sa) == _stats_tuple(st), writer
    assert sa.sims == G * SIMS and sa.faults == 0
    if children_readable:                                            # (a kept root of a 40-simulation search has few visited children)
        _assert_children_equal(a, t, G, writer, nonempty=writer != "mcts_advance")
    if writer == "mcts_advance":
        assert list(a.mcts_tree_nodes()) == list(t.mcts_tree_nodes())
    a.close(); t.close(); lg.close()
