"""Workloads and expected values for the training-row tests at every board size (tests/test_hostsim_training_rows.py,
tests/test_gpu_training_rows.py; DESIGN.md sections 12 and 19): k_examples_gather, k_pool_count / k_pool_scan / k_pool_copy and k_pool_rows.

The expectation of a recorded run uses neither kernel under test.  It is built from the start states and the plays the run returned: the
oracle replays the plays (orc.batch_step) and gives board_to_matrix and the side to move before every move, z / final come from
examples_util.z_of on the final states (whose status the tests set by hand), and the sparse policy (actions, Nsa, n_children, overflow,
move_no) is the plain copy of tafl_examples_read.  Dense rows then follow pool_util.PoolModel.expect_gather / examples_util.dense_pi."""
import ctypes as C
import functools

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflPlay, TaflState
from oracle import oracle as orc
from tests import examples_util as xu
from tests import parity_util as pu
from tests import pool_util as qu

# Copenhagen rules on 15 x 15, the largest side tafl_ctx_create accepts: the king on the centre, a diamond of twelve defenders, six
# attackers on every edge.  225 of the 256 threads of the board write, BW = 57, action_size 6300.
COPENHAGEN15 = "5ttttt5/7t7/15/15/15/t6T6t/t5TTT5t/tt3TTKTT3tt/t5TTT5t/t6T6t/15/15/15/7t7/5ttttt5"

# name: (rules, start FEN, word_bits, side length, modulus of the random plies before the run)
LAYOUTS = {name: pu.CONFIGS[name] + (n, mod) for name, n, mod in (("tablut9", 9, 60), ("brandubh7_u128", 7, 30), ("copenhagen11", 11, 120),
                                                                   ("copenhagen13", 13, 120), ("tablut13_u256", 13, 120))}
LAYOUTS["copenhagen15"] = (abi.rules.COPENHAGEN, COPENHAGEN15, 256, 15, 120)
NAMES = ("tablut9", "brandubh7_u128", "copenhagen11", "copenhagen13", "tablut13_u256", "copenhagen15")

G, SIMS, MOVES, CAP, K, K_SMALL = 200, 16, 5, 64, 64, 8       # G: three full waves and a tail of 8 lanes; K_SMALL: below the usual root width
SEED, SAMPLE_SEED, ADVANCE_SEED = 8, 11, 3
OVER_AT_START = tuple(range(5, G, 23))                          # lanes whose status says "over" before the run: they record nothing
SPOT_LANES = (0, 63, 64, G - 1)

# The position with more than 256 legal plays: thirteen attackers (to move) on rows and columns of their own on an otherwise sparse
# 15 x 15 board, the king and four defenders in the middle.
WIDE_ATTACKERS = ((0, 3), (1, 9), (2, 5), (3, 12), (4, 1), (5, 10), (6, 13), (8, 2), (9, 11), (10, 4), (11, 8), (12, 6), (13, 0))
WIDE_DEFENDERS = ((6, 7), (8, 7), (7, 6), (7, 8))
WIDE_CRAFTED, WIDE_ORDINARY, WIDE_CAP, WIDE_K = 64, 6, 16, 340       # WIDE_K: a pool row of 404 words ends in a partial chunk that holds children


class Workload:
    """What a recording run is made of: lanes, moves, search parameters and the start states."""

    def __init__(self, name, lanes, n_moves, sims, cap, flags, start):
        self.name, self.G, self.n_moves, self.sims, self.cap, self.flags, self._start = name, lanes, n_moves, sims, cap, flags, start
        self.rules, self.fen, self.wb, self.n, _ = LAYOUTS[name]

    def start(self):
        return pu.clone_states(self._start, self.G)

    def logic(self):
        return orc.GameLogic(self.rules, self.n)

    def params(self):
        return TaflMctsParams(self.sims, self.cap, 1.0, SEED, 0, self.flags)


@functools.lru_cache(maxsize=None)
def workload(name):
    """G games of the layout, (5 * g) % mod random plies into the game, the lanes OVER_AT_START marked as won before the run."""
    rules, fen, wb, n, mod = LAYOUTS[name]
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    orc.batch_random_advance(orc.GameLogic(rules, n), states, G, wb, ADVANCE_SEED, (C.c_uint32 * G)(*[(g * 5) % mod for g in range(G)]), 0)
    for g in OVER_AT_START:
        states[g].status, states[g].winner = 1, abi.DEFENDER
    return Workload(name, G, MOVES, SIMS, CAP, 0, states)


def _fen_of(n, cells):
    rows = []
    for r in range(n):
        out, run = "", 0
        for c in range(n):
            ch = cells.get((r, c))
            if ch is None:
                run += 1
            else:
                out, run = out + (str(run) if run else "") + ch, 0
        rows.append(out + (str(run) if run else ""))
    return "/".join(rows)


def wide_fen():
    cells = {t: "t" for t in WIDE_ATTACKERS}
    cells.update({t: "T" for t in WIDE_DEFENDERS})
    cells[(7, 7)] = "K"
    return _fen_of(15, cells)


@functools.lru_cache(maxsize=None)
def wide_legal_count():
    """Legal plays of the crafted position, from the oracle's move generation."""
    rules, _, wb, n, _ = LAYOUTS["copenhagen15"]
    st = pu.start_states(orc, wide_fen(), abi.ATTACKER, wb, 1)
    return int(orc.batch_movegen(orc.GameLogic(rules, n), st, 1, wb, want_masks=False)[0][0])


@functools.lru_cache(maxsize=None)
def wide_workload():
    """WIDE_CRAFTED lanes of the crafted position, then WIDE_ORDINARY lanes of the 15 x 15 start some random plies in: one move with
    TAFL_MCTS_FLAG_FPU_INF (every legal play of the root is tried before any is tried twice) and S = legal count + 8."""
    rules, fen, wb, n, _ = LAYOUTS["copenhagen15"]
    lanes = WIDE_CRAFTED + WIDE_ORDINARY
    states = (TaflState * lanes)()
    crafted = pu.start_states(orc, wide_fen(), abi.ATTACKER, wb, WIDE_CRAFTED)
    ordinary = pu.start_states(orc, fen, rules.starting_side, wb, WIDE_ORDINARY)
    orc.batch_random_advance(orc.GameLogic(rules, n), ordinary, WIDE_ORDINARY, wb, ADVANCE_SEED, (C.c_uint32 * WIDE_ORDINARY)(*[7 * g for g in range(WIDE_ORDINARY)]), 0)
    C.memmove(states, crafted, C.sizeof(TaflState) * WIDE_CRAFTED)
    C.memmove(C.byref(states, C.sizeof(TaflState) * WIDE_CRAFTED), ordinary, C.sizeof(TaflState) * WIDE_ORDINARY)
    return Workload("copenhagen15", lanes, 1, wide_legal_count() + 8, WIDE_CAP, abi.MCTS_FLAG_FPU_INF, states)


def hand_set_results(states, lanes):
    """The status of every game set by hand, as test_finalize_outcomes_including_a_draw does: ongoing / attackers won / defenders won /
    draw by g % 4.  Taken rows then carry z = +1, -1 and 1e-4, and the examples of every fourth lane stay open."""
    for g in range(lanes):
        states[g].status, states[g].winner = (abi.ONGOING, 1, 1, 2)[g % 4], (0, abi.ATTACKER, abi.DEFENDER, 0)[g % 4]


class Recording:
    """A recorded and finalized run: ex (engine.Examples or examples_util.HostExamples), K, the states before the run, the plays
    [m * G + g] it returned, the states after it (end) and the states it was finalized against (final), sparse(es) -> the arrays
    (n_children, overflow, played, move_no, actions, visits) of the entries es."""

    def __init__(self, w, ex, k, plays, end, final, sparse):
        self.w, self.ex, self.K, self.start, self.plays, self.end, self.final, self.sparse = w, ex, k, w.start(), plays, end, final, sparse


def device_recorded(glg, w, k=K):
    """tafl_selfplay_record in rollout mode on the device, every move drawn from the visit counts, then tafl_examples_finalize against
    the hand-set results."""
    b = glg.new_batch(w.G)
    b.upload(w.start())
    ex = glg.new_examples(w.G, w.n_moves, k)
    plays = b.selfplay_record(ex, w.n_moves, w.sims, 1.0, SEED, w.cap, flags=w.flags, sample_seed=SAMPLE_SEED, temp_moves=w.n_moves, want_plays=True)
    assert b.mcts_stats().faults == 0
    end = pu.clone_states(b.download(), w.G)
    final = pu.clone_states(end, w.G)
    hand_set_results(final, w.G)
    b.upload(final)
    ex.finalize(b)
    b.close()
    return Recording(w, ex, k, plays, end, final, ex.read)


def host_recorded(w, k=K):
    """The same run through the host harness (tests/hostsim: hsx_record, hsx_finalize)."""
    hx = xu.HostExamples(w.rules, w.n, w.wb, w.G, w.n_moves, k)
    end = w.start()
    xu.hlib().hsx_set_dense13(int(w.name == "copenhagen13"))
    try:
        plays, stats = hx.record(end, w.params(), w.n_moves, 0, SAMPLE_SEED, w.n_moves)
    finally:
        xu.hlib().hsx_set_dense13(0)
    assert stats.faults == 0
    final = pu.clone_states(end, w.G)
    hand_set_results(final, w.G)
    hx.finalize(final)

    def sparse(es):
        nc, ov, pl, mv = (np.zeros(len(es), t) for t in (np.uint32, np.uint8, np.uint32, np.uint32))
        acts, vis = np.zeros((len(es), k), np.uint32), np.zeros((len(es), k), np.uint32)
        for i, e in enumerate(es):
            (_rows, _side, a, v, played, move_no), overflow = hx._example(int(e) // w.G, int(e) % w.G, C.byref(C.c_float()), C.byref(C.c_uint8()))
            nc[i], ov[i], pl[i], mv[i] = len(a), overflow, played, move_no
            acts[i, :len(a)], vis[i, :len(v)] = a, v
        return nc, ov, pl, mv, acts, vis

    return Recording(w, hx, k, plays, end, final, sparse)


def expected_table(rec):
    """The pool_util.Table of a Recording from the oracle's replay of its plays (module docstring).  Asserted on the way: the replay
    ends in the states the run ended in, every example's move number is the move it was recorded at and its play is the play returned."""
    w = rec.w
    lg, cur = w.logic(), pu.clone_states(rec.start, w.G)
    lens, rows = [0] * w.G, []
    for m in range(w.n_moves):
        sub = (TaflPlay * w.G)()
        for g in range(w.G):
            p = rec.plays[m * w.G + g]
            if pu.play_tuple4(p) == (0, 0, 0, 0):
                continue                                           # no play: the game was over
            assert lens[g] < w.n_moves
            board = np.array(orc.GameState.from_abi(cur[g], w.wb).board_to_matrix(), np.uint8).reshape(w.n, w.n)
            rows.append((lens[g] * w.G + g, g, board, cur[g].side_to_play, m, abi.action_encode(w.n, p)))
            lens[g] += 1
            sub[g] = TaflPlay(p.from_row, p.from_col, p.axis, p.disp)
        orc.batch_step(lg, cur, w.G, w.wb, sub)
    assert pu.states_equal(cur, rec.end, w.G), (w.name, pu.first_state_diff(cur, rec.end, w.G))
    t = qu.Table(w.G, w.n_moves, rec.K, w.n, lens)
    rows.sort(key=lambda r: r[0])
    es = np.asarray([r[0] for r in rows], np.uint32)
    assert es.tolist() == t.valid()
    if es.size:
        nc, ov, pl, mv, acts, vis = rec.sparse(es)
        assert mv.tolist() == [r[4] for r in rows] and pl.tolist() == [r[5] for r in rows], w.name
        t.overflow[es], t.nc[es], t.move_no[es], t.actions[es], t.visits[es] = ov, nc, mv, acts, vis
        for e, g, board, side, _m, _a in rows:
            t.boards[e], t.side[e] = board, side
            t.z[e], t.final[e] = xu.z_of(rec.final[g], side)
    return t


def expect_example_rows(t, es, sym):
    """(boards, sides, pi, z, final) tafl_examples_gather owes for the entries es of the table under the symmetries sym, in numpy."""
    n, A = t.n, abi.action_size(t.n)
    boards, pi = np.zeros((len(es), n, n), np.uint8), np.zeros((len(es), A), np.float32)
    for i, (e, k) in enumerate(zip(es, sym)):
        e, k, nc = int(e), int(k), int(t.nc[e])
        boards[i] = xu.sym_board_np(t.boards[e], k)
        N = np.float64(t.visits[e, :nc].sum(dtype=np.uint64))
        for a, v in zip(t.actions[e, :nc], t.visits[e, :nc]):
            pi[i, xu.sym_action_py(n, int(a), k)] = np.float32(np.float64(v) / N)
    es = np.asarray(es, np.int64)
    return boards, t.side[es], pi, t.z[es], t.final[es]


def assert_same_table(a, b, where=""):
    """Two tables hold the same examples: lens, and every field of every entry that holds an example."""
    assert (a.G, a.max_moves, a.K, a.n) == (b.G, b.max_moves, b.K, b.n) and np.array_equal(a.lens, b.lens), (where, "lens")
    es = np.asarray(a.valid(), np.int64)
    for f in ("overflow", "final", "nc", "side", "move_no", "z", "actions", "visits", "boards"):
        assert getattr(a, f)[es].tobytes() == getattr(b, f)[es].tobytes(), (where, f)


def summary(t):
    """Coverage of a table + the widest root among its examples, for the reports of the tests."""
    es = np.asarray(t.valid(), np.int64)
    return dict(qu.coverage(t), widest=int(t.nc[es].max(initial=0)))
