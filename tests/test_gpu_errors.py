"""Return codes of the C-ABI for calls that are refused before anything is launched: the code (TaflError.code) and, where the message names
the entry point, that name.  One table, run in order on a 64-game Copenhagen 11x11 batch and a 64-game Brandubh 7x7 batch; a refused call
must leave the batch usable, so the same batch then runs an ordinary search that the oracle reproduces.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd._lib import TaflError, check, lib
from alphazeroforhnefatafl_amd.abi import TaflEffects, TaflGmctsStats, TaflMctsParams, TaflMctsStats, TaflPlay, TaflRootChild
from oracle import oracle as orc
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

G, SIMS, CAP, SEED, BASE = 64, 8, 128, 5, 300
INVALID, UNSUPPORTED, CAPACITY = -1, -5, -7
VP = C.c_void_p


class Env:
    def __init__(self, name):
        from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
        self.name = name
        self.rules, fen, self.wb = pu.CONFIGS[name]
        self.n = abi.fen_side_len(fen)
        self.olg = orc.GameLogic(self.rules, self.n)
        self.states = pu.start_states(orc, fen, self.rules.starting_side, self.wb, G)
        orc.batch_random_advance(self.olg, self.states, G, self.wb, 9, (C.c_uint32 * G)(*[(i * 5) % 24 for i in range(G)]), BASE)
        self.lg = BatchedGameLogic(self.rules, self.n, self.wb)
        self.b = self.lg.new_batch(G)
        self.b.upload(self.states)
        self.A = self.lg.action_size
        self.kids, self.cnt = (TaflRootChild * (G * 256))(), (C.c_uint32 * G)()
        self.plays, self.eff = (TaflPlay * G)(), (TaflEffects * G)()
        self.u32 = (C.c_uint32 * (G * self.A))()
        self.dbl = (C.c_double * (G * self.A))()
        self.u8 = (C.c_uint8 * (G * self.n * self.n))()
        self.f32 = (C.c_float * (G * self.A))()
        self.ex = None

    def params(self, n_sims=SIMS, flags=0):
        self._p = TaflMctsParams(n_sims, CAP, 1.0, SEED, 0, flags)
        return C.byref(self._p)

    def search(self):
        check(lib().tafl_mcts_run(self.b._h, self.params(), BASE))

    def examples(self):
        if self.ex is None:
            self.ex = self.lg.new_examples(G, 2, 8)
        return self.ex._h

    def wrong_side_len(self):
        st = pu.clone_states(self.states, 1)
        st[0].side_len = self.n + 2
        return st


def _gather_host(e):
    idx = (C.c_uint32 * 1)(0)
    v = C.cast(e.u8, VP)
    return lib().tafl_examples_gather(e.examples(), C.cast(idx, VP), None, 1, v, v, C.cast(e.f32, VP), C.cast(e.f32, VP), v, 0)


def _read(e):
    idx = (C.c_uint32 * 1)(0)
    return lib().tafl_examples_read(e.examples(), C.cast(idx, VP), 1, C.cast(e.u32, VP), None, None, None, None, None)


def _examples_create(e, max_children):
    h = VP()
    return lib().tafl_examples_create(e.lg._h, G, 2, max_children, C.byref(h))


# (row of the table, what is called, the call, expected code, name the message must contain or None, configuration it is for or None).
# The rows run in this order on one batch per configuration: "before any search" comes before the first search, "before tafl_gmcts_begin"
# before the first begin.  `prep` rows (code None) must succeed.
L = lib
ROWS = [
    (1, "mcts_wait, never searched", lambda e: L().tafl_mcts_wait(e.b._h), INVALID, "tafl_mcts_wait", None),
    (2, "mcts_root_children, no search", lambda e: L().tafl_mcts_root_children(e.b._h, e.kids, 256, e.cnt), INVALID, None, None),
    (2, "mcts_root_visits, no search", lambda e: L().tafl_mcts_root_visits(e.b._h, e.u32), INVALID, None, None),
    (2, "mcts_best_play, no search", lambda e: L().tafl_mcts_best_play(e.b._h, e.plays, e.cnt), INVALID, None, None),
    (2, "mcts_play_best, no search", lambda e: L().tafl_mcts_play_best(e.b._h, e.plays, e.eff), INVALID, None, None),
    (2, "mcts_policy_device, no search", lambda e: L().tafl_mcts_policy_device(e.b._h, 1.0, C.cast(e.dbl, VP), 0), INVALID, None, None),
    (3, "mcts_get_stats, no search", lambda e: L().tafl_mcts_get_stats(e.b._h, C.byref(TaflMctsStats())), INVALID, None, None),
    (3, "mcts_round_trace, no search", lambda e: L().tafl_mcts_round_trace(e.b._h, e.u32, e.u32, 16, C.byref(C.c_uint32())), INVALID, None, None),
    (4, "mcts_reserve(0)", lambda e: L().tafl_mcts_reserve(e.b._h, 0), INVALID, None, None),
    (4, "mcts_reserve(60001)", lambda e: L().tafl_mcts_reserve(e.b._h, 60001), INVALID, None, None),
    (5, "mcts_run, n_sims = 0", lambda e: L().tafl_mcts_run(e.b._h, e.params(n_sims=0), BASE), INVALID, None, None),
    (6, "mcts_run, unknown flag bit", lambda e: L().tafl_mcts_run(e.b._h, e.params(flags=1 << 20), BASE), UNSUPPORTED, None, None),
    (7, "mcts_run, fused pipeline on the 128-bit board",
     lambda e: L().tafl_mcts_run(e.b._h, e.params(flags=abi.mcts_tune(pipeline=abi.MCTS_PIPELINE_FUSED)), BASE), UNSUPPORTED, None, "copenhagen11"),
    (8, "mcts_run, fused pipeline with 4 slots",
     lambda e: L().tafl_mcts_run(e.b._h, e.params(flags=abi.mcts_tune(pipeline=abi.MCTS_PIPELINE_FUSED, slots=4)), BASE), UNSUPPORTED, None, "brandubh7"),
    (9, "mcts_advance(NULL), no retained tree", lambda e: L().tafl_mcts_advance(e.b._h, None, e.plays, e.eff), INVALID, "tafl_mcts_advance", None),
    (10, "prep: an 8-simulation search", lambda e: L().tafl_mcts_run(e.b._h, e.params(), BASE), None, None, None),
    (10, "mcts_root_children, max_children = 1", lambda e: L().tafl_mcts_root_children(e.b._h, e.kids, 1, e.cnt), CAPACITY, None, None),
    (11, "selfplay_run, n_moves = 0", lambda e: L().tafl_selfplay_run(e.b._h, e.params(), 0, BASE, None), INVALID, "tafl_selfplay_run", None),
    (12, "selfplay_run, KEEP_TREE", lambda e: L().tafl_selfplay_run(e.b._h, e.params(flags=abi.MCTS_FLAG_KEEP_TREE), 1, BASE, None),
     UNSUPPORTED, "tafl_selfplay_run", None),
    (13, "gmcts_step before begin", lambda e: L().tafl_gmcts_step(e.b._h, None, None, 0, 1.0, 1, None), INVALID, "tafl_gmcts_step", None),
    (13, "gmcts_leaves before begin", lambda e: L().tafl_gmcts_leaves(e.b._h, C.cast(e.u8, VP), C.cast(e.u8, VP), C.cast(e.u8, VP), 0),
     INVALID, "tafl_gmcts_leaves", None),
    (13, "gmcts_root_children before begin", lambda e: L().tafl_gmcts_root_children(e.b._h, e.kids, 256, e.cnt), INVALID, "tafl_gmcts_root_children", None),
    (13, "gmcts_root_visits before begin", lambda e: L().tafl_gmcts_root_visits(e.b._h, C.cast(e.u32, VP), 0), INVALID, "tafl_gmcts_root_visits", None),
    (13, "gmcts_policy before begin", lambda e: L().tafl_gmcts_policy(e.b._h, 1.0, C.cast(e.dbl, VP), 0), INVALID, "tafl_gmcts_policy", None),
    (13, "gmcts_advance before begin", lambda e: L().tafl_gmcts_advance(e.b._h, None, e.plays, e.eff), INVALID, "tafl_gmcts_advance", None),
    (13, "gmcts_get_stats before begin", lambda e: L().tafl_gmcts_get_stats(e.b._h, C.byref(TaflGmctsStats())), INVALID, "tafl_gmcts_get_stats", None),
    (14, "gmcts_begin_ex, unknown flag", lambda e: L().tafl_gmcts_begin_ex(e.b._h, 4, 64, 1 << 5), UNSUPPORTED, "tafl_gmcts_begin_ex", None),
    (15, "gmcts_begin_ex, max_sims = 0", lambda e: L().tafl_gmcts_begin_ex(e.b._h, 0, 64, 0), INVALID, "tafl_gmcts_begin", None),
    (16, "prep: gmcts_begin(4, 64)", lambda e: L().tafl_gmcts_begin(e.b._h, 4, 64), None, None, None),
    (16, "gmcts_step, n_sims = 5 of 4 reserved", lambda e: L().tafl_gmcts_step(e.b._h, None, None, 0, 1.0, 5, None), CAPACITY, "tafl_gmcts_step", None),
    (17, "gmcts_step, priors without values", lambda e: L().tafl_gmcts_step(e.b._h, C.cast(e.f32, VP), None, 0, 1.0, 4, None), INVALID, "tafl_gmcts_step", None),
    (18, "batch_upload, first + count > n", lambda e: L().tafl_batch_upload(e.b._h, e.states, G - 1, 2), INVALID, None, None),
    (19, "batch_upload, a state of another side_len", lambda e: L().tafl_batch_upload(e.b._h, e.wrong_side_len(), 0, 1), INVALID, None, None),
    (20, "examples_create, max_children = 0", lambda e: _examples_create(e, 0), INVALID, "tafl_examples_create", None),
    (21, "examples_create, max_children = 65536", lambda e: _examples_create(e, 65536), INVALID, "tafl_examples_create", None),
    (22, "examples_gather (host pointers), nothing recorded", _gather_host, INVALID, "tafl_examples_gather", None),
    (22, "examples_read, nothing recorded", _read, INVALID, "tafl_examples_read", None),
    (23, "ctx_destroy while a batch is alive", lambda e: L().tafl_ctx_destroy(e.lg._h), INVALID, "tafl_ctx_destroy", None),
]


@pytest.mark.parametrize("name", ["copenhagen11", "brandubh7"])
def test_refused_calls_return_their_codes_and_leave_the_batch_usable(name):
    e = Env(name)
    wrong = []
    for row, what, call, code, needle, only in ROWS:
        if only is not None and only != name:
            continue
        rc = call(e)
        if code is None:
            check(rc)
            continue
        try:
            check(rc)
            got, msg = 0, ""
        except TaflError as err:
            got, msg = err.code, str(err)
        print(f"row {row:2d} {what}: code {got} {msg!r}")
        if got != code or (needle is not None and needle not in msg):
            wrong.append((row, what, got, code, msg))
    assert not wrong, wrong
    # the batch still holds the uploaded states and searches like any other: 8 games against the oracle, bit for bit
    assert pu.states_equal(e.states, e.b.download(), G)
    e.search()
    gk, gn = e.b.mcts_root_children(256)
    p = TaflMctsParams(SIMS, CAP, 1.0, SEED, 0, 0)
    ok, on, _ = orc.batch_mcts(e.olg, e.states, 8, e.wb, p, BASE)
    assert list(on) == list(gn)[:8] and sum(on) > 8
    for g in range(8):
        for j in range(on[g]):
            x, y = ok[g * 256 + j], gk[g * 256 + j]
            assert (pu.play_tuple4(x.play), x.action, x.visits, float(x.q).hex()) == (pu.play_tuple4(y.play), y.action, y.visits, float(y.q).hex()), (g, j)
    st = e.b.mcts_stats()
    assert st.sims == G * SIMS and st.faults == 0
    e.lg.close()
