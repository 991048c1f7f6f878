"""Expected values and drivers for the guided self-play tests (include/taflhip.h tafl_gselfplay_*): the oracle loop
- orc.GameLogic.gmcts, the pick rule and the RNG word restated in tests/examples_util.py, the oracle's do_play - and the loader of the
host harness's guided run (tests/hostsim, hsg_*: Guided::selfplay_step compiled for the CPU)."""
import ctypes as C

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflSelfplayOpts, TaflState
from tests import examples_util as eu
from tests import parity_util as pu
from tests.hostsim import hostsim
from tests.stub_net import matrix_bytes_of, stub_predict

_STUB = {}


def stub(matrix_bytes: bytes, side: int, action_size: int, salt: int):
    """stub_predict, remembered: the oracle loop, the harness and the device runs of one test ask for the same leaves."""
    key = (matrix_bytes, side, action_size, salt)
    hit = _STUB.get(key)
    if hit is None:
        hit = _STUB[key] = stub_predict(matrix_bytes, side, action_size, salt)
    return hit


def stub_rows(boards, sides, waiting, n, side_len, action_size, salts):
    """nnet.predict for every waiting game: (priors float32 [n, A], values float32 [n]) as numpy arrays."""
    nn = side_len * side_len
    raw = bytes(boards)
    pri, val = np.zeros((n, action_size), np.float32), np.zeros(n, np.float32)
    for g in range(n):
        if waiting[g]:
            pri[g], val[g] = stub(raw[g * nn:(g + 1) * nn], int(sides[g]), action_size, salts[g])
    return pri, val


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def start_states(orc, lg, rules, fen, wb, G, modulus, seed=21):
    """Game i = the start position advanced by (7 i) mod `modulus` random plies (modulus 0: the start position)."""
    base = orc.GameState(fen, rules.starting_side, wb)
    return (TaflState * G)(*[(lg.random_advance(base, seed, g, (7 * g) % modulus) if modulus else base).to_abi() for g in range(G)])


class Run:
    """What a run leaves: plays[m][g] as 4-tuples, final states (bytes per game), moves made per game, examples per game
    (examples_util.Example.fields() tuples), sims."""

    def __init__(self, G, n_moves):
        self.plays = [[(0, 0, 0, 0)] * G for _ in range(n_moves)]
        self.states, self.moves, self.examples, self.sims = [None] * G, [0] * G, [[] for _ in range(G)], 0


def oracle_run(orc, lg, states, wb, S, c_puct, salts, n_moves, sample_seed, temp_moves, move_base=0, base=0, games=None):
    """The loop of include/taflhip.h on the oracle, per game: gmcts from a fresh root, the pick, the example, do_play."""
    G = len(states)
    n = states[0].side_len
    A = abi.action_size(n)
    out = Run(G, n_moves)
    for g in (range(G) if games is None else games):
        st = orc.GameState.from_abi(states[g], wb)
        for m in range(n_moves):
            if st.to_abi().status != abi.ONGOING:
                break
            kids, _ns, _pri, _cnt = lg.gmcts(st, S, c_puct, lambda s, g=g: stub(matrix_bytes_of(s.board_to_matrix()), int(s.side_to_play), A, salts[g]), wb)
            out.sims += S
            vs = [v for (_p, _a, v, _q) in kids]
            if not vs:
                break
            M = move_base + m
            j = eu.pick_rule(vs, eu.sample_word(sample_seed, base + g, M)) if M < temp_moves else vs.index(max(vs))
            e = eu.Example()
            e.board, e.side = st.board_to_matrix(), st.to_abi().side_to_play
            e.actions, e.visits, e.played, e.move_no = [a for (_p, a, _v, _q) in kids], vs, kids[j][1], M
            out.examples[g].append(e.fields())
            play = abi.action_decode(n, kids[j][1])
            code, st, _eff = lg.do_play(play, st)
            assert code == 0, (g, m, code)
            out.plays[m][g] = pu.play_tuple4(play)
            out.moves[g] = m + 1
        out.states[g] = bytes(st.to_abi())
    return out


# ---- the host harness ---------------------------------------------------------------------------------------------------------
hlib = hostsim.lib


class HostExamples(hostsim.HostExamples):
    pre = "hsg_ex_"

    def example(self, j, g):
        """(Example.fields() tuple, overflow) of example (j, g)."""
        return self._example(j, g)

    def all(self):
        """(examples per game as fields tuples, overflow marks per game)."""
        lens, _ = self.counts()
        got = [[self.example(j, g) for j in range(min(lens[g], self.max_moves))] for g in range(self.G)]
        return [[f for f, _ in row] for row in got], [[o for _, o in row] for row in got]


def host_run(rules, n, wb, states, S, c_puct, salts, n_moves, sample_seed, temp_moves, ex=None, move_base=0, base=0, edges_per_node=256):
    """tafl_gselfplay_begin / the step loop / tafl_gselfplay_end on the harness, with the stub network.  Returns (Run, faults [G], rounds);
    Run.examples is left empty (read them from `ex`)."""
    L = hlib()
    G, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(sample_seed, temp_moves, move_base, 0)
    h = L.hsg_begin(C.byref(rc), n, wb, states, G, S, edges_per_node, c_puct, C.byref(o), n_moves, base, ex.h if ex is not None else None)
    assert h
    try:
        boards, sides, waiting = (C.c_uint8 * (G * n * n))(), (C.c_uint8 * G)(), (C.c_uint8 * G)()
        L.hsg_leaves(h, boards, sides, waiting)
        w, rounds = sum(waiting), 0
        while w:
            pri, val = stub_rows(boards, sides, waiting, G, n, A, salts)
            w = L.hsg_step(h, fptr(pri), fptr(val))
            L.hsg_leaves(h, boards, sides, waiting)
            assert sum(waiting) == w
            rounds += 1
        st, plays, moves, cnt, faults = (TaflState * G)(), (TaflPlay * (G * n_moves))(), (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint8 * G)()
        L.hsg_end(h, st, plays, moves, cnt, faults)
    finally:
        L.hsg_free(h)
    out = Run(G, n_moves)
    out.plays = [[pu.play_tuple4(plays[m * G + g]) for g in range(G)] for m in range(n_moves)]
    out.states, out.moves, out.sims = [bytes(st[g]) for g in range(G)], list(moves), cnt[0]
    out.abi_states, out.stat_faults = st, cnt[3]
    return out, list(faults), rounds


def device_examples(ex, G, n):
    """(examples per game as examples_util.Example.fields() tuples, overflow marks per game) read back from the device."""
    lens, total = ex.counts()
    lens = list(lens)
    assert total == sum(lens)
    idx = np.array([j * G + g for g in range(G) for j in range(lens[g])], np.uint32)
    out, over = [[] for _ in range(G)], [[] for _ in range(G)]
    if idx.size:
        nc, ov, pl, mv, acts, vis = ex.read(idx)
        boards, sides, _pi, _z, _fin = ex.gather(idx)
        for i, e in enumerate(idx):
            g, k = int(e) % G, int(nc[i])
            out[g].append((boards[i].tolist(), int(sides[i]), acts[i, :k].tolist(), vis[i, :k].tolist(), int(pl[i]), int(mv[i])))
            over[g].append(int(ov[i]))
    return out, over


def device_run(batch, ex, n, S, c_puct, salts, n_moves, sample_seed, temp_moves, move_base=0, base=0, edges_per_node=256):
    """tafl_gselfplay_begin / the step loop / tafl_gselfplay_end through the C-ABI on `batch` (states uploaded), with the stub network in
    host buffers.  Returns (Run with the examples read from `ex`, overflow marks per game, stats)."""
    G, A = batch.n, abi.action_size(n)
    batch.gselfplay_begin(ex, n_moves, S, c_puct, edges_per_node, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves, move_base=move_base)
    w = batch.gselfplay_step()
    while w:
        boards, sides, waiting = batch.gmcts_leaves()
        assert sum(waiting) == w
        pri, val = stub_rows(boards, sides, waiting, G, n, A, salts)
        w = batch.gselfplay_step(fptr(pri), fptr(val))
    plays, moves = batch.gselfplay_end()
    stats = batch.gmcts_stats()
    st = batch.download()
    run = Run(G, n_moves)
    run.plays = [[pu.play_tuple4(plays[m * G + g]) for g in range(G)] for m in range(n_moves)]
    run.states, run.moves, run.sims = [bytes(st[g]) for g in range(G)], list(moves), stats.sims
    run.examples, over = device_examples(ex, G, n)
    return run, over, stats


def fates(states_before, run):
    """(games over at the start, games that ended during the run, games still going after it)."""
    G = len(states_before)
    over0 = [g for g in range(G) if states_before[g].status != abi.ONGOING]
    after = [TaflState.from_buffer_copy(run.states[g]).status for g in range(G)]
    ended = [g for g in range(G) if g not in over0 and after[g] != abi.ONGOING]
    going = [g for g in range(G) if after[g] == abi.ONGOING]
    return over0, ended, going


def assert_same_run(got: Run, want: Run, got_examples, games=None, where=""):
    G = len(want.states)
    for g in (range(G) if games is None else games):
        assert [row[g] for row in got.plays] == [row[g] for row in want.plays], (where, "plays", g)
        assert got.moves[g] == want.moves[g], (where, "moves", g, got.moves[g], want.moves[g])
        assert got.states[g] == want.states[g], (where, "state", g)
        assert len(got_examples[g]) == len(want.examples[g]), (where, "examples", g, len(got_examples[g]), len(want.examples[g]))
        for j, (a, b) in enumerate(zip(got_examples[g], want.examples[g])):
            assert a == b, (where, "example", g, j, a, b)
