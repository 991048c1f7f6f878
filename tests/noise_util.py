"""Expected values for the root-noise tests (include/taflhip.h tafl_root_noise).

The oracle cannot express the mix (its callback delivers float32 priors before normalisation), so the expectation is a TWIN: a guided
search in plain Python over the oracle's rules - GameLogic.all_plays / do_play for the game, np.sum for the pairwise sum, the arithmetic
of src/mcts.py:55-136 in Python floats - that takes (epsilon, eta row) for its root.  With epsilon == 0 it must equal orc.GameLogic.gmcts
exactly (pin_twin); only then is it used.  eta itself is never restated: a side's search (the device's, or the host harness's) is compared
with the twin fed that side's own eta, and eta is checked by its exact properties and against numpy's Dirichlet sampler.

Two back ends serve the same checks: HostSide (tests/hostsim_noise: the per-game functions of tafl_guided.hpp compiled for the CPU) and
DeviceSide (the C-ABI on a GPU)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflRootChild, TaflRootNoise, TaflSelfplayOpts, TaflState
from tests import examples_util as eu
from tests import gselfplay_util as gsu
from tests import parity_util as pu
from tests.stub_net import matrix_bytes_of

MCTS_EPS = 1e-8            # src/mcts.py:6
CPUCT = 1.25
S, EDGES = 24, 256
G_PLAIN = 70               # one full wave plus a partial one; the two crafted games follow
ALPHA, EPSILON, NOISE_SEED = 0.3, 0.25, 0xD1CE
LAYOUTS = ("brandubh7", "copenhagen11", "copenhagen13")
# per layout: (random plies after which the game is over, (game id, plies) of a position from which the noisy run of check 2 ends the game)
CRAFTED = {"brandubh7": (400, (3, 52)), "copenhagen11": (2000, (0, 898)), "copenhagen13": (3000, (1, 807))}


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
class _Node:
    __slots__ = ("st", "es", "acts", "ps", "ns", "q", "n", "child")

    def __init__(self, st):
        self.st, self.es, self.acts, self.ps, self.ns, self.q, self.n, self.child = st, None, None, None, 0, {}, {}, {}


def game_ended(st: TaflState) -> float:
    """getGameEnded(board, 1): the value for the player to move; a draw is 1e-4."""
    if st.status == abi.ONGOING:
        return 0.0
    if st.status == abi.DRAW:
        return 1e-4
    return 1.0 if st.winner == st.side_to_play else -1.0


class Twin:
    """One search: mcts.py:55-136 on an explicit tree, as the oracle's gm_search.  noise = (epsilon, eta row [A]) is mixed into the root's
    normalised priors; depth1_epsilon (the mutation of check 3) mixes a flat 1/n into the priors of the root's children as well."""

    def __init__(self, lg, state, c_puct, predict, noise=None, depth1_epsilon=0.0):
        self.lg, self.n, self.c_puct, self.predict, self.noise, self.d1 = lg, lg.side_len, c_puct, predict, noise, depth1_epsilon
        self.A = abi.action_size(self.n)
        self.root = _Node(state)
        self.sims = self.predicts = self.terminal_hits = self.depth_sum = 0

    def run(self, n_sims):
        for _ in range(n_sims):
            self.search(self.root, 0)
            self.sims += 1
        return self

    def expand(self, nd, depth):
        pri, v = self.predict(nd.st)
        self.predicts += 1
        acts = sorted(abi.action_encode(self.n, p) for p in self.lg.all_plays(nd.st))
        ps = np.zeros(self.A, np.float64)
        ps[acts] = np.asarray(pri, np.float32)[acts].astype(np.float64) * 1.0          # mcts.py:87
        sum_ps = float(np.sum(ps))                                                       # :88
        if sum_ps > 0:
            ps = ps / sum_ps
        else:                                                                            # :91-98
            valids = np.zeros(self.A, np.float64)
            valids[acts] = 1.0
            ps = ps + valids
            ps = ps / float(np.sum(ps))
        p = {a: float(ps[a]) for a in acts}
        if depth == 0 and self.noise is not None:
            eps, eta = self.noise
            for a in acts:
                p[a] = (1.0 - eps) * p[a] + eps * float(eta[a])
        if depth == 1 and self.d1:
            for a in acts:
                p[a] = (1.0 - self.d1) * p[a] + self.d1 * (1.0 / len(acts))
        nd.acts, nd.ps, nd.ns = acts, p, 0
        return -float(v)

    def search(self, nd, depth):
        if nd.es is None:
            nd.es = game_ended(nd.st.to_abi())
        if nd.es != 0:
            self.terminal_hits += 1
            return -nd.es
        if nd.ps is None:
            return self.expand(nd, depth)
        self.depth_sum += 1
        cur_best, best = -math.inf, -1
        sq, sq0 = math.sqrt(float(nd.ns)), math.sqrt(float(nd.ns) + MCTS_EPS)
        for a in nd.acts:
            if a in nd.q:
                u = nd.q[a] + self.c_puct * nd.ps[a] * sq / float(1 + nd.n[a])
            else:
                u = self.c_puct * nd.ps[a] * sq0
            if u > cur_best:
                cur_best, best = u, a
        a = best
        if a < 0:
            return 0.0
        if a not in nd.child:
            code, nxt, _eff = self.lg.do_play(abi.action_decode(self.n, a), nd.st)
            assert code == 0, code
            nd.child[a] = _Node(nxt)
        v = self.search(nd.child[a], depth + 1)
        if a in nd.q:
            nd.q[a] = (float(nd.n[a]) * nd.q[a] + v) / float(nd.n[a] + 1)
            nd.n[a] += 1
        else:
            nd.q[a], nd.n[a] = v, 1
        nd.ns += 1
        return -v

    def kids(self):
        """[(action, visits, Qsa bits)] of the visited root edges, ascending."""
        r = self.root
        return [(a, r.n[a], qbits(r.q[a])) for a in (r.acts or []) if a in r.q]

    def priors(self):
        row = np.zeros(self.A, np.float64)
        if self.root.ps is not None:
            for a, p in self.root.ps.items():
                row[a] = p
        return row

    def counts(self):
        return (self.sims, self.predicts, self.terminal_hits)


def qbits(q: float) -> int:
    return int(np.float64(q).view(np.uint64))


def predictor(A, salt):
    return lambda s: gsu.stub(matrix_bytes_of(s.board_to_matrix()), int(s.side_to_play), A, salt)


def twin_search(orc, lg, states, wb, salts, noise_rows=None, epsilon=0.0, depth1_epsilon=0.0, games=None):
    """Per game of `games`: (kids, priors row, counts) of a twin search of S simulations; noise_rows [G, A]: that game's eta."""
    A = abi.action_size(lg.side_len)
    out = {}
    for g in (range(len(states)) if games is None else games):
        st = orc.GameState.from_abi(states[g], wb)
        noise = (epsilon, noise_rows[g]) if noise_rows is not None else None
        t = Twin(lg, st, CPUCT, predictor(A, salts[g]), noise, depth1_epsilon).run(S)
        out[g] = (t.kids(), t.priors(), t.counts())
    return out


def pin_twin(orc, lg, states, wb, salts, games):
    """epsilon == 0: the twin equals orc.GameLogic.gmcts exactly - visited children, visits, Qsa bits, root priors, counts."""
    A = abi.action_size(lg.side_len)
    got = twin_search(orc, lg, states, wb, salts, games=games)
    for g in games:
        st = orc.GameState.from_abi(states[g], wb)
        kids, ns, pri, cnt = lg.gmcts(st, S, CPUCT, predictor(A, salts[g]), wb)
        tk, tp, tc = got[g]
        assert tk == [(a, v, qbits(q)) for (_p, a, v, q) in kids], ("twin children", g)
        if st.to_abi().status == abi.ONGOING:
            assert tp.tobytes() == np.array(pri, np.float64).tobytes(), ("twin priors", g)
            assert sum(v for _a, v, _q in tk) == ns
        assert tc == tuple(cnt[:3]), ("twin counts", g, tc, cnt)


def twin_run(orc, lg, states, wb, salts, n_moves, sample_seed, temp_moves, move_base, base, eta_of, epsilon, games=None):
    """The loop of tafl_gselfplay_* on the twin (gselfplay_util.oracle_run with the twin as the search).  eta_of(states [G], M) -> rows
    [G, A]: eta for every game's state at move number M with gid = base + g (epsilon == 0: never called)."""
    G, n = len(states), lg.side_len
    A = abi.action_size(n)
    out = gsu.Run(G, n_moves)
    games = list(range(G) if games is None else games)
    cur = {g: orc.GameState.from_abi(states[g], wb) for g in games}
    live = set(games)
    for m in range(n_moves):
        live = {g for g in live if cur[g].to_abi().status == abi.ONGOING}
        if not live:
            break
        M = move_base + m
        rows = None
        if epsilon:
            now = (TaflState * G)(*[cur[g].to_abi() if g in cur else states[g] for g in range(G)])
            rows = eta_of(now, M)
        for g in sorted(live):
            st = cur[g]
            t = Twin(lg, st, CPUCT, predictor(A, salts[g]), (epsilon, rows[g]) if epsilon else None).run(S)
            out.sims += S
            kids = t.kids()
            vs = [v for _a, v, _q in kids]
            if not vs:
                live.discard(g)
                continue
            j = eu.pick_rule(vs, eu.sample_word(sample_seed, base + g, M)) if M < temp_moves else vs.index(max(vs))
            e = eu.Example()
            e.board, e.side = st.board_to_matrix(), st.to_abi().side_to_play
            e.actions, e.visits, e.played, e.move_no = [a for a, _v, _q in kids], vs, kids[j][0], M
            out.examples[g].append(e.fields())
            play = abi.action_decode(n, kids[j][0])
            code, cur[g], _eff = lg.do_play(play, st)
            assert code == 0, (g, m, code)
            out.plays[m][g] = pu.play_tuple4(play)
            out.moves[g] = m + 1
    for g in games:
        out.states[g] = bytes(cur[g].to_abi())
    return out


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
_SETUP = {}


def setup(orc, cfg):
    """(rules, n, wb, oracle logic, states [G_PLAIN + 2], salts): game g < G_PLAIN is the start position advanced by (7 g) mod 5 random
    plies; game G_PLAIN is over at the start; game G_PLAIN + 1 ends inside the run of check 2."""
    if cfg not in _SETUP:
        rules, fen, wb = pu.CONFIGS[cfg]
        n = abi.fen_side_len(fen)
        lg = orc.GameLogic(rules, n)
        plain = gsu.start_states(orc, lg, rules, fen, wb, G_PLAIN, 5)
        base = orc.GameState(fen, rules.starting_side, wb)
        over_plies, (end_id, end_plies) = CRAFTED[cfg]
        over = lg.random_advance(base, 77, 0, over_plies).to_abi()
        ending = lg.random_advance(base, 77, end_id, end_plies).to_abi()
        assert over.status != abi.ONGOING and ending.status == abi.ONGOING, cfg
        states = (TaflState * (G_PLAIN + 2))(*(list(plain) + [over, ending]))
        _SETUP[cfg] = (rules, n, wb, lg, states, [(3 * g + 1) % 256 for g in range(G_PLAIN + 2)])
    return _SETUP[cfg]


def noise_cfg(alpha=ALPHA, epsilon=EPSILON, seed=NOISE_SEED, base=0, move_no=0):
    return TaflRootNoise(alpha, epsilon, seed, base, move_no, 0, 0)


# ---- the host harness (tests/hostsim_noise) ----------------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_noise")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_noise.so"))
        P, u8, u32, u64, vp, dbl = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double
        L.hsn_begin.restype = vp
        L.hsn_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), u32, u32, u32, dbl, P(TaflRootNoise), P(TaflSelfplayOpts), u32, u64, vp]
        L.hsn_free.restype = None; L.hsn_free.argtypes = [vp]
        L.hsn_step.restype = u32; L.hsn_step.argtypes = [vp, P(C.c_float), P(C.c_float)]
        L.hsn_leaves.restype = None; L.hsn_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hsn_root_children.restype = None; L.hsn_root_children.argtypes = [vp, P(TaflRootChild), u32, P(u32)]
        L.hsn_root_priors.restype = None; L.hsn_root_priors.argtypes = [vp, P(dbl)]
        L.hsn_end.restype = None; L.hsn_end.argtypes = [vp, P(TaflState), P(TaflPlay), P(u32), P(u64), P(u8)]
        L.hsn_eta.restype = C.c_int; L.hsn_eta.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), u32, P(TaflRootNoise), P(dbl)]
        L.hsn_ex_new.restype = vp; L.hsn_ex_new.argtypes = [u32, u8, u32, u32]
        L.hsn_ex_free.restype = None; L.hsn_ex_free.argtypes = [vp]
        L.hsn_ex_counts.restype = None; L.hsn_ex_counts.argtypes = [vp, P(u32), P(u64)]
        L.hsn_ex_example.restype = C.c_int; L.hsn_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32)]
        _HLIB = L
    return _HLIB


def _kids_of(kids, cnt, G, cap):
    return [[(kids[g * cap + j].action, kids[g * cap + j].visits, qbits(kids[g * cap + j].q)) for j in range(cnt[g])] for g in range(G)]


class HostSide:
    """The checks' back end on the host harness."""
    name = "host"

    def __init__(self, rules, n, wb):
        self.rules, self.n, self.wb, self.A = rules.to_c(), n, wb, abi.action_size(n)

    def eta(self, states, cfg):
        G = len(states)
        out = np.zeros((G, self.A), np.float64)
        assert hlib().hsn_eta(C.byref(self.rules), self.n, self.wb, states, G, C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return out

    def _drive(self, h, G, salts):
        L = hlib()
        boards, sides, waiting = (C.c_uint8 * (G * self.n * self.n))(), (C.c_uint8 * G)(), (C.c_uint8 * G)()
        L.hsn_leaves(h, boards, sides, waiting)
        w = sum(waiting)
        while w:
            pri, val = gsu.stub_rows(boards, sides, waiting, G, self.n, self.A, salts)
            w = L.hsn_step(h, gsu.fptr(pri), gsu.fptr(val))
            L.hsn_leaves(h, boards, sides, waiting)
            assert sum(waiting) == w

    def search(self, states, salts, cfg):
        """(children per game, root priors [G, A], (sims, predicts, terminal hits, faults)) of a lock-step search; cfg None: no noise."""
        L, G = hlib(), len(states)
        h = L.hsn_begin(C.byref(self.rules), self.n, self.wb, states, G, S, EDGES, CPUCT, C.byref(cfg) if cfg is not None else None, None, 0, 0, None)
        assert h
        try:
            self._drive(h, G, salts)
            kids, cnt = (TaflRootChild * (G * 512))(), (C.c_uint32 * G)()
            L.hsn_root_children(h, kids, 512, cnt)
            pri = np.zeros((G, self.A), np.float64)
            L.hsn_root_priors(h, pri.ctypes.data_as(C.POINTER(C.c_double)))
            c4 = (C.c_uint64 * 4)()
            L.hsn_end(h, None, None, None, c4, None)
        finally:
            L.hsn_free(h)
        return _kids_of(kids, cnt, G, 512), pri, tuple(c4)

    def run(self, states, salts, cfg, n_moves, sample_seed, temp_moves, move_base, base):
        """A recording guided self-play run: gselfplay_util.Run with its examples."""
        L, G = hlib(), len(states)
        ex = L.hsn_ex_new(G, self.n, n_moves, S)
        o = TaflSelfplayOpts(sample_seed, temp_moves, move_base, 0)
        h = L.hsn_begin(C.byref(self.rules), self.n, self.wb, states, G, S, EDGES, CPUCT, C.byref(cfg) if cfg is not None else None, C.byref(o), n_moves, base, ex)
        assert h
        try:
            self._drive(h, G, salts)
            st, plays, moves, c4, faults = (TaflState * G)(), (TaflPlay * (G * n_moves))(), (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint8 * G)()
            L.hsn_end(h, st, plays, moves, c4, faults)
            out = gsu.Run(G, n_moves)
            out.plays = [[pu.play_tuple4(plays[m * G + g]) for g in range(G)] for m in range(n_moves)]
            out.states, out.moves, out.sims = [bytes(st[g]) for g in range(G)], list(moves), c4[0]
            assert not any(faults) and c4[3] == 0
            lens, ct = (C.c_uint32 * G)(), (C.c_uint64 * 4)()
            L.hsn_ex_counts(ex, lens, ct)
            assert ct[0] == 0 and ct[1] == 0
            for g in range(G):
                for j in range(lens[g]):
                    out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (self.n * self.n))()
                    acts, vis = (C.c_uint32 * S)(), (C.c_uint32 * S)()
                    assert L.hsn_ex_example(ex, j * G + g, out5, board, acts, vis) == 0 and out5[2] == 0
                    k = out5[0]
                    rows = [list(board[r * self.n:(r + 1) * self.n]) for r in range(self.n)]
                    out.examples[g].append((rows, out5[1], list(acts[:k]), list(vis[:k]), out5[3], out5[4]))
        finally:
            L.hsn_free(h)
            L.hsn_ex_free(ex)
        return out


class DeviceSide:
    """The checks' back end on the C-ABI (a GPU).  `glg`: a BatchedGameLogic."""
    name = "device"

    def __init__(self, glg, n):
        self.glg, self.n, self.A = glg, n, abi.action_size(n)

    def _batch(self, states):
        b = self.glg.new_batch(len(states))
        b.upload(states)
        return b

    def eta(self, states, cfg):
        b = self._batch(states)
        out = b.root_noise_eval(cfg.alpha, cfg.epsilon, cfg.seed, cfg.game_id_base, cfg.move_no)
        b.close()
        return np.frombuffer(out, np.float64).reshape(len(states), self.A).copy()

    def search_on(self, b, salts):
        G = b.n
        b.gmcts_begin(S, EDGES)
        w = b.gmcts_step(None, None, CPUCT, S)
        while w:
            boards, sides, waiting = b.gmcts_leaves()
            pri, val = gsu.stub_rows(boards, sides, waiting, G, self.n, self.A, salts)
            w = b.gmcts_step(gsu.fptr(pri), gsu.fptr(val), CPUCT, S)
        kids, cnt = b.gmcts_root_children(512)
        pri = np.frombuffer(b.gmcts_root_priors(), np.float64).reshape(G, self.A).copy()
        st = b.gmcts_stats()
        return _kids_of(kids, cnt, G, 512), pri, (st.sims, st.predicts, st.terminal_hits, st.faults)

    def search(self, states, salts, cfg):
        b = self._batch(states)
        if cfg is not None:
            b.set_root_noise(cfg.alpha, cfg.epsilon, cfg.seed, cfg.game_id_base, cfg.move_no)
        out = self.search_on(b, salts)
        b.close()
        return out

    def run(self, states, salts, cfg, n_moves, sample_seed, temp_moves, move_base, base):
        b = self._batch(states)
        if cfg is not None:
            b.set_root_noise(cfg.alpha, cfg.epsilon, cfg.seed, cfg.game_id_base, cfg.move_no)
        ex = self.glg.new_examples(len(states), n_moves, S)
        run, over, stats = gsu.device_run(b, ex, self.n, S, CPUCT, salts, n_moves, sample_seed, temp_moves, move_base=move_base, base=base, edges_per_node=EDGES)
        assert stats.faults == 0 and not any(any(o) for o in over)
        ex.close(); b.close()
        return run


# ---- the checks both sides run -------------------------------------------------------------------------------------------------------------
_ETA, _SEARCH, _TWIN, _RUN = {}, {}, {}, {}
RUN_MOVES, RUN_TEMP, RUN_BASE, RUN_IDS, RUN_SEED = 3, 1, 2, 1000, 5


def eta_rows(side, orc, cfg):
    key = (side.name, cfg)
    if key not in _ETA:
        _ETA[key] = side.eta(setup(orc, cfg)[4], noise_cfg())
    return _ETA[key]


def noisy_search(side, orc, cfg):
    key = (side.name, cfg)
    if key not in _SEARCH:
        _rules, _n, _wb, _lg, states, salts = setup(orc, cfg)
        _SEARCH[key] = side.search(states, salts, noise_cfg())
    return _SEARCH[key]


def noisy_twin(side, orc, cfg):
    key = (side.name, cfg)
    if key not in _TWIN:
        _rules, _n, wb, lg, states, salts = setup(orc, cfg)
        _TWIN[key] = twin_search(orc, lg, states, wb, salts, eta_rows(side, orc, cfg), EPSILON)
    return _TWIN[key]


def assert_search_equals_twin(got, want, P, eta, epsilon, states, where):
    """got = (children, priors, counts) of a side; want: the twin fed that side's eta; P: the noise-free twin's root priors per game."""
    kids, pri, cnt = got
    for g in range(len(states)):
        tk, tp, _tc = want[g]
        assert kids[g] == tk, (where, "children", g)
        assert pri[g].tobytes() == tp.tobytes(), (where, "priors", g)
        mixed = (1.0 - epsilon) * P[g] + epsilon * eta[g]                    # numpy float64: two multiplications and one addition (0 off the legal actions)
        assert pri[g].tobytes() == mixed.tobytes(), (where, "mix", g)
    assert cnt[:3] == tuple(sum(want[g][2][i] for g in want) for i in range(3)) and cnt[3] == 0, (where, cnt)


def check_lockstep(side, orc, cfg):
    """Check 1: root priors == (1 - eps) P + eps eta exactly with P from the twin; children and stats equal the twin for every game."""
    _rules, _n, wb, lg, states, salts = setup(orc, cfg)
    G = len(states)
    pin_twin(orc, lg, states, wb, salts, [0, 1, 2, 3, 4, G - 2, G - 1])
    plain = twin_search(orc, lg, states, wb, salts)
    P = [plain[g][1] for g in range(G)]
    assert_search_equals_twin(noisy_search(side, orc, cfg), noisy_twin(side, orc, cfg), P, eta_rows(side, orc, cfg), EPSILON, states, cfg)
    # the game that is over: no root, no noise
    kids, pri, _ = noisy_search(side, orc, cfg)
    assert kids[G_PLAIN] == [] and not pri[G_PLAIN].any() and not eta_rows(side, orc, cfg)[G_PLAIN].any()
    return P


def check_extremes(side, orc, cfg, P):
    """epsilon == 1 and alpha == 0.03, once each, on the first 20 games and the crafted ones."""
    _rules, _n, wb, lg, states, salts = setup(orc, cfg)
    pick = list(range(20)) + [G_PLAIN, G_PLAIN + 1]
    sub = (TaflState * len(pick))(*[states[g] for g in pick])
    ssalts = [salts[g] for g in pick]
    for alpha, eps in ((ALPHA, 1.0), (0.03, EPSILON)):
        ncfg = noise_cfg(alpha, eps, base=500)
        eta = side.eta(sub, ncfg)
        assert np.isfinite(eta).all()
        want = twin_search(orc, lg, sub, wb, ssalts, eta, eps)
        assert_search_equals_twin(side.search(sub, ssalts, ncfg), want, [P[g] for g in pick], eta, eps, sub, (cfg, alpha, eps))


def whole_run(side, orc, cfg):
    key = (side.name, cfg)
    if key not in _RUN:
        _rules, _n, _wb, _lg, states, salts = setup(orc, cfg)
        _RUN[key] = side.run(states, salts, noise_cfg(), RUN_MOVES, RUN_SEED, RUN_TEMP, RUN_BASE, RUN_IDS)
    return _RUN[key]


def check_selfplay(side, orc, cfg):
    """Check 2: plays, final states, move counts, every example field and the simulations equal the twin loop; both fates are met; two
    shards with their own game_id_base equal the whole batch."""
    _rules, _n, wb, lg, states, salts = setup(orc, cfg)
    G = len(states)
    got = whole_run(side, orc, cfg)
    want = twin_run(orc, lg, states, wb, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, RUN_BASE, RUN_IDS,
                    lambda now, M: side.eta(now, noise_cfg(base=RUN_IDS, move_no=M)), EPSILON)
    over0, ended, going = gsu.fates(states, want)
    assert over0 == [G_PLAIN] and G_PLAIN + 1 in ended and going, (cfg, over0, ended)
    gsu.assert_same_run(got, want, got.examples, where=cfg)
    assert got.sims == want.sims
    for first, count in ((0, 35), (35, G - 35)):
        part = side.run((TaflState * count)(*[states[first + g] for g in range(count)]), salts[first:first + count], noise_cfg(), RUN_MOVES, RUN_SEED, RUN_TEMP,
                        RUN_BASE, RUN_IDS + first)
        for g in range(count):
            assert [row[g] for row in part.plays] == [row[first + g] for row in got.plays], (cfg, first, g)
            assert part.moves[g] == got.moves[first + g] and part.states[g] == got.states[first + g], (cfg, first, g)
            assert part.examples[g] == got.examples[first + g], (cfg, first, g)


def check_only_the_root(side, orc, cfg):
    """Check 3: noise changes the root priors of every ongoing game, and nothing below the root: a twin that also mixes noise into the
    root's children no longer equals the side's search."""
    _rules, _n, wb, lg, states, salts = setup(orc, cfg)
    G = len(states)
    kids, pri, _ = noisy_search(side, orc, cfg)
    _k0, pri0, _ = side.search(states, salts, None)
    for g in range(G):
        assert (states[g].status != abi.ONGOING) == (pri[g].tobytes() == pri0[g].tobytes()), (cfg, g)
    games = list(range(12))
    mutant = twin_search(orc, lg, states, wb, salts, eta_rows(side, orc, cfg), EPSILON, depth1_epsilon=EPSILON, games=games)
    broken = [g for g in games if mutant[g][0] != kids[g]]
    assert broken, cfg
    return len(broken), len(games)


def check_eta_properties(side, orc, cfg):
    """Check 4."""
    _rules, n, wb, lg, states, _salts = setup(orc, cfg)
    G = len(states)
    eta = eta_rows(side, orc, cfg)
    assert np.isfinite(eta).all() and (eta >= 0).all()
    for g in range(G):
        st = orc.GameState.from_abi(states[g], wb)
        legal = sorted(abi.action_encode(n, p) for p in lg.all_plays(st)) if states[g].status == abi.ONGOING else []
        off = np.ones(eta.shape[1], bool)
        off[legal] = False
        assert not eta[g][off].any(), (cfg, g)
        if legal:
            assert abs(math.fsum(eta[g][legal]) - 1.0) <= len(legal) * 2.0 ** -52, (cfg, g)
        else:
            assert not eta[g].any()
    assert side.eta(states, noise_cfg()).tobytes() == eta.tobytes()                                   # a second call
    for g in (0, 7, 64, G - 1):                                                                       # alone, under its own id
        one = side.eta((TaflState * 1)(states[g]), noise_cfg(base=g))
        assert one[0].tobytes() == eta[g].tobytes(), (cfg, g)
    live = [g for g in range(G) if states[g].status == abi.ONGOING]
    for other in (noise_cfg(seed=NOISE_SEED + 1), noise_cfg(move_no=1), noise_cfg(base=1)):
        changed = side.eta(states, other)
        assert all(changed[g].tobytes() != eta[g].tobytes() for g in live), cfg
    # games 0 and 5 hold the start position ((7 g) mod 5 == 0)
    assert bytes(states[0]) == bytes(states[5]) and eta[0].tobytes() != eta[5].tobytes()


def ks_distance(a, b):
    a, b = np.sort(a), np.sort(b)
    allv = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, allv, side="right") / a.size - np.searchsorted(b, allv, side="right") / b.size)))


def check_eta_distribution(side, orc, cfg, alpha, ks):
    """Check 5: 4096 games at the start position against numpy's own Dirichlet sampler (a fixed seed) and the closed form of E sum eta^2."""
    rules, fen, wb = pu.CONFIGS[cfg]
    N = 4096
    st = orc.GameState(fen, rules.starting_side, wb).to_abi()
    eta = side.eta((TaflState * N)(*([st] * N)), noise_cfg(alpha=alpha, seed=99))
    n_side = abi.fen_side_len(fen)
    legal = np.array(sorted(abi.action_encode(n_side, p) for p in orc.GameLogic(rules, n_side).all_plays(orc.GameState(fen, rules.starting_side, wb))))
    off = np.ones(eta.shape[1], bool)
    off[legal] = False
    assert not eta[:, off].any() and np.isfinite(eta).all() and (eta >= 0).all()
    n = int(legal.size)
    rows = eta[:, legal]
    T = (rows * rows).sum(axis=1)
    ref = np.random.default_rng(20240614).dirichlet([alpha] * n, N)
    Tr = (ref * ref).sum(axis=1)
    se, ser = T.std(ddof=1) / math.sqrt(N), Tr.std(ddof=1) / math.sqrt(N)
    z_ref = (T.mean() - Tr.mean()) / math.hypot(se, ser)
    z_closed = (T.mean() - (alpha + 1.0) / (n * alpha + 1.0)) / se
    print(f"{side.name} {cfg} alpha={alpha}: n={n} mean T={T.mean():.6f} numpy={Tr.mean():.6f} closed={(alpha + 1.0) / (n * alpha + 1.0):.6f} z_ref={z_ref:.2f} z_closed={z_closed:.2f}")
    assert abs(z_ref) <= 5.0 and abs(z_closed) <= 5.0, (cfg, alpha, z_ref, z_closed)
    if ks:
        d = ks_distance(rows[:, 0], ref[:, 0])
        print(f"  KS distance at the first legal action: {d:.4f}")
        assert d < 1.95 * math.sqrt(2.0 / N), (cfg, alpha, d)
    return n
