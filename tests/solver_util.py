"""Expected values and drivers for exact win/loss proofs in guided self-play (include/taflhip.h tafl_solver).  The
expectation is a Python restatement on tests/noise_util.Twin (which pin_twin pins against orc.GameLogic.gmcts): SolverTwin applies rules
1-5 (with a k it also forces at the root, as forced_util.ForcedTwin), prune applies rule 6 and then forced_util.prune to what is left,
twin_run is the loop of tafl_gselfplay_* that draws from and records n'.  The coverage conditions are asserted on the expectation, never
on the code under test.

Two drivers run the same loop: host_solver (tests/hostsim_solver: selfplay_step_solver compiled for the CPU) and device_solver (the C-ABI
on a GPU).  A lane whose salt is None is fed the flat predictor (priors all 1.0f, value 0) instead of the stub network."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflForcedPlayouts, TaflPlay, TaflPlayoutCap, TaflRootChild, TaflRootNoise, TaflSelfplayOpts, TaflSolver, TaflState
from tests import episodes_util as epu
from tests import examples_util as eu
from tests import forced_util as fu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import parity_util as pu
from tests import playout_cap_util as pcu

S, CPUCT, EDGES = nu.S, nu.CPUCT, nu.EDGES
NONE, WON, LOST = 0, 1, 2
LOSING, WINNING = 1, 2
IDS, BACK = 18, 4                       # the endgame set: 18 random Brandubh games, their last four plies
G = IDS * BACK
SPOTS = (0, 3, 7, 12, 21, 33, 46, 63, 64, 71)
FLOORS = {"roots won": 6, "ended early": 5, "unproven with a losing move": 6, "nodes won": 15, "differ": 10}
STATS = ("root_won", "root_lost", "skipped_sims", "nodes_won", "nodes_lost", "pruned_visits", "pruned_children", "moves")
# the crafted positions of the issue: (layout, FEN, side to move, S)
CRAFTED = [("brandubh7", "7/7/7/K6/7/7/t5T", abi.ATTACKER, 64),
           ("brandubh7", "3K3/7/7/7/7/7/3t3", abi.ATTACKER, 64),
           ("brandubh7", "7/7/1K5/7/7/6t/7", abi.DEFENDER, 256),
           ("copenhagen11", "11/11/11/11/11/11/K10/11/11/11/t9T", abi.ATTACKER, 128),
           ("copenhagen13", "13/13/13/13/13/13/13/K12/13/13/13/13/t11T", abi.ATTACKER, 128)]


# ---- the expectation ---------------------------------------------------------------------------------------------------------------------
class _SNode(nu._Node):
    __slots__ = ("proof", "mark")

    def __init__(self, st):
        super().__init__(st)
        self.proof, self.mark = NONE, {}


class SolverTwin(nu.Twin):
    """nu.Twin with rules 1-5 of tafl_solver; k (None: no forcing) adds rule 1 of tafl_forced_playouts at the root."""

    def __init__(self, lg, state, c_puct, predict, noise=None, k=None):
        super().__init__(lg, state, c_puct, predict, noise)
        self.root = _SNode(state)
        self.k, self.forced, self.skipped, self.nodes_won, self.nodes_lost = k, 0, 0, 0, 0

    def run(self, n_sims, done=0):
        """`done`: the simulations a fast move of a capped run starts from (n_sims - fast_sims)."""
        for i in range(done, n_sims):
            if self.root.proof != NONE:                                   # rule 5
                self.skipped += n_sims - i
                break
            self.search(self.root, 0)
            self.sims += 1
        return self

    def search(self, nd, depth):
        if nd.es is None:
            nd.es = nu.game_ended(nd.st.to_abi())
            if nd.es == 1.0 or nd.es == -1.0:                             # rule 1 (a draw is 1e-4 and proves nothing)
                nd.proof = WON if nd.es == 1.0 else LOST
        if nd.es != 0:
            self.terminal_hits += 1
            return -nd.es
        if nd.ps is None:
            return self.expand(nd, depth)
        assert nd.proof == NONE, "a proven node is never descended into"
        self.depth_sum += 1
        cur_best, best = -math.inf, -1
        sq, sq0 = math.sqrt(float(nd.ns)), math.sqrt(float(nd.ns) + nu.MCTS_EPS)
        for a in nd.acts:
            if a in nd.q:
                u = nd.q[a] + self.c_puct * nd.ps[a] * sq / float(1 + nd.n[a])
                if self.k is not None and depth == 0 and float(nd.n[a]) * float(nd.n[a]) < (self.k * nd.ps[a]) * float(nd.ns):
                    u = math.inf
            else:
                u = self.c_puct * nd.ps[a] * sq0
            if nd.mark.get(a) == LOSING:                                  # rule 4
                continue
            if u > cur_best:
                cur_best, best = u, a
        a = best
        assert a >= 0, "a node without a proof has a move that is not a losing move"
        if self.k is not None and depth == 0 and cur_best == math.inf:
            self.forced += 1
        if a not in nd.child:
            code, nxt, _eff = self.lg.do_play(abi.action_decode(self.n, a), nd.st)
            assert code == 0, code
            nd.child[a] = _SNode(nxt)
        ch = nd.child[a]
        v = self.search(ch, depth + 1)
        if a in nd.q:
            nd.q[a] = (float(nd.n[a]) * nd.q[a] + v) / float(nd.n[a] + 1)
            nd.n[a] += 1
        else:
            nd.q[a], nd.n[a] = v, 1
        nd.ns += 1
        if ch.proof != NONE:                                              # rules 2 and 3
            nd.mark[a] = LOSING if ch.proof == WON else WINNING
            if ch.proof == LOST:
                nd.proof = WON
            elif all(nd.mark.get(b) == LOSING for b in nd.acts):
                nd.proof = LOST
            if nd.proof != NONE and depth > 0:
                if nd.proof == WON:
                    self.nodes_won += 1
                else:
                    self.nodes_lost += 1
        return -v

    def depth1_lost(self):
        """Non-terminal children of the root that rule 3 proved LOST."""
        return sum(1 for c in self.root.child.values() if c.proof == LOST and c.es == 0)


class _Root:
    """What forced_util.prune reads of a root, with the counts rule 6 left."""

    def __init__(self, root, kept):
        self.acts, self.ps, self.ns = root.acts, root.ps, root.ns
        self.q = {a: root.q[a] for a in kept}
        self.n = dict(kept)


def prune(root, c_puct, k=None):
    """Rule 6 on a finished root, then (k not None) rule 2 of tafl_forced_playouts on what is left: ([(action, n, n', Qsa bits)] of the
    edges the search visited, ascending; visits and children rule 6 took; visits and children the forced pruning took)."""
    acts = [a for a in (root.acts or []) if a in root.q]
    n1 = {a: root.n[a] for a in acts}
    if root.proof == WON:
        w = next(a for a in root.acts if root.mark.get(a) == WINNING)
        n1 = {a: (root.n[a] if a == w else 0) for a in acts}
    elif any(root.mark.get(a) != LOSING for a in acts):
        n1 = {a: (0 if root.mark.get(a) == LOSING else root.n[a]) for a in acts}
    sv = (sum(root.n[a] - n1[a] for a in acts), sum(n1[a] == 0 for a in acts))
    n2, fp = dict(n1), (0, 0)
    if k is not None:
        rows = fu.prune(_Root(root, {a: v for a, v in n1.items() if v > 0}), c_puct, k)
        for a, n, m, _F, _q, _b in rows:
            n2[a] = m
        fp = (sum(r[1] - r[2] for r in rows), sum(r[2] == 0 for r in rows))
    return [(a, root.n[a], n2[a], nu.qbits(root.q[a])) for a in acts], sv, fp


class Tally:
    """What tafl_gselfplay_solver_stats counts (STATS order), and the forced-playouts counters of a composition."""

    def __init__(self):
        for name in STATS:
            setattr(self, name, 0)
        self.forced_sims = self.fp_pruned_visits = self.fp_pruned_children = self.fp_full_moves = 0
        self.won_inside_temp = 0

    def stats(self):
        return tuple(getattr(self, name) for name in STATS)

    def fp_stats(self):
        return (self.forced_sims, self.fp_pruned_visits, self.fp_pruned_children, self.fp_full_moves)


def predictor(A, salt):
    if salt is None:
        flat = np.ones(A, np.float32)
        return lambda s: (flat, 0.0)
    return nu.predictor(A, salt)


def one_move(lg, st, predict, gid, M, sample_seed, temp_moves, tally, n_sims=S, k=None, noise=None, done=0):
    """One search with the setting from the oracle state `st`, pruned, and its pick: (the twin, rows of `prune`, index of the played row
    among the rows with n' > 0 or None when no edge was visited).  `k`: the move is a full move of a run with forced playouts."""
    t = SolverTwin(lg, st, CPUCT, predict, noise, k).run(n_sims, done)
    rows, sv, fp = prune(t.root, CPUCT, k)
    tally.root_won += t.root.proof == WON
    tally.root_lost += t.root.proof == LOST
    tally.skipped_sims += t.skipped
    tally.nodes_won += t.nodes_won
    tally.nodes_lost += t.nodes_lost
    tally.forced_sims += t.forced
    if t.root.ps is not None:
        tally.pruned_visits += sv[0]
        tally.pruned_children += sv[1]
        tally.fp_pruned_visits += fp[0]
        tally.fp_pruned_children += fp[1]
    kept = [r for r in rows if r[2] > 0]
    if not kept:
        return t, rows, None
    vs = [r[2] for r in kept]
    if M < temp_moves:
        j = eu.pick_rule(vs, eu.sample_word(sample_seed, gid, M))
        tally.won_inside_temp += t.root.proof == WON
    else:
        j = vs.index(max(vs))
    tally.moves += 1
    tally.fp_full_moves += k is not None
    return t, rows, j


def example_of(st, kept, j, M):
    e = eu.Example()
    e.board, e.side = st.board_to_matrix(), st.to_abi().side_to_play
    e.actions, e.visits, e.played, e.move_no = [r[0] for r in kept], [r[2] for r in kept], kept[j][0], M
    return e.fields()


def twin_run(orc, lg, states, wb, salts, n_moves, sample_seed, temp_moves, move_base, base, sims, games=None, k=None, eta_of=None, epsilon=0.0):
    """forced_util.twin_run with the solver twin at `sims` simulations per move (.sims counts those that ran).  Returns
    (gselfplay_util.Run with .budget = the sum of the per-move budgets, Tally)."""
    n_games, n = len(states), lg.side_len
    A = abi.action_size(n)
    out, tally = gsu.Run(n_games, n_moves), Tally()
    out.budget = 0
    games = list(range(n_games) if games is None else games)
    cur = {g: orc.GameState.from_abi(states[g], wb) for g in games}
    live = set(games)
    for m in range(n_moves):
        live = {g for g in live if cur[g].to_abi().status == abi.ONGOING}
        if not live:
            break
        M = move_base + m
        rows_eta = None
        if epsilon:
            now = (TaflState * n_games)(*[cur[g].to_abi() if g in cur else states[g] for g in range(n_games)])
            rows_eta = eta_of(now, M)
        for g in sorted(live):
            st = cur[g]
            t, rows, j = one_move(lg, st, predictor(A, salts[g]), base + g, M, sample_seed, temp_moves, tally, sims, k, (epsilon, rows_eta[g]) if epsilon else None)
            out.sims += t.sims
            out.budget += sims
            if j is None:
                live.discard(g)
                continue
            kept = [r for r in rows if r[2] > 0]
            out.examples[g].append(example_of(st, kept, j, M))
            play = abi.action_decode(n, kept[j][0])
            code, cur[g], _eff = lg.do_play(play, st)
            assert code == 0, (g, m, code)
            out.plays[m][g] = pu.play_tuple4(play)
            out.moves[g] = m + 1
    for g in games:
        out.states[g] = bytes(cur[g].to_abi())
    return out, tally


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
_ENDGAME, _CRAFTED, _SEARCH = {}, {}, {}


def endgame(orc):
    """(rules, n, wb, oracle logic, states [72], salts): lane 4 id + back - 1 is random game id of Brandubh, `back` plies before its end."""
    if "set" not in _ENDGAME:
        rules, fen, wb = pu.CONFIGS["brandubh7"]
        n = abi.fen_side_len(fen)
        lg = orc.GameLogic(rules, n)
        start = orc.GameState(fen, rules.starting_side, wb)
        states = []
        for gid in range(IDS):
            L = next(p for p in range(1, 4000) if lg.random_advance(start, 77, gid, p).to_abi().status != abi.ONGOING)
            assert L > BACK, (gid, L)
            states += [lg.random_advance(start, 77, gid, L - back).to_abi() for back in range(1, BACK + 1)]
        assert all(s.status == abi.ONGOING for s in states)
        _ENDGAME["set"] = (rules, n, wb, lg, (TaflState * G)(*states), [(3 * gid + 1) % 256 for gid in range(IDS) for _ in range(BACK)])
    return _ENDGAME["set"]


def crafted(orc, cfg):
    """(rules, n, wb, oracle logic, states [8], salts (all None: the flat predictor), S per lane): the issue's positions of the layout, on
    the larger boards also their defender-to-move twin (a win in one), repeated to fill 8 lanes."""
    if cfg not in _CRAFTED:
        rules, fen0, wb = pu.CONFIGS[cfg]
        n = abi.fen_side_len(fen0)
        lg = orc.GameLogic(rules, n)
        mine = [(orc.GameState(fen, side, wb).to_abi(), s) for c, fen, side, s in CRAFTED if c == cfg]
        if cfg != "brandubh7":
            mine += [(orc.GameState(fen, abi.DEFENDER, wb).to_abi(), s) for c, fen, _side, s in CRAFTED if c == cfg]
        assert all(st.status == abi.ONGOING for st, _s in mine), cfg
        lanes = [mine[i % len(mine)] for i in range(8)]
        _CRAFTED[cfg] = (rules, n, wb, lg, (TaflState * 8)(*[st for st, _s in lanes]), [None] * 8, [s for _st, s in lanes])
    return _CRAFTED[cfg]


def searches(orc, key, lg, states, wb, salts, sims, games=None):
    """One search of every game of `games` (default: all): {g: (the solver twin, pruned rows, a Tally of this search alone, the plain
    twin's kids)}, remembered per (key, game, sims)."""
    A = abi.action_size(lg.side_len)
    out = {}
    for g in (range(len(states)) if games is None else games):
        s = sims[g] if isinstance(sims, (list, tuple)) else sims
        kk = (key, g, s)
        if kk not in _SEARCH:
            st = orc.GameState.from_abi(states[g], wb)
            tally = Tally()
            t, rows, j = one_move(lg, st, predictor(A, salts[g]), 0, 0, 0, 0, tally, s)
            u = nu.Twin(lg, st, CPUCT, predictor(A, salts[g])).run(s)
            _SEARCH[kk] = (t, rows, tally, u.kids(), j)
        out[g] = _SEARCH[kk]
    return out


def coverage(found):
    """The five conditions of the issue's table over `found` (what `searches` returns)."""
    c = dict.fromkeys(FLOORS, 0)
    for t, _rows, tally, plain, _j in found.values():
        c["roots won"] += t.root.proof == WON
        c["ended early"] += t.skipped > 0
        c["unproven with a losing move"] += t.root.proof == NONE and LOSING in t.root.mark.values()
        c["nodes won"] += tally.nodes_won
        c["differ"] += t.kids() != plain
    return c


# ---- the host harness (tests/hostsim_solver) -------------------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_solver")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_solver.so"))
        P, u8, u32, u64, vp, dbl = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double
        L.hss_solver_check.restype = C.c_int; L.hss_solver_check.argtypes = [P(TaflSolver)]
        L.hss_sizes.restype = None; L.hss_sizes.argtypes = [P(u32)]
        L.hss_begin.restype = vp
        L.hss_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), P(TaflState), u32, u32, u32, dbl, P(TaflRootNoise), P(TaflPlayoutCap), P(TaflForcedPlayouts),
                                P(TaflSolver), P(TaflSelfplayOpts), u32, u64, C.c_int, u64, u32, vp]
        L.hss_free.restype = None; L.hss_free.argtypes = [vp]
        L.hss_step.restype = u32; L.hss_step.argtypes = [vp, P(C.c_float), P(C.c_float)]
        L.hss_leaves.restype = None; L.hss_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hss_root_children.restype = None; L.hss_root_children.argtypes = [vp, P(TaflRootChild), u32, P(u32)]
        L.hss_end.restype = None; L.hss_end.argtypes = [vp, P(TaflState), P(TaflPlay), P(u32), P(u64), P(u8), P(u32), P(u64), P(u64), P(u64), P(u64)]
        L.hss_ex_new.restype = vp; L.hss_ex_new.argtypes = [u32, u8, u32, u32]
        L.hss_ex_free.restype = None; L.hss_ex_free.argtypes = [vp]
        L.hss_ex_counts.restype = None; L.hss_ex_counts.argtypes = [vp, P(u32), P(u64), P(u32)]
        L.hss_ex_example.restype = C.c_int; L.hss_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32), P(C.c_float), P(u8)]
        _HLIB = L
    return _HLIB


class HostExamples(fu.HostExamples):
    """forced_util.HostExamples on this harness's buffer (the same ExEp)."""

    def __init__(self, n, n_lanes, max_moves, max_children):
        self.n, self.G, self.max_moves, self.K = n, n_lanes, max_moves, max_children
        self.h = hlib().hss_ex_new(n_lanes, n, max_moves, max_children)

    def __del__(self):
        if getattr(self, "h", None):
            hlib().hss_ex_free(self.h)
            self.h = None

    def counts(self):
        ln, ct, of = (C.c_uint32 * self.G)(), (C.c_uint64 * 4)(), (C.c_uint32 * self.G)()
        hlib().hss_ex_counts(self.h, ln, ct, of)
        return list(ln), {"dropped": ct[0], "overflowed": ct[1]}, list(of)

    def all(self):
        lens, _, _ = self.counts()
        out = [[] for _ in range(self.G)]
        for g in range(self.G):
            for j in range(min(lens[g], self.max_moves)):
                out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (self.n * self.n))()
                acts, vis, z, fin = (C.c_uint32 * self.K)(), (C.c_uint32 * self.K)(), C.c_float(), C.c_uint8()
                assert hlib().hss_ex_example(self.h, j * self.G + g, out5, board, acts, vis, C.byref(z), C.byref(fin)) == 0, (j, g)
                assert out5[2] == 0, ("overflow", j, g)
                k = out5[0]
                rows = [list(board[r * self.n:(r + 1) * self.n]) for r in range(self.n)]
                out[g].append(((rows, out5[1], list(acts[:k]), list(vis[:k]), out5[3], out5[4]), float(z.value), int(fin.value)))
        return out


def net_rows(boards, sides, waiting, n_lanes, n, A, salts):
    """gselfplay_util.stub_rows, with the flat predictor for the lanes whose salt is None."""
    pri, val = gsu.stub_rows(boards, sides, [w and salts[g] is not None for g, w in enumerate(waiting)], n_lanes, n, A, [s or 0 for s in salts])
    for g in range(n_lanes):
        if waiting[g] and salts[g] is None:
            pri[g] = 1.0
    return pri, val


def host_solver(rules, n, wb, states, salts, n_moves, sample_seed, temp_moves, n_sims=S, solver=True, k=None, cap=None, ex=None, episodes=False, base=0, stride=0,
                episode_moves=0, move_base=0, noise=None, kids=False, read_examples=True):
    """forced_util.host_forced on tests/hostsim_solver with the solver setting latched (`solver` False: the run tests/hostsim_forced
    makes): epu.Lanes with .moves, .cap_stats, .fp_stats, .sv_stats (the eight counters in STATS order), .faults, .stat_faults, .kids."""
    L = hlib()
    n_lanes, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(sample_seed, temp_moves, move_base, 0)
    fc = fu.forced_cfg(k) if k is not None else None
    sc = TaflSolver(0) if solver else None
    h = L.hss_begin(C.byref(rc), n, wb, states, None, n_lanes, n_sims, EDGES, CPUCT, C.byref(noise) if noise is not None else None, C.byref(cap) if cap is not None else None,
                    C.byref(fc) if fc is not None else None, C.byref(sc) if sc is not None else None, C.byref(o), n_moves, base, 1 if episodes else 0, stride, episode_moves,
                    ex.h if ex is not None else None)
    assert h
    try:
        boards, sides, waiting = (C.c_uint8 * (n_lanes * n * n))(), (C.c_uint8 * n_lanes)(), (C.c_uint8 * n_lanes)()
        L.hss_leaves(h, boards, sides, waiting)
        w = sum(waiting)
        while w:
            pri, val = net_rows(boards, sides, waiting, n_lanes, n, A, salts)
            w = L.hss_step(h, gsu.fptr(pri), gsu.fptr(val))
            L.hss_leaves(h, boards, sides, waiting)
            assert sum(waiting) == w
        st, plays, moves, c4, faults = (TaflState * n_lanes)(), (TaflPlay * (n_lanes * n_moves))(), (C.c_uint32 * n_lanes)(), (C.c_uint64 * 4)(), (C.c_uint8 * n_lanes)()
        eps, ec, cc, f4, s8 = (C.c_uint32 * n_lanes)(), (C.c_uint64 * 4)(), (C.c_uint64 * 2)(), (C.c_uint64 * 4)(), (C.c_uint64 * 8)()
        L.hss_end(h, st, plays, moves, c4, faults, eps, ec, cc, f4, s8)
        found = None
        if kids:
            rk, cnt = (TaflRootChild * (n_lanes * 512))(), (C.c_uint32 * n_lanes)()
            L.hss_root_children(h, rk, 512, cnt)
            found = nu._kids_of(rk, cnt, n_lanes, 512)
    finally:
        L.hss_free(h)
    examples = ex.all() if ex is not None and read_examples else [[] for _ in range(n_lanes)]
    out = epu.lanes_of(n_lanes, n_moves, plays, list(moves), st, eps, ec, c4[0], c4[1], examples)
    out.moves, out.cap_stats, out.fp_stats, out.sv_stats, out.faults, out.stat_faults, out.kids = list(moves), (cc[0], cc[1]), tuple(f4), tuple(s8), list(faults), c4[3], found
    if ex is not None:
        out.open_from = ex.counts()[2]
    return out if episodes else pcu._plain(out)


# ---- the library -----------------------------------------------------------------------------------------------------------------------------
def device_solver(batch, ex, n, salts, n_moves, sample_seed, temp_moves, n_sims=S, solver=True, k=None, cap=None, episodes=False, base=0, stride=0, episode_moves=0,
                  move_base=0, noise=None, on_round=None):
    """The same loop through the C-ABI on `batch` (states uploaded), the network in host buffers: epu.Lanes as host_solver returns them
    (.sv_stats None without the setting, .fp_stats None without k, .cap_stats None without a cap).  on_round(batch, round number) is
    called before every step that delivers evaluations."""
    n_lanes, A = batch.n, abi.action_size(n)
    epu.set_noise(batch, noise)
    pcu.set_cap(batch, cap)
    if k is None:
        batch.clear_forced_playouts()
    else:
        batch.set_forced_playouts(k)
    if solver:
        batch.set_solver()
    else:
        batch.clear_solver()
    if episodes:
        batch.gselfplay_begin_episodes(ex, n_moves, n_sims, CPUCT, EDGES, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves, episode_moves=episode_moves,
                                       id_stride=stride)
    else:
        batch.gselfplay_begin(ex, n_moves, n_sims, CPUCT, EDGES, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves, move_base=move_base)
    w, rounds = batch.gselfplay_step(), 0
    while w:
        boards, sides, waiting = batch.gmcts_leaves()
        assert sum(waiting) == w
        pri, val = net_rows(boards, sides, waiting, n_lanes, n, A, salts)
        if on_round is not None:
            on_round(batch, rounds)
        w = batch.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        rounds += 1
    plays, moves = batch.gselfplay_end()
    stats = batch.gmcts_stats()
    if episodes:
        eps, es = batch.gselfplay_episode_stats()
        counters = (es.attacker_wins, es.defender_wins, es.draws, es.cut)
    else:
        eps, counters = [0] * n_lanes, (0, 0, 0, 0)
    examples, over = epu.device_examples(ex, n_lanes, n) if ex is not None else ([[] for _ in range(n_lanes)], None)
    assert over is None or not any(any(o) for o in over)
    out = epu.lanes_of(n_lanes, n_moves, plays, list(moves), batch.download(), eps, counters, stats.sims, stats.predicts, examples)
    cs = batch.playout_cap_stats() if cap is not None else None
    fs = batch.forced_playouts_stats() if k is not None else None
    ss = batch.solver_stats() if solver else None
    out.moves, out.stat_faults, out.rounds = list(moves), stats.faults, rounds
    out.cap_stats = (cs.full_moves, cs.fast_moves) if cs else None
    out.fp_stats = (fs.forced_sims, fs.pruned_visits, fs.pruned_children, fs.full_moves) if fs else None
    out.sv_stats = tuple(getattr(ss, name) for name in STATS) if ss else None
    return out if episodes else pcu._plain(out)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------
def assert_same_lanes(got, want, where=""):
    """Two drivers' Lanes (the device's against the harness's): everything they both leave."""
    epu.assert_same(got, want, where)
    assert got.moves == want.moves and got.sv_stats == want.sv_stats, (where, got.sv_stats, want.sv_stats)
    if want.fp_stats is not None and got.fp_stats is not None:
        assert got.fp_stats == want.fp_stats, (where, got.fp_stats, want.fp_stats)
    if want.cap_stats is not None and got.cap_stats is not None:
        assert got.cap_stats == want.cap_stats, (where, got.cap_stats, want.cap_stats)


def assert_search_equals_twin(got, found, games, where=""):
    """A one-move run's Lanes (with .kids and one example per lane) against `searches`: the pruned root block and the example."""
    for g in games:
        _t, rows, _tally, _plain, j = found[g]
        kept = [(a, m, q) for a, _n, m, q in rows if m > 0]
        assert got.kids[g] == kept, (where, "children", g, got.kids[g], kept)
        if kept:
            (fields, _z, _fin), = got.examples[g]
            assert (fields[2], fields[3]) == ([a for a, _m, _q in kept], [m for _a, m, _q in kept]), (where, "example", g)
            assert fields[4] == kept[j][0], (where, "played", g)
        else:
            assert got.examples[g] == [] and got.moves[g] == 0, (where, g)


def capped_composition(orc, side, full_per, noise, k, lanes=None, base=epu.IDS, budget=6, fast=fu.FAST):
    """The expectation for an episodes run of the endgame set with the cap (forced_util.CAP_SEED, fast, full_per), the run's noise and
    forced playouts k, all with the setting: playout_cap_util.composition in which a full move is one solver twin move with forcing (fed
    `side`'s eta) and a fast move one solver twin move of `fast` simulations without noise or forcing.  Returns (Lanes, Tally)."""
    rules, n, wb, lg, states, salts = endgame(orc)
    A, n_lanes = abi.action_size(n), len(states)
    over = lg.random_advance(orc.GameState(pu.CONFIGS["brandubh7"][1], rules.starting_side, wb), 77, 0, 400).to_abi()
    assert over.status != abi.ONGOING
    tally = Tally()

    def route(batch, live, full, gb, M):
        run = gsu.Run(n_lanes, 1)
        for g in range(n_lanes):
            run.states[g] = bytes(batch[g])
        eta = side.eta(batch, nu.noise_cfg(base=gb, move_no=M)) if noise and full else None
        sims = 0
        for g in live:
            st = orc.GameState.from_abi(batch[g], wb)
            t, rows, j = one_move(lg, st, predictor(A, salts[g]), gb + g, M, pcu.SSEED, pcu.TEMP, tally, S, k if full else None,
                                  (nu.EPSILON, eta[g]) if eta is not None else None, 0 if full else S - fast)
            sims += t.sims
            if j is None:
                continue
            kept = [r for r in rows if r[2] > 0]
            if full:
                run.examples[g].append(example_of(st, kept, j, M))
            play = abi.action_decode(n, kept[j][0])
            code, nxt, _eff = lg.do_play(play, st)
            assert code == 0
            run.plays[0][g], run.moves[g], run.states[g] = pu.play_tuple4(play), 1, bytes(nxt.to_abi())
        return run, sims, None

    start = states if lanes is None else (TaflState * n_lanes)(*[states[g] if g in lanes else over for g in range(n_lanes)])
    want = pcu.composition(route, start, over, budget, fu.CAP_SEED, full_per, True, base=base, stride=n_lanes, openings=start)
    return want, tally
