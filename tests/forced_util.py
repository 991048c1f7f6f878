"""Expected values and drivers for forced playouts with policy target pruning in guided self-play (include/taflhip.h
tafl_forced_playouts).  The expectation is a Python restatement on tests/noise_util.Twin (which pin_twin pins
against orc.GameLogic.gmcts): ForcedTwin applies rule 1 in its root selection, prune applies rule 2 to the finished root, twin_run is the
loop of tafl_gselfplay_* that draws from and records n'.  A capped episodes run is playout_cap_util.composition with the forced twin as
the route of the full moves.  The coverage conditions are asserted on the expectation, never on the code under test.

Two drivers run the same loop: host_forced (tests/hostsim_forced: selfplay_step_forced compiled for the CPU) and device_forced (the
C-ABI on a GPU)."""
import ctypes as C
import math
import os
import subprocess

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflForcedPlayouts, TaflPlay, TaflPlayoutCap, TaflRootChild, TaflRootNoise, TaflSelfplayOpts, TaflState
from tests import episodes_util as epu
from tests import examples_util as eu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import parity_util as pu
from tests import playout_cap_util as pcu

K = 2.0
S, CPUCT, EDGES = nu.S, nu.CPUCT, nu.EDGES
LAYOUTS = nu.LAYOUTS
G = nu.G_PLAIN + 2
SPOTS = (0, 1, 2, 33, 63, 64, 65, 69, nu.G_PLAIN, nu.G_PLAIN + 1)      # both waves, and the two crafted games
FAST, CAP_SEED = 6, 3
FLOORS = {"differ": 20, "forced": 100, "zeroed": 20, "partial": 20, "blocked": 20, "full subtraction": 20}


# ---- the expectation ---------------------------------------------------------------------------------------------------------------------
class ForcedTwin(nu.Twin):
    """nu.Twin whose selection at the root applies rule 1: a visited edge with n * n < (k * p) * Ns scores +inf."""

    def __init__(self, lg, state, c_puct, predict, k, noise=None):
        super().__init__(lg, state, c_puct, predict, noise)
        self.k, self.forced = k, 0

    def search(self, nd, depth):
        if nd.es is None:
            nd.es = nu.game_ended(nd.st.to_abi())
        if nd.es != 0:
            self.terminal_hits += 1
            return -nd.es
        if nd.ps is None:
            return self.expand(nd, depth)
        self.depth_sum += 1
        cur_best, best = -math.inf, -1
        sq, sq0 = math.sqrt(float(nd.ns)), math.sqrt(float(nd.ns) + nu.MCTS_EPS)
        for a in nd.acts:
            if a in nd.q:
                u = nd.q[a] + self.c_puct * nd.ps[a] * sq / float(1 + nd.n[a])
                if depth == 0 and float(nd.n[a]) * float(nd.n[a]) < (self.k * nd.ps[a]) * float(nd.ns):
                    u = math.inf
            else:
                u = self.c_puct * nd.ps[a] * sq0
            if u > cur_best:
                cur_best, best = u, a
        a = best
        if a < 0:
            return 0.0
        if depth == 0 and cur_best == math.inf:
            self.forced += 1
        if a not in nd.child:
            code, nxt, _eff = self.lg.do_play(abi.action_decode(self.n, a), nd.st)
            assert code == 0, code
            nd.child[a] = nu._Node(nxt)
        v = self.search(nd.child[a], depth + 1)
        if a in nd.q:
            nd.q[a] = (float(nd.n[a]) * nd.q[a] + v) / float(nd.n[a] + 1)
            nd.n[a] += 1
        else:
            nd.q[a], nd.n[a] = v, 1
        nd.ns += 1
        return -v


def ceil_sqrt(x: float) -> int:
    """The smallest integer F >= 0 with float(F) * float(F) >= x."""
    F = int(math.sqrt(x))
    while float(F) * float(F) < x:
        F += 1
    while F > 0 and float(F - 1) * float(F - 1) >= x:
        F -= 1
    return F


def prune(root, c_puct, k):
    """Rule 2 on a finished root (a noise_util._Node): [(action, n, n', F, Qsa bits, is b)] of the visited edges, ascending."""
    acts = [a for a in (root.acts or []) if a in root.q]
    if not acts:
        return []
    ns = [root.n[a] for a in acts]
    b = acts[ns.index(max(ns))]
    fns = float(root.ns)
    sq = math.sqrt(fns)
    ustar = root.q[b] + c_puct * root.ps[b] * sq / float(1 + root.n[b])
    out = []
    for a in acts:
        n, p, q = root.n[a], root.ps[a], root.q[a]
        if a == b:
            out.append((a, n, n, 0, nu.qbits(q), True))
            continue
        F = ceil_sqrt((k * p) * fns)
        m = n
        for _ in range(F):
            if m == 0:
                break
            if q + c_puct * p * sq / float(1 + (m - 1)) < ustar:
                m -= 1
            else:
                break
        if m < n and m <= 1:
            m = 0
        out.append((a, n, m, F, nu.qbits(q), False))
    return out


class Tally:
    """What tafl_gselfplay_forced_playouts_stats counts, and for the coverage conditions the draws whose position moved."""

    def __init__(self):
        self.forced_sims = self.pruned_visits = self.pruned_children = self.full_moves = self.draws_moved = 0

    def stats(self):
        return (self.forced_sims, self.pruned_visits, self.pruned_children, self.full_moves)


def one_move(orc, lg, st, predict, gid, M, sample_seed, temp_moves, k, noise, tally, n_sims=S):
    """The forced search of a full move from the oracle state `st`, pruned, and its pick: (the twin, pruned rows, index of the played row
    among the rows with n' > 0 or None when no edge was visited)."""
    t = ForcedTwin(lg, st, CPUCT, predict, k, noise).run(n_sims)
    rows = prune(t.root, CPUCT, k)
    tally.forced_sims += t.forced
    kept = [r for r in rows if r[2] > 0]
    if not kept:
        return t, rows, None
    tally.pruned_visits += sum(r[1] - r[2] for r in rows)
    tally.pruned_children += sum(r[2] == 0 for r in rows)
    vs = [r[2] for r in kept]
    if M < temp_moves:
        r = eu.sample_word(sample_seed, gid, M)
        j = eu.pick_rule(vs, r)
        tally.draws_moved += rows[eu.pick_rule([x[1] for x in rows], r)][0] != kept[j][0]      # (the draw over the raw n lands elsewhere)
    else:
        j = vs.index(max(vs))
    tally.full_moves += 1
    return t, rows, j


def example_of(st, kept, j, M):
    e = eu.Example()
    e.board, e.side = st.board_to_matrix(), st.to_abi().side_to_play
    e.actions, e.visits, e.played, e.move_no = [r[0] for r in kept], [r[2] for r in kept], kept[j][0], M
    return e.fields()


def twin_run(orc, lg, states, wb, salts, n_moves, sample_seed, temp_moves, move_base, base, k, games=None, eta_of=None, epsilon=0.0, n_sims=S):
    """noise_util.twin_run with the forced twin: the draw and the example use n'.  Returns (gselfplay_util.Run, Tally)."""
    n_games, n = len(states), lg.side_len
    A = abi.action_size(n)
    out, tally = gsu.Run(n_games, n_moves), Tally()
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
            _t, rows, j = one_move(orc, lg, st, nu.predictor(A, salts[g]), base + g, M, sample_seed, temp_moves, k, (epsilon, rows_eta[g]) if epsilon else None, tally, n_sims)
            out.sims += n_sims
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


_SEARCH = {}


def searches(orc, cfg, games=None, k=K):
    """One search of every game of `games` (default: all) in noise_util.setup's shape: {g: (forced twin's raw kids, pruned rows, forced
    selections, counts, unforced twin's kids)}, remembered per (layout, game)."""
    _rules, n, wb, lg, states, salts = nu.setup(orc, cfg)
    A = abi.action_size(n)
    out = {}
    for g in (range(len(states)) if games is None else games):
        key = (cfg, g, k)
        if key not in _SEARCH:
            st = orc.GameState.from_abi(states[g], wb)
            t = ForcedTwin(lg, st, CPUCT, nu.predictor(A, salts[g]), k).run(S)
            u = nu.Twin(lg, st, CPUCT, nu.predictor(A, salts[g])).run(S)
            _SEARCH[key] = (t.kids(), prune(t.root, CPUCT, k), t.forced, t.counts(), u.kids())
        out[g] = _SEARCH[key]
    return out


def coverage(found):
    """The six conditions of the issue over `found` (what `searches` returns)."""
    c = dict.fromkeys(FLOORS, 0)
    for kids, rows, forced, _cnt, plain in found.values():
        c["differ"] += kids != plain
        c["forced"] += forced
        for _a, n, m, F, _q, is_b in rows:
            c["zeroed"] += m == 0
            c["partial"] += 0 < n - m < min(F, n) and m > 1
            c["blocked"] += (not is_b) and m == n
            c["full subtraction"] += (not is_b) and n - m == F
    return c


# ---- the host harness (tests/hostsim_forced) ------------------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_forced")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_forced.so"))
        P, u8, u32, u64, vp, dbl = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double
        L.hsf_forced_check.restype = C.c_int; L.hsf_forced_check.argtypes = [P(TaflForcedPlayouts)]
        L.hsf_begin.restype = vp
        L.hsf_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), P(TaflState), u32, u32, u32, dbl, P(TaflRootNoise), P(TaflPlayoutCap), P(TaflForcedPlayouts),
                                P(TaflSelfplayOpts), u32, u64, C.c_int, u64, u32, vp]
        L.hsf_free.restype = None; L.hsf_free.argtypes = [vp]
        L.hsf_step.restype = u32; L.hsf_step.argtypes = [vp, P(C.c_float), P(C.c_float)]
        L.hsf_leaves.restype = None; L.hsf_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hsf_root_children.restype = None; L.hsf_root_children.argtypes = [vp, P(TaflRootChild), u32, P(u32)]
        L.hsf_end.restype = None; L.hsf_end.argtypes = [vp, P(TaflState), P(TaflPlay), P(u32), P(u64), P(u8), P(u32), P(u64), P(u64), P(u64)]
        L.hsf_ex_new.restype = vp; L.hsf_ex_new.argtypes = [u32, u8, u32, u32]
        L.hsf_ex_free.restype = None; L.hsf_ex_free.argtypes = [vp]
        L.hsf_ex_counts.restype = None; L.hsf_ex_counts.argtypes = [vp, P(u32), P(u64), P(u32)]
        L.hsf_ex_example.restype = C.c_int; L.hsf_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32), P(C.c_float), P(u8)]
        _HLIB = L
    return _HLIB


class HostExamples:
    """tafl_examples with its open_from array on host memory (ExEp of hostsim_forced.cpp)."""

    def __init__(self, n, n_lanes, max_moves, max_children):
        self.n, self.G, self.max_moves, self.K = n, n_lanes, max_moves, max_children
        self.h = hlib().hsf_ex_new(n_lanes, n, max_moves, max_children)

    def __del__(self):
        if getattr(self, "h", None):
            hlib().hsf_ex_free(self.h)
            self.h = None

    def counts(self):
        """(examples per lane, {dropped, overflowed}, open_from per lane)."""
        ln, ct, of = (C.c_uint32 * self.G)(), (C.c_uint64 * 4)(), (C.c_uint32 * self.G)()
        hlib().hsf_ex_counts(self.h, ln, ct, of)
        return list(ln), {"dropped": ct[0], "overflowed": ct[1]}, list(of)

    def all(self):
        """Per lane, in column order: (Example.fields() tuple, z, final)."""
        lens, _, _ = self.counts()
        out = [[] for _ in range(self.G)]
        for g in range(self.G):
            for j in range(min(lens[g], self.max_moves)):
                out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (self.n * self.n))()
                acts, vis, z, fin = (C.c_uint32 * self.K)(), (C.c_uint32 * self.K)(), C.c_float(), C.c_uint8()
                assert hlib().hsf_ex_example(self.h, j * self.G + g, out5, board, acts, vis, C.byref(z), C.byref(fin)) == 0, (j, g)
                assert out5[2] == 0, ("overflow", j, g)
                k = out5[0]
                rows = [list(board[r * self.n:(r + 1) * self.n]) for r in range(self.n)]
                out[g].append(((rows, out5[1], list(acts[:k]), list(vis[:k]), out5[3], out5[4]), float(z.value), int(fin.value)))
        return out


def forced_cfg(k=K):
    return TaflForcedPlayouts(k, 0)


def cap_cfg(full_per, fast=FAST, seed=CAP_SEED):
    return TaflPlayoutCap(seed, fast, full_per, 0)


def host_forced(rules, n, wb, states, salts, n_moves, sample_seed, temp_moves, k=K, cap=None, ex=None, episodes=False, base=0, stride=0, episode_moves=0,
                move_base=0, noise=None, n_sims=S, kids=False, read_examples=True):
    """tafl_gselfplay_begin (episodes False) or _begin_episodes with forced playouts `k` (None: off), the cap `cap` and the noise `noise`
    latched / the step loop / tafl_gselfplay_end on the harness with the stub network: epu.Lanes with the examples of `ex` and .moves,
    .cap_stats, .fp_stats, .faults, .stat_faults; with `kids` also .kids, the visited root children [(action, visits, Q bits)] each lane's
    arena holds at the end."""
    L = hlib()
    n_lanes, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(sample_seed, temp_moves, move_base, 0)
    fc = forced_cfg(k) if k is not None else None
    h = L.hsf_begin(C.byref(rc), n, wb, states, None, n_lanes, n_sims, EDGES, CPUCT, C.byref(noise) if noise is not None else None, C.byref(cap) if cap is not None else None,
                    C.byref(fc) if fc is not None else None, C.byref(o), n_moves, base, 1 if episodes else 0, stride, episode_moves, ex.h if ex is not None else None)
    assert h
    try:
        boards, sides, waiting = (C.c_uint8 * (n_lanes * n * n))(), (C.c_uint8 * n_lanes)(), (C.c_uint8 * n_lanes)()
        L.hsf_leaves(h, boards, sides, waiting)
        w = sum(waiting)
        while w:
            pri, val = gsu.stub_rows(boards, sides, waiting, n_lanes, n, A, salts)
            w = L.hsf_step(h, gsu.fptr(pri), gsu.fptr(val))
            L.hsf_leaves(h, boards, sides, waiting)
            assert sum(waiting) == w
        st, plays, moves, c4, faults = (TaflState * n_lanes)(), (TaflPlay * (n_lanes * n_moves))(), (C.c_uint32 * n_lanes)(), (C.c_uint64 * 4)(), (C.c_uint8 * n_lanes)()
        eps, ec, cc, f4 = (C.c_uint32 * n_lanes)(), (C.c_uint64 * 4)(), (C.c_uint64 * 2)(), (C.c_uint64 * 4)()
        L.hsf_end(h, st, plays, moves, c4, faults, eps, ec, cc, f4)
        found = None
        if kids:
            rk, cnt = (TaflRootChild * (n_lanes * 512))(), (C.c_uint32 * n_lanes)()
            L.hsf_root_children(h, rk, 512, cnt)
            found = nu._kids_of(rk, cnt, n_lanes, 512)
    finally:
        L.hsf_free(h)
    examples = ex.all() if ex is not None and read_examples else [[] for _ in range(n_lanes)]
    out = epu.lanes_of(n_lanes, n_moves, plays, list(moves), st, eps, ec, c4[0], c4[1], examples)
    out.moves, out.cap_stats, out.fp_stats, out.faults, out.stat_faults, out.kids = list(moves), (cc[0], cc[1]), tuple(f4), list(faults), c4[3], found
    if ex is not None:
        out.open_from = ex.counts()[2]
    return out if episodes else pcu._plain(out)


# ---- the library -----------------------------------------------------------------------------------------------------------------------------
def device_forced(batch, ex, n, salts, n_moves, sample_seed, temp_moves, k=K, cap=None, episodes=False, base=0, stride=0, episode_moves=0, move_base=0, noise=None,
                  n_sims=S):
    """The same loop through the C-ABI on `batch` (states uploaded), the stub network in host buffers: epu.Lanes as host_forced returns
    them (.fp_stats None when k is None, .cap_stats None without a cap)."""
    n_lanes, A = batch.n, abi.action_size(n)
    epu.set_noise(batch, noise)
    pcu.set_cap(batch, cap)
    if k is None:
        batch.clear_forced_playouts()
    else:
        batch.set_forced_playouts(k)
    if episodes:
        batch.gselfplay_begin_episodes(ex, n_moves, n_sims, CPUCT, EDGES, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves, episode_moves=episode_moves,
                                       id_stride=stride)
    else:
        batch.gselfplay_begin(ex, n_moves, n_sims, CPUCT, EDGES, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves, move_base=move_base)
    w = batch.gselfplay_step()
    while w:
        boards, sides, waiting = batch.gmcts_leaves()
        assert sum(waiting) == w
        pri, val = gsu.stub_rows(boards, sides, waiting, n_lanes, n, A, salts)
        w = batch.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
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
    out.moves, out.stat_faults = list(moves), stats.faults
    out.cap_stats = (cs.full_moves, cs.fast_moves) if cs else None
    out.fp_stats = (fs.forced_sims, fs.pruned_visits, fs.pruned_children, fs.full_moves) if fs else None
    return out if episodes else pcu._plain(out)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------
def assert_lanes_equal_run(got, want, n_moves, where="", games=None):
    """A plain run's Lanes (a driver's) against a gselfplay_util.Run (the twin's, or gselfplay_util.host_run's with .examples filled)."""
    for g in (range(len(want.states)) if games is None else games):
        assert got.plays[g] == [want.plays[m][g] for m in range(want.moves[g])], (where, "plays", g)
        assert got.moves[g] == want.moves[g], (where, "moves", g, got.moves[g], want.moves[g])
        assert got.states[g] == want.states[g], (where, "state", g)
        assert [f for f, _z, _fin in got.examples[g]] == want.examples[g], (where, "examples", g, got.examples[g], want.examples[g])


def assert_same_lanes(got, want, where=""):
    """Two drivers' Lanes (the device's against the harness's): everything they both leave."""
    epu.assert_same(got, want, where)
    assert got.moves == want.moves and got.fp_stats == want.fp_stats, (where, got.fp_stats, want.fp_stats)
    if want.cap_stats is not None and got.cap_stats is not None:
        assert got.cap_stats == want.cap_stats, (where, got.cap_stats, want.cap_stats)


def capped_composition(orc, cfg, side, full_per, noise, k=K, lanes=None, base=epu.IDS, budget=6, fast=FAST):
    """Item 4's expectation for an episodes run of noise_util.setup's lanes (`lanes`: only those are played, every other one holds the
    finished position) with the cap (CAP_SEED, fast, full_per) and the run's noise: playout_cap_util.composition in which a full move is
    one forced twin move (fed `side`'s eta) and a fast move the uncapped unforced one-move harness run.  Returns (Lanes, Tally)."""
    rules, n, wb, lg, states, salts = nu.setup(orc, cfg)
    A, n_lanes = abi.action_size(n), len(states)
    over = states[nu.G_PLAIN]
    tally = Tally()
    fast_route = pcu.host_route(rules, n, wb, salts, fast, None, S_=S)

    def route(batch, live, full, gb, M):
        if not full:
            return fast_route(batch, live, False, gb, M)
        run = gsu.Run(n_lanes, 1)
        for g in range(n_lanes):
            run.states[g] = bytes(batch[g])
        eta = side.eta(batch, nu.noise_cfg(base=gb, move_no=M)) if noise else None
        for g in live:
            st = orc.GameState.from_abi(batch[g], wb)
            _t, rows, j = one_move(orc, lg, st, nu.predictor(A, salts[g]), gb + g, M, pcu.SSEED, pcu.TEMP, k, (nu.EPSILON, eta[g]) if noise else None, tally)
            if j is None:
                continue
            kept = [r for r in rows if r[2] > 0]
            run.examples[g].append(example_of(st, kept, j, M))
            play = abi.action_decode(n, kept[j][0])
            code, nxt, _eff = lg.do_play(play, st)
            assert code == 0
            run.plays[0][g], run.moves[g], run.states[g] = pu.play_tuple4(play), 1, bytes(nxt.to_abi())
        return run, S * len(live), None

    start = states if lanes is None else (TaflState * n_lanes)(*[states[g] if g in lanes else over for g in range(n_lanes)])
    want = pcu.composition(route, start, over, budget, CAP_SEED, full_per, True, base=base, stride=n_lanes, openings=start)
    return want, tally
