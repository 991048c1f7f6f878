"""Expected values and drivers for match play (include/taflhip.h tafl_gmatch_*): the seat / owner rule restated in
Python, the oracle match loop (gselfplay_util.oracle_run's body with the stub's salt chosen per move as SALT[owner], plus close and
reopen as episodes_util.reference does them), the reference route on a device batch (the existing tafl_gselfplay_begin_episodes loop
whose full-size priors carry stub(leaf g, SALT[owner(g)]) in row g), and the drivers of the host harness (tests/hostsim_match) and of
the library.  The coverage conditions of the tests are asserted on the oracle or reference route, never on the code under test."""
import ctypes as C
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflSelfplayOpts, TaflState
from tests import episodes_util as epu
from tests import examples_util as eu
from tests import gselfplay_util as gsu
from tests import parity_util as pu
from tests.stub_net import matrix_bytes_of

# the base setting: episodes_util's lanes and openings (Brandubh 7x7, 24 lanes, the start position advanced by (7 g) mod 60 plies)
G0, MODULUS, S0, BUDGET, TEMP, CPUCT, SSEED, IDS, SALT = 24, 60, 16, 40, 4, 1.25, 5, 1000, (11, 200)


def seat(base, g, k, swap):
    """The evaluator that plays the attackers in episode k of lane g."""
    return (base + g + k + swap) & 1


def owner(base, g, k, swap, side_to_play):
    """The evaluator of every leaf of the search whose root has `side_to_play` to move."""
    return (seat(base, g, k, swap) + (1 if side_to_play == abi.DEFENDER else 0)) & 1


def result_of(st):
    """The column of tafl_match_stats.games / tafl_episode_stats an episode that stands at `st` is counted in."""
    return 3 if st.status == abi.ONGOING else 2 if st.status == abi.DRAW else 1 if st.winner == abi.DEFENDER else 0


def oracle_match(orc, lg, wb, states, openings, S, c_puct, salts, budget, sample_seed, temp_moves, base=0, stride=0, episode_moves=0, swap=0, only=None):
    """The match on the oracle, one lane after the other: (episodes_util.Lanes, games[2][4]).  `only`: the lanes to follow."""
    G, n = len(states), states[0].side_len
    A, stride = abi.action_size(n), stride or G
    out, games = epu.Lanes(G), [[0] * 4, [0] * 4]
    for g in range(G):
        out.states[g] = bytes(states[g])
    for g in (range(G) if only is None else only):
        st, k, m_ep, left, seg = orc.GameState.from_abi(states[g], wb), 0, 0, budget, []
        while left > 0 and st.to_abi().status == abi.ONGOING:
            salt = salts[owner(base, g, k, swap, st.to_abi().side_to_play)]
            kids, _ns, _pri, _cnt = lg.gmcts(st, S, c_puct, lambda s, salt=salt: gsu.stub(matrix_bytes_of(s.board_to_matrix()), int(s.side_to_play), A, salt), wb)
            out.sims += S
            vs = [v for (_p, _a, v, _q) in kids]
            if not vs:
                break
            j = eu.pick_rule(vs, eu.sample_word(sample_seed, base + k * stride + g, m_ep)) if m_ep < temp_moves else vs.index(max(vs))
            e = eu.Example()
            e.board, e.side = st.board_to_matrix(), st.to_abi().side_to_play
            e.actions, e.visits, e.played, e.move_no = [a for (_p, a, _v, _q) in kids], vs, kids[j][1], m_ep
            seg.append(e.fields())
            play = abi.action_decode(n, kids[j][1])
            code, st, _eff = lg.do_play(play, st)
            assert code == 0, (g, k, m_ep, code)
            out.plays[g].append(pu.play_tuple4(play))
            left, m_ep = left - 1, m_ep + 1
            now = st.to_abi()
            over = now.status != abi.ONGOING
            if left == 0:                                       # the budget is used up: the episode stays open
                out.ended_on_last[g] = over
                break
            if over or (episode_moves and m_ep == episode_moves):
                out.examples[g] += [(f,) + (epu.outcome(bytes(now), f[1]) if over else (0.0, 0)) for f in seg]
                seg = []
                games[seat(base, g, k, swap)][result_of(now)] += 1
                out.counters[result_of(now)] += 1
                out.episodes[g] += 1
                out.ended[g] += over
                out.capped[g] += not over
                out.open_from[g] = len(out.examples[g])
                k, m_ep = k + 1, 0
                if openings[g].status != abi.ONGOING:           # the lane stops, its batch state stays
                    break
                st = orc.GameState.from_abi(openings[g], wb)
        out.examples[g] += [(f, 0.0, 0) for f in seg]
        out.states[g] = bytes(st.to_abi())
    out.predicts = None
    return out, games


def games_from_lanes(lanes, base, swap):
    """games[2][4] from what a route left: a lane's column of examples splits into episodes where move_no returns to 0; the first
    `episodes` of them were closed or cut (final = 0: cut), and a closed one's result is read off z and the side to move of its last
    example.  Needs an examples object that dropped nothing."""
    games = [[0] * 4, [0] * 4]
    for g, col in enumerate(lanes.examples):
        starts = [j for j, (f, _z, _fin) in enumerate(col) if f[5] == 0] + [len(col)]
        assert len(starts) - 1 in (lanes.episodes[g], lanes.episodes[g] + 1), (g, starts, lanes.episodes[g])
        for k in range(lanes.episodes[g]):
            f, z, fin = col[starts[k + 1] - 1]
            if not fin:
                r = 3
            elif z == epu.DRAW_Z:
                r = 2
            else:
                winner = f[1] if z > 0 else (abi.DEFENDER if f[1] == abi.ATTACKER else abi.ATTACKER)
                r = 1 if winner == abi.DEFENDER else 0
            games[seat(base, g, k, swap)][r] += 1
    return games


def stub_rows(count, boards, sides, side_len, action_size, salt):
    """nnet.predict of one evaluator for the first `count` rows of its dense batch: (priors float32 [count, A], values float32 [count])."""
    nn = side_len * side_len
    raw = bytes(boards)
    pri, val = np.zeros((max(count, 1), action_size), np.float32), np.zeros(max(count, 1), np.float32)
    for r in range(count):
        pri[r], val[r] = gsu.stub(raw[r * nn:(r + 1) * nn], int(sides[r]), action_size, salt)
    return pri, val


# ---- the host harness (tests/hostsim_match) ------------------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_match")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_match.so"))
        P, u8, u32, u64, vp, dbl, fl = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double, C.c_float
        L.hsm_begin.restype = vp
        L.hsm_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), P(TaflState), u32, u32, u32, dbl, P(TaflSelfplayOpts), u32, u64, u64, u32, u32, vp]
        L.hsm_free.restype = None; L.hsm_free.argtypes = [vp]
        L.hsm_leaves.restype = None; L.hsm_leaves.argtypes = [vp, P(u8), P(u8), P(u32), P(u8), P(u8), P(u32), P(u32)]
        L.hsm_step.restype = None; L.hsm_step.argtypes = [vp, P(fl), P(fl), P(fl), P(fl)]
        L.hsm_end.restype = None; L.hsm_end.argtypes = [vp, P(TaflState), P(TaflPlay), P(u32), P(u64), P(u8), P(u32), P(u64), P(u64)]
        L.hsm_ex_new.restype = vp; L.hsm_ex_new.argtypes = [u32, u8, u32, u32]
        L.hsm_ex_free.restype = None; L.hsm_ex_free.argtypes = [vp]
        L.hsm_ex_counts.restype = None; L.hsm_ex_counts.argtypes = [vp, P(u32), P(u64), P(u32)]
        L.hsm_ex_example.restype = C.c_int; L.hsm_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32), P(fl), P(u8)]
        _HLIB = L
    return _HLIB


class HostExamples:
    """tafl_examples with its open_from array on host memory (ExEp of hostsim_match.cpp)."""

    def __init__(self, n, G, max_moves, K):
        self.n, self.G, self.max_moves, self.K = n, G, max_moves, K
        self.h = hlib().hsm_ex_new(G, n, max_moves, K)

    def __del__(self):
        if getattr(self, "h", None):
            hlib().hsm_ex_free(self.h)
            self.h = None

    def counts(self):
        """(examples per lane, {dropped, overflowed}, open_from per lane)."""
        ln, ct, of = (C.c_uint32 * self.G)(), (C.c_uint64 * 4)(), (C.c_uint32 * self.G)()
        hlib().hsm_ex_counts(self.h, ln, ct, of)
        return list(ln), {"dropped": ct[0], "overflowed": ct[1]}, list(of)

    def all(self):
        """Per lane, in column order: (Example.fields() tuple, z, final)."""
        lens, _, _ = self.counts()
        out = [[] for _ in range(self.G)]
        for g in range(self.G):
            for j in range(min(lens[g], self.max_moves)):
                out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (self.n * self.n))()
                acts, vis, z, fin = (C.c_uint32 * self.K)(), (C.c_uint32 * self.K)(), C.c_float(), C.c_uint8()
                assert hlib().hsm_ex_example(self.h, j * self.G + g, out5, board, acts, vis, C.byref(z), C.byref(fin)) == 0, (j, g)
                k = out5[0]
                rows = [list(board[r * self.n:(r + 1) * self.n]) for r in range(self.n)]
                out[g].append(((rows, out5[1], list(acts[:k]), list(vis[:k]), out5[3], out5[4]), float(z.value), int(fin.value)))
        return out


def host_match(rules, n, wb, states, S, c_puct, salts, budget, sample_seed, temp_moves, ex, base=0, stride=0, episode_moves=0, swap=0, openings=None, edges_per_node=256):
    """tafl_gmatch_begin / the leaves-step loop / tafl_gselfplay_end on the harness with the two stub networks: (Lanes with the examples of
    `ex`, games[2][4], fault flags per lane, rounds).  Every round the rows of both evaluators are checked to be the waiting lanes in
    ascending order."""
    L = hlib()
    G, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(sample_seed, temp_moves, 0, 0)
    h = L.hsm_begin(C.byref(rc), n, wb, states, openings, G, S, edges_per_node, c_puct, C.byref(o), budget, base, stride, episode_moves, swap, ex.h if ex is not None else None)
    assert h
    try:
        boards, sides = [(C.c_uint8 * (G * n * n))() for _ in range(2)], [(C.c_uint8 * G)() for _ in range(2)]
        lanes, cnt, rounds = [(C.c_uint32 * G)() for _ in range(2)], (C.c_uint32 * 2)(), 0
        while True:
            L.hsm_leaves(h, boards[0], sides[0], lanes[0], boards[1], sides[1], lanes[1], cnt)
            if not (cnt[0] or cnt[1]):
                break
            for e in range(2):
                assert list(lanes[e][:cnt[e]]) == sorted(set(lanes[e][:cnt[e]])), (e, rounds)
            ev = [stub_rows(cnt[e], boards[e], sides[e], n, A, salts[e]) for e in range(2)]
            L.hsm_step(h, gsu.fptr(ev[0][0]), gsu.fptr(ev[0][1]), gsu.fptr(ev[1][0]), gsu.fptr(ev[1][1]))
            rounds += 1
        st, plays, moves, c4, faults = (TaflState * G)(), (TaflPlay * (G * budget))(), (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint8 * G)()
        eps, ec, gm = (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint64 * 8)()
        L.hsm_end(h, st, plays, moves, c4, faults, eps, ec, gm)
    finally:
        L.hsm_free(h)
    examples = ex.all() if ex is not None else [[] for _ in range(G)]
    out = epu.lanes_of(G, budget, plays, list(moves), st, eps, ec, c4[0], c4[1], examples)
    out.abi_states, out.stat_faults, out.terminal_hits = st, c4[3], c4[2]
    return out, [list(gm[:4]), list(gm[4:])], list(faults), rounds


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def games_of(stats):
    return [[int(stats.games[a][r]) for r in range(4)] for a in range(2)]


def finish(batch, ex, n, budget, examples=True):
    """What a run left on `batch` (after its loop): (Lanes, stats); Lanes.terminal_hits and .faults carry the other two counters."""
    G = batch.n
    plays, moves = batch.gselfplay_end()
    stats = batch.gmcts_stats()
    eps, es = batch.gselfplay_episode_stats()
    got, over = epu.device_examples(ex, G, n) if ex is not None and examples else ([[] for _ in range(G)], None)
    assert over is None or not any(any(o) for o in over)
    out = epu.lanes_of(G, budget, plays, list(moves), batch.download(), eps, (es.attacker_wins, es.defender_wins, es.draws, es.cut), stats.sims, stats.predicts, got)
    out.terminal_hits, out.faults, out.moves = stats.terminal_hits, stats.faults, list(moves)
    if ex is not None:
        assert (ex.stats().dropped, ex.stats().overflowed) == (0, 0)
    return out, stats


def device_match(batch, ex, n, S, c_puct, evaluate, budget, sample_seed, temp_moves, base=0, stride=0, episode_moves=0, swap=0, openings=None, edges_per_node=256,
                 each_round=None):
    """The match through the C-ABI on `batch` (states uploaded), host pointers: evaluate(e, count, boards, sides) -> (priors float32
    [count, A], values float32 [count]) as numpy arrays.  each_round(counts, boards, sides, waiting, lanes), if given, runs before the
    evaluators.  Returns (Lanes, games[2][4], stats, rounds)."""
    batch.clear_root_noise()
    batch.gmatch_begin(ex, budget, S, c_puct, edges_per_node, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves, episode_moves=episode_moves,
                       id_stride=stride, openings=openings, swap=swap)
    rounds = 0
    while True:
        counts, boards, sides, waiting, lanes = batch.gmatch_leaves()
        if each_round is not None:
            each_round(counts, boards, sides, waiting, lanes)
        if not (counts[0] or counts[1]):
            break
        ev = [evaluate(e, counts[e], boards[e], sides[e]) if counts[e] else (None, None) for e in range(2)]
        batch.gmatch_step([gsu.fptr(p) if p is not None else None for p, _v in ev], [gsu.fptr(v) if v is not None else None for _p, v in ev])
        rounds += 1
    out, stats = finish(batch, ex, n, budget)
    return out, games_of(batch.gmatch_stats()), stats, rounds


def stub_evaluate(n, salts):
    A = abi.action_size(n)
    return lambda e, count, boards, sides: stub_rows(count, boards, sides, n, A, salts[e])


def reference_route(batch, ex, n, S, c_puct, evaluate_full, budget, sample_seed, temp_moves, base=0, stride=0, episode_moves=0, swap=0, openings=None, edges_per_node=256):
    """The same match on the existing entry points: tafl_gselfplay_begin_episodes / tafl_gselfplay_step on `batch`, where row g of the
    full-size priors is the answer of evaluator owner(g); owner(g) comes from the lane's downloaded batch state and its episode count.
    evaluate_full(owners [G], boards, sides, waiting) -> (priors float32 [G, A], values float32 [G]).  Returns (Lanes, stats, rounds,
    rounds in which one evaluator had leaves and the other had none)."""
    G = batch.n
    batch.clear_root_noise()
    batch.gselfplay_begin_episodes(ex, budget, S, c_puct, edges_per_node, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves,
                                   episode_moves=episode_moves, id_stride=stride, openings=openings)
    w, rounds, lonely = batch.gselfplay_step(), 0, 0
    while w:
        boards, sides, waiting = batch.gmcts_leaves()
        st, (eps, _es) = batch.download(), batch.gselfplay_episode_stats()
        owners = [owner(base, g, eps[g], swap, st[g].side_to_play) for g in range(G)]
        per = [sum(1 for g in range(G) if waiting[g] and owners[g] == e) for e in range(2)]
        lonely += (per[0] == 0) != (per[1] == 0)
        pri, val = evaluate_full(owners, boards, sides, waiting)
        w = batch.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        rounds += 1
    out, stats = finish(batch, ex, n, budget)
    return out, stats, rounds, lonely


def stub_evaluate_full(n, salts):
    A = abi.action_size(n)
    return lambda owners, boards, sides, waiting: gsu.stub_rows(boards, sides, waiting, len(owners), n, A, [salts[o] for o in owners])


def assert_equivalent(got, want, where=""):
    """Every output of the equivalence: episodes_util.assert_same and the two counters it does not cover, the moves per lane, open_from."""
    epu.assert_same(got, want, where)
    assert (got.terminal_hits, got.faults) == (want.terminal_hits, want.faults), (where, "terminal hits, faults")
    assert got.moves == want.moves, (where, "moves")


def vector_evaluators(n):
    """Two vectorised evaluators that differ: evaluator 0 uniform priors, value 0.25; evaluator 1 priors 1 + (a mod 7), value -0.25."""
    A = abi.action_size(n)
    rows = [np.ones(A, np.float32), (1 + (np.arange(A) % 7)).astype(np.float32)]
    vals = [np.float32(0.25), np.float32(-0.25)]

    def evaluate(e, count, boards, sides):
        return np.ascontiguousarray(np.broadcast_to(rows[e], (count, A))), np.full(count, vals[e], np.float32)

    def evaluate_full(owners, boards, sides, waiting):
        own = np.asarray(owners)
        return np.ascontiguousarray(np.stack(rows)[own]), np.asarray(vals, np.float32)[own].copy()
    return evaluate, evaluate_full
