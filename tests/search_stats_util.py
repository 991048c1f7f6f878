"""Search statistics per training row (include/taflhip.h "search value and policy surprise"): the expectation from
the Python twins of the guided searches - noise_util.Twin for plain and noise runs, forced_util.one_move for the full moves of a capped
run with forced playouts, solver_util.one_move for solver runs - as (action, n', float32(q), float32(p)) per stored child, value by the
sequential float64 loop and surprise with numpy.log in float64; and two drivers that leave the same structure: the host harness
(tests/hostsim_search_stats) and the library through the C-ABI."""
import ctypes as C
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import (TaflForcedPlayouts, TaflPlay, TaflPlayoutCap, TaflRootNoise, TaflSelfplayOpts, TaflSolver, TaflState)
from tests import examples_util as eu
from tests import forced_util as fu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import parity_util as pu
from tests import playout_cap_util as pcu
from tests import solver_util as su

CPUCT, EDGES = nu.CPUCT, nu.EDGES
SEED, TEMP, BASE = 5, 2, 1000
FAST, FULL_PER, CAP_SEED = 6, 32768, 3
# the runs of the issue: name -> settings (n_moves is the lane budget; an episodes run cuts after three moves, so every lane reopens)
MODES = {
    "plain": dict(),
    "noise": dict(noise=True),
    "cap_forced": dict(cap=True, k=fu.K),
    "solver": dict(solver=True),
    "episodes": dict(episodes=True, episode_moves=3, n_moves=5),
}
TINY = 2.0 ** -126


class Row:
    """One recorded example: actions, visits (n'), q and p as float32 arrays, the play, the move number and the side to move."""

    def __init__(self, actions, visits, q, p, played, move_no, side):
        self.actions, self.visits = [int(a) for a in actions], [int(v) for v in visits]
        self.q, self.p = np.asarray(q, np.float32), np.asarray(p, np.float32)
        self.played, self.move_no, self.side = int(played), int(move_no), int(side)

    def value(self):
        """acc = acc + (double)Nsa_k * (double)cq_k, ascending; (float)(acc / (double)N)."""
        if not self.visits:
            return np.float32(0.0)
        acc = 0.0
        for v, q in zip(self.visits, self.q):
            acc = acc + float(v) * float(q)
        return np.float32(acc / float(sum(self.visits)))

    def surprise(self):
        if not self.visits:
            return np.float32(0.0)
        N, s = float(sum(self.visits)), 0.0
        for v, p in zip(self.visits, self.p):
            pi = float(v) / N
            s = s + pi * (float(np.log(np.float64(pi))) - float(np.log(np.float64(max(float(p), TINY)))))
        return np.float32(max(s, 0.0))

    def key(self):
        return (self.actions, self.visits, self.q.tobytes(), self.p.tobytes(), self.played, self.move_no, self.side)


def _f64(bits):
    return float(np.uint64(bits).view(np.float64))


def shape(orc, cfg, G, modulus=40):
    """(rules, n, wb, oracle logic, states [G] at (7 g) mod `modulus` random plies, salts, a finished position per lane)."""
    rules, fen, wb = pu.CONFIGS[cfg]
    return shape_of(orc, rules, fen, wb, G, modulus)


def shape_of(orc, rules, fen, wb, G, modulus=40):
    n = abi.fen_side_len(fen)
    lg = orc.GameLogic(rules, n)
    states = gsu.start_states(orc, lg, rules, fen, wb, G, modulus)
    start = orc.GameState(fen, rules.starting_side, wb)
    over = []
    for g in range(G):
        plies = 1000
        st = lg.random_advance(start, 77, g, plies).to_abi()
        while st.status == abi.ONGOING:
            plies *= 2
            st = lg.random_advance(start, 77, g, plies).to_abi()
        over.append(st)
    return rules, n, wb, lg, states, [(3 * g + 1) % 256 for g in range(G)], (TaflState * G)(*over)


def z_of(side, over_state):
    if over_state.status == abi.DRAW:
        return 1e-4
    return 1.0 if over_state.winner == side else -1.0


def twin_run(orc, lg, states, wb, salts, side, S, n_moves=3, noise=False, cap=False, k=None, solver=False, episodes=False, episode_moves=0):
    """The expectation: per lane the Rows its run records, in order.  `side`: noise_util.HostSide / DeviceSide, whose eta feeds the noise."""
    n, G = lg.side_len, len(states)
    A = abi.action_size(n)
    out = [[] for _ in range(G)]
    for g in range(G):
        opening = orc.GameState.from_abi(states[g], wb)
        st, episode, m0, md = opening, 0, 0, 0
        predict = nu.predictor(A, salts[g])
        while md < n_moves and st.to_abi().status == abi.ONGOING:
            gid, M = BASE + episode * G + g, md - m0
            full = pcu.is_full(CAP_SEED, gid, M, FULL_PER) if cap else True
            nz = None
            if noise and full:
                one = (TaflState * 1)(st.to_abi())
                nz = (nu.EPSILON, side.eta(one, nu.noise_cfg(base=gid, move_no=M))[0])
            if solver:
                t, rows, j = su.one_move(lg, st, predict, gid, M, SEED, TEMP, su.Tally(), S, k if full else None, nz, 0 if full else S - FAST)
                kept = [(r[0], r[2], r[3]) for r in rows if r[2] > 0]
            elif k is not None and full:
                t, rows, j = fu.one_move(orc, lg, st, predict, gid, M, SEED, TEMP, k, nz, fu.Tally(), S)
                kept = [(r[0], r[2], r[4]) for r in rows if r[2] > 0]
            else:
                t = nu.Twin(lg, st, CPUCT, predict, nz).run(S if full else FAST)
                kept = t.kids()
                vs = [v for _a, v, _q in kept]
                j = None if not vs else (eu.pick_rule(vs, eu.sample_word(SEED, gid, M)) if M < TEMP else vs.index(max(vs)))
            if j is None:
                break
            if full:
                out[g].append(Row([a for a, _v, _q in kept], [v for _a, v, _q in kept], [np.float32(_f64(q)) for _a, _v, q in kept],
                                  [np.float32(t.root.ps[a]) for a, _v, _q in kept], kept[j][0], M, st.to_abi().side_to_play))
            code, st, _eff = lg.do_play(abi.action_decode(n, kept[j][0]), st)
            assert code == 0
            md += 1
            if episodes and md < n_moves and (st.to_abi().status != abi.ONGOING or (episode_moves and md - m0 >= episode_moves)):
                episode, m0, st = episode + 1, md, opening
    return out


def coverage(want, over):
    rows = [(r, over[g]) for g, lane in enumerate(want) for r in lane]
    return dict(examples=len(rows), two_children=sum(len(r.visits) >= 2 for r, _o in rows),
                sign_differs=sum(float(r.value()) * z_of(r.side, o) < 0 for r, o in rows), positive=sum(float(r.surprise()) > 0 for r, _o in rows))


def assert_floors(want, over, where=""):
    c = coverage(want, over)
    print(where, c)
    assert c["examples"] > 0 and 2 * c["two_children"] >= c["examples"] and c["sign_differs"] >= 1 and 2 * c["positive"] >= c["examples"], (where, c)


def assert_rows(got, want, where=""):
    """cq, cp (and the example they belong to) bit for bit, value bit for bit, surprise within 2^-23 |want| + 1e-10."""
    assert len(got.rows) == len(want), where
    for g, (gl, wl) in enumerate(zip(got.rows, want)):
        assert len(gl) == len(wl), (where, g, len(gl), len(wl))
        for j, (a, b) in enumerate(zip(gl, wl)):
            assert a.key() == b.key(), (where, g, j, a.key(), b.key())
            v, s = got.value[(g, j)], got.surprise[(g, j)]
            wv, ws = b.value(), b.surprise()
            assert np.float32(v).tobytes() == wv.tobytes(), (where, "value", g, j, float(v), float(wv))
            assert abs(float(s) - float(ws)) <= 2.0 ** -23 * abs(float(ws)) + 1e-10, (where, "surprise", g, j, float(s), float(ws))


class Recorded:
    """What a driver leaves: rows[g] (Rows in order), value / surprise {(g, j): float32}, plays, final states, counters."""


# ---- the host harness (tests/hostsim_search_stats) ---------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_search_stats")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_search_stats.so"))
        P, u8, u32, u64, vp, dbl, f32 = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double, C.c_float
        L.hqs_ex_new.restype = vp; L.hqs_ex_new.argtypes = [u32, u8, u32, u32]
        L.hqs_ex_free.restype = None; L.hqs_ex_free.argtypes = [vp]
        L.hqs_begin.restype = vp
        L.hqs_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), P(TaflState), u32, u32, u32, dbl, P(TaflRootNoise), P(TaflPlayoutCap), P(TaflForcedPlayouts),
                                P(TaflSolver), P(TaflSelfplayOpts), u32, u64, C.c_int, u64, u32, vp]
        L.hss_begin.restype = vp; L.hss_begin.argtypes = L.hqs_begin.argtypes
        L.hqs_session.restype = vp; L.hqs_session.argtypes = [vp]
        L.hqs_free.restype = None; L.hqs_free.argtypes = [vp]
        L.hss_free.restype = None; L.hss_free.argtypes = [vp]
        L.hqs_step.restype = u32; L.hqs_step.argtypes = [vp, P(f32), P(f32)]
        L.hss_step.restype = u32; L.hss_step.argtypes = [vp, P(f32), P(f32)]
        L.hss_leaves.restype = None; L.hss_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hss_end.restype = None; L.hss_end.argtypes = [vp, P(TaflState), P(TaflPlay), P(u32), P(u64), P(u8), P(u32), P(u64), P(u64), P(u64), P(u64)]
        L.hss_ex_counts.restype = None; L.hss_ex_counts.argtypes = [vp, P(u32), P(u64), P(u32)]
        L.hss_ex_example.restype = C.c_int; L.hss_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32), P(f32), P(u8)]
        L.hqs_ex_finalize.restype = None; L.hqs_ex_finalize.argtypes = [vp, P(TaflState)]
        L.hqs_ex_raw.restype = None; L.hqs_ex_raw.argtypes = [vp, vp, vp]
        L.hqs_ex_read_stats.restype = C.c_int; L.hqs_ex_read_stats.argtypes = [vp, vp, u32, vp, vp]
        L.hqs_ex_gather_stats.restype = C.c_int; L.hqs_ex_gather_stats.argtypes = [vp, vp, u32, vp, vp]
        _HLIB = L
    return _HLIB


def _settings(noise, cap, k, solver):
    nz = nu.noise_cfg() if noise else None
    cp = TaflPlayoutCap(CAP_SEED, FAST, FULL_PER, 0) if cap else None
    fc = fu.forced_cfg(k) if k is not None else None
    sc = TaflSolver(0) if solver else None
    return nz, cp, fc, sc


def _ref(x):
    return C.byref(x) if x is not None else None


def host_run(rules, n, wb, states, salts, S, K, stats=True, over=None, n_moves=3, max_moves=None, noise=False, cap=False, k=None, solver=False, episodes=False, episode_moves=0):
    """The run on the harness; stats False: the same run through hss_begin / hss_step alone (nothing of this feature runs)."""
    L = hlib()
    G, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(SEED, TEMP, 0, 0)
    nz, cp, fc, sc = _settings(noise, cap, k, solver)
    max_moves = n_moves if max_moves is None else max_moves
    ex = L.hqs_ex_new(G, n, max_moves, K)
    begin = L.hqs_begin if stats else L.hss_begin
    h = begin(C.byref(rc), n, wb, states, None, G, S, EDGES, CPUCT, _ref(nz), _ref(cp), _ref(fc), _ref(sc), C.byref(o), n_moves, BASE, 1 if episodes else 0, G, episode_moves, ex)
    assert h
    hs = L.hqs_session(h) if stats else h
    out = Recorded()
    try:
        boards, sides, waiting = (C.c_uint8 * (G * n * n))(), (C.c_uint8 * G)(), (C.c_uint8 * G)()
        L.hss_leaves(hs, boards, sides, waiting)
        w = sum(waiting)
        while w:
            pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
            w = (L.hqs_step if stats else L.hss_step)(h, gsu.fptr(pri), gsu.fptr(val))
            L.hss_leaves(hs, boards, sides, waiting)
        st, plays, moves, c4, faults = (TaflState * G)(), (TaflPlay * (G * n_moves))(), (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint8 * G)()
        eps, ec, cc, f4, s8 = (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint64 * 2)(), (C.c_uint64 * 4)(), (C.c_uint64 * 8)()
        L.hss_end(hs, st, plays, moves, c4, faults, eps, ec, cc, f4, s8)
        assert not any(faults) and c4[3] == 0
        out.plays, out.states, out.moves = [pu.play_tuple4(p) for p in plays], [bytes(s) for s in st], list(moves)
        out.counters = (tuple(c4), tuple(ec), tuple(cc), tuple(f4), tuple(s8), list(eps))
        if over is not None:
            L.hqs_ex_finalize(ex, over)
        lens, ct, of = (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint32 * G)()
        L.hss_ex_counts(ex, lens, ct, of)
        out.lens, out.dropped, out.overflowed = list(lens), ct[0], ct[1]
        out.rows, out.value, out.surprise, out.examples = [[] for _ in range(G)], {}, {}, []
        raw_q, raw_p = np.zeros(G * max_moves * K, np.float32), np.zeros(G * max_moves * K, np.float32)
        L.hqs_ex_raw(ex, raw_q.ctypes.data, raw_p.ctypes.data)
        out.raw_q, out.raw_p = raw_q.reshape(max_moves, K, G), raw_p.reshape(max_moves, K, G)
        out.over_flags = {}
        for g in range(G):
            for j in range(min(lens[g], max_moves)):
                e = j * G + g
                out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (n * n))()
                acts, vis, z, fin = (C.c_uint32 * K)(), (C.c_uint32 * K)(), C.c_float(), C.c_uint8()
                assert L.hss_ex_example(ex, e, out5, board, acts, vis, C.byref(z), C.byref(fin)) == 0
                nc = out5[0] if not out5[2] else 0
                out.over_flags[(g, j)] = out5[2]
                out.examples.append((g, j, bytes(board), tuple(out5), tuple(acts[:nc]), tuple(vis[:nc]), float(z.value), int(fin.value)))
                idx = np.asarray([e], np.uint32)
                q, p, v, s = np.zeros(K, np.float32), np.zeros(K, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
                if stats:
                    assert L.hqs_ex_read_stats(ex, idx.ctypes.data, 1, q.ctypes.data, p.ctypes.data) == 0
                    assert L.hqs_ex_gather_stats(ex, idx.ctypes.data, 1, v.ctypes.data, s.ctypes.data) == 0
                out.rows[g].append(Row(acts[:nc], vis[:nc], q[:nc], p[:nc], out5[3], out5[4], out5[1]))
                out.value[(g, j)], out.surprise[(g, j)] = v[0], s[0]
        bad = np.asarray([G * max_moves, 0xFFFFFFFF] + [j * G + g for g in range(G) for j in range(lens[g], max_moves)][:3], np.uint32)
        v, s = np.ones(bad.size, np.float32), np.ones(bad.size, np.float32)
        out.bad = (L.hqs_ex_gather_stats(ex, bad.ctypes.data, bad.size, v.ctypes.data, s.ctypes.data), bad.size, not v.any() and not s.any()) if stats else None
    finally:
        (L.hqs_free if stats else L.hss_free)(h)
        L.hqs_ex_free(ex)
    return out


# ---- the library -----------------------------------------------------------------------------------------------------------------------------
def device_run(glg, n, states, salts, S, K, stats=True, over=None, n_moves=3, max_moves=None, noise=False, cap=False, k=None, solver=False, episodes=False, episode_moves=0,
               overflowing=False, sym_seed=None):
    """The same run through the C-ABI (solver_util.device_solver drives it): Recorded, read back with Examples.read, .read_stats and
    .gather_stats (host pointers)."""
    G = len(states)
    max_moves = n_moves if max_moves is None else max_moves
    b = glg.new_batch(G)
    b.upload(states)
    ex = glg.new_examples(G, max_moves, K, search_stats=stats)
    nz, cp, _fc, _sc = _settings(noise, cap, k, solver)
    out = Recorded()
    if overflowing or sym_seed is not None:
        # a plain run driven here: solver_util.device_solver insists on examples that all hold a policy; and with sym_seed the run
        # latches an evaluation symmetry and is fed eval_symmetry_util's conjugated network, so that it must record what the plain
        # run records (the priors indexed by the original action)
        from tests import eval_symmetry_util as esu
        A = abi.action_size(n)
        b.clear_solver(); b.clear_forced_playouts()
        if sym_seed is not None:
            b.set_eval_symmetry(sym_seed, 123456)
        b.gselfplay_begin(ex, n_moves, S, CPUCT, EDGES, game_id_base=BASE, sample_seed=SEED, temp_moves=TEMP)
        out.syms = set()
        w = b.gselfplay_step()
        while w:
            boards, sides, waiting = b.gmcts_leaves()
            if sym_seed is not None:
                syms = b.gmcts_leaf_symmetry()
                out.syms |= {syms[g] for g in range(G) if waiting[g]}
                pri, val = esu.conjugated_rows(boards, sides, waiting, syms, G, n, A, salts)
            else:
                pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
            w = b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        out.plays, out.moves = b.gselfplay_end()
        out.states = None
    else:
        lanes = su.device_solver(b, ex, n, salts, n_moves, SEED, TEMP, n_sims=S, solver=solver, k=k, cap=cp, episodes=episodes, base=BASE, stride=G, episode_moves=episode_moves, noise=nz)
        out.plays, out.states, out.moves = lanes.plays, lanes.states, lanes.moves
    if over is not None:
        ob = glg.new_batch(G)
        ob.upload(over)
        ex.finalize(ob)
    lens, _tot = ex.counts()
    out.lens = list(lens)
    index = [j * G + g for g in range(G) for j in range(min(lens[g], max_moves))]
    out.index = index
    out.rows, out.value, out.surprise = [[] for _ in range(G)], {}, {}
    if index:
        nc, ov, pl, mv, acts, vis = ex.read(index)
        _b, sides, _pi, z, fin = ex.gather(index)
        out.z, out.fin = z, fin
        if stats:
            q, p = ex.read_stats(index)
            v, s = ex.gather_stats(index)
        else:
            q = p = np.zeros((len(index), K), np.float32)
            v = s = np.zeros(len(index), np.float32)
        for i, e in enumerate(index):
            g, j, c = e % G, e // G, int(nc[i])
            out.rows[g].append(Row(acts[i][:c], vis[i][:c], q[i][:c], p[i][:c], pl[i], mv[i], sides[i]))
            out.value[(g, j)], out.surprise[(g, j)] = v[i], s[i]
    out.ex, out.batch = ex, b
    return out


# ---- the pool --------------------------------------------------------------------------------------------------------------------------------
from tests import pool_weights_util as pwu  # noqa: E402


class PoolExpectation:
    """value / surprise per slot, the live window (pool_weights_util.Window) and the weights (WeightModel) of a pool of C slots that
    ingests whole runs: every example of `want` (the twin's Rows per lane, all final, none overflowed) is taken in ascending index order."""

    def __init__(self, C_):
        self.win = pwu.Window(C_)
        self.model = pwu.WeightModel(self.win)
        self.value, self.surprise, self.generation = {}, {}, {}

    def ingest(self, want):
        G, depth = len(want), max(len(lane) for lane in want)
        taken = [want[g][j] for j in range(depth) for g in range(G) if j < len(want[g])]
        T, C_, before = len(taken), self.win.C, self.win.written
        self.win.took(T)
        for r in range(T - min(T, C_), T):
            s = (before + r) % C_
            self.value[s], self.surprise[s], self.generation[s] = taken[r].value(), taken[r].surprise(), self.win.ingests
        self.model.ingested(T, before)
        return T

    def weights_from_surprise(self, read_back, base, per_nat, generation=0):
        """wt[s] = min(2^32 - 1, base + floor(float64(surprise read back) * per_nat)) for the live slots of the generation."""
        for s in self.win.live_slots():
            if generation and self.generation[s] != generation:
                continue
            x = float(np.float64(read_back[s]) * np.float64(per_nat))
            add = int(x) if x < 2.0 ** 32 else pwu.MAXW
            self.model.wt[s] = min(pwu.MAXW, base + add)

    def check(self, slots, value, surprise, where=""):
        for i, s in enumerate(slots):
            assert np.float32(value[i]).tobytes() == self.value[s].tobytes(), (where, "value", s)
            ws = float(self.surprise[s])
            assert abs(float(surprise[i]) - ws) <= 2.0 ** -23 * abs(ws) + 1e-10, (where, "surprise", s)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class HostStatsPool:
    """The pool of tests/hostsim_search_stats (PoolSHost over tests/hostsim_pool_weights' PoolWHost)."""

    def __init__(self, C_, Kp, n):
        L = hlib()
        vp, u32, u64, P = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER
        L.hqs_pool_new.restype = vp; L.hqs_pool_new.argtypes = [u32, u32, C.c_uint8]
        L.hqs_pool_free.restype = None; L.hqs_pool_free.argtypes = [vp]
        L.hqs_pool_weights.restype = vp; L.hqs_pool_weights.argtypes = [vp]
        L.hqs_pool_set_search_stats.restype = C.c_int; L.hqs_pool_set_search_stats.argtypes = [vp, C.c_int]
        L.hqs_pool_ingest.restype = C.c_int; L.hqs_pool_ingest.argtypes = [vp, vp, C.c_int, P(u64)]
        L.hqs_pool_gather_stats.restype = C.c_int; L.hqs_pool_gather_stats.argtypes = [vp, vp, u32, vp, vp, C.c_int]
        L.hqs_pool_weights_from_surprise.restype = C.c_int; L.hqs_pool_weights_from_surprise.argtypes = [vp, P(abi.TaflPoolSurpriseWeights)]
        L.hspw_set_weighting.restype = None; L.hspw_set_weighting.argtypes = [vp, C.c_int, u32]
        L.hspw_trim.restype = C.c_int; L.hspw_trim.argtypes = [vp, u32]
        L.hspw_clear.restype = None; L.hspw_clear.argtypes = [vp]
        L.hspw_raw_weights.restype = C.c_int; L.hspw_raw_weights.argtypes = [vp, vp]
        L.hspw_draw.restype = C.c_int; L.hspw_draw.argtypes = [vp, u64, u64, u32, u32, u32, vp, vp, vp, P(u64), vp]
        L.hspw_pool.restype = vp; L.hspw_pool.argtypes = [vp]
        L.hsp_stats.restype = None; L.hsp_stats.argtypes = [vp, P(u64)]
        self.L, self.C = L, C_
        self.h = L.hqs_pool_new(C_, Kp, n)
        self.w = L.hqs_pool_weights(self.h)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.hqs_pool_free(self.h)
            self.h = None

    def set_search_stats(self, on):
        return self.L.hqs_pool_set_search_stats(self.h, int(on))

    def set_weighting(self, w):
        self.L.hspw_set_weighting(self.w, 0 if w is None else 1, w or 0)

    def ingest(self, ex, with_stats=True):
        o3 = (C.c_uint64 * 3)()
        rc = self.L.hqs_pool_ingest(self.h, ex, int(with_stats), o3)
        return rc, o3[0]

    def trim(self, keep):
        return self.L.hspw_trim(self.w, keep)

    def clear(self):
        self.L.hspw_clear(self.w)

    def stats(self):
        o = (C.c_uint64 * 8)()
        self.L.hsp_stats(self.L.hspw_pool(self.w), o)
        return dict(zip(("written", "live", "ingests", "oldest_generation", "skipped_open", "skipped_overflow", "bad_slot", "device_bytes"), o))

    def gather_stats(self, slots, strict):
        sl = np.ascontiguousarray(slots, np.uint32)
        v, s = np.ones(sl.size, np.float32), np.ones(sl.size, np.float32)
        return self.L.hqs_pool_gather_stats(self.h, _vp(sl), sl.size, _vp(v), _vp(s), int(strict)), v, s

    def weights_from_surprise(self, base, per_nat, generation=0, flags=0, reserved=None):
        cfg = abi.TaflPoolSurpriseWeights(base=base, generation=generation, per_nat=per_nat, flags=flags)
        if reserved is not None:
            cfg._reserved[reserved] = 1
        return self.L.hqs_pool_weights_from_surprise(self.h, C.byref(cfg))

    def raw_weights(self):
        out = np.zeros(self.C, np.uint32)
        assert self.L.hspw_raw_weights(self.w, _vp(out)) == 0
        return out

    def draw(self, count, seed, step):
        sl, sy, wt, tot = np.zeros(count, np.uint32), np.zeros(count, np.uint8), np.zeros(count, np.uint32), C.c_uint64()
        assert self.L.hspw_draw(self.w, seed, step, 0, count, 1, _vp(sl), _vp(sy), _vp(wt), C.byref(tot), None) == 0
        return sl, sy, wt, tot.value


def host_examples_run(rules, n, wb, states, salts, S, K, over, n_moves):
    """A plain recording run on the harness whose examples object is kept: (the object's handle, a closer)."""
    L = hlib()
    G, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(SEED, TEMP, 0, 0)
    ex = L.hqs_ex_new(G, n, n_moves, K)
    h = L.hqs_begin(C.byref(rc), n, wb, states, None, G, S, EDGES, CPUCT, None, None, None, None, C.byref(o), n_moves, BASE, 0, G, 0, ex)
    assert h
    hs = L.hqs_session(h)
    boards, sides, waiting = (C.c_uint8 * (G * n * n))(), (C.c_uint8 * G)(), (C.c_uint8 * G)()
    L.hss_leaves(hs, boards, sides, waiting)
    w = sum(waiting)
    while w:
        pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
        w = L.hqs_step(h, gsu.fptr(pri), gsu.fptr(val))
        L.hss_leaves(hs, boards, sides, waiting)
    L.hqs_free(h)
    L.hqs_ex_finalize(ex, over)
    return ex
