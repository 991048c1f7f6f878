"""Expected values for the eval-symmetry tests (include/taflhip.h tafl_eval_symmetry).

Evaluating under a symmetry is by definition a wrapper around predict, so the expectation is the ORACLE's own guided search,
orc.GameLogic.gmcts, run with predict'(b) = (unpermute_s(P), v) where (P, v) = predict(transform_s(b)) and s the draw rule restated here
over orc.GameLogic.state_hash.  The board transform and the action permutation are the Python restatements of tests/examples_util.py.
Nothing here comes from the code under test.

For the self-play families, which the oracle has no loop for, the check is by CONJUGATION: the device is handed a network that undoes s on
the boards it is shown (with the symmetries the getter reports), asks the stub, and writes out[sym_action(s, a)] = P[a]; a run with the
setting on and that network must equal the run with the setting off and the plain stub in everything."""
import ctypes as C
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflEvalSymmetry, TaflRootChild, TaflState
from tests import examples_util as eu
from tests import gselfplay_util as gsu
from tests import parity_util as pu

CPUCT = 1.25
EDGES = 256
SYM_KEY = 0x53594D4D45545259          # "SYMMETRY"
SEED, BASE = 0x5EED5, 700             # the setting of the shared workloads


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------
def draw_rule(seed, gid, h):
    """s = ply_rand(sim_key(game_key(seed, gid) ^ "SYMMETRY", h), 0) >> 29 with h the leaf key."""
    return eu.ply_rand(eu.sim_key(eu.game_key(seed, gid) ^ SYM_KEY, h), 0) >> 29


def draw_of(orc, state, seed, gid):
    """The draw for an oracle GameState."""
    return draw_rule(seed, gid, orc.GameLogic.state_hash(state))


def transform(board, s):
    """The board (n x n array) under symmetry s: the byte of tile (r, c) goes to tile sym_rc(r, c)."""
    b = np.asarray(board, np.uint8)
    n = b.shape[0]
    out = np.empty_like(b)
    for r in range(n):
        for c in range(n):
            r2, c2 = eu.sym_rc(n, r, c, s)
            out[r2, c2] = b[r, c]
    return out


def untransform(shown, s):
    """The inverse of transform."""
    b = np.asarray(shown, np.uint8)
    n = b.shape[0]
    out = np.empty_like(b)
    for r in range(n):
        for c in range(n):
            r2, c2 = eu.sym_rc(n, r, c, s)
            out[r, c] = b[r2, c2]
    return out


_PERM = {}


def perm(n, s):
    """perm[a] = sym_action(s, a) for every dense action of an n x n board."""
    key = (n, s)
    if key not in _PERM:
        _PERM[key] = np.array([eu.sym_action_py(n, a, s) for a in range(abi.action_size(n))], np.int64)
    return _PERM[key]


# ---- predict' on the oracle's side ---------------------------------------------------------------------------------------------------------
class Tally:
    """What the wrapped predictors of one workload saw: draws per symmetry, leaves, all-masked leaves."""

    def __init__(self):
        self.draws, self.leaves, self.all_masked = [0] * 8, 0, 0


def wrapped_predictor(orc, lg, seed, gid, salt, tally=None):
    """predict'(b) = (unpermute_s(P), v), (P, v) = stub(transform_s(b)), s = the draw of (seed, gid, b)."""
    n = lg.side_len
    A = abi.action_size(n)

    def predict(st):
        s = draw_of(orc, st, seed, gid)
        shown = transform(st.board_to_matrix(), s)
        P, v = gsu.stub(shown.tobytes(), int(st.side_to_play), A, salt)
        back = P[perm(n, s)]
        if tally is not None:
            tally.draws[s] += 1
            tally.leaves += 1
            legal = [abi.action_encode(n, p) for p in lg.all_plays(st)]
            tally.all_masked += not back[legal].any()
        return back, v
    return predict


def plain_predictor(n, salt):
    A = abi.action_size(n)
    return lambda st: gsu.stub(bytes(np.asarray(st.board_to_matrix(), np.uint8).tobytes()), int(st.side_to_play), A, salt)


def kids_of(kids):
    return [(a, v, q.hex()) for (_p, a, v, q) in kids]


def oracle_search(orc, lg, states, wb, S, salts, seed=None, base=0, tally=None):
    """Per game (root children as (action, visits, q.hex()), counts) of lg.gmcts with the wrapped predictor (seed None: the plain stub)."""
    out = []
    for g in range(len(states)):
        st = orc.GameState.from_abi(states[g], wb)
        pr = plain_predictor(lg.side_len, salts[g]) if seed is None else wrapped_predictor(orc, lg, seed, base + g, salts[g], tally)
        kids, _ns, _pri, cnt = lg.gmcts(st, S, CPUCT, pr, wb)
        out.append((kids_of(kids), tuple(cnt[:3])))
    return out


# ---- the networks a side under test is handed -------------------------------------------------------------------------------------------------
def conjugated_rows(boards, sides, waiting, syms, G, n, A, salts):
    """The conjugated batch network: undo s on the shown boards, ask the stub, write out[sym_action(s, a)] = P[a]."""
    raw = np.frombuffer(bytes(boards), np.uint8).reshape(G, n, n)
    pri, val = np.zeros((G, A), np.float32), np.zeros(G, np.float32)
    for g in range(G):
        if waiting[g]:
            s = int(syms[g])
            P, v = gsu.stub(untransform(raw[g], s).tobytes(), int(sides[g]), A, salts[g])
            pri[g][perm(n, s)] = P
            val[g] = v
    return pri, val


# ---- workloads ---------------------------------------------------------------------------------------------------------------------------------
def salts_of(G):
    return [(3 * g + 1) % 256 for g in range(G)]


_WORK = {}


def workload(orc, name):
    """(rules, n, wb, oracle logic, states, S, salts) of a lock-step workload:
    copenhagen11  65 Copenhagen 11 x 11 games (a full wave plus a lone lane) (7 g) mod 40 random plies in, S = 24
    brandubh7     65 Brandubh 7 x 7 games (7 g) mod 40 plies in, S = 32
    copenhagen13  16 games on 13 x 13 / u256 (15-column stride), S = 12
    side8         16 games on the side-8 board of tests/board_sizes_util.py on u128 (an even side), S = 12"""
    if name not in _WORK:
        if name == "side8":
            from tests import board_sizes_util as bsu
            pair = (8, 128)
            rules, n, wb, G, S = bsu.ruleset(pair, "copenhagen"), 8, 128, 16, 12
            states, _plies = bsu.advanced_start(pair, "copenhagen", G, 21, 0)
            lg = orc.GameLogic(rules, n)
        else:
            rules, fen, wb = pu.CONFIGS[name]
            n = abi.fen_side_len(fen)
            lg = orc.GameLogic(rules, n)
            G, S, mod = {"copenhagen11": (65, 24, 40), "brandubh7": (65, 32, 40), "copenhagen13": (16, 12, 40)}[name]
            states = gsu.start_states(orc, lg, rules, fen, wb, G, mod)
        _WORK[name] = (rules, n, wb, lg, states, S, salts_of(len(states)))
    return _WORK[name]


_WANT = {}


def expectation(orc, name):
    """(wrapped oracle search per game, Tally, plain oracle search per game) of a workload, computed once."""
    if name not in _WANT:
        _rules, _n, wb, lg, states, S, salts = workload(orc, name)
        tally = Tally()
        on = oracle_search(orc, lg, states, wb, S, salts, SEED, BASE, tally)
        off = oracle_search(orc, lg, states, wb, S, salts)
        _WANT[name] = (on, tally, off)
    return _WANT[name]


# ---- the host harness (tests/hostsim_evalsym) ---------------------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_evalsym")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_evalsym.so"))
        P, u8, u32, u64, vp, dbl = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double
        L.hse_begin.restype = vp
        L.hse_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), u32, u32, u32, dbl, P(TaflEvalSymmetry)]
        L.hse_free.restype = None; L.hse_free.argtypes = [vp]
        L.hse_step.restype = u32; L.hse_step.argtypes = [vp, P(C.c_float), P(C.c_float)]
        L.hse_leaves.restype = None; L.hse_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hse_leaf_symmetry.restype = None; L.hse_leaf_symmetry.argtypes = [vp, P(u8)]
        L.hse_root_children.restype = None; L.hse_root_children.argtypes = [vp, P(TaflRootChild), u32, P(u32)]
        L.hse_counts.restype = None; L.hse_counts.argtypes = [vp, P(u64)]
        L.hse_draw.restype = C.c_int; L.hse_draw.argtypes = [u8, u32, P(TaflState), u32, P(TaflEvalSymmetry), P(u8)]
        _HLIB = L
    return _HLIB


def host_draw(n, wb, states, seed, base):
    G = len(states)
    out = (C.c_uint8 * G)()
    cfg = TaflEvalSymmetry(seed, base, 0)
    assert hlib().hse_draw(n, wb, states, G, C.byref(cfg), out) == 0
    return list(out)


def conjugated_net(G, n, salts):
    A = abi.action_size(n)
    return lambda boards, sides, waiting, syms: conjugated_rows(boards, sides, waiting, syms, G, n, A, salts)


def host_search(rules, n, wb, states, S, salts, seed=None, base=0, rounds_out=None, net=None):
    """The harness's lock-step search with the plain stub (or `net`(boards, sides, waiting, syms)).  Returns (children per game, (sims, predicts, terminal hits, faults)); every
    round's (boards, sides, waiting, syms) is appended to rounds_out."""
    L, G, A = hlib(), len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    cfg = TaflEvalSymmetry(seed, base, 0) if seed is not None else None
    h = L.hse_begin(C.byref(rc), n, wb, states, G, S, EDGES, CPUCT, C.byref(cfg) if cfg is not None else None)
    assert h
    try:
        boards, sides, waiting, syms = (C.c_uint8 * (G * n * n))(), (C.c_uint8 * G)(), (C.c_uint8 * G)(), (C.c_uint8 * G)()
        w = L.hse_step(h, None, None)
        while w:
            L.hse_leaves(h, boards, sides, waiting)
            L.hse_leaf_symmetry(h, syms)
            assert sum(waiting) == w
            if rounds_out is not None:
                rounds_out.append((bytes(boards), bytes(sides), bytes(waiting), bytes(syms)))
            pri, val = net(boards, sides, waiting, syms) if net else gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
            w = L.hse_step(h, gsu.fptr(pri), gsu.fptr(val))
        kids, cnt, c4 = (TaflRootChild * (G * 512))(), (C.c_uint32 * G)(), (C.c_uint64 * 4)()
        L.hse_root_children(h, kids, 512, cnt)
        L.hse_counts(h, c4)
    finally:
        L.hse_free(h)
    return [[(kids[g * 512 + j].action, kids[g * 512 + j].visits, kids[g * 512 + j].q.hex()) for j in range(cnt[g])] for g in range(G)], tuple(c4)


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------
def device_search(b, n, S, salts, rounds_out=None, begin=True, net=None):
    """tafl_gmcts_begin / the step loop on batch `b` (its eval-symmetry setting as the caller left it) with the plain stub (or `net`).
    Returns (children per game, stats)."""
    G, A = b.n, abi.action_size(n)
    if begin:
        b.gmcts_begin(S, EDGES)
    w = b.gmcts_step(None, None, CPUCT, S)
    while w:
        boards, sides, waiting = b.gmcts_leaves()
        syms = b.gmcts_leaf_symmetry()
        assert sum(waiting) == w
        if rounds_out is not None:
            rounds_out.append((bytes(boards), bytes(sides), bytes(waiting), bytes(syms)))
        pri, val = net(boards, sides, waiting, syms) if net else gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
        w = b.gmcts_step(gsu.fptr(pri), gsu.fptr(val), CPUCT, S)
    kids, cnt = b.gmcts_root_children(512)
    return [[(kids[g * 512 + j].action, kids[g * 512 + j].visits, kids[g * 512 + j].q.hex()) for j in range(cnt[g])] for g in range(G)], b.gmcts_stats()


def assert_rounds_transformed(on_rounds, off_rounds, n):
    """Round by round, an on-search driven by the conjugated network against the off-search with the plain stub: the same games wait,
    sides are equal, and every shown row of a waiting game is the transform of the off-search's row under the reported s."""
    assert len(on_rounds) == len(off_rounds) and on_rounds
    seen = set()
    for (b_on, s_on, w_on, syms), (b_off, s_off, w_off, syms_off) in zip(on_rounds, off_rounds):
        assert w_on == w_off and s_on == s_off and not any(syms_off)
        G = len(w_on)
        on = np.frombuffer(b_on, np.uint8).reshape(G, n, n)
        off = np.frombuffer(b_off, np.uint8).reshape(G, n, n)
        for g in range(G):
            assert syms[g] < 8 and (w_on[g] or syms[g] == 0), (g, syms[g])
            assert (on[g] == transform(off[g], syms[g])).all(), (g, syms[g])
            if w_on[g]:
                seen.add(syms[g])
    return seen


# ---- the self-play families on the device, by conjugation -------------------------------------------------------------------------------------------
VARIANTS = ("plain", "noise", "cap_forced", "solver")
SP_SIMS, SP_MOVES, SP_TEMP, SP_LANE_MOVES, SP_EPISODE_MOVES, SP_BASE, SP_SAMPLE_SEED = 16, 6, 3, 8, 3, 4000, 17


def _counters(st):
    return tuple(getattr(st, f) for f, _t in st._fields_ if not f.startswith("_"))


def device_selfplay(glg, states, n, salts, variant, episodes, sym_seed=None, conjugated=False):
    """One recording guided self-play run on a fresh batch: `variant` of VARIANTS; per pace (SP_MOVES moves) or in episodes (SP_LANE_MOVES
    per lane, episodes cut after SP_EPISODE_MOVES moves, so that every lane reopens); sym_seed None: the setting off; conjugated: the
    conjugated network in place of the plain stub.  Returns (everything the run leaves as one comparable dict, the symmetries the getter
    reported for waiting leaves)."""
    from tests import episodes_util as epu
    G, A = len(states), abi.action_size(n)
    budget = SP_LANE_MOVES if episodes else SP_MOVES
    b = glg.new_batch(G)
    b.upload(states)
    ex = glg.new_examples(G, budget, SP_SIMS)
    if variant == "noise":
        b.set_root_noise(0.3, 0.25, 0xD1CE)
    if variant == "cap_forced":
        b.set_playout_cap(8, 0.5, 0xCA9)
        b.set_forced_playouts(2.0)
    if variant == "solver":
        b.set_solver()
    if sym_seed is not None:
        b.set_eval_symmetry(sym_seed, 123456)            # (a run uses its own game_id_base, not this one)
    if episodes:
        b.gselfplay_begin_episodes(ex, budget, SP_SIMS, CPUCT, EDGES, game_id_base=SP_BASE, sample_seed=SP_SAMPLE_SEED, temp_moves=SP_TEMP,
                                   episode_moves=SP_EPISODE_MOVES)
    else:
        b.gselfplay_begin(ex, budget, SP_SIMS, CPUCT, EDGES, game_id_base=SP_BASE, sample_seed=SP_SAMPLE_SEED, temp_moves=SP_TEMP)
    seen = set()
    w = b.gselfplay_step()
    while w:
        boards, sides, waiting = b.gmcts_leaves()
        syms = b.gmcts_leaf_symmetry()
        assert sum(waiting) == w
        seen |= {syms[g] for g in range(G) if waiting[g]}
        assert all(waiting[g] or syms[g] == 0 for g in range(G))
        if conjugated:
            pri, val = conjugated_rows(boards, sides, waiting, syms, G, n, A, salts)
        else:
            pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
        w = b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
    plays, moves = b.gselfplay_end()
    st = b.gmcts_stats()
    examples, over = epu.device_examples(ex, G, n)
    out = {"plays": [pu.play_tuple4(plays[i]) for i in range(G * budget)], "moves": list(moves), "states": bytes(b.download()),
           "examples": examples, "overflow": over, "stats": (st.sims, st.predicts, st.terminal_hits, st.faults)}
    if episodes:
        eps, es = b.gselfplay_episode_stats()
        out["episodes"] = (list(eps), _counters(es))
    if variant == "cap_forced":
        out["cap"], out["forced"] = _counters(b.playout_cap_stats()), _counters(b.forced_playouts_stats())
    if variant == "solver":
        out["solver"] = _counters(b.solver_stats())
    ex.close(); b.close()
    return out, seen
