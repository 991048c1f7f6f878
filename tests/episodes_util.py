"""Expected values and drivers for the episodes run of guided self-play (include/taflhip.h tafl_gselfplay_begin_episodes, DESIGN.md
section 15).

No new twin: a run is deterministic per (state, gid, M) and every move starts from a fresh root, so episode k of lane g equals the plain
run (tafl_gselfplay_begin, pinned against the oracle) from the lane's opening with game_id_base + k * id_stride and move_base = 0,
truncated to the moves the lane had left or to episode_moves.  `reference` builds that concatenation from any plain route: the oracle
loop, the host harness's plain run (tests/hostsim, tests/hostsim_noise) or the plain run of the library on a second batch.  The coverage
conditions of the tests are asserted on what `reference` returns, never on the code under test."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflRootNoise, TaflSelfplayOpts, TaflState
from tests import gselfplay_util as gsu
from tests import parity_util as pu

DRAW_Z = float(np.float32(1e-4))
ZERO_PLAY = (0, 0, 0, 0)

# the smallest setting that meets every branch (Brandubh 7x7): 24 lanes, the start position advanced by (7 g) mod 60 plies
G0, MODULUS, S0, BUDGET, TEMP, CPUCT, SSEED, IDS = 24, 60, 16, 20, 4, 1.25, 5, 1000


class Lanes:
    """What an episodes run leaves, per lane: plays in lane order, the final batch state, examples in column order as (fields, z, final),
    episodes closed or cut; the counters (attacker wins, defender wins, draws, cut); sims and predicts (None where the route has none)."""

    def __init__(self, G):
        self.plays, self.states, self.examples, self.episodes = [[] for _ in range(G)], [None] * G, [[] for _ in range(G)], [0] * G
        self.counters, self.sims, self.predicts = [0, 0, 0, 0], 0, 0
        # for the coverage conditions: per lane the number of games that ended, whether one ended on the last budgeted move, whether the
        # budget cut a later episode short, whether a cap cut one
        self.ended, self.ended_on_last, self.budget_cut, self.capped = [0] * G, [False] * G, [False] * G, [0] * G
        self.open_from = [0] * G          # (reference route) the examples object's open_from: the index after the last closed or cut episode


def outcome(state_bytes, side):
    """(z, final) of an example whose side to move was `side`, from the position its game stands at (tafl_examples_finalize)."""
    st = TaflState.from_buffer_copy(state_bytes)
    if st.status == abi.ONGOING:
        return 0.0, 0
    if st.status == abi.DRAW:
        return DRAW_Z, 1
    return (1.0 if st.winner == side else -1.0), 1


def reference(plain, states, openings, over_state, budget, episode_moves=0, base=0, stride=0, only=None):
    """The concatenation of plain runs.  plain(batch states, live lanes, n_moves, game_id_base) -> (gselfplay_util.Run with examples,
    sims, predicts or None): a plain run of the whole batch in which every lane but the live ones holds the finished position
    `over_state`.  Lanes with the same number of moves to go share a run, so the sums of sims and predicts are exact.  `only`: the lanes
    to follow (the others are left as they are)."""
    G = len(states)
    stride = stride or G
    out = Lanes(G)
    left = [budget] * G
    for g in range(G):
        out.states[g] = bytes(states[g])
    alive = [g for g in (range(G) if only is None else only) if states[g].status == abi.ONGOING]
    k = 0
    while alive:
        cur = states if k == 0 else openings
        groups = collections.defaultdict(list)
        for g in alive:
            groups[min(left[g], episode_moves) if episode_moves else left[g]].append(g)
        nxt = []
        for L, lanes in sorted(groups.items()):
            batch = (TaflState * G)(*[cur[g] if g in lanes else over_state for g in range(G)])
            run, sims, predicts = plain(batch, lanes, L, base + k * stride)
            out.sims += sims
            out.predicts = None if predicts is None or out.predicts is None else out.predicts + predicts
            for g in lanes:
                made = run.moves[g]
                assert made <= L and len(run.examples[g]) == made
                out.plays[g] += [run.plays[m][g] for m in range(made)]
                out.states[g] = run.states[g]
                left[g] -= made
                st = TaflState.from_buffer_copy(run.states[g])
                over = st.status != abi.ONGOING
                out.ended[g] += over
                if left[g] == 0:                                    # the budget is used up: the episode stays open
                    out.examples[g] += [(f, 0.0, 0) for f in run.examples[g]]
                    out.ended_on_last[g] = over
                    out.budget_cut[g] = (not over) and k > 0 and not (episode_moves and made == episode_moves)
                elif over or (episode_moves and made == episode_moves):
                    out.examples[g] += [(f,) + (outcome(run.states[g], f[1]) if over else (0.0, 0)) for f in run.examples[g]]
                    out.episodes[g] += 1
                    out.open_from[g] = len(out.examples[g])
                    out.capped[g] += not over
                    out.counters[3 if not over else 2 if st.status == abi.DRAW else 1 if st.winner == abi.DEFENDER else 0] += 1
                    if openings[g].status == abi.ONGOING:
                        nxt.append(g)
                else:                                               # a fault, or a root without a visited edge: the lane stops
                    out.examples[g] += [(f, 0.0, 0) for f in run.examples[g]]
        alive = sorted(nxt)
        k += 1
    return out


def oracle_plain(orc, lg, wb, S, c_puct, salts, sample_seed, temp_moves):
    """The plain route on the oracle loop (gselfplay_util.oracle_run); it counts simulations, not predicts."""
    def plain(batch, lanes, L, base):
        run = gsu.oracle_run(orc, lg, batch, wb, S, c_puct, salts, L, sample_seed, temp_moves, base=base, games=lanes)
        return run, run.sims, None
    return plain


def host_plain(rules, n, wb, S, c_puct, salts, sample_seed, temp_moves, edges_per_node=256, max_moves=None, K=None):
    """The plain route on the host harness (tests/hostsim: hsg_*, the loop of gselfplay_util.host_run), with the predicts of the run."""
    def plain(batch, lanes, L, base):
        H = gsu.hlib()
        G, A = len(batch), abi.action_size(n)
        ex = gsu.HostExamples(n, G, max_moves or L, K or S)
        rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
        o = TaflSelfplayOpts(sample_seed, temp_moves, 0, 0)
        h = H.hsg_begin(C.byref(rc), n, wb, batch, G, S, edges_per_node, c_puct, C.byref(o), L, base, ex.h)
        assert h
        try:
            boards, sides, waiting = (C.c_uint8 * (G * n * n))(), (C.c_uint8 * G)(), (C.c_uint8 * G)()
            H.hsg_leaves(h, boards, sides, waiting)
            while sum(waiting):
                pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
                H.hsg_step(h, gsu.fptr(pri), gsu.fptr(val))
                H.hsg_leaves(h, boards, sides, waiting)
            st, plays, moves, cnt, faults = (TaflState * G)(), (TaflPlay * (G * L))(), (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint8 * G)()
            H.hsg_end(h, st, plays, moves, cnt, faults)
        finally:
            H.hsg_free(h)
        run = gsu.Run(G, L)
        run.plays = [[pu.play_tuple4(plays[m * G + g]) for g in range(G)] for m in range(L)]
        run.states, run.moves = [bytes(st[g]) for g in range(G)], list(moves)
        run.examples, _over = ex.all()
        return run, cnt[0], cnt[1]
    return plain


def assert_same(got: Lanes, want: Lanes, where="", games=None):
    """Everything, or with `games` what those lanes left."""
    G = len(want.states)
    for g in (range(G) if games is None else games):
        assert got.plays[g] == want.plays[g], (where, "plays", g, got.plays[g], want.plays[g])
        assert got.states[g] == want.states[g], (where, "state", g)
        assert len(got.examples[g]) == len(want.examples[g]), (where, "examples", g, len(got.examples[g]), len(want.examples[g]))
        for j, (a, b) in enumerate(zip(got.examples[g], want.examples[g])):
            assert a == b, (where, "example", g, j, a, b)
        assert got.episodes[g] == want.episodes[g], (where, "episodes", g)
    if games is not None:
        return
    assert list(got.episodes) == list(want.episodes), (where, "episodes", list(got.episodes), want.episodes)
    assert list(got.counters) == list(want.counters), (where, "counters", list(got.counters), want.counters)
    assert got.sims == want.sims, (where, "sims", got.sims, want.sims)
    if want.predicts is not None:
        assert got.predicts == want.predicts, (where, "predicts", got.predicts, want.predicts)


def lanes_of(G, n_moves, plays, moves, states, episodes, counters, sims, predicts, examples):
    """Lanes from the flat outputs of a run: plays [m * G + g]; every play beyond a lane's moves must be all-zero."""
    out = Lanes(G)
    for g in range(G):
        col = [pu.play_tuple4(plays[m * G + g]) for m in range(n_moves)]
        assert all(p == ZERO_PLAY for p in col[moves[g]:]), ("a play beyond the moves made", g)
        out.plays[g] = col[:moves[g]]
        out.states[g] = bytes(states[g])
    out.episodes, out.counters, out.sims, out.predicts, out.examples = list(episodes), list(counters), sims, predicts, examples
    return out


# ---- the host harness (tests/hostsim_episodes) ---------------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_episodes")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_episodes.so"))
        P, u8, u32, u64, vp, dbl = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double
        L.hse_begin.restype = vp
        L.hse_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), P(TaflState), u32, u32, u32, dbl, P(TaflRootNoise), P(TaflSelfplayOpts), u32, u64, u64, u32, vp]
        L.hse_free.restype = None; L.hse_free.argtypes = [vp]
        L.hse_step.restype = u32; L.hse_step.argtypes = [vp, P(C.c_float), P(C.c_float)]
        L.hse_leaves.restype = None; L.hse_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hse_end.restype = None; L.hse_end.argtypes = [vp, P(TaflState), P(TaflPlay), P(u32), P(u64), P(u8), P(u32), P(u64)]
        L.hse_ex_new.restype = vp; L.hse_ex_new.argtypes = [u32, u8, u32, u32]
        L.hse_ex_free.restype = None; L.hse_ex_free.argtypes = [vp]
        L.hse_ex_counts.restype = None; L.hse_ex_counts.argtypes = [vp, P(u32), P(u64), P(u32)]
        L.hse_ex_example.restype = C.c_int; L.hse_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32), P(C.c_float), P(u8)]
        L.hse_ex_finalize.restype = C.c_int; L.hse_ex_finalize.argtypes = [vp, u32, P(TaflState)]
        _HLIB = L
    return _HLIB


class HostExamples:
    """tafl_examples with its open_from array on host memory (ExEp of hostsim_episodes.cpp)."""

    def __init__(self, n, G, max_moves, K):
        self.n, self.G, self.max_moves, self.K = n, G, max_moves, K
        self.h = hlib().hse_ex_new(G, n, max_moves, K)

    def __del__(self):
        if getattr(self, "h", None):
            hlib().hse_ex_free(self.h)
            self.h = None

    def counts(self):
        """(examples per lane, {dropped, overflowed}, open_from per lane)."""
        ln, ct, of = (C.c_uint32 * self.G)(), (C.c_uint64 * 4)(), (C.c_uint32 * self.G)()
        hlib().hse_ex_counts(self.h, ln, ct, of)
        return list(ln), {"dropped": ct[0], "overflowed": ct[1]}, list(of)

    def all(self):
        """Per lane, in column order: (Example.fields() tuple, z, final); and the overflow marks."""
        lens, _, _ = self.counts()
        out, over = [[] for _ in range(self.G)], [[] for _ in range(self.G)]
        for g in range(self.G):
            for j in range(min(lens[g], self.max_moves)):
                out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (self.n * self.n))()
                acts, vis, z, fin = (C.c_uint32 * self.K)(), (C.c_uint32 * self.K)(), C.c_float(), C.c_uint8()
                assert hlib().hse_ex_example(self.h, j * self.G + g, out5, board, acts, vis, C.byref(z), C.byref(fin)) == 0, (j, g)
                k = out5[0]
                rows = [list(board[r * self.n:(r + 1) * self.n]) for r in range(self.n)]
                out[g].append(((rows, out5[1], list(acts[:k]), list(vis[:k]), out5[3], out5[4]), float(z.value), int(fin.value)))
                over[g].append(out5[2])
        return out, over

    def finalize(self, wb, states):
        assert hlib().hse_ex_finalize(self.h, wb, states) == 0


def host_episodes(rules, n, wb, states, S, c_puct, salts, budget, sample_seed, temp_moves, ex, base=0, stride=0, episode_moves=0, openings=None, noise=None,
                  edges_per_node=256):
    """tafl_gselfplay_begin_episodes / the step loop / tafl_gselfplay_end on the harness with the stub network: (Lanes with the examples
    of `ex`, fault flags per lane, rounds)."""
    L = hlib()
    G, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(sample_seed, temp_moves, 0, 0)
    h = L.hse_begin(C.byref(rc), n, wb, states, openings, G, S, edges_per_node, c_puct, C.byref(noise) if noise is not None else None, C.byref(o), budget, base, stride,
                    episode_moves, ex.h if ex is not None else None)
    assert h
    try:
        boards, sides, waiting = (C.c_uint8 * (G * n * n))(), (C.c_uint8 * G)(), (C.c_uint8 * G)()
        L.hse_leaves(h, boards, sides, waiting)
        w, rounds = sum(waiting), 0
        while w:
            pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
            w = L.hse_step(h, gsu.fptr(pri), gsu.fptr(val))
            L.hse_leaves(h, boards, sides, waiting)
            assert sum(waiting) == w                                     # a reopened root is counted and served in the same round
            rounds += 1
        st, plays, moves, c4, faults = (TaflState * G)(), (TaflPlay * (G * budget))(), (C.c_uint32 * G)(), (C.c_uint64 * 4)(), (C.c_uint8 * G)()
        eps, ec = (C.c_uint32 * G)(), (C.c_uint64 * 4)()
        L.hse_end(h, st, plays, moves, c4, faults, eps, ec)
    finally:
        L.hse_free(h)
    examples = ex.all()[0] if ex is not None else [[] for _ in range(G)]
    out = lanes_of(G, budget, plays, list(moves), st, eps, ec, c4[0], c4[1], examples)
    out.abi_states, out.stat_faults = st, c4[3]
    return out, list(faults), rounds


def device_examples(ex, G, n):
    """Per lane, in column order: (Example.fields() tuple, z, final) read back from the device; and the overflow marks."""
    lens, total = ex.counts()
    lens = list(lens)
    assert total == sum(lens)
    idx = np.array([j * G + g for g in range(G) for j in range(lens[g])], np.uint32)
    out, over = [[] for _ in range(G)], [[] for _ in range(G)]
    if idx.size:
        nc, ov, pl, mv, acts, vis = ex.read(idx)
        boards, sides, _pi, z, fin = ex.gather(idx)
        for i, e in enumerate(idx):
            g, k = int(e) % G, int(nc[i])
            out[g].append(((boards[i].tolist(), int(sides[i]), acts[i, :k].tolist(), vis[i, :k].tolist(), int(pl[i]), int(mv[i])), float(z[i]), int(fin[i])))
            over[g].append(int(ov[i]))
    return out, over


def set_noise(batch, noise):
    """`noise` (a TaflRootNoise, or None: off) as the setting of the batch; a run latches it at its begin and keys it by its own ids."""
    if noise is None:
        batch.clear_root_noise()
    else:
        batch.set_root_noise(noise.alpha, noise.epsilon, noise.seed, noise.game_id_base, noise.move_no)


def device_episodes(batch, ex, n, S, c_puct, salts, budget, sample_seed, temp_moves, base=0, stride=0, episode_moves=0, openings=None, edges_per_node=256, noise=None):
    """The same loop through the C-ABI on `batch` (states uploaded), the stub network in host buffers: (Lanes, overflow marks, stats)."""
    G, A = batch.n, abi.action_size(n)
    set_noise(batch, noise)
    batch.gselfplay_begin_episodes(ex, budget, S, c_puct, edges_per_node, game_id_base=base, sample_seed=sample_seed, temp_moves=temp_moves,
                                   episode_moves=episode_moves, id_stride=stride, openings=openings)
    w = batch.gselfplay_step()
    while w:
        boards, sides, waiting = batch.gmcts_leaves()
        assert sum(waiting) == w
        pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
        w = batch.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
    plays, moves = batch.gselfplay_end()
    stats = batch.gmcts_stats()
    eps, es = batch.gselfplay_episode_stats()
    examples, over = device_examples(ex, G, n) if ex is not None else ([[] for _ in range(G)], None)
    out = lanes_of(G, budget, plays, list(moves), batch.download(), eps, (es.attacker_wins, es.defender_wins, es.draws, es.cut), stats.sims, stats.predicts, examples)
    return out, over, stats


def device_plain(glg, n, S, c_puct, salts, sample_seed, temp_moves, edges_per_node=256, noise=None):
    """The plain route on the library: tafl_gselfplay_begin on a batch and an examples object of its own, through the existing entry points."""
    def plain(batch_states, lanes, L, base):
        G = len(batch_states)
        b = glg.new_batch(G)
        b.upload(batch_states)
        set_noise(b, noise)
        ex = glg.new_examples(G, L, S)
        run, over, stats = gsu.device_run(b, ex, n, S, c_puct, salts, L, sample_seed, temp_moves, base=base, edges_per_node=edges_per_node)
        assert not any(any(o) for o in over)
        ex.close(); b.close()
        return run, stats.sims, stats.predicts
    return plain


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
_SETUP = {}


def setup(orc, cfg="brandubh7", G=G0, modulus=MODULUS):
    """(rules, n, wb, oracle logic, states [G], salts, a finished position)."""
    key = (cfg, G, modulus)
    if key not in _SETUP:
        from tests import noise_util as nu
        rules, fen, wb = pu.CONFIGS[cfg]
        n = abi.fen_side_len(fen)
        lg = orc.GameLogic(rules, n)
        states = gsu.start_states(orc, lg, rules, fen, wb, G, modulus)
        over = lg.random_advance(orc.GameState(fen, rules.starting_side, wb), 77, 0, nu.CRAFTED[cfg][0]).to_abi()
        assert over.status != abi.ONGOING
        _SETUP[key] = (rules, n, wb, lg, states, [(3 * g + 1) % 256 for g in range(G)], over)
    return _SETUP[key]
