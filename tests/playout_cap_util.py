"""Expected values and drivers for playout cap randomization in guided self-play (include/taflhip.h tafl_playout_cap, DESIGN.md section
17): the class rule restated with the RNG words of tests/examples_util.py, the chain of one-move oracle runs, the per-move composition of
two uncapped one-move runs (one at S recording, one at fast_sims not recording) from any route - the existing host harnesses or the
library's own tafl_gselfplay_begin on a second batch - and the drivers of the host harness (tests/hostsim_caps) and of the library.  The
coverage conditions of the tests are asserted on the expectation, never on the code under test."""
import collections
import ctypes as C
import os
import subprocess

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflPlayoutCap, TaflRootNoise, TaflSelfplayOpts, TaflState
from tests import episodes_util as epu
from tests import examples_util as eu
from tests import gselfplay_util as gsu
from tests import parity_util as pu

G, S, FAST, FULL_PER, TEMP = 72, 16, 4, 16384, 4
CPUCT, SSEED, IDS = epu.CPUCT, epu.SSEED, epu.IDS
# per layout: (modulus of the openings rule, S, lane budget): tests/test_gpu_episodes.SHAPES
SHAPES = {"brandubh7": (60, 16, 20), "copenhagen11": (500, 16, 12), "copenhagen13": (500, 16, 20)}
# the cap seed per layout, chosen on the CPU so that the conditions of tests/test_hostsim_playout_cap.py hold on the expectation
CAP_SEED = {"brandubh7": 3, "copenhagen11": 3, "copenhagen13": 3}
CAP_KEY = 0x504C41594F555443


def is_full(seed, gid, move_no, full_per=FULL_PER):
    """The class of move `move_no` of game `gid`: (w >> 16) < full_per_65536, w = ply_rand(sim_key(game_key(seed, gid) ^ CAP_KEY, M), 0)."""
    return (eu.ply_rand(eu.sim_key(eu.game_key(seed, gid) ^ CAP_KEY, move_no), 0) >> 16) < full_per


def cap_of(cfg, full_per=FULL_PER, fast=FAST):
    return TaflPlayoutCap(CAP_SEED[cfg], fast, full_per, 0)


def shape(orc, cfg):
    """(rules, n, wb, oracle logic, states [72], salts, a finished position, S, budget)."""
    modulus, S_, budget = SHAPES[cfg]
    return epu.setup(orc, cfg, G, modulus) + (S_, budget)


def _plain(lanes):
    """A plain run writes no z and no final: its examples compare by their fields."""
    lanes.examples = [[(f, 0.0, 0) for f, _z, _fin in col] for col in lanes.examples]
    return lanes


# ---- the expectations -------------------------------------------------------------------------------------------------------------------
def oracle_chain(orc, lg, wb, states, salts, budget, seed, full_per, fast, spots, base=0, move_base=0, S_=S):
    """The capped plain run of the lanes `spots` as a chain of one-move oracle runs (gselfplay_util.oracle_run with n_moves = 1,
    move_base = M, S = the cap of the class of (gid, M)): epu.Lanes with .moves and .classes."""
    n_lanes = len(states)
    out = epu.Lanes(n_lanes)
    out.moves, out.classes = [0] * n_lanes, [[] for _ in range(n_lanes)]
    for g in spots:
        cur = (TaflState * n_lanes)(*states)
        for m in range(budget):
            if cur[g].status != abi.ONGOING:
                break
            M = move_base + m
            full = is_full(seed, base + g, M, full_per)
            run = gsu.oracle_run(orc, lg, cur, wb, S_ if full else fast, CPUCT, salts, 1, SSEED, TEMP, move_base=M, base=base, games=[g])
            if run.moves[g] == 0:
                break
            out.sims += S_ if full else fast
            out.plays[g].append(run.plays[0][g])
            out.classes[g].append(full)
            if full:
                out.examples[g].append((run.examples[g][0], 0.0, 0))
            cur[g] = TaflState.from_buffer_copy(run.states[g])
            out.moves[g] = m + 1
        out.states[g] = bytes(cur[g])
    return out


def composition(route, states, over_state, budget, seed, full_per, episodes, base=0, stride=0, episode_moves=0, move_base=0, openings=None):
    """The capped run as the per-move merge of uncapped one-move runs.  route(batch states, lanes, full, game_id_base, M) -> (a
    gselfplay_util.Run of ONE move with move_base = M in which every lane but `lanes` holds `over_state` - at S simulations, recording and
    with the run's noise when `full`, at fast_sims, not recording and without noise otherwise -, sims, predicts).  Every lane takes the
    state, the play and the example of the route of its class; closing, cutting and reopening are done here as
    episodes_util.reference does them.  Returns epu.Lanes with .moves, .classes, .full, .fast and .closed (examples per closed episode)."""
    n_lanes = len(states)
    stride = stride or n_lanes
    openings = states if openings is None else openings
    out = epu.Lanes(n_lanes)
    out.moves, out.classes, out.full, out.fast, out.closed, out.open_at_budget = [0] * n_lanes, [[] for _ in range(n_lanes)], 0, 0, [], [False] * n_lanes
    cur = [TaflState.from_buffer_copy(bytes(s)) for s in states]
    k, m_ep, seg = [0] * n_lanes, [0] * n_lanes, [[] for _ in range(n_lanes)]
    alive = [g for g in range(n_lanes) if states[g].status == abi.ONGOING]
    while alive:
        groups = collections.defaultdict(list)
        for g in alive:
            gb, M = (base + k[g] * stride, m_ep[g]) if episodes else (base, move_base + out.moves[g])
            groups[(gb, M, is_full(seed, gb + g, M, full_per))].append(g)
        nxt = []
        for (gb, M, full), lanes in sorted(groups.items()):
            batch = (TaflState * n_lanes)(*[cur[g] if g in lanes else over_state for g in range(n_lanes)])
            run, sims, predicts = route(batch, lanes, full, gb, M)
            out.sims += sims
            out.predicts = None if predicts is None or out.predicts is None else out.predicts + predicts
            for g in lanes:
                assert len(run.examples[g]) == (run.moves[g] if full else 0)
                if run.moves[g] == 0:                               # a fault, or a root without a visited edge: the lane stops
                    continue
                out.plays[g].append(run.plays[0][g])
                cur[g] = TaflState.from_buffer_copy(run.states[g])
                out.moves[g] += 1
                m_ep[g] += 1
                out.classes[g].append(full)
                out.full, out.fast = out.full + full, out.fast + (not full)
                if full:
                    seg[g].append(run.examples[g][0])
                over = cur[g].status != abi.ONGOING
                if out.moves[g] == budget:                          # the budget is used up: the episode stays open
                    out.ended_on_last[g] = over
                    out.open_at_budget[g] = episodes and not over
                elif not episodes:
                    if not over:
                        nxt.append(g)
                elif over or (episode_moves and m_ep[g] == episode_moves):
                    out.examples[g] += [(f,) + (epu.outcome(bytes(cur[g]), f[1]) if over else (0.0, 0)) for f in seg[g]]
                    out.closed.append(len(seg[g]))
                    seg[g] = []
                    out.episodes[g] += 1
                    out.open_from[g] = len(out.examples[g])
                    out.counters[3 if not over else 2 if cur[g].status == abi.DRAW else 1 if cur[g].winner == abi.DEFENDER else 0] += 1
                    k[g], m_ep[g] = k[g] + 1, 0
                    if openings[g].status == abi.ONGOING:           # (otherwise the lane stops and its batch state stays)
                        cur[g] = TaflState.from_buffer_copy(bytes(openings[g]))
                        nxt.append(g)
                else:
                    nxt.append(g)
        alive = sorted(nxt)
    for g in range(n_lanes):
        out.examples[g] += [(f, 0.0, 0) for f in seg[g]]
        out.states[g] = bytes(cur[g])
    return out


def host_route(rules, n, wb, salts, fast, noise=None, S_=S):
    """The two uncapped one-move routes on the host: without noise the plain run of tests/hostsim (gselfplay_util.host_run), with noise
    the uncapped plain run of tests/hostsim_caps (the product's selfplay_step with its RootNoise argument)."""
    def route(batch, lanes, full, gb, M):
        sims = S_ if full else fast
        if noise is not None and full:
            ex = HostExamples(n, len(batch), 1, sims)
            got = host_capped(rules, n, wb, batch, sims, salts, 1, None, ex, episodes=False, base=gb, move_base=M, noise=noise)
            run = gsu.Run(len(batch), 1)
            run.plays, run.states, run.moves = [[(p[0] if p else (0, 0, 0, 0)) for p in got.plays]], got.states, got.moves
            run.examples = [[f for f, _z, _fin in col] for col in got.examples]
            return run, got.sims, got.predicts
        ex = gsu.HostExamples(n, len(batch), 1, sims) if full else None
        run, faults, _rounds = gsu.host_run(rules, n, wb, batch, sims, CPUCT, salts, 1, SSEED, TEMP, ex=ex, move_base=M, base=gb)
        assert not any(faults)
        run.examples = ex.all()[0] if full else [[] for _ in batch]
        return run, run.sims, None
    return route


def device_route(glg, n, salts, fast, noise=None, S_=S):
    """The two uncapped one-move routes on the library: tafl_gselfplay_begin with n_moves = 1 on a second batch (no cap set on it), the
    states of the move merged into it by tafl_batch_upload."""
    box = {}

    def route(batch, lanes, full, gb, M):
        n_lanes, A = len(batch), abi.action_size(n)
        if "b" not in box:
            box["b"], box["ex"] = glg.new_batch(n_lanes), glg.new_examples(n_lanes, 1, S_)
        b, ex = box["b"], box["ex"]
        b.upload(batch)
        b.clear_playout_cap()
        epu.set_noise(b, noise if full else None)
        ex.clear()
        b.gselfplay_begin(ex if full else None, 1, S_ if full else fast, CPUCT, 256, game_id_base=gb, sample_seed=SSEED, temp_moves=TEMP, move_base=M)
        w = b.gselfplay_step()
        while w:
            boards, sides, waiting = b.gmcts_leaves()
            pri, val = gsu.stub_rows(boards, sides, waiting, n_lanes, n, A, salts)
            w = b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        plays, moves = b.gselfplay_end()
        stats, st = b.gmcts_stats(), b.download()
        assert stats.faults == 0
        run = gsu.Run(n_lanes, 1)
        run.plays = [[pu.play_tuple4(plays[g]) for g in range(n_lanes)]]
        run.states, run.moves = [bytes(st[g]) for g in range(n_lanes)], list(moves)
        run.examples = gsu.device_examples(ex, n_lanes, n)[0] if full else [[] for _ in range(n_lanes)]
        return run, stats.sims, stats.predicts

    def close():
        for x in box.values():
            x.close()
        box.clear()
    route.close = close
    return route


# ---- the host harness (tests/hostsim_caps) -----------------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_caps")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_caps.so"))
        P, u8, u32, u64, vp, dbl = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double
        L.hsc_cap_check.restype = C.c_int; L.hsc_cap_check.argtypes = [P(TaflPlayoutCap), u32]
        L.hsc_is_full.restype = C.c_int; L.hsc_is_full.argtypes = [u64, u32, u64, u32]
        L.hsc_begin.restype = vp
        L.hsc_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), P(TaflState), u32, u32, u32, dbl, P(TaflRootNoise), P(TaflPlayoutCap), P(TaflSelfplayOpts), u32, u64,
                                C.c_int, u64, u32, vp]
        L.hsc_free.restype = None; L.hsc_free.argtypes = [vp]
        L.hsc_step.restype = u32; L.hsc_step.argtypes = [vp, P(C.c_float), P(C.c_float)]
        L.hsc_leaves.restype = None; L.hsc_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hsc_end.restype = None; L.hsc_end.argtypes = [vp, P(TaflState), P(TaflPlay), P(u32), P(u64), P(u8), P(u32), P(u64), P(u64)]
        L.hsc_ex_new.restype = vp; L.hsc_ex_new.argtypes = [u32, u8, u32, u32]
        L.hsc_ex_free.restype = None; L.hsc_ex_free.argtypes = [vp]
        L.hsc_ex_counts.restype = None; L.hsc_ex_counts.argtypes = [vp, P(u32), P(u64), P(u32)]
        L.hsc_ex_example.restype = C.c_int; L.hsc_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32), P(C.c_float), P(u8)]
        _HLIB = L
    return _HLIB


class HostExamples:
    """tafl_examples with its open_from array on host memory (ExEp of hostsim_caps.cpp)."""

    def __init__(self, n, n_lanes, max_moves, K):
        self.n, self.G, self.max_moves, self.K = n, n_lanes, max_moves, K
        self.h = hlib().hsc_ex_new(n_lanes, n, max_moves, K)

    def __del__(self):
        if getattr(self, "h", None):
            hlib().hsc_ex_free(self.h)
            self.h = None

    def counts(self):
        """(examples per lane, {dropped, overflowed}, open_from per lane)."""
        ln, ct, of = (C.c_uint32 * self.G)(), (C.c_uint64 * 4)(), (C.c_uint32 * self.G)()
        hlib().hsc_ex_counts(self.h, ln, ct, of)
        return list(ln), {"dropped": ct[0], "overflowed": ct[1]}, list(of)

    def all(self):
        """Per lane, in column order: (Example.fields() tuple, z, final)."""
        lens, _, _ = self.counts()
        out = [[] for _ in range(self.G)]
        for g in range(self.G):
            for j in range(min(lens[g], self.max_moves)):
                out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (self.n * self.n))()
                acts, vis, z, fin = (C.c_uint32 * self.K)(), (C.c_uint32 * self.K)(), C.c_float(), C.c_uint8()
                assert hlib().hsc_ex_example(self.h, j * self.G + g, out5, board, acts, vis, C.byref(z), C.byref(fin)) == 0, (j, g)
                assert out5[2] == 0, ("overflow", j, g)
                k = out5[0]
                rows = [list(board[r * self.n:(r + 1) * self.n]) for r in range(self.n)]
                out[g].append(((rows, out5[1], list(acts[:k]), list(vis[:k]), out5[3], out5[4]), float(z.value), int(fin.value)))
        return out


def host_capped(rules, n, wb, states, S_, salts, n_moves, cap, ex, episodes, base=0, stride=0, episode_moves=0, move_base=0, noise=None, openings=None,
                edges_per_node=256):
    """tafl_gselfplay_begin (episodes False) or tafl_gselfplay_begin_episodes with the cap `cap` (a TaflPlayoutCap; None: no cap) and the
    noise `noise` latched / the step loop / tafl_gselfplay_end on the harness with the stub network: epu.Lanes with the examples of `ex`
    and .moves, .cap_stats (full, fast), .faults, .stat_faults, .rounds."""
    L = hlib()
    n_lanes, A = len(states), abi.action_size(n)
    rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
    o = TaflSelfplayOpts(SSEED, TEMP, move_base, 0)
    h = L.hsc_begin(C.byref(rc), n, wb, states, openings, n_lanes, S_, edges_per_node, CPUCT, C.byref(noise) if noise is not None else None,
                    C.byref(cap) if cap is not None else None, C.byref(o), n_moves, base, 1 if episodes else 0, stride, episode_moves, ex.h if ex is not None else None)
    assert h
    try:
        boards, sides, waiting = (C.c_uint8 * (n_lanes * n * n))(), (C.c_uint8 * n_lanes)(), (C.c_uint8 * n_lanes)()
        L.hsc_leaves(h, boards, sides, waiting)
        w, rounds = sum(waiting), 0
        while w:
            pri, val = gsu.stub_rows(boards, sides, waiting, n_lanes, n, A, salts)
            w = L.hsc_step(h, gsu.fptr(pri), gsu.fptr(val))
            L.hsc_leaves(h, boards, sides, waiting)
            assert sum(waiting) == w
            rounds += 1
        st, plays, moves, c4, faults = (TaflState * n_lanes)(), (TaflPlay * (n_lanes * n_moves))(), (C.c_uint32 * n_lanes)(), (C.c_uint64 * 4)(), (C.c_uint8 * n_lanes)()
        eps, ec, cc = (C.c_uint32 * n_lanes)(), (C.c_uint64 * 4)(), (C.c_uint64 * 2)()
        L.hsc_end(h, st, plays, moves, c4, faults, eps, ec, cc)
    finally:
        L.hsc_free(h)
    examples = ex.all() if ex is not None else [[] for _ in range(n_lanes)]
    out = epu.lanes_of(n_lanes, n_moves, plays, list(moves), st, eps, ec, c4[0], c4[1], examples)
    out.moves, out.cap_stats, out.faults, out.stat_faults, out.rounds, out.terminal_hits = list(moves), (cc[0], cc[1]), list(faults), c4[3], rounds, c4[2]
    if ex is not None:
        out.open_from = ex.counts()[2]
    return out if episodes else _plain(out)


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def set_cap(batch, cap):
    if cap is None:
        batch.clear_playout_cap()
    else:
        from alphazeroforhnefatafl_amd._lib import check, lib
        check(lib().tafl_gselfplay_set_playout_cap(batch._h, C.byref(cap)))


def device_capped(batch, ex, n, S_, salts, n_moves, cap, episodes, base=0, stride=0, episode_moves=0, move_base=0, noise=None, openings=None, edges_per_node=256):
    """The same loop through the C-ABI on `batch` (states uploaded), the stub network in host buffers: epu.Lanes as host_capped returns
    them (.cap_stats None without a cap) and .stats."""
    n_lanes, A = batch.n, abi.action_size(n)
    epu.set_noise(batch, noise)
    set_cap(batch, cap)
    if episodes:
        batch.gselfplay_begin_episodes(ex, n_moves, S_, CPUCT, edges_per_node, game_id_base=base, sample_seed=SSEED, temp_moves=TEMP, episode_moves=episode_moves,
                                       id_stride=stride, openings=openings)
    else:
        batch.gselfplay_begin(ex, n_moves, S_, CPUCT, edges_per_node, game_id_base=base, sample_seed=SSEED, temp_moves=TEMP, move_base=move_base)
    w, rounds = batch.gselfplay_step(), 0
    while w:
        boards, sides, waiting = batch.gmcts_leaves()
        assert sum(waiting) == w
        pri, val = gsu.stub_rows(boards, sides, waiting, n_lanes, n, A, salts)
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
    out.moves, out.cap_stats, out.stat_faults, out.rounds, out.stats, out.terminal_hits = list(moves), (cs.full_moves, cs.fast_moves) if cs else None, stats.faults, rounds, stats, stats.terminal_hits
    return out if episodes else _plain(out)


def assert_equal(got, want, where="", games=None, predicts=True):
    """Plays, final states, examples (fields, order, z, final), episode counts and counters, moves per lane, sims (and predicts)."""
    if not predicts:
        keep, want.predicts = want.predicts, None
    try:
        epu.assert_same(got, want, where, games)
    finally:
        if not predicts:
            want.predicts = keep
    for g in (range(len(want.states)) if games is None else games):
        assert got.moves[g] == want.moves[g], (where, "moves", g, got.moves[g], want.moves[g])
