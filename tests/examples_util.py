"""Expected values for the training-example tests (include/taflhip.h tafl_selfplay_record), from the oracle and
from Python restatements of the build-defined rules - never from the code under test - and the front end of the host harness's
recording run (tests/hostsim, hsx_*: the product's per-game functions compiled for the CPU)."""
import ctypes as C

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflMctsStats, TaflPlay, TaflSelfplayOpts, TaflState
from tests import parity_util as pu
from tests.hostsim import hostsim

M32 = 0xFFFFFFFF
DRAW_Z = np.float32(1e-4)


# ---- the RNG words (tafl_core.hpp: fmix32 / game_key / sim_key / ply_rand), restated ---------------------------------------------
def fmix32(h):
    h &= M32; h ^= h >> 16; h = (h * 0x85EBCA6B) & M32; h ^= h >> 13; h = (h * 0xC2B2AE35) & M32; h ^= h >> 16
    return h


def game_key(seed, gid):
    f = fmix32
    slo, shi, glo, ghi = seed & M32, (seed >> 32) & M32, gid & M32, (gid >> 32) & M32
    h0 = f(slo ^ f(shi + 0x9E3779B9)); h1 = f(shi ^ f(slo + 0x7F4A7C15))
    lo = f(f(h0 ^ glo) + ghi); hi = f(f(h1 ^ ghi) + glo * 0x9E3779B1)
    return lo | (hi << 32)


def sim_key(gk, sim):
    return fmix32((gk & M32) ^ ((sim * 0x9E3779B1 + 0x7F4A7C15) & M32)) ^ fmix32(((gk >> 32) + sim * 0x85EBCA77 + 0x165667B1) & M32)


def ply_rand(sk, ply):
    return fmix32((sk + ply * 0x85EBCA77) & M32)


def sample_word(sample_seed, gid, move_no):
    """r of include/taflhip.h: ply_rand(sim_key(game_key(sample_seed, gid), M), 0)."""
    return ply_rand(sim_key(game_key(sample_seed, gid), move_no), 0)


def pick_rule(visits, r):
    """k = (r * N) >> 32; the first child whose running sum of Nsa exceeds k."""
    k = (r * sum(visits)) >> 32
    run = 0
    for j, v in enumerate(visits):
        run += v
        if run > k:
            return j
    raise AssertionError("no child drawn")


# ---- symmetries, restated from the header ------------------------------------------------------------------------------------
def sym_rc(n, r, c, k):
    if k & 4:
        r, c = c, r
    if k & 1:
        r = n - 1 - r
    if k & 2:
        c = n - 1 - c
    return r, c


def action_tiles(n, a):
    """include/taflhip.h "dense action space": action -> ((r, c), (r2, c2))."""
    nm = n - 1
    t, s = divmod(a, 2 * nm)
    r, c = divmod(t, n)
    if s < nm - r:
        return (r, c), (r + s + 1, c)
    if s < nm:
        return (r, c), (r - (s - (nm - r) + 1), c)
    if s < nm + (nm - c):
        return (r, c), (r, c + (s - nm + 1))
    return (r, c), (r, c - (s - nm - (nm - c) + 1))


def tiles_action(n, frm, to):
    nm = n - 1
    (r, c), (r2, c2) = frm, to
    if c2 == c:
        s = (r2 - r - 1) if r2 > r else (nm - r) + (r - r2) - 1
    else:
        s = nm + (c2 - c) - 1 if c2 > c else nm + (nm - c) + (c - c2) - 1
    return (r * n + c) * 2 * nm + s


def sym_action_py(n, a, k):
    frm, to = action_tiles(n, a)
    return tiles_action(n, sym_rc(n, *frm, k), sym_rc(n, *to, k))


def sym_board_np(board, k):
    """The board under symmetry k with numpy: .T, np.flipud, np.fliplr in the stated order."""
    b = np.asarray(board)
    if k & 4:
        b = b.T
    if k & 1:
        b = np.flipud(b)
    if k & 2:
        b = np.fliplr(b)
    return np.ascontiguousarray(b)


# ---- the oracle loop ----------------------------------------------------------------------------------------------------------
class Example:
    __slots__ = ("board", "side", "actions", "visits", "played", "move_no", "z", "final")

    def fields(self):
        return (self.board, self.side, self.actions, self.visits, self.played, self.move_no)


def z_of(state: TaflState, side):
    """(z, final) of an example whose side to move was `side`, from the game's state."""
    if state.status == abi.ONGOING:
        return np.float32(0.0), 0
    if state.status == 2:
        return DRAW_Z, 1
    return np.float32(1.0 if state.winner == side else -1.0), 1


def oracle_record(orc, lg, states, G, wb, sims, cap, cpuct, seed, base, n_moves, sample_seed, temp_moves, move_base=0, sim_offset=0,
                  max_children=256, ids=None, workers=0):
    """The loop tafl_selfplay_record replaces, on the oracle.  Per move: orc.batch_mcts (sim_offset + m * sims), the pick by the rule
    restated above, the example from GameState.board_to_matrix() and the visited root children, orc.batch_step.  `states` is advanced in
    place.  ids: global game ids per state (default base + g).  workers: the searches of a move run game by game, side by side on that
    many host threads (the same children: a search is a function of its position and its global id).  Returns (plays [m][g], examples
    per game, info) with info = {non_argmax, game_moves, widest, searches}; searches: the (game, move) pairs whose game was ONGOING."""
    n = states[0].side_len
    plays_all, ex = [], [[] for _ in range(G)]
    info = {"non_argmax": 0, "game_moves": 0, "widest": 0, "searches": 0}
    for m in range(n_moves):
        p = TaflMctsParams(sims, cap, cpuct, seed, sim_offset + m * sims, 0)
        info["searches"] += sum(states[g].status == abi.ONGOING for g in range(G))
        if ids is None and not workers:
            kids, cnt, _ = orc.batch_mcts(lg, states, G, wb, p, base, max_children)
        else:
            jobs = [(g, states[g], ids[g] if ids is not None else base + g) for g in range(G)]
            per = pu.oracle_children_parallel(orc, lg, wb, p, jobs, max_children, workers or 16)
        sub = (TaflPlay * G)()
        row = []
        for g in range(G):
            if ids is None and not workers:
                ch = [(kids[g * max_children + j].action, kids[g * max_children + j].visits) for j in range(cnt[g])]
            else:
                ch = [(a, v) for a, v, _ in per[g]]
            vs = [v for _, v in ch]
            if vs and max(vs) > 0 and states[g].status == abi.ONGOING:
                first_max = vs.index(max(vs))
                M = move_base + m
                gid = ids[g] if ids is not None else base + g
                j = pick_rule(vs, sample_word(sample_seed, gid, M)) if M < temp_moves else first_max
                info["game_moves"] += 1
                info["non_argmax"] += j != first_max
                info["widest"] = max(info["widest"], len(ch))
                e = Example()
                e.board = orc.GameState.from_abi(states[g], wb).board_to_matrix()
                e.side = states[g].side_to_play
                e.actions, e.visits = [a for a, _ in ch], vs
                e.played, e.move_no = ch[j][0], M
                ex[g].append(e)
                play = abi.action_decode(n, ch[j][0])
                C.memmove(C.byref(sub[g]), C.byref(play), C.sizeof(TaflPlay))
                row.append(pu.play_tuple4(play))
            else:
                row.append((0, 0, 0, 0))
        orc.batch_step(lg, states, G, wb, sub)
        plays_all.append(row)
    for g in range(G):
        for e in ex[g]:
            e.z, e.final = z_of(states[g], e.side)
    return plays_all, ex, info


def dense_pi(n, e: Example, k=0):
    """The gather row of an example: np.float32(np.float64(Nsa) / np.float64(N)) at sigma(action), zeros elsewhere."""
    row = np.zeros(abi.action_size(n), np.float32)
    N = np.float64(sum(e.visits))
    for a, v in zip(e.actions, e.visits):
        row[sym_action_py(n, a, k)] = np.float32(np.float64(v) / N)
    return row


# ---- the host harness ---------------------------------------------------------------------------------------------------------
hlib = hostsim.lib


class HostExamples(hostsim.HostExamples):
    """tafl_examples on host memory + the recording run, finalize and gather of the harness."""

    def __init__(self, rules, n, wb, G, max_moves, K):
        self.rules = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
        self.wb = wb
        super().__init__(n, G, max_moves, K)

    def record(self, states, params, n_moves, base, sample_seed, temp_moves, move_base=0, spec=(4, 0, 0), record=True):
        plays, stats = (TaflPlay * (self.G * n_moves))(), TaflMctsStats()
        o = TaflSelfplayOpts(sample_seed, temp_moves, move_base, 0)
        rc = hlib().hsx_record(C.byref(self.rules), self.n, self.wb, states, self.G, C.byref(params), base, n_moves, C.byref(o),
                               self.h if record else None, plays, C.byref(stats), *spec)
        assert rc == 0, rc
        return plays, stats

    def finalize(self, states):
        assert hlib().hsx_finalize(self.h, self.n, self.wb, states) == 0

    def example(self, j, g):
        """Example (j, g) as the tuple Example.fields() gives + (overflow, z, final)."""
        z, fin = C.c_float(), C.c_uint8()
        fields, overflow = self._example(j, g, C.byref(z), C.byref(fin))
        return fields, overflow, np.float32(z.value), fin.value

    def gather(self, index, sym=None):
        idx = np.ascontiguousarray(index, np.uint32)
        k, n, A = idx.size, self.n, abi.action_size(self.n)
        sy = None if sym is None else np.ascontiguousarray(sym, np.uint8)
        boards, sides = np.full((k, n, n), 0xAA, np.uint8), np.full(k, 0xAA, np.uint8)
        pi, z, fin = np.full((k, A), 7.0, np.float32), np.full(k, 7.0, np.float32), np.full(k, 0xAA, np.uint8)
        vp = C.c_void_p
        bad = hlib().hsx_gather(self.h, idx.ctypes.data_as(vp), sy.ctypes.data_as(vp) if sy is not None else None, k, boards.ctypes.data_as(vp),
                                sides.ctypes.data_as(vp), pi.ctypes.data_as(vp), z.ctypes.data_as(vp), fin.ctypes.data_as(vp))
        return (boards, sides, pi, z, fin), bad


def check_examples(get_example, lens, want, G, where=""):
    """lens[g] and every field of every example against the oracle loop's (`want`: examples per game, with z / final)."""
    for g in range(G):
        assert lens[g] == len(want[g]), (where, g, lens[g], len(want[g]))
        for j, e in enumerate(want[g]):
            got, overflow, z, fin = get_example(j, g)
            assert got == e.fields(), (where, g, j, got, e.fields())
            assert overflow == 0 and z == e.z and fin == e.final, (where, g, j, overflow, z, e.z, fin, e.final)
