"""Value targets from search values (include/taflhip.h "value targets"): the expectation from the Python twins alone -
the per-move twins search_stats_util uses give (action, n', q, p) and hence `value` per example, the episode loop of
search_stats_util.twin_run gives the concatenation of episodes per lane, hence the boundaries, z, final and move_no - with the chain in
sequential float64 and lam_pow as the 16-step loop; and two drivers that leave the same structure: the host harness
(tests/hostsim_value_targets) and the library through the C-ABI.  Everything is compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlayoutCap, TaflSelfplayOpts, TaflSolver, TaflState, TaflValueTargetsCfg, TaflValueTargetsResult  # noqa: F401
from tests import examples_util as eu
from tests import forced_util as fu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import playout_cap_util as pcu
from tests import search_stats_util as ssu
from tests import solver_util as su

CPUCT, EDGES, SEED, TEMP, BASE = ssu.CPUCT, ssu.EDGES, ssu.SEED, ssu.TEMP, ssu.BASE
FAST, FULL_PER, CAP_SEED = 8, 32768, 3
G, MODULUS, S, BUDGET, K = 65, 60, 16, 20, 16
DRAW_Z = float(np.float32(1e-4))
# the runs of the issue: name -> settings
MODES = {
    "episodes": dict(episodes=True),
    "cut": dict(episodes=True, episode_moves=5),
    "cap_forced": dict(episodes=True, cap=True, k=fu.K),
    "noise": dict(episodes=True, noise=True),
    "solver": dict(episodes=True, solver=True),
}


class Entry:
    """One recorded example of the expectation: its search_stats_util.Row, ep_end, z and final as the run leaves them."""

    def __init__(self, row):
        self.row, self.ep_end, self.z, self.fin = row, 0, 0.0, 0


class Expect:
    """lanes[g]: the Entries of lane g; what the coverage conditions count."""

    def __init__(self, G_):
        self.lanes = [[] for _ in range(G_)]
        self.quiet_reopens = 0          # reopens in a round that appended no example (a fast move, or an episode that ended on one)
        self.empty_episodes = 0         # episodes that closed or were cut without a recorded example
        self.closed = self.cut = 0
        self.episodes_of = [0] * G_


def z_of(side, st):
    if st.status == abi.DRAW:
        return DRAW_Z
    return 1.0 if st.winner == side else -1.0


def twin(orc, lg, states, wb, salts, side, n_sims=S, n_moves=BUDGET, noise=False, cap=False, k=None, solver=False, episodes=False, episode_moves=0, base=BASE,
         move_base=0, into=None):
    """The loop of search_stats_util.twin_run with the episode bookkeeping kept: boundaries where the run reopens, z and final of the
    episodes it closes.  `into`: an Expect a former run left (the run continues its lanes; move numbers go on from move_base)."""
    n, G_ = lg.side_len, len(states)
    A = abi.action_size(n)
    out = into if into is not None else Expect(G_)
    for g in range(G_):
        lane = out.lanes[g]
        opening = orc.GameState.from_abi(states[g], wb)
        st, episode, m0, md, first = opening, 0, 0, 0, len(lane)
        predict = nu.predictor(A, salts[g])
        while md < n_moves and st.to_abi().status == abi.ONGOING:
            gid, M = base + episode * G_ + g, move_base + md - m0
            full = pcu.is_full(CAP_SEED, gid, M, FULL_PER) if cap else True
            nz = None
            if noise and full:
                one = (TaflState * 1)(st.to_abi())
                nz = (nu.EPSILON, side.eta(one, nu.noise_cfg(base=gid, move_no=M))[0])
            if solver:
                t, rows, j = su.one_move(lg, st, predict, gid, M, SEED, TEMP, su.Tally(), n_sims, k if full else None, nz, 0 if full else n_sims - FAST)
                kept = [(r[0], r[2], r[3]) for r in rows if r[2] > 0]
            elif k is not None and full:
                t, rows, j = fu.one_move(orc, lg, st, predict, gid, M, SEED, TEMP, k, nz, fu.Tally(), n_sims)
                kept = [(r[0], r[2], r[4]) for r in rows if r[2] > 0]
            else:
                t = nu.Twin(lg, st, CPUCT, predict, nz).run(n_sims if full else FAST)
                kept = t.kids()
                vs = [v for _a, v, _q in kept]
                j = None if not vs else (eu.pick_rule(vs, eu.sample_word(SEED, gid, M)) if M < TEMP else vs.index(max(vs)))
            if j is None:
                break
            if full:
                lane.append(Entry(ssu.Row([a for a, _v, _q in kept], [v for _a, v, _q in kept], [np.float32(ssu._f64(q)) for _a, _v, q in kept],
                                          [np.float32(t.root.ps[a]) for a, _v, _q in kept], kept[j][0], M, st.to_abi().side_to_play)))
            code, st, _eff = lg.do_play(abi.action_decode(n, kept[j][0]), st)
            assert code == 0
            md += 1
            over = st.to_abi().status != abi.ONGOING
            if episodes and md < n_moves and (over or (episode_moves and md - m0 >= episode_moves)):
                if over:
                    for en in lane[first:]:
                        en.z, en.fin = z_of(en.row.side, st.to_abi()), 1
                out.closed += over
                out.cut += not over
                out.quiet_reopens += not full
                out.empty_episodes += len(lane) == first
                out.episodes_of[g] += 1
                if lane:
                    lane[-1].ep_end = 1
                episode, m0, st, first = episode + 1, md, opening, len(lane)
    return out


def finalize(want, over):
    """tafl_examples_finalize against the finished positions `over`: the open tail of every lane (after its last boundary) is settled."""
    for g, lane in enumerate(want.lanes):
        tail = len(lane)
        while tail > 0 and not lane[tail - 1].ep_end:
            tail -= 1
        for en in lane[tail:]:
            en.z, en.fin = z_of(en.row.side, over[g]), 1


def lam_pow(lam, d):
    r, b = 1.0, float(lam)
    for bit in range(16):
        if (d >> bit) & 1:
            r = r * b
        b = b * b
    return r


class Targets:
    """vt (float32) and kind per (g, j), z / fin after the call, the four counters."""


def episodes_of(lane, limit):
    out, cur = [], []
    for j, en in enumerate(lane[:limit]):
        cur.append(j)
        if en.ep_end:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def targets(want, lam, settle=False, Kmax=None, max_moves=None):
    """The normative chain in sequential float64.  Kmax: examples with more stored children overflowed and take no part."""
    t = Targets()
    t.vt, t.kind, t.z, t.fin = {}, {}, {}, {}
    t.closed = t.unfinished = t.rows = t.settled = 0
    t.gaps = 0
    for g, lane in enumerate(want.lanes):
        limit = len(lane) if max_moves is None else min(len(lane), max_moves)
        for j in range(limit):
            t.vt[(g, j)], t.kind[(g, j)], t.z[(g, j)], t.fin[(g, j)] = np.float32(0.0), 0, np.float32(lane[j].z), lane[j].fin
        for ep in episodes_of(lane, limit):
            part = [j for j in ep if sum(lane[j].row.visits) > 0 and (Kmax is None or len(lane[j].row.visits) <= Kmax)]
            if not part:
                continue
            s = [1.0 if lane[j].row.side == abi.ATTACKER else -1.0 for j in part]
            u = [s[i] * float(lane[j].row.value()) for i, j in enumerate(part)]
            closed = lane[part[-1]].fin == 1
            t.closed += closed
            t.unfinished += not closed
            t.rows += len(part)
            Aacc, L = 0.0, 1.0
            for i in range(len(part) - 1, -1, -1):
                if i < len(part) - 1:
                    d = max(1, min(65535, lane[part[i + 1]].row.move_no - lane[part[i]].row.move_no))
                    t.gaps += d > 1
                    p = lam_pow(lam, d)
                    Aacc = (1.0 - p) * u[i + 1] + p * Aacc
                    L = p * L
                j = part[i]
                term = float(np.float32(lane[j].z)) if closed else s[i] * u[-1]
                t.vt[(g, j)], t.kind[(g, j)] = np.float32(s[i] * Aacc + L * term), 1 if closed else 2
                if settle and not closed:
                    t.z[(g, j)], t.fin[(g, j)] = np.float32(s[i] * u[-1]), 2
                    t.settled += 1
    return t


def coverage(want, lam=0.5):
    t = targets(want, lam)
    lanes = want.lanes
    tails = sum(1 for lane in lanes if lane and not lane[-1].ep_end)
    flips = sum(1 for g, lane in enumerate(lanes) for j, en in enumerate(lane) if t.kind[(g, j)] == 1 and float(t.vt[(g, j)]) * en.z < 0)
    return dict(closed=want.closed, cut=want.cut, tails=tails, three=sum(e + (1 if l and not l[-1].ep_end else 0) >= 3 for e, l in zip(want.episodes_of, lanes)),
                gaps=t.gaps, quiet=want.quiet_reopens, empty=want.empty_episodes, flips=flips, rows=t.rows)


# ---- the host harness (tests/hostsim_value_targets) --------------------------------------------------------------------------------------
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_value_targets")
_HLIB = None


def hlib():
    global _HLIB
    if _HLIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_value_targets.so"))
        P, u8, u32, u64, vp, dbl, f32 = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_void_p, C.c_double, C.c_float
        L.hvt_ex_new.restype = vp; L.hvt_ex_new.argtypes = [u32, u8, u32, u32]
        L.hvt_ex_free.restype = None; L.hvt_ex_free.argtypes = [vp]
        L.hvt_ex_clear.restype = None; L.hvt_ex_clear.argtypes = [vp]
        L.hvt_ex_valid.restype = C.c_int; L.hvt_ex_valid.argtypes = [vp]
        L.hvt_ex_stats.restype = vp; L.hvt_ex_stats.argtypes = [vp]
        L.hvt_begin.restype = vp
        L.hvt_begin.argtypes = [P(abi.TaflRules), u8, u32, P(TaflState), P(TaflState), u32, u32, u32, dbl, P(abi.TaflRootNoise), P(TaflPlayoutCap), P(abi.TaflForcedPlayouts),
                                P(TaflSolver), P(TaflSelfplayOpts), u32, u64, C.c_int, u64, u32, vp]
        L.hqs_begin.restype = vp; L.hqs_begin.argtypes = L.hvt_begin.argtypes
        L.hvt_run.restype = vp; L.hvt_run.argtypes = [vp]
        L.hqs_session.restype = vp; L.hqs_session.argtypes = [vp]
        L.hvt_free.restype = None; L.hvt_free.argtypes = [vp]
        L.hqs_free.restype = None; L.hqs_free.argtypes = [vp]
        L.hvt_step.restype = u32; L.hvt_step.argtypes = [vp, P(f32), P(f32)]
        L.hqs_step.restype = u32; L.hqs_step.argtypes = [vp, P(f32), P(f32)]
        L.hss_leaves.restype = None; L.hss_leaves.argtypes = [vp, P(u8), P(u8), P(u8)]
        L.hss_ex_counts.restype = None; L.hss_ex_counts.argtypes = [vp, P(u32), P(u64), P(u32)]
        L.hss_ex_example.restype = C.c_int; L.hss_ex_example.argtypes = [vp, u32, P(u32), P(u8), P(u32), P(u32), P(f32), P(u8)]
        L.hvt_ex_finalize.restype = None; L.hvt_ex_finalize.argtypes = [vp, P(TaflState)]
        L.hqs_ex_read_stats.restype = C.c_int; L.hqs_ex_read_stats.argtypes = [vp, vp, u32, vp, vp]
        L.hvt_value_targets.restype = C.c_int; L.hvt_value_targets.argtypes = [vp, P(TaflValueTargetsCfg), P(u64)]
        L.hvt_gather_targets.restype = C.c_int; L.hvt_gather_targets.argtypes = [vp, vp, u32, vp, vp, vp, C.c_int]
        L.hvt_pool_new.restype = vp; L.hvt_pool_new.argtypes = [u32, u32, u8]
        L.hvt_pool_free.restype = None; L.hvt_pool_free.argtypes = [vp]
        L.hvt_pool_weights.restype = vp; L.hvt_pool_weights.argtypes = [vp]
        L.hvt_pool_set_search_stats.restype = C.c_int; L.hvt_pool_set_search_stats.argtypes = [vp, C.c_int]
        L.hvt_pool_set_value_targets.restype = C.c_int; L.hvt_pool_set_value_targets.argtypes = [vp, C.c_int]
        L.hvt_pool_ingest.restype = C.c_int; L.hvt_pool_ingest.argtypes = [vp, vp, C.c_int, P(u64)]
        L.hvt_pool_gather_targets.restype = C.c_int; L.hvt_pool_gather_targets.argtypes = [vp, vp, u32, vp, vp, C.c_int]
        L.hspw_trim.restype = C.c_int; L.hspw_trim.argtypes = [vp, u32]
        L.hspw_clear.restype = None; L.hspw_clear.argtypes = [vp]
        L.hspw_pool.restype = vp; L.hspw_pool.argtypes = [vp]
        L.hsp_stats.restype = None; L.hsp_stats.argtypes = [vp, P(u64)]
        _HLIB = L
    return _HLIB


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class HostExamples:
    """The ExVt of the harness: runs record into it, the readers below read it."""

    def __init__(self, n, G_, max_moves, K_):
        self.L, self.n, self.G, self.max_moves, self.K = hlib(), n, G_, max_moves, K_
        self.h = self.L.hvt_ex_new(G_, n, max_moves, K_)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.hvt_ex_free(self.h)
            self.h = None

    def run(self, rules, wb, states, salts, n_sims=S, n_moves=BUDGET, noise=False, cap=False, k=None, solver=False, episodes=False, episode_moves=0, base=BASE, move_base=0,
            targets_on=True):
        """One run into the object; targets_on False: the same run through hqs_begin / hqs_step alone (nothing of this feature runs)."""
        L, n, G_ = self.L, self.n, len(states)
        A = abi.action_size(n)
        rc = rules.to_c() if isinstance(rules, abi.Ruleset) else rules
        o = TaflSelfplayOpts(SEED, TEMP, move_base, 0)
        nz = nu.noise_cfg() if noise else None
        cp = TaflPlayoutCap(CAP_SEED, FAST, FULL_PER, 0) if cap else None
        fc = fu.forced_cfg(k) if k is not None else None
        sc = TaflSolver(0) if solver else None
        ref = ssu._ref
        begin, step, sess, free = (L.hvt_begin, L.hvt_step, lambda h: L.hqs_session(L.hvt_run(h)), L.hvt_free) if targets_on else (L.hqs_begin, L.hqs_step, L.hqs_session, L.hqs_free)
        h = begin(C.byref(rc), n, wb, states, None, G_, n_sims, EDGES, CPUCT, ref(nz), ref(cp), ref(fc), ref(sc), C.byref(o), n_moves, base, 1 if episodes else 0, G_, episode_moves,
                  self.h if targets_on else L.hvt_ex_stats(self.h))
        assert h
        try:
            hs = sess(h)
            boards, sides, waiting = (C.c_uint8 * (G_ * n * n))(), (C.c_uint8 * G_)(), (C.c_uint8 * G_)()
            L.hss_leaves(hs, boards, sides, waiting)
            w = sum(waiting)
            while w:
                pri, val = gsu.stub_rows(boards, sides, waiting, G_, n, A, salts)
                w = step(h, gsu.fptr(pri), gsu.fptr(val))
                L.hss_leaves(hs, boards, sides, waiting)
        finally:
            free(h)

    def finalize(self, over):
        self.L.hvt_ex_finalize(self.h, over)

    def clear(self):
        self.L.hvt_ex_clear(self.h)

    def valid(self):
        return bool(self.L.hvt_ex_valid(self.h))

    def lens(self):
        lens, ct = (C.c_uint32 * self.G)(), (C.c_uint64 * 4)()
        self.L.hss_ex_counts(self.L.hvt_ex_stats(self.h), lens, ct, None)
        return [min(x, self.max_moves) for x in lens], ct[0], ct[1]

    def value_targets(self, lam, settle=False, flags=None, reserved=None):
        cfg = TaflValueTargetsCfg(lam=lam, flags=(abi.VT_SETTLE_UNFINISHED if settle else 0) if flags is None else flags)
        if reserved is not None:
            cfg._reserved[reserved] = 1
        o4 = (C.c_uint64 * 4)()
        return self.L.hvt_value_targets(self.h, C.byref(cfg), o4), tuple(o4)

    def gather_targets(self, index, strict=True, want=(True, True, True)):
        idx = np.ascontiguousarray(index, np.uint32)
        t, kd, ee = np.ones(idx.size, np.float32), np.ones(idx.size, np.uint8), np.ones(idx.size, np.uint8)
        rc = self.L.hvt_gather_targets(self.h, _vp(idx), idx.size, _vp(t if want[0] else None), _vp(kd if want[1] else None), _vp(ee if want[2] else None), int(strict))
        return rc, t, kd, ee

    def rows(self):
        """Per lane the recorded examples as (search_stats_util.Row, z, final), and every parent array as a comparable tuple."""
        L, G_, K_, n = self.L, self.G, self.K, self.n
        xs = L.hvt_ex_stats(self.h)
        lens, _d, _o = self.lens()
        out, plain = [[] for _ in range(G_)], []
        for g in range(G_):
            for j in range(lens[g]):
                e = j * G_ + g
                out5, board = (C.c_uint32 * 5)(), (C.c_uint8 * (n * n))()
                acts, vis, z, fin = (C.c_uint32 * K_)(), (C.c_uint32 * K_)(), C.c_float(), C.c_uint8()
                assert L.hss_ex_example(xs, e, out5, board, acts, vis, C.byref(z), C.byref(fin)) == 0
                nc = out5[0] if not out5[2] else 0
                idx = np.asarray([e], np.uint32)
                q, p = np.zeros(K_, np.float32), np.zeros(K_, np.float32)
                assert L.hqs_ex_read_stats(xs, _vp(idx), 1, _vp(q), _vp(p)) == 0
                out[g].append((ssu.Row(acts[:nc], vis[:nc], q[:nc], p[:nc], out5[3], out5[4], out5[1]), np.float32(z.value), int(fin.value), int(out5[2])))
                plain.append((g, j, bytes(board), tuple(out5), tuple(acts[:nc]), tuple(vis[:nc]), q[:nc].tobytes(), p[:nc].tobytes(), np.float32(z.value).tobytes(), int(fin.value)))
        return out, plain


def index_of(lens, G_):
    return [j * G_ + g for g in range(G_) for j in range(lens[g])]


def assert_recorded(rows, want, where="", max_moves=None):
    """The examples a driver read back (rows[g][j] = (Row, z, final, overflow)) against the expectation's: rows, z and final before any settlement."""
    for g, lane in enumerate(want.lanes):
        limit = len(lane) if max_moves is None else min(len(lane), max_moves)
        assert len(rows[g]) == limit, (where, g, len(rows[g]), limit)
        for j in range(limit):
            r, z, fin, over = rows[g][j]
            if not over:
                assert r.key() == lane[j].row.key(), (where, g, j)
            assert np.float32(z).tobytes() == np.float32(lane[j].z).tobytes() and fin == lane[j].fin, (where, "z", g, j, z, fin, lane[j].z, lane[j].fin)


def assert_targets(got_index, G_, t, kd, ee, want, exp, where="", z=None, fin=None):
    """vt, kind and ep_end of the rows `got_index` (and z, final where given) against the expectation, bit for bit."""
    for i, e in enumerate(got_index):
        g, j = e % G_, e // G_
        assert np.float32(t[i]).tobytes() == exp.vt[(g, j)].tobytes(), (where, "vt", g, j, float(t[i]), float(exp.vt[(g, j)]))
        assert int(kd[i]) == exp.kind[(g, j)], (where, "kind", g, j)
        if ee is not None:
            assert int(ee[i]) == want.lanes[g][j].ep_end, (where, "ep_end", g, j)
        if z is not None:
            assert np.float32(z[i]).tobytes() == np.float32(exp.z[(g, j)]).tobytes() and int(fin[i]) == exp.fin[(g, j)], (where, "z", g, j, z[i], fin[i])


def taken_order(want, exp, Kmax=None, max_moves=None):
    """The (g, j) an ingest takes, in the order of the per-example arrays: final != 0 and a stored policy."""
    depth = max(len(lane) for lane in want.lanes)
    depth = depth if max_moves is None else min(depth, max_moves)
    return [(g, j) for j in range(depth) for g in range(len(want.lanes))
            if j < len(want.lanes[g]) and exp.fin[(g, j)] != 0 and (Kmax is None or len(want.lanes[g][j].row.visits) <= Kmax)]


class HostPool:
    def __init__(self, C_, Kp, n):
        self.L, self.C = hlib(), C_
        self.h = self.L.hvt_pool_new(C_, Kp, n)
        self.w = self.L.hvt_pool_weights(self.h)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.hvt_pool_free(self.h)
            self.h = None

    def set_search_stats(self, on=True):
        return self.L.hvt_pool_set_search_stats(self.h, int(on))

    def set_value_targets(self, on=True):
        return self.L.hvt_pool_set_value_targets(self.h, int(on))

    def ingest(self, ex, with_targets=True):
        o3 = (C.c_uint64 * 3)()
        return self.L.hvt_pool_ingest(self.h, ex.h, int(with_targets), o3), tuple(o3)

    def trim(self, keep):
        return self.L.hspw_trim(self.w, keep)

    def clear(self):
        self.L.hspw_clear(self.w)

    def stats(self):
        o = (C.c_uint64 * 8)()
        self.L.hsp_stats(self.L.hspw_pool(self.w), o)
        return dict(zip(("written", "live", "ingests", "oldest_generation", "skipped_open", "skipped_overflow", "bad_slot", "device_bytes"), o))

    def gather_targets(self, slots, strict=True):
        sl = np.ascontiguousarray(slots, np.uint32)
        t, kd = np.ones(sl.size, np.float32), np.ones(sl.size, np.uint8)
        return self.L.hvt_pool_gather_targets(self.h, _vp(sl), sl.size, _vp(t), _vp(kd), int(strict)), t, kd


class PoolModel:
    """vt and kind per slot of a pool of C slots that ingests lists of (vt, kind) in rank order; the live window."""

    def __init__(self, C_):
        self.C, self.written, self.live, self.gens = C_, 0, 0, []
        self.slot = {}

    def ingest(self, items):
        T = len(items)
        for r in range(T - min(T, self.C), T):
            self.slot[(self.written + r) % self.C] = items[r]
        self.written += T
        self.gens.append(T)
        self.live = min(self.C, self.live + T)
        return T

    def trim(self, keep):
        self.live = min(self.live, sum(self.gens[-keep:]))

    def live_slots(self):
        return [(self.written - self.live + a) % self.C for a in range(self.live)]

    def check(self, slots, t, kd, where=""):
        for i, s in enumerate(slots):
            vt, kind = self.slot[s]
            assert np.float32(t[i]).tobytes() == vt.tobytes() and int(kd[i]) == kind, (where, s)
