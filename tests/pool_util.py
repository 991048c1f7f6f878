"""Expected values for the training-pool tests (include/taflhip.h tafl_pool_*): ingest, trim, draw and gather
restated in Python / numpy from the plain fields of the examples - never from the code under test - and the front end of the host harness
(tests/hostsim_pool: the product's tafl_pool.hpp compiled for the CPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from tests import examples_util as xu

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_pool")
_LIB = None
POOL_KEY = 0x504F4F4C44524157          # "POOLDRAW"
FLOORS = {"taken": 50, "open": 5, "overflow": 5, "short_lanes": 5, "empty_lanes": 1}


# ---- the plain fields of an examples object ------------------------------------------------------------------------------------------
class Table:
    """Every entry e = j * G + g of the per-example arrays of an examples object: lens [G], and per e (garbage where no example is)
    overflow, final, nc, side, move_no, z, actions / visits [E, K], boards [E, n, n]."""

    def __init__(self, G, max_moves, K, n, lens):
        E = G * max_moves
        self.G, self.max_moves, self.K, self.n, self.lens = G, max_moves, K, n, np.asarray(lens, np.int64)
        self.overflow, self.final = np.zeros(E, np.uint8), np.zeros(E, np.uint8)
        self.nc, self.side, self.move_no = np.zeros(E, np.uint32), np.zeros(E, np.uint8), np.zeros(E, np.uint32)
        self.z = np.zeros(E, np.float32)
        self.actions, self.visits = np.zeros((E, K), np.uint32), np.zeros((E, K), np.uint32)
        self.boards = np.zeros((E, n, n), np.uint8)

    def valid(self):
        """The entries that hold an example, ascending."""
        return [j * self.G + g for j in range(self.max_moves) for g in range(self.G) if j < min(self.lens[g], self.max_moves)]


def host_table(hx):
    """Table of a tests/hostsim examples buffer (examples_util.HostExamples), example by example."""
    lens, _ = hx.counts()
    t = Table(hx.G, hx.max_moves, hx.K, hx.n, lens)
    for e in t.valid():
        (rows, side, acts, vis, _played, move_no), overflow, z, fin = hx.example(e // hx.G, e % hx.G)
        t.overflow[e], t.final[e], t.nc[e], t.side[e], t.move_no[e], t.z[e] = overflow, fin, len(acts), side, move_no, z
        t.actions[e, :len(acts)], t.visits[e, :len(vis)], t.boards[e] = acts, vis, rows
    return t


def device_table(ex):
    """Table of an engine.Examples object, from Examples.counts / read / gather."""
    lens, _ = ex.counts()
    t = Table(ex.n_games, ex.max_moves, ex.max_children, ex.logic.side_len, list(lens))
    es = np.asarray(t.valid(), np.uint32)
    if es.size:
        nc, ov, _pl, mv, acts, vis = ex.read(es)
        boards, sides, _pi, z, fin = ex.gather(es)
        t.overflow[es], t.final[es], t.nc[es], t.side[es], t.move_no[es], t.z[es] = ov, fin, nc, sides, mv, z
        t.actions[es], t.visits[es], t.boards[es] = acts, vis, boards
    return t


def coverage(t):
    """What an ingest of the table meets: taken / open / overflow examples, lanes with len < max_moves, lanes with no example."""
    es = np.asarray(t.valid(), np.int64)
    over = t.overflow[es] != 0
    fin = t.final[es] != 0
    return {"taken": int((~over & fin).sum()), "open": int((~over & ~fin).sum()), "overflow": int(over.sum()),
            "short_lanes": int((t.lens < t.max_moves).sum()), "empty_lanes": int((t.lens == 0).sum())}


def assert_floors(t, where=""):
    cov = coverage(t)
    for k, floor in FLOORS.items():
        assert cov[k] >= floor, (where, k, cov)
    return cov


# ---- ingest and trim, restated from the header -----------------------------------------------------------------------------------------
class PoolModel:
    """The pool as the header states it: slot -> the plain fields of the row it holds, the generation of every row ever taken."""

    def __init__(self, C, Kp, n):
        self.C, self.Kp, self.n = C, Kp, n
        self.clear()

    def clear(self):
        self.written = self.ingests = self.skipped_open = self.skipped_overflow = 0
        self.first_kept = 0              # rows below it were trimmed away
        self.gen_of, self.slots = [], {}

    def ingest(self, t):
        taken, so, sv = [], 0, 0
        for e in range(t.G * t.max_moves):
            j, g = divmod(e, t.G)
            if j >= min(t.lens[g], t.max_moves):
                continue
            if t.overflow[e]:
                sv += 1
                continue
            if not t.final[e]:
                so += 1
                continue
            taken.append(e)
        T, gen = len(taken), self.ingests + 1
        for r, e in enumerate(taken):
            if r >= T - min(T, self.C):
                acts, vis = np.zeros(self.Kp, np.uint32), np.zeros(self.Kp, np.uint32)
                k = int(t.nc[e])
                acts[:k], vis[:k] = t.actions[e, :k], t.visits[e, :k]
                self.slots[(self.written + r) % self.C] = dict(e=e, nc=k, side=int(t.side[e]), N=int(vis.sum()), move_no=int(t.move_no[e]), generation=gen,
                                                               z=np.float32(t.z[e]), actions=acts, visits=vis, board=t.boards[e].copy())
        self.gen_of += [gen] * T
        self.written += T
        self.ingests += 1
        self.skipped_open += so
        self.skipped_overflow += sv
        return T, so, sv

    def trim(self, keep):
        assert keep >= 1
        kept = [q for q in range(self.written) if self.gen_of[q] > self.ingests - keep]
        self.first_kept = max(self.first_kept, kept[0] if kept else self.written)

    def first_live(self):
        return max(self.first_kept, self.written - self.C, 0)

    @property
    def live(self):
        return self.written - self.first_live()

    def live_slots(self):
        """The live slots, oldest row first."""
        return [q % self.C for q in range(self.first_live(), self.written)]

    def oldest_generation(self):
        return self.gen_of[self.first_live()] if self.live else 0

    def stats(self):
        return dict(written=self.written, live=self.live, ingests=self.ingests, oldest_generation=self.oldest_generation(),
                    skipped_open=self.skipped_open, skipped_overflow=self.skipped_overflow)

    def source(self, slots):
        """The entries e of the examples object the rows in `slots` were taken from."""
        return np.asarray([self.slots[int(s)]["e"] for s in slots], np.uint32)

    def expect_read(self, slots):
        rows = [self.slots[int(s)] for s in slots]
        return (np.asarray([r["nc"] for r in rows], np.uint32), np.asarray([r["move_no"] for r in rows], np.uint32),
                np.asarray([r["generation"] for r in rows], np.uint32), np.stack([r["actions"] for r in rows]), np.stack([r["visits"] for r in rows]))

    def expect_gather(self, slots, sym):
        """boards, sides, pi, z of the rows in `slots` under `sym`, in numpy from the plain fields (header: tafl_examples_gather)."""
        n, A = self.n, abi.action_size(self.n)
        boards, sides = np.zeros((len(slots), n, n), np.uint8), np.zeros(len(slots), np.uint8)
        pi, z = np.zeros((len(slots), A), np.float32), np.zeros(len(slots), np.float32)
        for i, (s, k) in enumerate(zip(slots, sym)):
            r = self.slots[int(s)]
            boards[i], sides[i], z[i] = xu.sym_board_np(r["board"], int(k)), r["side"], r["z"]
            for a, v in zip(r["actions"][:r["nc"]], r["visits"][:r["nc"]]):
                pi[i, xu.sym_action_py(n, int(a), int(k))] = np.float32(np.float64(v) / np.float64(r["N"]))
        return boards, sides, pi, z


# ---- the draw, restated ------------------------------------------------------------------------------------------------------------------
def draw(seed, step, row, written, live, C, sym=True):
    """(slot, sym, a) of row `row` of the sample (seed, step)."""
    dk = xu.sim_key(xu.game_key(seed, step) ^ POOL_KEY, row)
    a = (xu.ply_rand(dk, 0) * live) >> 32
    return (written - live + a) % C, (xu.ply_rand(dk, 1) >> 29) if sym else 0, a


def draw_many(seed, step, row_base, count, written, live, C, sym=True):
    d = [draw(seed, step, row_base + i, written, live, C, sym) for i in range(count)]
    return np.asarray([x[0] for x in d], np.uint32), np.asarray([x[1] for x in d], np.uint8), np.asarray([x[2] for x in d], np.int64)


def check_rows(model, slots, sym, got_read, got_gather, where=""):
    """Every field of Pool.read(slots) and Pool.gather(slots, sym) (or the harness's) against the model, exactly."""
    for name, got, want in zip(("n_children", "move_no", "generation", "actions", "visits"), got_read, model.expect_read(slots)):
        assert np.array_equal(np.asarray(got), want), (where, name)
    for name, got, want in zip(("boards", "sides", "pi", "z"), got_gather, model.expect_gather(slots, sym)):
        assert np.asarray(got).tobytes() == want.tobytes(), (where, name)


# ---- the host harness ----------------------------------------------------------------------------------------------------------------------
def hlib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_pool.so"))
        vp, u8, u32, u64, i32 = C.c_void_p, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int
        L.hsp_new.restype = vp; L.hsp_new.argtypes = [u32, u32, u8]
        L.hsp_free.restype = None; L.hsp_free.argtypes = [vp]
        L.hsp_clear.restype = None; L.hsp_clear.argtypes = [vp]
        L.hsp_ingest.restype = i32; L.hsp_ingest.argtypes = [vp, vp, vp]
        L.hsp_trim.restype = i32; L.hsp_trim.argtypes = [vp, u32]
        L.hsp_stats.restype = None; L.hsp_stats.argtypes = [vp, vp]
        L.hsp_row_words.restype = u32; L.hsp_row_words.argtypes = [vp]
        L.hsp_rows.restype = None; L.hsp_rows.argtypes = [vp, vp]
        L.hsp_read.restype = i32; L.hsp_read.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
        L.hsp_draw.restype = None; L.hsp_draw.argtypes = [u64, u64, u32, u32, u32, u64, u64, u32, vp, vp]
        L.hsp_sample.restype = i32; L.hsp_sample.argtypes = [vp, u64, u64, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        L.hsp_gather.restype = u32; L.hsp_gather.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
        _LIB = L
    return _LIB


STAT_NAMES = ("written", "live", "ingests", "oldest_generation", "skipped_open", "skipped_overflow", "bad_slot", "device_bytes")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostPool:
    """tafl_pool on host memory (tests/hostsim_pool)."""

    def __init__(self, C_, Kp, n):
        self.C, self.Kp, self.n = C_, Kp, n
        self.h = hlib().hsp_new(C_, Kp, n)
        assert self.h

    def __del__(self):
        if getattr(self, "h", None):
            hlib().hsp_free(self.h)
            self.h = None

    def ingest(self, hx):
        """(taken, skipped open, skipped overflow) of the ingest of a tests/hostsim examples buffer."""
        out = np.zeros(3, np.uint64)
        rc = hlib().hsp_ingest(self.h, hx.h, _p(out))
        assert rc == 0, rc
        return tuple(int(v) for v in out)

    def trim(self, keep):
        return hlib().hsp_trim(self.h, keep)

    def clear(self):
        hlib().hsp_clear(self.h)

    def stats(self):
        out = np.zeros(8, np.uint64)
        hlib().hsp_stats(self.h, _p(out))
        return dict(zip(STAT_NAMES, (int(v) for v in out)))

    def raw(self):
        out = np.zeros(self.C * hlib().hsp_row_words(self.h), np.uint32)
        hlib().hsp_rows(self.h, _p(out))
        return out.reshape(self.C, -1)

    def read(self, slots):
        s = np.ascontiguousarray(slots, np.uint32)
        k = s.size
        nc, mv, gen = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        acts, vis = np.zeros((k, self.Kp), np.uint32), np.zeros((k, self.Kp), np.uint32)
        rc = hlib().hsp_read(self.h, _p(s), k, _p(nc), _p(mv), _p(gen), _p(acts), _p(vis))
        return rc, (nc, mv, gen, acts, vis)

    def _out(self, k):
        n, A = self.n, abi.action_size(self.n)
        return np.full((k, n, n), 0xAA, np.uint8), np.full(k, 0xAA, np.uint8), np.full((k, A), 7.0, np.float32), np.full(k, 7.0, np.float32)

    def gather(self, slots, sym=None):
        """((boards, sides, pi, z), rows whose slot was not live)."""
        s = np.ascontiguousarray(slots, np.uint32)
        sy = None if sym is None else np.ascontiguousarray(sym, np.uint8)
        out = self._out(s.size)
        bad = hlib().hsp_gather(self.h, _p(s), _p(sy) if sy is not None else None, s.size, *[_p(a) for a in out])
        return out, bad

    def sample(self, count, seed, step, row_base=0, flags=1):
        """(rc, (boards, sides, pi, z), out_slot, out_sym)."""
        out = self._out(count)
        slot, sym = np.zeros(count, np.uint32), np.zeros(count, np.uint8)
        rc = hlib().hsp_sample(self.h, seed, step, row_base, count, flags, *[_p(a) for a in out], _p(slot), _p(sym))
        return rc, out, slot, sym


def host_draw(seed, step, row_base, count, flags, written, live, C_):
    slot, sym = np.zeros(count, np.uint32), np.zeros(count, np.uint8)
    hlib().hsp_draw(seed, step, row_base, count, flags, written, live, C_, _p(slot), _p(sym))
    return slot, sym
