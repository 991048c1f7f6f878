"""Expected values for the weighted sampling of the training pool (include/taflhip.h tafl_pool_set_weighting / _set_weights /
_sample_weighted): the weight array, the max rule, the ingest rule, the live mask and the draw restated in Python
integers on examples_util's RNG words - never from the code under test - and the front end of the host harness
(tests/hostsim_pool_weights: the product's tafl_pool.hpp compiled for the CPU)."""
import bisect
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from tests import examples_util as xu

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_pool_weights")
_LIB = None
POOLW_KEY = 0x504F4F4C57445257          # "POOLWDRW"
TILE = 256                               # slots per tile of the product's prefix structure (the tests place their edges by it)
MAXW = 2 ** 32 - 1
STAT_NAMES = ("enabled", "ingest_weight", "total_weight", "positive", "bad_slot", "rebuilds", "device_bytes", "_reserved")


class Window:
    """The live window of a pool alone - written, live, the trims - for pools too large to model row by row (pool_util.PoolModel holds
    the rows too and offers the same fields)."""

    def __init__(self, C_):
        self.C = C_
        self.clear()

    def clear(self):
        self.written = self.ingests = self.first_kept = 0
        self.ends = []                   # ends[g - 1]: written after the ingest of generation g

    def took(self, T):
        self.written += T
        self.ingests += 1
        self.ends.append(self.written)

    def trim(self, keep):
        assert keep >= 1
        if keep < self.ingests:
            self.first_kept = max(self.first_kept, self.ends[self.ingests - keep - 1])

    def first_live(self):
        return max(self.first_kept, self.written - self.C, 0)

    @property
    def live(self):
        return self.written - self.first_live()

    def live_slots(self):
        return [q % self.C for q in range(self.first_live(), self.written)]


class WeightModel:
    """The weights of a pool as the header states them, over a window `win` (a PoolModel or a Window): wt[s] per slot, kept as Python
    integers; the caller tells it what the window did (ingested, and win's own trim / clear)."""

    def __init__(self, win):
        self.win = win
        self.on, self.wt, self.ingest_weight, self.bad_slot = False, None, 0, 0

    def set_weighting(self, w):
        if w is None:
            self.on, self.wt, self.bad_slot = False, None, 0
            return
        assert 0 <= w <= MAXW
        if not self.on:
            self.on, self.wt, self.bad_slot = True, [w] * self.win.C, 0       # every slot, live or not
        self.ingest_weight = w

    def ingested(self, T, written_before):
        """An ingest took T rows into a pool that had `written_before`: the rows it stored (ranks r >= T - min(T, C)) get ingest_weight."""
        if self.on:
            for r in range(T - min(T, self.win.C), T):
                self.wt[(written_before + r) % self.win.C] = self.ingest_weight

    def set_weights(self, slots, weights, strict):
        """The max rule.  strict (host pointers): False and nothing written if a slot is not live; else such entries count in bad_slot."""
        live = set(self.win.live_slots())
        slots, weights = [int(s) for s in slots], [int(w) for w in weights]
        if strict and any(s not in live for s in slots):
            return False
        best = {}
        for s, w in zip(slots, weights):
            if s in live:
                best[s] = max(best.get(s, 0), w)
            else:
                self.bad_slot += 1
        for s, w in best.items():
            self.wt[s] = w
        return True

    def eff(self):
        live = set(self.win.live_slots())
        return [w if s in live else 0 for s, w in enumerate(self.wt)]

    def prefix(self):
        """W(0) .. W(C): the serial running sum of eff in slot order."""
        return [0] + list(itertools.accumulate(self.eff()))

    @property
    def total(self):
        return sum(self.eff())

    @property
    def positive(self):
        return sum(1 for e in self.eff() if e)

    def get(self, slots):
        """What the device route of tafl_pool_get_weights reports: 0 for a slot that is not live."""
        eff = self.eff()
        return np.asarray([eff[int(s)] if 0 <= int(s) < self.win.C else 0 for s in slots], np.uint32)

    def stats(self):
        return dict(enabled=1, ingest_weight=self.ingest_weight, total_weight=self.total, positive=self.positive, bad_slot=self.bad_slot) if self.on else \
            dict(enabled=0, ingest_weight=0, total_weight=0, positive=0, bad_slot=0, rebuilds=0, device_bytes=0)

    def draw_many(self, seed, step, row_base, count, sym=True):
        """(slot uint32 [count], sym uint8, weight uint32, total, k list) of the rows row_base .. row_base + count - 1."""
        W = self.prefix()
        total = W[-1]
        assert total > 0
        slots, syms, ks = [], [], []
        for i in range(count):
            k, y = draw_k(seed, step, row_base + i, total, sym)
            s = bisect.bisect_right(W, k) - 1                     # the one s with W(s) <= k < W(s + 1)
            assert W[s] <= k < W[s + 1]
            slots.append(s); syms.append(y); ks.append(k)
        return (np.asarray(slots, np.uint32), np.asarray(syms, np.uint8), np.asarray([self.wt[s] for s in slots], np.uint32), total, ks)

    def draw_serial(self, seed, step, row, sym=True):
        """One draw as the running sum itself, slot after slot: (slot, sym, weight)."""
        eff = self.eff()
        k, y = draw_k(seed, step, row, sum(eff), sym)
        run = 0
        for s, e in enumerate(eff):
            if run <= k < run + e:
                return s, y, e
            run += e
        raise AssertionError("k >= total")


def draw_k(seed, step, row, total, sym=True):
    """(k, sym) of the header: k = (r * total) >> 64 with r = ply_rand(dk, 2) << 32 | ply_rand(dk, 3)."""
    dk = xu.sim_key(xu.game_key(seed, step) ^ POOLW_KEY, row)
    r = (xu.ply_rand(dk, 2) << 32) | xu.ply_rand(dk, 3)
    return (r * total) >> 64, (xu.ply_rand(dk, 1) >> 29) if sym else 0


def tiles_hit(slots):
    return set(int(s) // TILE for s in slots)


# ---- weight patterns over the live slots (slot order) -----------------------------------------------------------------------------------------
def pattern_random_third_zero(live_slots, seed):
    """(slots, weights): every live slot once, in slot order; every third one 0, the others random in 1 .. 2^32 - 1."""
    rng = np.random.default_rng(seed)
    sl = sorted(int(s) for s in live_slots)
    w = [0 if i % 3 == 0 else int(v) for i, v in enumerate(rng.integers(1, MAXW, len(sl), dtype=np.uint64, endpoint=True))]
    return sl, w


# ---- the host harness ----------------------------------------------------------------------------------------------------------------------
def wlib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_pool_weights.so"))
        vp, u8, u32, u64, i32 = C.c_void_p, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int
        L.hspw_new.restype = vp; L.hspw_new.argtypes = [u32, u32, u8]
        L.hspw_free.restype = None; L.hspw_free.argtypes = [vp]
        L.hspw_pool.restype = vp; L.hspw_pool.argtypes = [vp]
        L.hspw_set_weighting.restype = None; L.hspw_set_weighting.argtypes = [vp, i32, u32]
        L.hspw_ingest.restype = i32; L.hspw_ingest.argtypes = [vp, vp, vp]
        L.hspw_trim.restype = i32; L.hspw_trim.argtypes = [vp, u32]
        L.hspw_clear.restype = None; L.hspw_clear.argtypes = [vp]
        L.hspw_set_weights.restype = i32; L.hspw_set_weights.argtypes = [vp, vp, vp, u32, i32]
        L.hspw_raw_weights.restype = i32; L.hspw_raw_weights.argtypes = [vp, vp]
        L.hspw_get_weights.restype = i32; L.hspw_get_weights.argtypes = [vp, vp, u32, vp]
        L.hspw_stats.restype = None; L.hspw_stats.argtypes = [vp, vp]
        L.hspw_tiles.restype = u32; L.hspw_tiles.argtypes = [vp, vp, vp]
        L.hspw_draw.restype = i32; L.hspw_draw.argtypes = [vp, u64, u64, u32, u32, u32, vp, vp, vp, vp, vp]
        L.hspw_mulhi64.restype = u64; L.hspw_mulhi64.argtypes = [u64, u64]
        L.hsp_stats.restype = None; L.hsp_stats.argtypes = [vp, vp]
        L.hsp_gather.restype = u32; L.hsp_gather.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostWPool:
    """tafl_pool with weighted sampling on host memory (tests/hostsim_pool_weights)."""

    def __init__(self, C_, Kp, n):
        self.C, self.Kp, self.n = C_, Kp, n
        self.h = wlib().hspw_new(C_, Kp, n)
        assert self.h

    def __del__(self):
        if getattr(self, "h", None):
            wlib().hspw_free(self.h)
            self.h = None

    def set_weighting(self, w):
        wlib().hspw_set_weighting(self.h, 0 if w is None else 1, 0 if w is None else w)

    def ingest(self, hx):
        out = np.zeros(3, np.uint64)
        rc = wlib().hspw_ingest(self.h, hx.h, _p(out))
        assert rc == 0, rc
        return tuple(int(v) for v in out)

    def trim(self, keep):
        return wlib().hspw_trim(self.h, keep)

    def clear(self):
        wlib().hspw_clear(self.h)

    def pool_stats(self):
        out = np.zeros(8, np.uint64)
        wlib().hsp_stats(wlib().hspw_pool(self.h), _p(out))
        return dict(zip(("written", "live", "ingests"), (int(v) for v in out[:3])))

    def set_weights(self, slots, weights, strict):
        s, w = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(weights, np.uint32)
        return wlib().hspw_set_weights(self.h, _p(s), _p(w), s.size, 1 if strict else 0)

    def raw_weights(self):
        out = np.zeros(self.C, np.uint32)
        assert wlib().hspw_raw_weights(self.h, _p(out)) == 0
        return out

    def get_weights(self, slots):
        s = np.ascontiguousarray(slots, np.uint32)
        out = np.zeros(s.size, np.uint32)
        assert wlib().hspw_get_weights(self.h, _p(s), s.size, _p(out)) == 0
        return out

    def stats(self):
        out = np.zeros(8, np.uint64)
        wlib().hspw_stats(self.h, _p(out))
        return dict(zip(STAT_NAMES, (int(v) for v in out)))

    def tiles(self):
        nt = (self.C + TILE - 1) // TILE
        ts, tp = np.zeros(nt, np.uint64), np.zeros(nt, np.uint64)
        assert wlib().hspw_tiles(self.h, _p(ts), _p(tp)) == nt
        return ts, tp

    def draw(self, count, seed, step, row_base=0, flags=1):
        """(rc, slot, sym, weight, total, probe steps of the tile search)."""
        slot, sym, w, steps = np.zeros(count, np.uint32), np.zeros(count, np.uint8), np.zeros(count, np.uint32), np.zeros(count, np.uint32)
        total = C.c_uint64(0)
        rc = wlib().hspw_draw(self.h, seed, step, row_base, count, flags, _p(slot), _p(sym), _p(w), C.cast(C.byref(total), C.c_void_p), _p(steps))
        return rc, slot, sym, w, int(total.value), steps

    def gather(self, slots, sym):
        n, A = self.n, abi.action_size(self.n)
        s, sy = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(sym, np.uint8)
        out = (np.zeros((s.size, n, n), np.uint8), np.zeros(s.size, np.uint8), np.zeros((s.size, A), np.float32), np.zeros(s.size, np.float32))
        bad = wlib().hsp_gather(wlib().hspw_pool(self.h), _p(s), _p(sy), s.size, *[_p(a) for a in out])
        return out, bad
