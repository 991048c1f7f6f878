"""Expected values for the de-duplication of the training pool (include/taflhip.h tafl_pool_dedup / _gather_dedup / _weights_from_dedup,
DESIGN.md section 24): images, hashes, keys, groups and the weight rules restated in Python / numpy over pool_util.PoolModel and
pool_weights_util.WeightModel - never from the code under test - the workload of the tests with its floors, and the front end of the
host harness (tests/hostsim_pool_dedup: the product's tafl_pool.hpp compiled for the CPU)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams
from tests import examples_util as xu
from tests import pool_util as qu

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_pool_dedup")
_LIB = None
M64 = 2 ** 64 - 1
GOLD = 0x9E3779B97F4A7C15
DRAW = float(np.float32(1e-4))           # (double)(float)TAFL_DRAW_VALUE
DIVIDE, REPRESENTATIVES = 1, 2
# the workload of the issue: Brandubh 7x7 / u64, 65 lanes from the start position, S = 8, 96 moves, K = 8
N, WB, G, MOVES, K, SIMS, CAP = 7, 64, 65, 96, 8, 8, 64
RUNS = {"A": (8, 11), "B": (9, 12)}      # search seed, sample seed
TEMP_MOVES = 4
FLOORS = {"taken": 1000, "open": 500, "groups_of_two_or_more": 100, "largest": 30, "both_results": 30, "joined_by_symmetry": 20, "singletons": 500}


# ---- images, hashes, keys ------------------------------------------------------------------------------------------------------------
def images(boards, sigma):
    """The images of boards [k, n, n] under sigma: byte b[t] at tile sym_tile(sigma, t) - transpose, then mirror the rows, then the columns."""
    b = np.asarray(boards)
    if sigma & 4:
        b = b.transpose(0, 2, 1)
    if sigma & 1:
        b = b[:, ::-1, :]
    if sigma & 2:
        b = b[:, :, ::-1]
    return np.ascontiguousarray(b)


def check_images(n, seed=1):
    """images() against the scatter through sym_tile (restated as examples_util.sym_rc), against numpy's rot90 / transpose names of the
    eight symmetries, and against the harness's sym_tile."""
    b = np.random.default_rng(seed).integers(0, 256, (3, n, n)).astype(np.uint8)
    names = {0: lambda a: a, 1: np.flipud, 2: np.fliplr, 3: lambda a: np.rot90(a, 2), 4: lambda a: a.T, 5: lambda a: np.rot90(a, 1),
             6: lambda a: np.rot90(a, 3), 7: lambda a: np.rot90(a, 2).T}
    for sigma in range(8):
        img = images(b, sigma)
        want = np.zeros_like(b)
        for r in range(n):
            for c in range(n):
                r2, c2 = xu.sym_rc(n, r, c, sigma)
                want[:, r2, c2] = b[:, r, c]
                assert dlib().hspd_sym_tile(sigma, r * n + c, n) == r2 * n + c2
        assert np.array_equal(img, want), sigma
        assert all(np.array_equal(img[i], names[sigma](b[i])) and np.array_equal(img[i], xu.sym_board_np(b[i], sigma)) for i in range(3)), sigma


def mix64(x):
    """The splitmix64 finaliser on uint64 arrays (wrapping)."""
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def mix64_int(x):
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def hashes(boards, sides, sigma):
    """h(sigma) of every row: uint64 [k]."""
    img = images(boards, sigma)
    k, n = img.shape[0], img.shape[1]
    BW = (n * n + 3) // 4
    padded = np.zeros((k, 4 * BW), np.uint8)
    padded[:, :n * n] = img.reshape(k, n * n)
    words = padded.view("<u4").astype(np.uint64)                               # tile u: byte u & 3 of word u >> 2
    x = np.uint64(GOLD) ^ np.asarray(sides, np.uint64)
    for i in range(BW):
        x = mix64(x ^ words[:, i])
    return x


def keys(boards, sides, symmetries, key_bits=64):
    """(key [k] as Python integers, canon [k])."""
    if symmetries:
        H = np.stack([hashes(boards, sides, s) for s in range(8)])
        canon = H.argmin(axis=0)                                               # (the first index that attains the minimum)
        h = H.min(axis=0)
    else:
        h, canon = hashes(boards, sides, 0), np.zeros(len(sides), np.int64)
    bits = key_bits or 64
    out = [int(v) & ((1 << bits) - 1) for v in h]
    return [v or 1 for v in out], [int(c) for c in canon]


def zmean(m, wins, losses):
    return np.float32((float(wins) - float(losses) + float(m - wins - losses) * DRAW) / float(m))


# ---- groups ---------------------------------------------------------------------------------------------------------------------------
class Dedup:
    """What tafl_pool_dedup leaves for the live rows of a PoolModel: rep / mult / zm per live slot (dictionaries), key / canon per live
    slot, and live, distinct, largest, collisions."""

    def __init__(self, model, symmetries=False, key_bits=64):
        slots = model.live_slots()                                              # oldest first: the position is the age rank
        rows = [model.slots[s] for s in slots]
        boards, sides = np.stack([r["board"] for r in rows]), np.asarray([r["side"] for r in rows], np.uint64)
        ks, canon = keys(boards, sides, symmetries, key_bits)
        groups = {}
        for age, k in enumerate(ks):
            groups.setdefault(k, []).append(age)
        self.slots, self.key, self.canon = slots, dict(zip(slots, ks)), dict(zip(slots, canon))
        self.rep, self.mult, self.zm, self.groups = {}, {}, {}, groups
        self.collisions = 0
        canonical = [(int(sides[a]), images(boards[a:a + 1], canon[a]).tobytes()) for a in range(len(slots))]
        for members in groups.values():
            newest = max(members)
            z = [float(rows[a]["z"]) for a in members]
            wins, losses = sum(v == 1.0 for v in z), sum(v == -1.0 for v in z)
            for a in members:
                s = slots[a]
                self.rep[s], self.mult[s], self.zm[s] = slots[newest], len(members), zmean(len(members), wins, losses)
                self.collisions += canonical[a] != canonical[newest]
        self.live, self.distinct, self.largest = len(slots), len(groups), max(len(m) for m in groups.values())

    def result(self):
        return dict(live=self.live, distinct=self.distinct, largest=self.largest, collisions=self.collisions)

    def expect_gather(self, slots):
        """rep, mult, zmean of `slots` by the device route: zeros for a slot that is not live; and the number of those."""
        ok = [int(s) in self.rep for s in slots]
        return (np.asarray([self.rep[int(s)] if o else 0 for s, o in zip(slots, ok)], np.uint32),
                np.asarray([self.mult[int(s)] if o else 0 for s, o in zip(slots, ok)], np.uint32),
                np.asarray([self.zm[int(s)] if o else 0.0 for s, o in zip(slots, ok)], np.float32), len(ok) - sum(ok))

    def apply_weights(self, wm, scale, flags=0):
        """tafl_pool_weights_from_dedup on a WeightModel: an assignment to every live slot."""
        for s in self.slots:
            if flags == REPRESENTATIVES:
                wm.wt[s] = scale if self.rep[s] == s else 0
            elif flags == DIVIDE:
                wm.wt[s] = 0 if wm.wt[s] == 0 else max(1, wm.wt[s] // self.mult[s])
            else:
                assert flags == 0
                wm.wt[s] = max(1, scale // self.mult[s])


def census(model):
    """What the floors are about, from the plain fields of the live rows (no hash): groups by (side, board bytes), and by the set of
    the eight images."""
    raw, sym = {}, {}
    for s in model.live_slots():
        r = model.slots[s]
        ident = (r["side"], r["board"].tobytes())
        raw.setdefault(ident, []).append(r)
        orbit = (r["side"], min(xu.sym_board_np(r["board"], k).tobytes() for k in range(8)))
        sym.setdefault(orbit, set()).add(ident)
    zs = [{float(r["z"]) for r in g} for g in raw.values()]
    return {"groups": len(raw), "groups_of_two_or_more": sum(len(g) >= 2 for g in raw.values()), "largest": max(len(g) for g in raw.values()),
            "both_results": sum(1.0 in z and -1.0 in z for z in zs), "singletons": sum(len(g) == 1 for g in raw.values()),
            "sym_groups": len(sym), "joined_by_symmetry": sum(len(v) >= 2 for v in sym.values()),
            "both_generations": sum(len({r["generation"] for r in g}) >= 2 for g in raw.values())}


def assert_floors(table, where=""):
    """The floors of the workload, on the Python expectation alone: a pool with room takes the table, its census is counted."""
    cov = qu.coverage(table)
    model = qu.PoolModel(cov["taken"] + 1, K, table.n)
    model.ingest(table)
    got = dict(census(model), taken=cov["taken"], open=cov["open"])
    for k, floor in FLOORS.items():
        assert got[k] >= floor, (where, k, got)
    return got


@functools.lru_cache(maxsize=None)
def host_workload():
    """(hx A, table A, hx B, table B): the two runs recorded and finalized by the host harness."""
    from oracle import oracle as orc
    from tests import parity_util as pu
    rules, fen, wb = pu.CONFIGS["brandubh7"]
    out = []
    for seed, sample_seed in RUNS.values():
        states = pu.start_states(orc, fen, rules.starting_side, wb, G)
        hx = xu.HostExamples(rules, N, wb, G, MOVES, K)
        hx.record(states, TaflMctsParams(SIMS, CAP, 1.0, seed, 0, 0), MOVES, 0, sample_seed, TEMP_MOVES)
        hx.finalize(states)
        out += [hx, qu.host_table(hx)]
    return tuple(out)


# ---- the host harness ----------------------------------------------------------------------------------------------------------------------
def dlib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_pool_dedup.so"))
        vp, u8, u32, u64, i32 = C.c_void_p, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int
        L.hspd_new.restype = vp; L.hspd_new.argtypes = [u32, u32, u8]
        L.hspd_free.restype = None; L.hspd_free.argtypes = [vp]
        L.hspd_wpool.restype = vp; L.hspd_wpool.argtypes = [vp]
        L.hspd_pool.restype = vp; L.hspd_pool.argtypes = [vp]
        L.hspd_ingest.restype = i32; L.hspd_ingest.argtypes = [vp, vp, vp]
        L.hspd_trim.restype = i32; L.hspd_trim.argtypes = [vp, u32]
        L.hspd_clear.restype = None; L.hspd_clear.argtypes = [vp]
        L.hspd_release.restype = None; L.hspd_release.argtypes = [vp]
        L.hspd_dedup.restype = i32; L.hspd_dedup.argtypes = [vp, u32, u32, u32, vp, u32, vp]
        L.hspd_keys.restype = i32; L.hspd_keys.argtypes = [vp, vp, vp]
        L.hspd_gather.restype = i32; L.hspd_gather.argtypes = [vp, vp, u32, vp, vp, vp, i32]
        L.hspd_weights.restype = i32; L.hspd_weights.argtypes = [vp, u32, u32]
        L.hspd_zmean.restype = C.c_float; L.hspd_zmean.argtypes = [u32, u32, u32]
        L.hspd_table_size.restype = u32; L.hspd_table_size.argtypes = [u64]
        L.hspd_sym_tile.restype = u32; L.hspd_sym_tile.argtypes = [u32, u32, u32]
        L.hspw_set_weighting.restype = None; L.hspw_set_weighting.argtypes = [vp, i32, u32]
        L.hspw_set_weights.restype = i32; L.hspw_set_weights.argtypes = [vp, vp, vp, u32, i32]
        L.hspw_raw_weights.restype = i32; L.hspw_raw_weights.argtypes = [vp, vp]
        L.hspw_draw.restype = i32; L.hspw_draw.argtypes = [vp, u64, u64, u32, u32, u32, vp, vp, vp, vp, vp]
        L.hsp_stats.restype = None; L.hsp_stats.argtypes = [vp, vp]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


RESULT_NAMES = ("live", "distinct", "largest", "collisions", "device_bytes")


class HostDPool:
    """tafl_pool with weighted sampling and de-duplication on host memory (tests/hostsim_pool_dedup)."""

    def __init__(self, C_, Kp, n):
        self.C, self.Kp, self.n = C_, Kp, n
        self.h = dlib().hspd_new(C_, Kp, n)
        assert self.h

    def __del__(self):
        if getattr(self, "h", None):
            dlib().hspd_free(self.h)
            self.h = None

    def ingest(self, hx):
        out = np.zeros(3, np.uint64)
        rc = dlib().hspd_ingest(self.h, hx.h, _p(out))
        assert rc == 0, rc
        return tuple(int(v) for v in out)

    def trim(self, keep):
        return dlib().hspd_trim(self.h, keep)

    def clear(self):
        dlib().hspd_clear(self.h)

    def release(self):
        dlib().hspd_release(self.h)

    def pool_stats(self):
        out = np.zeros(8, np.uint64)
        dlib().hsp_stats(dlib().hspd_pool(self.h), _p(out))
        return dict(zip(qu.STAT_NAMES, (int(v) for v in out)))

    def dedup(self, symmetries=False, key_bits=64, table_size=0, perm=None, wave=1):
        """(rc, result dict)."""
        out = np.zeros(5, np.uint64)
        pm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
        rc = dlib().hspd_dedup(self.h, 1 if symmetries else 0, key_bits, table_size, _p(pm) if pm is not None else None, wave, _p(out))
        return rc, dict(zip(RESULT_NAMES, (int(v) for v in out)))

    def keys(self):
        key, canon = np.zeros(self.C, np.uint64), np.zeros(self.C, np.uint8)
        assert dlib().hspd_keys(self.h, _p(key), _p(canon)) == 0
        return key, canon

    def gather(self, slots, strict=False):
        """(rc, rep, mult, zmean)."""
        s = np.ascontiguousarray(slots, np.uint32)
        rep, mult, zm = np.full(s.size, 0xAAAAAAAA, np.uint32), np.full(s.size, 0xAAAAAAAA, np.uint32), np.full(s.size, 7.0, np.float32)
        rc = dlib().hspd_gather(self.h, _p(s), s.size, _p(rep), _p(mult), _p(zm), 1 if strict else 0)
        return rc, rep, mult, zm

    def set_weighting(self, w):
        dlib().hspw_set_weighting(dlib().hspd_wpool(self.h), 0 if w is None else 1, 0 if w is None else w)

    def set_weights(self, slots, weights):
        s, w = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(weights, np.uint32)
        return dlib().hspw_set_weights(dlib().hspd_wpool(self.h), _p(s), _p(w), s.size, 1)

    def weights_from_dedup(self, scale, flags=0):
        return dlib().hspd_weights(self.h, scale, flags)

    def raw_weights(self):
        out = np.zeros(self.C, np.uint32)
        assert dlib().hspw_raw_weights(dlib().hspd_wpool(self.h), _p(out)) == 0
        return out

    def draw(self, count, seed, step, row_base=0, flags=1):
        """(rc, slot, sym, weight, total)."""
        slot, sym, w = np.zeros(count, np.uint32), np.zeros(count, np.uint8), np.zeros(count, np.uint32)
        total = C.c_uint64(0)
        rc = dlib().hspw_draw(dlib().hspd_wpool(self.h), seed, step, row_base, count, flags, _p(slot), _p(sym), _p(w), C.cast(C.byref(total), C.c_void_p), None)
        return rc, slot, sym, w, int(total.value)


def device_bytes(C_):
    """What the header states tafl_pool_dedup allocates for a pool of C_ slots, without the staging of host-pointer gathers."""
    ts = 64
    while ts < 2 * C_:
        ts *= 2
    return 25 * C_ + 24 * ts + 32
