"""Weighted sampling of the training pool on the device (include/taflhip.h tafl_pool_set_weighting / _set_weights / _get_weights /
_sample_weighted / _weight_stats): k_poolw_fill / _ingest / _zero / _max / _get, the rebuild k_poolw_tiles +
k_poolw_scan and the draw k_poolw_draw against the Python restatement of tests/pool_weights_util.py.  Every comparison is exact.
7x7 Brandubh, rows of 112 bytes (Kp = 8); the examples come from one rollout-mode tafl_selfplay_record run at S = 8, ply cap 64, as in
tests/test_gpu_pool.py, and large pools are filled by ingesting the same examples object again and again.  The prefix structure has
tiles of 256 slots and k_poolw_scan walks 256 tiles per chunk, so the pools have 1, 5, 300 (a partial second tile) and 66 000 slots
(258 tiles: a second chunk of the walk, and two steps of the 64-ary tile search)."""
import ctypes as C

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd._lib import TaflError
from tests import pool_util as qu
from tests import pool_weights_util as wu

pytestmark = pytest.mark.gpu

N, K, KP, SIMS, CAP = 7, 6, 8, 8, 64
G, MAX_MOVES = 4400, 12
BIG = 66000
SEED, STEP = 0xFEDCBA9876543210, 12
MAXW = wu.MAXW
INVALID_ARG, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def logic():
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    lg = BatchedGameLogic(abi.rules.BRANDUBH, N, device=0)
    yield lg
    lg.close()


@pytest.fixture(scope="module")
def recorded(logic):
    """(Examples, T): one recorded and finalized run, T = the examples an ingest takes by the restatement of tests/pool_util.py."""
    b = logic.new_batch(G, abi.boards.BRANDUBH)
    b.random_advance(3, (C.c_uint32 * G)(*[(i * 5) % 30 for i in range(G)]), 0)
    ex = logic.new_examples(G, MAX_MOVES, K)
    b.selfplay_record(ex, MAX_MOVES, SIMS, 1.0, 8, CAP, sample_seed=11, temp_moves=4, want_plays=False)
    ex.finalize(b)
    b.close()
    T = qu.coverage(qu.device_table(ex))["taken"]
    assert T > 700
    return ex, T


def code(fn, *a, **kw):
    with pytest.raises(TaflError) as e:
        fn(*a, **kw)
    return e.value.code


def dev_i32(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint32).view(np.int32).copy()).to(torch.device("cuda", 0))


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


class Rig:
    """A device pool, the model of its live window and the WeightModel, driven together."""

    def __init__(self, logic, Cp, recorded, weighting=None):
        self.ex, self.T = recorded
        self.pool, self.win = logic.new_pool(Cp, KP), wu.Window(Cp)
        self.wm = wu.WeightModel(self.win)
        if weighting is not None:
            self.set_weighting(weighting)

    def set_weighting(self, w):
        self.pool.set_weighting(w); self.wm.set_weighting(w)

    def ingest(self, times=1):
        for _ in range(times):
            before = self.win.written
            assert self.pool.ingest(self.ex)[0] == self.T
            self.win.took(self.T); self.wm.ingested(self.T, before)

    def trim(self, keep):
        self.pool.trim(keep); self.win.trim(keep)

    def set_weights(self, slots, weights):
        """The host route: refused as a whole if a slot is not live."""
        if self.wm.set_weights(slots, weights, True):
            self.pool.set_weights(slots, weights)
            return True
        assert code(self.pool.set_weights, slots, weights) == INVALID_ARG
        return False

    def check_weights(self, where=""):
        st, pst = self.pool.weight_stats(), self.pool.stats()
        assert (pst.written, pst.live) == (self.win.written, self.win.live), where
        for k, v in self.wm.stats().items():
            assert getattr(st, k) == v, (where, k, getattr(st, k), v)
        live = sorted(self.win.live_slots())
        assert np.array_equal(self.pool.weights(live), np.asarray([self.wm.wt[s] for s in live], np.uint32)), where
        every = np.arange(self.win.C + 2, dtype=np.uint32)                       # dead slots and two beyond C: reported as 0
        assert np.array_equal(host_u32(self.pool.weights(dev_i32(every))), self.wm.get(every)), where

    def check_sample(self, count, row_base=0, device=False, symmetries=True, where=""):
        got = self.pool.sample_weighted(count, SEED, STEP, row_base=row_base, symmetries=symmetries, device=device)
        slot, sym, weight, total, _ = self.wm.draw_many(SEED, STEP, row_base, count, symmetries)
        if device:
            got = [t.cpu().numpy() for t in got[:7]] + [got[7]]
            got[4], got[6] = got[4].view(np.uint32), got[6].view(np.uint32)
        assert got[7] == total and np.array_equal(got[4], slot) and np.array_equal(got[5], sym) and np.array_equal(got[6], weight), where
        for g, w in zip(got[:4], self.pool.gather(slot, sym)):
            assert g.tobytes() == w.tobytes(), where
        assert (weight > 0).all()
        return slot, sym, weight, total


@pytest.fixture(scope="module")
def big(logic, recorded):
    """66 000 slots, weighting on from the start, filled until the ring has wrapped.  The tests set every live weight they rely on."""
    rig = Rig(logic, BIG, recorded, weighting=MAXW)
    rig.ingest(BIG // rig.T + 2)
    assert rig.win.written > BIG + rig.T and rig.win.live == BIG
    return rig


@pytest.mark.parametrize("Cp", [1, 5, 300])
def test_small_pools(logic, recorded, Cp):
    """One ingest far larger than the pool (T > C: the ring wraps inside the call, min(T, C) rows are stored), a second one after the
    ingest weight changed; then the patterns.  300 slots: the second tile is partial (44 slots)."""
    rig = Rig(logic, Cp, recorded, weighting=3)
    rig.check_weights("empty")
    assert code(rig.pool.sample_weighted, 1, 1, 1) == INVALID_ARG                # live == 0
    rig.ingest()
    rig.check_weights("3 everywhere")
    slot, _, w, total = rig.check_sample(1)
    assert total == 3 * Cp and w[0] == 3
    rig.check_sample(600, device=True)
    rig.set_weighting(MAXW)                                                      # on -> on: later ingests only
    rig.check_weights("on -> on")
    rig.ingest()
    assert rig.wm.wt == [MAXW] * Cp
    rig.check_weights("every weight 2^32 - 1")
    assert rig.check_sample(600)[3] == Cp * MAXW
    for s in (0, 255, 256, Cp - 1):                                              # all the weight on one row at the ends of the tiles
        if s >= Cp:
            assert not rig.set_weights([s], [1])
            continue
        assert rig.set_weights(list(range(Cp)) + [s], [0] * Cp + [9])            # (s is named twice: the maximum holds)
        rig.check_weights(("one row", s))
        slot, _, w, total = rig.check_sample(300, device=bool(s & 1))
        assert total == 9 and (slot == s).all() and (w == 9).all() and rig.pool.weight_stats().positive == 1
    assert rig.set_weights(list(range(Cp)), [0] * Cp)
    assert code(rig.pool.sample_weighted, 1, 1, 1) == INVALID_ARG                # total == 0
    if Cp >= 5:
        sl, w = wu.pattern_random_third_zero(rig.win.live_slots(), Cp)
        assert rig.set_weights(sl, w)
        rig.check_weights("random")
        slot, *_ = rig.check_sample(600, row_base=77)
        assert not (set(int(s) for s in slot) & {s for s, v in zip(sl, w) if v == 0})
    rig.pool.close()


def test_big_pool(big):
    """66 000 slots, first with every slot live, then trimmed (one pool, filled once)."""
    _wrapped(big)
    _trimmed(big)


def _wrapped(big):
    """258 tiles, every slot live.  Every weight 2^32 - 1 (total above 2^32); then random weights with every third row silenced: the host
    route at 8 192 + 257 rows (two staging chunks) and at one row, the device route, two ranks against one call."""
    import torch
    rig = big
    every = list(range(BIG))
    assert rig.set_weights(every, [MAXW] * BIG)
    rig.check_weights("2^32 - 1")
    count = 8192 + 257
    slot, _, _, total = rig.check_sample(count, where="2^32 - 1")
    assert total == BIG * MAXW > 2 ** 32 and len(wu.tiles_hit(slot)) >= 200
    sl, w = wu.pattern_random_third_zero(every, 1)
    assert rig.set_weights(sl, w)
    rig.check_weights("random")
    zero = {s for s, v in zip(sl, w) if v == 0}
    assert len(zero) >= 20000 and rig.pool.weight_stats().positive == BIG - len(zero)
    slot, sym, weight, total = rig.check_sample(count, where="host route")
    hit = wu.tiles_hit(slot)
    assert len(hit) >= 200 and {0, 257} <= hit and not (set(int(s) for s in slot) & zero) and total > 2 ** 40
    assert set(np.unique(sym)) == set(range(8))
    rig.check_sample(1, row_base=count - 1, where="one row")
    rig.check_sample(count, device=True, where="device route")
    rig.check_sample(300, device=True, symmetries=False, where="no symmetries")
    half = 4224
    ranks = [rig.pool.sample_weighted(half, SEED, STEP, row_base=k * half, device=True) for k in range(2)]
    whole = rig.pool.sample_weighted(2 * half, SEED, STEP)
    for i in range(7):
        both = torch.cat([ranks[0][i], ranks[1][i]]).cpu().numpy()
        assert both.tobytes() == np.asarray(whole[i]).astype(both.dtype).tobytes(), i
    assert ranks[0][7] == ranks[1][7] == whole[7] == total
    for s in (0, 255, 256, BIG - 1):
        assert rig.set_weights([s, s], [0, MAXW])
    rig.check_weights("the ends of the tiles raised")


def _trimmed(big):
    """After a trim the window starts mid-tile and ends mid-tile: the dead slots keep the weight they held when their row fell out,
    2^32 - 1 here, and are never drawn."""
    rig = big
    rig.ingest(BIG // rig.T)                                                     # (a second time round the ring: 66 000 is no multiple of 256)
    assert rig.set_weights(list(range(BIG)), [MAXW] * BIG)
    g = rig.win.ingests
    # about a quarter of the generations stay; of the nearby choices the first whose window starts and ends inside a tile (on the model)
    keep = next(k for k in range(g // 4, g // 4 + 16) if rig.win.ends[g - k - 1] % BIG % wu.TILE and rig.win.written % BIG % wu.TILE)
    rig.trim(keep)
    first = rig.win.first_live() % BIG
    assert rig.win.live < BIG - wu.TILE and first % wu.TILE and (first + rig.win.live) % wu.TILE
    rig.check_weights("trimmed, stale weights in dead slots")
    live = sorted(rig.win.live_slots())
    dead = sorted(set(range(BIG)) - set(live))
    assert len(dead) >= wu.TILE and all(rig.wm.wt[s] == MAXW for s in dead)
    sl, w = wu.pattern_random_third_zero(live, 6)
    assert rig.set_weights(sl, w)
    rig.check_weights("trimmed, random")
    slot, *_ = rig.check_sample(8192 + 257, row_base=1000, where="trimmed")
    drawn = set(int(s) for s in slot)
    assert drawn <= set(live) and not (drawn & {s for s, v in zip(sl, w) if v == 0})
    assert {live[0] // wu.TILE, live[-1] // wu.TILE} <= wu.tiles_hit(slot)
    rig.check_sample(2000, device=True, where="trimmed, device route")
    assert not rig.set_weights([live[0], dead[0]], [1, 1])                       # the host route refuses and writes nothing
    rig.check_weights("refused")


def test_set_weights_and_get_weights_on_both_routes(logic, recorded):
    """Duplicates in either order give the maximum; a dead slot fails the host route before anything is written, the device route skips
    and counts it; Pool.weights reads back, 0 for a dead slot with device pointers."""
    rig = Rig(logic, 2 * recorded[1] + 50, recorded, weighting=100)              # 50 slots stay dead
    rig.ingest(2)
    live = sorted(rig.win.live_slots())
    dead = rig.win.C - 1
    a, b, c = live[0], live[len(live) // 2], live[-1]
    slots, weights = [a, b, a, c, b, a, b], [5, 0, 900, 7, 11, 30, 2]
    for order in (list(range(7)), list(reversed(range(7)))):
        assert rig.set_weights([slots[i] for i in order], [weights[i] for i in order])
        assert (rig.wm.wt[a], rig.wm.wt[b], rig.wm.wt[c]) == (900, 11, 7)
        rig.check_weights("host duplicates")
        sl, wt = dev_i32([slots[i] for i in order] + [dead]), dev_i32([weights[i] + 1 for i in order] + [MAXW])
        rig.wm.set_weights(host_u32(sl), host_u32(wt), False)
        rig.pool.set_weights(sl, wt, device=True)
        assert (rig.wm.wt[a], rig.wm.wt[b], rig.wm.wt[c], rig.wm.wt[dead]) == (901, 12, 8, 100)
        rig.check_weights("device duplicates")
    assert rig.wm.bad_slot == 2 and rig.pool.weight_stats().bad_slot == 2
    assert not rig.set_weights([a, dead, b], [1, 2, 3]) and not rig.set_weights([rig.win.C], [1]) and not rig.set_weights([0xFFFFFFFF], [1])
    rig.check_weights("refused")
    assert code(rig.pool.weights, [a, dead]) == INVALID_ARG
    many = np.random.default_rng(3).integers(0, rig.win.C + 20, 5000)            # a sample with replacement names slots again and again
    given = np.random.default_rng(4).integers(0, MAXW, 5000, endpoint=True)
    rig.wm.set_weights(many, given, False)
    rig.pool.set_weights(dev_i32(many), dev_i32(given), device=True)
    rig.check_weights("5000 entries")
    assert rig.wm.bad_slot > 2
    rig.check_sample(1000, where="after set_weights")
    rig.pool.close()


def test_fresh_rows_uniform_sample_and_device_bytes(logic, recorded):
    """Rows an ingest stores carry the ingest weight of that moment; off -> on -> off gives device_bytes back; tafl_pool_sample draws the
    same rows before, during and after weighting."""
    ex, T = recorded
    Cp = T + T // 2
    rig = Rig(logic, Cp, recorded)
    rig.ingest()
    uniform = [a.tobytes() for a in rig.pool.sample(700, SEED, STEP)]
    before = rig.pool.stats().device_bytes
    st = rig.pool.weight_stats()
    assert all(getattr(st, k) == 0 for k in wu.STAT_NAMES)
    assert code(rig.pool.sample_weighted, 4, 1, 2) == INVALID_ARG and code(rig.pool.set_weights, [0], [1]) == INVALID_ARG   # weighting off
    assert code(rig.pool.weights, [0]) == INVALID_ARG
    rig.set_weighting(5)
    nt = (Cp + wu.TILE - 1) // wu.TILE
    assert rig.pool.weight_stats().device_bytes == 4 * wu.TILE * nt + 20 * nt + 24 == rig.pool.stats().device_bytes - before
    rig.check_weights("5 everywhere")
    rig.set_weighting(17)
    rig.ingest()                                                                 # wraps: T // 2 rows of the first ingest stay, with 5
    fresh = {(T + r) % Cp for r in range(T)}
    assert rig.wm.wt == [17 if s in fresh else 5 for s in range(Cp)] and rig.pool.weight_stats().total_weight == 17 * T + 5 * (Cp - T)
    rig.check_weights("fresh rows")
    rig.check_sample(700, where="fresh rows")
    during = [a.tobytes() for a in rig.pool.sample(700, SEED, STEP)]
    rig.pool.clear(); rig.win.clear()
    st = rig.pool.weight_stats()
    assert (st.enabled, st.ingest_weight, st.total_weight, st.positive) == (1, 17, 0, 0)       # clear keeps the setting
    rig.ingest()
    rig.check_weights("after clear")
    rig.set_weighting(None)
    assert rig.pool.stats().device_bytes == before
    assert code(rig.pool.sample_weighted, 4, 1, 2) == INVALID_ARG
    # the same window as at `uniform` (one ingest into an empty pool): the uniform draw is what it was, and it ignored the weights
    assert [a.tobytes() for a in rig.pool.sample(700, SEED, STEP)] == uniform
    rig.set_weighting(1)
    rig.ingest()
    rig.set_weights(sorted(rig.win.live_slots())[::2], [0] * ((Cp + 1) // 2))
    assert [a.tobytes() for a in rig.pool.sample(700, SEED, STEP)] == during
    rig.pool.close()


def test_errors(logic, recorded):
    from alphazeroforhnefatafl_amd._lib import lib
    from alphazeroforhnefatafl_amd.abi import TaflPoolWeights
    rig = Rig(logic, 300, recorded)
    L, h = lib(), rig.pool._h
    assert L.tafl_pool_set_weighting(h, C.byref(TaflPoolWeights(ingest_weight=1, flags=1))) == UNSUPPORTED
    bad = TaflPoolWeights(ingest_weight=1)
    bad._reserved[5] = 1
    assert L.tafl_pool_set_weighting(h, C.byref(bad)) == UNSUPPORTED
    assert rig.pool.weight_stats().enabled == 0
    rig.set_weighting(2)
    out = [C.c_void_p()] * 8
    assert L.tafl_pool_sample_weighted(h, 1, 2, 0, 4, 1, *out, 0) == INVALID_ARG                 # live == 0
    rig.ingest()
    assert L.tafl_pool_sample_weighted(h, 1, 2, 0, 4, 2, *out, 0) == UNSUPPORTED                 # unknown flags
    assert L.tafl_pool_sample_weighted(h, 1, 2, 0xFFFFFFFF, 4, 1, *out, 0) == INVALID_ARG        # row_base + count above 32 bits
    assert L.tafl_pool_sample_weighted(h, 1, 2, 0xFFFFFFFB, 4, 1, *out, 0) == 0                  # every output may be NULL
    assert L.tafl_pool_set_weights(h, None, None, 3, 0) == INVALID_ARG
    assert L.tafl_pool_get_weights(h, None, 3, None, 0) == INVALID_ARG
    assert rig.set_weights(list(range(300)), [0] * 300)
    assert code(rig.pool.sample_weighted, 4, 1, 2) == INVALID_ARG                                # total == 0
    assert rig.pool.weight_stats().bad_slot == 0 and rig.pool.stats().bad_slot == 0
    rig.pool.close()


def test_two_fresh_pools_driven_identically_are_byte_identical(logic, recorded):
    """No atomic decides a value that depends on an order: weights, draws and rows of two pools after the same calls are the same bytes."""
    import torch
    T = recorded[1]
    outs = []
    many, given = np.random.default_rng(8).integers(0, 700, 4000), np.random.default_rng(9).integers(0, MAXW, 4000, endpoint=True)
    for _ in range(2):
        rig = Rig(logic, 700, recorded, weighting=6)
        rig.ingest()
        rig.pool.set_weights(dev_i32(many), dev_i32(given), device=True)
        rig.pool.set_weighting(40)
        rig.pool.ingest(rig.ex)
        got = rig.pool.sample_weighted(3000, SEED, STEP, device=True)
        outs.append([t.cpu() for t in got[:7]] + [torch.tensor(got[7] & 0x7FFFFFFFFFFFFFFF), rig.pool.weights(dev_i32(np.arange(700))).cpu()])
        rig.pool.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert T > 700
