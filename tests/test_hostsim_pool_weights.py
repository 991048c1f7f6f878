"""Weighted sampling of the training pool (include/taflhip.h tafl_pool_set_weighting / _set_weights / _sample_weighted, DESIGN.md section
19), CPU only: the product's tafl_pool.hpp (pool_eff, pool_wdraw, pool_mulhi64, the 64-ary tile search pool_wsearch_*, pool_wpick,
pool_stored_slot) compiled for the host with the tile structure around it (tests/hostsim_pool_weights) against the Python restatement of
tests/pool_weights_util.py.  Every comparison is exact.  The examples are the workload of tests/test_hostsim_pool.py (Brandubh, 64 lanes,
S = 8, K = 6); the same comparisons run against the real kernels in tests/test_gpu_pool_weights.py."""
import numpy as np
import pytest

from tests import pool_util as qu
from tests import pool_weights_util as wu
from tests import test_hostsim_pool as base

N, K = base.N, base.K
DRAWS = 10000
SEED, STEP = 0xC0FFEE1234567, 41
MAXW = wu.MAXW


class Rig:
    """A harness pool, the PoolModel of its rows and the WeightModel, driven together."""

    def __init__(self, Cp, weighting=None):
        self.pool, self.model = wu.HostWPool(Cp, K, N), qu.PoolModel(Cp, K, N)
        self.wm = wu.WeightModel(self.model)
        if weighting is not None:
            self.set_weighting(weighting)

    def set_weighting(self, w):
        self.pool.set_weighting(w); self.wm.set_weighting(w)

    def ingest(self, hx, t):
        before = self.model.written
        got = self.pool.ingest(hx)
        assert got == self.model.ingest(t)
        self.wm.ingested(got[0], before)

    def trim(self, keep):
        assert self.pool.trim(keep) == 0
        self.model.trim(keep)

    def set_weights(self, slots, weights, strict=True):
        ok = self.wm.set_weights(slots, weights, strict)
        assert self.pool.set_weights(slots, weights, strict) == (0 if ok else -1)
        return ok

    def check_weights(self, where=""):
        """Every slot's stored weight, dead slots included; the counters; the tile structure against the running sum."""
        assert [int(v) for v in self.pool.raw_weights()] == self.wm.wt, where
        st = self.pool.stats()
        for k, v in self.wm.stats().items():
            assert st[k] == v, (where, k, st[k], v)
        W = self.wm.prefix()
        ts, tp = self.pool.tiles()
        for t in range(len(ts)):
            assert int(tp[t]) == W[t * wu.TILE] and int(ts[t]) == W[min((t + 1) * wu.TILE, self.model.C)] - W[t * wu.TILE], (where, t)

    def check_draws(self, count=DRAWS, row_base=3, where=""):
        rc, slot, sym, w, total, steps = self.pool.draw(count, SEED, STEP, row_base)
        assert rc == 0, where
        ws, wy, ww, wt, ks = self.wm.draw_many(SEED, STEP, row_base, count)
        assert total == wt and np.array_equal(slot, ws) and np.array_equal(sym, wy) and np.array_equal(w, ww), where
        assert max(ks) < total and set(int(s) for s in slot) <= set(self.model.live_slots()) and (w > 0).all(), where
        assert set(np.unique(sym)) == set(range(8)), where
        for i in (0, 1, count // 2, count - 1):                                 # the running sum itself, slot after slot
            assert self.wm.draw_serial(SEED, STEP, row_base + i) == (int(slot[i]), int(sym[i]), int(w[i])), (where, i)
        return slot, w, total, steps


def build(state, weighting=None):
    """not_wrapped: A, B, A into a pool with 40 slots to spare (dead slots at the end, among them C - 1); wrapped: A, B, A, B into 300 slots;
    trimmed: the same and trim(2), which leaves a window that starts mid-tile and wraps.  Weighting goes on before the first ingest."""
    hx, ta, hy, tb, *_ = base.workload()
    Ta, Tb = qu.coverage(ta)["taken"], qu.coverage(tb)["taken"]
    if state == "not_wrapped":
        rig = Rig(2 * Ta + Tb + 40, weighting)
        for hz, tz in ((hx, ta), (hy, tb), (hx, ta)):
            rig.ingest(hz, tz)
        assert 257 < rig.model.written < rig.model.C and rig.model.live == rig.model.written
    else:
        rig = Rig(300, weighting)
        for hz, tz in ((hx, ta), (hy, tb), (hx, ta), (hy, tb)):
            rig.ingest(hz, tz)
        assert rig.model.written > 300 + 40 and rig.model.live == 300
        if state == "trimmed":
            rig.trim(2)
            first = rig.model.first_live() % 300
            assert rig.model.live == Ta + Tb < 300 and first % wu.TILE and first + rig.model.live > 300      # starts mid-tile, wraps
    assert rig.pool.pool_stats() == dict(written=rig.model.written, live=rig.model.live, ingests=rig.model.ingests)
    return rig


STATES = ["not_wrapped", "wrapped", "trimmed"]


def test_mulhi64():
    vals = [0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 0x123456789ABCDEF0, 0xFEDCBA9876543210, 300 * MAXW]
    for a in vals:
        for b in vals:
            assert wu.wlib().hspw_mulhi64(a, b) == (a * b) >> 64, (a, b)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("w", [1, 5, MAXW])
def test_all_weights_equal(state, w):
    """Every slot, dead ones too, carries w (off -> on gives every slot ingest_weight, ingests store it): the slot-order index of a draw
    is mulhi64(r, live * w) // w, and no dead slot is drawn although it carries the same weight."""
    rig = build(state, w)
    assert rig.wm.wt == [w] * rig.model.C
    rig.check_weights((state, w))
    slot, dw, total, steps = rig.check_draws(where=(state, w))
    order = sorted(rig.model.live_slots())
    assert total == rig.model.live * w and (dw == w).all()
    for i in range(0, DRAWS, 7):
        k, _ = wu.draw_k(SEED, STEP, 3 + i, total)
        assert int(slot[i]) == order[k // w]
    if state != "wrapped":
        assert rig.model.live < rig.model.C                                     # there are dead slots, carrying w
    elif w == MAXW:
        assert total > 2 ** 40
    assert wu.tiles_hit(slot) == wu.tiles_hit(order) and len(wu.tiles_hit(order)) == 2        # the first and the last live tile
    assert steps.max() == 1                                                    # two tiles: one step of the tile search


@pytest.mark.parametrize("state", STATES)
def test_one_row_with_a_weight(state):
    """All weight on slot 0, 255, 256 or C - 1 (the ends of the tiles): every draw is that slot.  Where the slot is not live the host
    route refuses the call and writes nothing."""
    rig = build(state, 0)
    tested = 0
    for s in (0, 255, 256, rig.model.C - 1):
        before = list(rig.wm.wt)
        if not rig.set_weights([s], [9]):
            assert s not in rig.model.live_slots() and rig.wm.wt == before
            rig.check_weights((state, s, "refused"))
            continue
        rig.check_weights((state, s))
        slot, w, total, _ = rig.check_draws(500, where=(state, s))
        assert total == 9 and (slot == s).all() and (w == 9).all() and rig.pool.stats()["positive"] == 1
        assert rig.set_weights([s], [0])
        tested += 1
    assert tested == (3 if state == "not_wrapped" else 4)
    assert rig.pool.draw(1, 1, 1)[0] == -1                                      # total == 0


@pytest.mark.parametrize("state", STATES)
def test_random_weights_with_every_third_row_silenced(state):
    """Dead slots carry 2^32 - 1 (from off -> on) and are never drawn; a third of the live rows has weight 0 and is never drawn."""
    rig = build(state, MAXW)
    sl, w = wu.pattern_random_third_zero(rig.model.live_slots(), 5)
    assert rig.set_weights(sl, w)
    rig.check_weights(state)
    zero = {s for s, v in zip(sl, w) if v == 0}
    assert 3 * len(zero) >= rig.model.live and rig.pool.stats()["positive"] == rig.model.live - len(zero)
    dead = set(range(rig.model.C)) - set(sl)
    if state != "wrapped":
        assert dead and all(rig.wm.wt[s] == MAXW for s in dead)
    slot, _, _, _ = rig.check_draws(where=state)
    drawn = set(int(s) for s in slot)
    assert not (drawn & zero) and not (drawn & dead)
    assert {min(sl) // wu.TILE, max(sl) // wu.TILE} <= wu.tiles_hit(slot)        # the first and the last live tile
    assert len(drawn) >= (rig.model.live - len(zero)) // 2


def test_every_weight_at_the_maximum_in_a_full_pool():
    rig = build("wrapped", 3)
    assert rig.set_weights(list(range(300)), [MAXW] * 300)
    rig.check_weights()
    _, w, total, _ = rig.check_draws()
    assert total == 300 * MAXW > 2 ** 40 and (w == MAXW).all()


def test_max_rule_with_duplicate_slots():
    """A slot named more than once holds the maximum afterwards, whatever the order; a smaller maximum than the stored weight lowers it;
    slots not named are unchanged; a dead slot fails the host route before anything is written and is skipped and counted otherwise."""
    rig = build("trimmed", 100)
    live = sorted(rig.model.live_slots())
    dead = sorted(set(range(300)) - set(live))
    a, b, c = live[0], live[len(live) // 2], live[-1]
    slots, weights = [a, b, a, c, b, a, b], [5, 0, 900, 7, 11, 30, 2]
    for order in (range(7), reversed(range(7))):
        order = list(order)
        assert rig.set_weights([slots[i] for i in order], [weights[i] for i in order])
        assert (rig.wm.wt[a], rig.wm.wt[b], rig.wm.wt[c]) == (900, 11, 7)
        rig.check_weights("duplicates")
        assert rig.set_weights([a, b, c], [100, 100, 100])
    before = list(rig.wm.wt)
    assert not rig.set_weights([a, dead[0], b], [1, 2, 3]) and not rig.set_weights([300], [1]) and rig.wm.wt == before
    rig.check_weights("refused")
    assert rig.set_weights([a, dead[0], b, 300, a, 0xFFFFFFFF], [1, 2, 3, 4, 6, 7], strict=False)
    assert rig.wm.bad_slot == 3 and (rig.wm.wt[a], rig.wm.wt[b], rig.wm.wt[dead[0]]) == (6, 3, 100)
    rig.check_weights("device route")
    assert np.array_equal(rig.pool.get_weights([a, dead[0], b, 300]), rig.wm.get([a, dead[0], b, 300]))
    assert list(rig.pool.get_weights([a, dead[0], 300])) == [6, 0, 0]
    rig.check_draws(2000, where="after the max rule")


def test_reweighting_after_an_ingest_that_overwrites():
    """An ingest gives the rows it stores the ingest weight of that moment and leaves the others; a changed ingest weight touches no stored
    weight; one ingest larger than the pool stores min(T, C) rows."""
    hx, ta, hy, tb, he, te = base.workload()
    rig = build("wrapped", 4)
    sl, w = wu.pattern_random_third_zero(rig.model.live_slots(), 9)
    assert rig.set_weights(sl, w)
    rig.set_weighting(77)
    rig.check_weights("on -> on changes nothing stored")
    assert rig.wm.wt == w
    before = rig.model.written
    rig.ingest(hy, tb)
    fresh = {(before + r) % 300 for r in range(qu.coverage(tb)["taken"])}
    assert all(rig.wm.wt[s] == (77 if s in fresh else w[s]) for s in range(300))
    rig.check_weights("overwritten")
    rig.check_draws(where="overwritten")
    rig.ingest(he, te)                                                          # T = 0: nothing stored
    rig.check_weights("empty ingest")
    assert rig.set_weights(sorted(fresh), [0] * len(fresh))                     # the trainer silences what it has not seen yet
    slot, _, _, _ = rig.check_draws(2000, where="fresh rows silenced")
    assert not (set(int(s) for s in slot) & fresh)
    small = Rig(50, 12)
    small.ingest(hx, ta)                                                        # T > C
    small.set_weighting(13)
    small.ingest(hy, tb)
    assert small.wm.wt == [13] * 50
    small.check_weights("T > C")
    small.check_draws(1000, where="T > C")
    one = Rig(1, 3)
    one.ingest(hx, ta)
    one.check_weights("C = 1")
    slot, w1, total, _ = one.check_draws(100, where="C = 1")
    assert total == 3 and not slot.any()


def test_trim_clear_and_switching_off():
    rig = build("wrapped", 6)
    rig.check_weights()
    r0 = rig.pool.stats()["rebuilds"]
    rig.check_draws(100); rig.check_draws(100)
    assert rig.pool.stats()["rebuilds"] == r0                                   # nothing changed: no rebuild
    rig.trim(1)
    rig.check_weights("trim 1")
    assert rig.pool.stats()["rebuilds"] == r0 + 1 and rig.pool.stats()["total_weight"] == 6 * rig.model.live
    rig.check_draws(1000, where="trim 1")
    rig.pool.clear(); rig.model.clear()
    assert rig.pool.draw(1, 1, 1)[0] == -1                                      # live == 0
    st = rig.pool.stats()
    assert st["enabled"] == 1 and st["ingest_weight"] == 6 and st["total_weight"] == 0 and st["positive"] == 0
    hx, ta, *_ = base.workload()
    rig.ingest(hx, ta)                                                          # the setting outlived the clear
    rig.check_weights("after clear")
    rig.check_draws(1000, where="after clear")
    rig.set_weighting(None)
    assert rig.pool.stats() == dict.fromkeys(wu.STAT_NAMES, 0) and rig.pool.draw(1, 1, 1)[0] == -1
    assert rig.pool.set_weights([0], [1], True) == -1
    rig.set_weighting(2)                                                        # on again: every slot starts at the new ingest weight
    rig.check_weights("on again")


def test_errors_and_four_ranks_equal_one_call():
    rig = build("trimmed", MAXW)
    sl, w = wu.pattern_random_third_zero(rig.model.live_slots(), 2)
    assert rig.set_weights(sl, w)
    rc, slot, sym, dw, total, _ = rig.pool.draw(DRAWS, SEED, STEP, 5)
    parts = [rig.pool.draw(DRAWS // 4, SEED, STEP, 5 + k * (DRAWS // 4)) for k in range(4)]
    for i, whole in ((1, slot), (2, sym), (3, dw)):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), whole)
    assert all(p[4] == total for p in parts)
    s0 = rig.pool.draw(100, SEED, STEP, 5, flags=0)
    assert np.array_equal(s0[1], slot[:100]) and not s0[2].any()                # without TAFL_POOL_SAMPLE_SYM: the same slots, sym = 0
    assert not np.array_equal(rig.pool.draw(100, SEED, STEP + 1, 5)[1], slot[:100])
    assert rig.pool.draw(1, SEED, STEP, flags=2)[0] == -5 and rig.pool.draw(2, SEED, STEP, row_base=0xFFFFFFFF)[0] == -1
    assert rig.pool.draw(1, SEED, STEP, row_base=0xFFFFFFFE)[0] == 0
    rows, bad = rig.pool.gather(slot[:64], sym[:64])                            # the rows of a draw are live rows
    assert bad == 0
    for got, want in zip(rows, rig.model.expect_gather(slot[:64], sym[:64])):
        assert got.tobytes() == want.tobytes()


def test_tile_search_over_more_than_64_tiles():
    """67 tiles: the 64-ary search takes two steps.  The pool is filled by some 200 ingests (the window alone is modelled), wraps, and is trimmed
    to a window that starts mid-tile."""
    hx, ta, hy, tb, *_ = base.workload()
    Cp = 66 * wu.TILE + 100
    pool, win = wu.HostWPool(Cp, K, N), wu.Window(Cp)
    wm = wu.WeightModel(win)
    pool.set_weighting(MAXW); wm.set_weighting(MAXW)
    g = 0
    while win.written < Cp + 3000:
        before = win.written
        T = pool.ingest(hx if g % 2 == 0 else hy)[0]
        win.took(T); wm.ingested(T, before)
        g += 1
    keep = g - 60
    assert pool.trim(keep) == 0
    win.trim(keep)
    assert pool.pool_stats() == dict(written=win.written, live=win.live, ingests=g) and win.live < Cp and (win.first_live() % Cp) % wu.TILE
    sl, w = wu.pattern_random_third_zero(win.live_slots(), 4)
    assert wm.set_weights(sl, w, True) and pool.set_weights(sl, w, True) == 0
    assert [int(v) for v in pool.raw_weights()] == wm.wt
    W = wm.prefix()
    ts, tp = pool.tiles()
    assert len(tp) == 67 and all(int(tp[t]) == W[t * wu.TILE] for t in range(67)) and W[-1] > 2 ** 40
    rc, slot, sym, dw, total, steps = pool.draw(DRAWS, SEED, STEP, 0)
    ws, wy, ww, wt, _ = wm.draw_many(SEED, STEP, 0, DRAWS)
    assert rc == 0 and total == wt and np.array_equal(slot, ws) and np.array_equal(sym, wy) and np.array_equal(dw, ww)
    assert steps.max() == 2
    zero = {s for s, v in zip(sl, w) if v == 0}
    drawn = set(int(s) for s in slot)
    assert 3 * len(zero) >= win.live and not (drawn & zero) and drawn <= set(sl)
    live_tiles = wu.tiles_hit(sl)
    assert len(wu.tiles_hit(slot)) >= len(live_tiles) - 2 and {0, 66} <= wu.tiles_hit(slot)
