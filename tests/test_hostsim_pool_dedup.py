"""De-duplication of the training pool (include/taflhip.h tafl_pool_dedup / _gather_dedup / _weights_from_dedup),
CPU only: the product's tafl_pool.hpp (pooldd_row_key, pooldd_insert, pooldd_same, pooldd_zmean, pooldd_weight) compiled for the host
with serial loops around it (tests/hostsim_pool_dedup) against the Python restatement of tests/pool_dedup_util.py.  Every comparison is
exact.  The workload is the one of the issue - Brandubh, 65 lanes from the start position, S = 8, 96 moves - with its floors asserted
on the restatement alone; the same comparisons run against the real kernels in tests/test_gpu_pool_dedup.py."""
import numpy as np
import pytest

from tests import pool_dedup_util as du
from tests import pool_util as qu
from tests import pool_weights_util as wu

N, K = du.N, du.K
SEED, STEP = 0xD0D0CAFE1234, 7


class Rig:
    """A harness pool, the PoolModel of its rows and the WeightModel, driven together."""

    def __init__(self, Cp, weighting=None):
        self.pool, self.model = du.HostDPool(Cp, K, N), qu.PoolModel(Cp, K, N)
        self.wm = wu.WeightModel(self.model)
        if weighting is not None:
            self.pool.set_weighting(weighting); self.wm.set_weighting(weighting)

    def ingest(self, hx, t):
        before = self.model.written
        got = self.pool.ingest(hx)
        assert got == self.model.ingest(t)
        self.wm.ingested(got[0], before)

    def trim(self, keep):
        assert self.pool.trim(keep) == 0
        self.model.trim(keep)

    def check(self, symmetries=False, key_bits=64, where="", **how):
        """One de-duplication against the restatement: keys and canon of every live row, rep / mult / zmean of every live slot through
        both routes of the gather, the result struct."""
        want = du.Dedup(self.model, symmetries, key_bits)
        rc, res = self.pool.dedup(symmetries, key_bits, **how)
        assert rc == 0, where
        for k, v in want.result().items():
            assert res[k] == v, (where, k, res[k], v)
        assert res["device_bytes"] == du.device_bytes(self.model.C), where
        key, canon = self.pool.keys()
        live = want.slots
        assert [int(key[s]) for s in live] == [want.key[s] for s in live] and [int(canon[s]) for s in live] == [want.canon[s] for s in live], where
        rc, rep, mult, zm = self.pool.gather(live, strict=True)
        wr, wmult, wz, bad = want.expect_gather(live)
        assert rc == 0 and bad == 0 and np.array_equal(rep, wr) and np.array_equal(mult, wmult) and zm.tobytes() == wz.tobytes(), where
        every = list(range(self.model.C + 2))
        before = self.pool.pool_stats()["bad_slot"]
        rc, rep, mult, zm = self.pool.gather(every)
        wr, wmult, wz, bad = want.expect_gather(every)
        assert rc == 0 and np.array_equal(rep, wr) and np.array_equal(mult, wmult) and zm.tobytes() == wz.tobytes(), where
        assert self.pool.pool_stats()["bad_slot"] - before == bad == self.model.C + 2 - self.model.live, where
        if bad:
            assert self.pool.gather(every, strict=True)[0] == -1, where
        return want, res


def state(name, weighting=None):
    """room: A into a pool with 50 slots to spare; small: A into 1 500 slots (the oldest ranks are never stored); wrapped: A then B
    across the ring's end of 3 000 slots; trimmed: the same and a trim to one generation."""
    hx, ta, hy, tb = du.host_workload()
    Ta = qu.coverage(ta)["taken"]
    if name == "room":
        rig = Rig(Ta + 50, weighting)
        rig.ingest(hx, ta)
        assert rig.model.live == Ta < rig.model.C
    elif name == "small":
        rig = Rig(1500, weighting)
        rig.ingest(hx, ta)
        assert rig.model.live == 1500 < Ta
    else:
        rig = Rig(3000, weighting)
        rig.ingest(hx, ta); rig.ingest(hy, tb)
        assert rig.model.written > 3000 and rig.model.live == 3000
        if name == "trimmed":
            rig.trim(1)
            assert rig.model.live == qu.coverage(tb)["taken"] < 3000 and rig.model.first_live() % 3000 + rig.model.live > 3000      # wraps
    return rig


STATES = ["room", "small", "wrapped", "trimmed"]


def test_workload_meets_the_floors():
    """On the restatement alone.  Run A by raw boards: 1 675 groups, the largest 38, 215 of two or more, 69 with both results, 1 460
    singletons; 1 629 groups under symmetries, 46 of them join different raw boards."""
    hx, ta, hy, tb = du.host_workload()
    got = du.assert_floors(ta, "A")
    du.assert_floors(tb, "B")
    assert got["groups"] > got["sym_groups"]
    both = qu.PoolModel(5000, K, N)
    both.ingest(ta); both.ingest(tb)
    assert du.census(both)["both_generations"] >= 1
    assert not (ta.z[ta.final != 0] == np.float32(1e-4)).any()                    # no drawn game: zmean with draws is tested on counts
    # the hash-free census and the grouping by keys agree at 64 bits
    dd = du.Dedup(both), du.Dedup(both, symmetries=True)
    c = du.census(both)
    assert (dd[0].distinct, dd[1].distinct, dd[0].collisions, dd[1].collisions) == (c["groups"], c["sym_groups"], 0, 0)
    assert sum(1 for v in dd[1].canon.values() if v) > 100                      # canon is not always the identity


def test_images_and_hash_primitives():
    for n in (3, 7, 8, 13):
        du.check_images(n)
    # the first two outputs of splitmix64 from state 0, as published
    assert du.mix64_int(0) == 0 and du.mix64_int(du.GOLD) == 0xE220A8397B1DCDAF == int(du.mix64(np.asarray([du.GOLD], np.uint64))[0])
    assert du.mix64_int((2 * du.GOLD) & du.M64) == 0x6E789E6AA1B965F4
    # one row by hand: Python integers, word by word
    b = np.random.default_rng(4).integers(0, 40, (1, 7, 7)).astype(np.uint8)
    flat = list(b.reshape(-1)) + [0] * 3
    x = du.GOLD ^ 1
    for i in range(13):
        x = du.mix64_int(x ^ sum(int(flat[4 * i + k]) << (8 * k) for k in range(4)))
    assert int(du.hashes(b, [1], 0)[0]) == x
    assert du.keys(b, [1], False, 6)[0][0] == ((x & 63) or 1) and du.keys(b, [1], False, 0)[0][0] == x
    for live, ts in ((1, 64), (32, 64), (33, 128), (2014, 4096), (2048, 4096), (2049, 8192)):
        assert du.dlib().hspd_table_size(live) == ts


@pytest.mark.parametrize("name", STATES)
@pytest.mark.parametrize("symmetries", [False, True])
def test_dedup_equals_the_restatement(name, symmetries):
    rig = state(name)
    want, res = rig.check(symmetries, where=(name, symmetries))
    assert res["collisions"] == 0 and res["largest"] >= (30 if name != "small" else 1) and res["distinct"] < res["live"]
    if name == "wrapped":
        gens = {s: rig.model.slots[s]["generation"] for s in want.slots}
        assert any(gens[s] != gens[want.rep[s]] for s in want.slots)             # groups with members of both generations


@pytest.mark.parametrize("symmetries", [False, True])
def test_outputs_do_not_depend_on_the_order_or_the_table(symmetries):
    """Three permutations of the insertion order, runs of equal keys inserted together in waves of 64 and of 7, the table at exactly
    `live` entries (full load: probes wrap the end) and one entry more: the same outputs as the restatement every time."""
    rig = state("wrapped")
    live = rig.model.live
    rng = np.random.default_rng(5)
    for how in (dict(perm=np.arange(live)[::-1]), dict(perm=rng.permutation(live)), dict(perm=rng.permutation(live), wave=64), dict(wave=64), dict(wave=7),
                dict(table_size=live), dict(table_size=live + 1, perm=rng.permutation(live)), dict(table_size=live, wave=64)):
        rig.check(symmetries, where=sorted(how))
    assert rig.pool.dedup(table_size=live - 1)[0] == -1


@pytest.mark.parametrize("name", ["room", "wrapped"])
@pytest.mark.parametrize("symmetries", [False, True])
def test_six_bit_keys_collide(name, symmetries):
    rig = state(name)
    want, res = rig.check(symmetries, key_bits=6, where=(name, symmetries))
    assert res["distinct"] <= 64 and res["collisions"] == want.collisions > 0
    rig.check(symmetries, key_bits=6, table_size=rig.model.live, perm=np.arange(rig.model.live)[::-1], where="full table")
    w1, r1 = rig.check(symmetries, key_bits=1, where="one bit")
    assert r1["distinct"] <= 2
    rig.check(symmetries, key_bits=0, where="0 means 64")


def test_zmean_on_synthetic_counts():
    f = du.dlib().hspd_zmean
    for m, wins, losses in ((1, 0, 0), (1, 1, 0), (1, 0, 1), (2, 1, 1), (3, 1, 1), (3, 0, 0), (7, 3, 2), (38, 20, 18), (1000003, 1, 2), (2 ** 32 - 1, 2 ** 31, 5)):
        got = np.float32(f(m, wins, losses))
        assert got.tobytes() == du.zmean(m, wins, losses).tobytes(), (m, wins, losses)
    assert np.float32(f(1, 0, 0)) == np.float32(1e-4) and np.float32(f(2, 1, 1)) == 0 and np.float32(f(5, 5, 0)) == 1 and np.float32(f(4, 0, 4)) == -1


@pytest.mark.parametrize("name", ["room", "trimmed"])
def test_weight_rules(name):
    """All three rules against the WeightModel, with scale below the largest group (weight 1 applies), a zero weight under DIVIDE, and
    the draws that follow."""
    rig = state(name, weighting=1000)
    want, res = rig.check(True)
    live = want.slots
    assert rig.pool.weights_from_dedup(5) == 0                                   # scale < m for the large groups
    want.apply_weights(rig.wm, 5)
    assert [int(v) for v in rig.pool.raw_weights()] == rig.wm.wt
    assert {rig.wm.wt[s] for s in live} >= {1, 2, 5} and res["largest"] > 5
    assert rig.pool.weights_from_dedup(10 ** 6) == 0
    want.apply_weights(rig.wm, 10 ** 6)
    assert [int(v) for v in rig.pool.raw_weights()] == rig.wm.wt
    # every distinct position carries (nearly) the same total
    total = {}
    for s in live:
        total[want.rep[s]] = total.get(want.rep[s], 0) + rig.wm.wt[s]
    assert all(10 ** 6 - want.mult[r] < t <= 10 ** 6 for r, t in total.items())
    rc, slot, sym, w, tot = rig.pool.draw(3000, SEED, STEP)
    ws, wy, ww, wt, _ = rig.wm.draw_many(SEED, STEP, 0, 3000)
    assert rc == 0 and tot == wt and np.array_equal(slot, ws) and np.array_equal(sym, wy) and np.array_equal(w, ww)
    # DIVIDE keeps what the rows carry: surprise-like weights, a zero among them, and a 3 in the largest group (3 // m = 0: weight 1)
    sl, given = wu.pattern_random_third_zero(live, 3)
    big = [s for s in live if want.mult[s] == res["largest"]]
    given[sl.index(big[0])], given[sl.index(big[1])] = 3, 0
    assert rig.pool.set_weights(sl, given) == 0 and rig.wm.set_weights(sl, given, True)
    assert rig.pool.weights_from_dedup(77, du.DIVIDE) == 0
    want.apply_weights(rig.wm, 77, du.DIVIDE)
    assert [int(v) for v in rig.pool.raw_weights()] == rig.wm.wt and rig.wm.wt[big[0]] == 1 and rig.wm.wt[big[1]] == 0
    assert rig.pool.weights_from_dedup(9, du.REPRESENTATIVES) == 0
    want.apply_weights(rig.wm, 9, du.REPRESENTATIVES)
    assert [int(v) for v in rig.pool.raw_weights()] == rig.wm.wt
    assert rig.wm.total == 9 * res["distinct"] and rig.wm.positive == res["distinct"]
    rc, slot, _, w, tot = rig.pool.draw(2000, SEED, STEP + 1)
    assert rc == 0 and tot == 9 * res["distinct"] and all(want.rep[int(s)] == int(s) for s in slot)
    dead = [s for s in range(rig.model.C) if s not in want.rep]
    assert dead and all(rig.wm.wt[s] == 1000 for s in dead)                      # dead slots are not assigned
    assert rig.pool.weights_from_dedup(1, 3) == -5 and rig.pool.weights_from_dedup(1, 4) == -5


def test_validity_and_refusals():
    hx, ta, hy, tb = du.host_workload()
    rig = Rig(3000, weighting=4)
    assert rig.pool.dedup()[0] == -1                                           # live == 0
    assert rig.pool.gather([0])[0] == -1 and rig.pool.weights_from_dedup(1) == -1
    rig.ingest(hx, ta)
    assert rig.pool.dedup(key_bits=65)[0] == -5
    assert rig.pool.gather([0])[0] == -1                                       # a refused call leaves no result
    for change in ("ingest", "trim", "clear"):
        rig.check(where=change)
        assert rig.pool.weights_from_dedup(3) == 0
        if change == "ingest":
            rig.ingest(hy, tb)
        elif change == "trim":
            rig.trim(5)                                                         # (keeps everything: the result is dropped all the same)
        else:
            rig.pool.clear(); rig.model.clear()
        assert rig.pool.gather([0])[0] == -1 and rig.pool.weights_from_dedup(3) == -1, change
    rig.ingest(hx, ta)
    rig.check(True, where="after clear")
    rig.pool.set_weighting(None)
    assert rig.pool.weights_from_dedup(3) == -1                                 # weighting off
    rig.pool.release()
    assert rig.pool.gather([0])[0] == -1
    assert rig.check(where="after release")[1]["device_bytes"] == du.device_bytes(3000)
