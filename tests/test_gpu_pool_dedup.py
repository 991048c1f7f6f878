"""De-duplication of the training pool on the device (include/taflhip.h tafl_pool_dedup / _gather_dedup / _weights_from_dedup, DESIGN.md
section 24): k_pooldd_key, k_pooldd_insert, k_pooldd_finish, k_pooldd_weights and k_pooldd_gather against the Python restatement of
tests/pool_dedup_util.py, through the C-ABI.  Every comparison is exact.  The examples come from rollout-mode tafl_selfplay_record runs
from the start position (Brandubh 7x7, 65 lanes, S = 8, 96 moves: the start position once per game, the early moves many times, in
runs that cross a wave's end); 13x13 on the 256-bit word and 8x8 on the 128-bit word for board images of several words and of a length
that is no multiple of four."""
import ctypes as C

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd._lib import TaflError
from tests import pool_dedup_util as du
from tests import pool_util as qu
from tests import pool_weights_util as wu

pytestmark = pytest.mark.gpu

N, K = du.N, du.K
SEED, STEP = 0xFEDCBA9876543210, 12
INVALID_ARG, UNSUPPORTED = -1, -5
_LOGICS = {}


def gpu_logic(rules, n, wb):
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    if (n, wb) not in _LOGICS:
        _LOGICS[(n, wb)] = BatchedGameLogic(rules, n, wb, device=0)
    return _LOGICS[(n, wb)]


def record(lg, fen, G, moves, k, seed, sample_seed, cap=du.CAP, hand_set=False):
    """(Examples, its Table) of a run from the start position.  hand_set: the results are set by hand before the examples are
    finalized (training_rows_util.hand_set_results: open / attackers / defenders / draw by g % 4), for boards on which no game ends
    within the run."""
    b = lg.new_batch(G, fen)
    ex = lg.new_examples(G, moves, k)
    b.selfplay_record(ex, moves, du.SIMS, 1.0, seed, cap, sample_seed=sample_seed, temp_moves=du.TEMP_MOVES, want_plays=False)
    if hand_set:
        from tests import parity_util as pu
        from tests import training_rows_util as tu
        final = pu.clone_states(b.download(), G)
        tu.hand_set_results(final, G)
        b.upload(final)
    ex.finalize(b)
    b.close()
    return ex, qu.device_table(ex)


@pytest.fixture(scope="module")
def logic():
    return gpu_logic(abi.rules.BRANDUBH, N, du.WB)


@pytest.fixture(scope="module")
def runs(logic):
    """(ex A, table A, ex B, table B): recorded and finalized once, left unchanged."""
    out = []
    for seed, sample_seed in du.RUNS.values():
        out += record(logic, abi.boards.BRANDUBH, du.G, du.MOVES, K, seed, sample_seed)
    return tuple(out)


def code(fn, *a, **kw):
    with pytest.raises(TaflError) as e:
        fn(*a, **kw)
    return e.value.code


def dev_i32(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint32).view(np.int32).copy()).to(torch.device("cuda", 0))


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


class Rig:
    """A device pool, the PoolModel of its rows and the WeightModel, driven together."""

    def __init__(self, lg, Cp, weighting=None, k=K):
        self.pool, self.model = lg.new_pool(Cp, k), qu.PoolModel(Cp, k, lg.side_len)
        self.wm = wu.WeightModel(self.model)
        if weighting is not None:
            self.pool.set_weighting(weighting); self.wm.set_weighting(weighting)

    def ingest(self, ex, t):
        before = self.model.written
        got = self.pool.ingest(ex)
        assert got == self.model.ingest(t)
        self.wm.ingested(got[0], before)

    def trim(self, keep):
        self.pool.trim(keep); self.model.trim(keep)

    def check(self, symmetries=False, key_bits=64, where=""):
        """One tafl_pool_dedup against the restatement: the result struct, rep / mult / zmean of every live slot with host pointers, of
        every slot and two beyond C with device pointers (zeros for the dead ones, counted)."""
        want = du.Dedup(self.model, symmetries, key_bits)
        res = self.pool.dedup(symmetries, key_bits)
        for k, v in want.result().items():
            assert getattr(res, k) == v, (where, k, getattr(res, k), v)
        live = want.slots
        wr, wmult, wz, _ = want.expect_gather(live)
        rep, mult, zm = self.pool.gather_dedup(live)
        assert np.array_equal(rep, wr) and np.array_equal(mult, wmult) and zm.tobytes() == wz.tobytes(), where
        every = np.arange(self.model.C + 2, dtype=np.uint32)
        before = self.pool.stats().bad_slot
        rep, mult, zm = (host(t) for t in self.pool.gather_dedup(dev_i32(every), device=True))
        wr, wmult, wz, bad = want.expect_gather(every)
        assert np.array_equal(rep, wr) and np.array_equal(mult, wmult) and zm.tobytes() == wz.tobytes(), where
        assert self.pool.stats().bad_slot - before == bad == self.model.C + 2 - self.model.live, where
        return want, res


def state(lg, runs, name, weighting=None):
    """room: A into 4 096 slots; small: A into 1 500 (the oldest ranks are never stored); wrapped: A then B across the end of a ring of
    3 000; trimmed: the same and a trim to one generation."""
    ex, ta, ey, tb = runs
    Ta = qu.coverage(ta)["taken"]
    rig = Rig(lg, {"room": 4096, "small": 1500}.get(name, 3000), weighting)
    rig.ingest(ex, ta)
    if name == "room":
        assert rig.model.live == Ta < 4096
    elif name == "small":
        assert rig.model.live == 1500 < Ta
    else:
        rig.ingest(ey, tb)
        assert rig.model.written > 3000 and rig.model.live == 3000
        if name == "trimmed":
            rig.trim(1)
            assert rig.model.live == qu.coverage(tb)["taken"] < 3000 and rig.model.first_live() % 3000 + rig.model.live > 3000      # wraps
    return rig


def test_workload_meets_the_floors(runs):
    """On the restatement alone, from Examples.read / Examples.gather of the recorded runs."""
    ex, ta, ey, tb = runs
    got = du.assert_floors(ta, "A")
    du.assert_floors(tb, "B")
    print("run A:", got)
    both = qu.PoolModel(5000, K, N)
    both.ingest(ta); both.ingest(tb)
    assert du.census(both)["both_generations"] >= 1
    assert not (ta.z[ta.final != 0] == np.float32(1e-4)).any()


@pytest.mark.parametrize("name", ["room", "small", "wrapped", "trimmed"])
def test_dedup_equals_the_restatement(logic, runs, name):
    """Both flag settings at 64 bits, then 6-bit keys (at most 64 groups, collisions as expected and above 0), then 64 bits again: a
    call leaves nothing of the call before it."""
    rig = state(logic, runs, name)
    for symmetries in (False, True):
        want, res = rig.check(symmetries, where=(name, symmetries))
        assert res.collisions == 0 and res.distinct < res.live and res.device_bytes >= du.device_bytes(rig.model.C)
        if name != "small":
            assert res.largest >= 30
        want6, res6 = rig.check(symmetries, key_bits=6, where=(name, symmetries, 6))
        assert res6.distinct <= 64 and res6.collisions == want6.collisions > 0
    rig.check(True, key_bits=0, where=(name, "0 means 64"))
    if name == "wrapped":
        want, _ = rig.check(where="generations")
        gens = {s: rig.model.slots[s]["generation"] for s in want.slots}
        assert any(gens[s] != gens[want.rep[s]] for s in want.slots)             # groups with members of both generations
    rig.pool.close()


def test_gather_dedup_on_both_routes(logic, runs):
    """Counts 1 and 257 (a second workgroup) with host and device pointers; any output may be NULL; a dead slot fails the host route
    before anything is written and gives zeros, counted, on the device route."""
    from alphazeroforhnefatafl_amd._lib import lib
    rig = state(logic, runs, "trimmed")
    want, _ = rig.check(True)
    live = want.slots
    dead = sorted(set(range(3000)) - set(live))
    assert len(dead) > 100
    for count in (1, 257):
        sl = np.asarray(live[-count:], np.uint32)
        wr, wmult, wz, _ = want.expect_gather(sl)
        rep, mult, zm = rig.pool.gather_dedup(sl)
        drep, dmult, dzm = (host(t) for t in rig.pool.gather_dedup(dev_i32(sl), device=True))
        for got in ((rep, mult, zm), (drep, dmult, dzm)):
            assert np.array_equal(got[0], wr) and np.array_equal(got[1], wmult) and got[2].tobytes() == wz.tobytes(), count
        mixed = sl.copy()
        mixed[count // 2] = dead[count % len(dead)]
        assert code(rig.pool.gather_dedup, mixed) == INVALID_ARG
        before = rig.pool.stats().bad_slot
        drep, dmult, dzm = (host(t) for t in rig.pool.gather_dedup(dev_i32(mixed), device=True))
        wr, wmult, wz, bad = want.expect_gather(mixed)
        assert bad == 1 and rig.pool.stats().bad_slot == before + 1
        assert np.array_equal(drep, wr) and np.array_equal(dmult, wmult) and dzm.tobytes() == wz.tobytes() and drep[count // 2] == 0 and dmult[count // 2] == 0
    L, h, vp = lib(), rig.pool._h, C.c_void_p
    sl = np.asarray(live[:5], np.uint32)
    only = np.zeros(5, np.uint32)
    assert L.tafl_pool_gather_dedup(h, sl.ctypes.data_as(vp), 5, None, only.ctypes.data_as(vp), None, 0) == 0
    assert np.array_equal(only, want.expect_gather(sl)[1])
    assert L.tafl_pool_gather_dedup(h, sl.ctypes.data_as(vp), 5, None, None, None, 0) == 0
    assert L.tafl_pool_gather_dedup(h, None, 5, None, None, None, 0) == INVALID_ARG and L.tafl_pool_gather_dedup(h, None, 0, None, None, None, 0) == 0
    rig.pool.close()


def _same_weights(rig, where):
    live = sorted(rig.model.live_slots())
    assert np.array_equal(rig.pool.weights(live), np.asarray([rig.wm.wt[s] for s in live], np.uint32)), where
    every = np.arange(rig.model.C, dtype=np.uint32)
    assert np.array_equal(host(rig.pool.weights(dev_i32(every))), rig.wm.get(every)), where
    st = rig.pool.weight_stats()
    assert (st.total_weight, st.positive) == (rig.wm.total, rig.wm.positive), where


def _same_sample(rig, count, where):
    got = rig.pool.sample_weighted(count, SEED, STEP)
    slot, sym, weight, total, _ = rig.wm.draw_many(SEED, STEP, 0, count)
    assert got[7] == total and np.array_equal(got[4], slot) and np.array_equal(got[5], sym) and np.array_equal(got[6], weight), where
    return slot


@pytest.mark.parametrize("name", ["room", "trimmed"])
def test_weights_from_dedup_and_the_draws_that_follow(logic, runs, name):
    rig = state(logic, runs, name, weighting=1000)
    want, res = rig.check(True)
    live = want.slots
    rig.pool.weights_from_dedup(5)                                               # scale < m for the large groups: weight 1
    want.apply_weights(rig.wm, 5)
    _same_weights(rig, "scale 5")
    assert {rig.wm.wt[s] for s in live} >= {1, 2, 5} and res.largest > 5
    rig.pool.weights_from_dedup(10 ** 6)
    want.apply_weights(rig.wm, 10 ** 6)
    _same_weights(rig, "scale 10^6")
    _same_sample(rig, 3000, "scale 10^6")
    sl, given = wu.pattern_random_third_zero(live, 3)
    big = [s for s in live if want.mult[s] == res.largest]
    given[sl.index(big[0])], given[sl.index(big[1])] = 3, 0
    rig.pool.set_weights(sl, given); assert rig.wm.set_weights(sl, given, True)
    rig.pool.weights_from_dedup(77, divide=True)
    want.apply_weights(rig.wm, 77, du.DIVIDE)
    _same_weights(rig, "divide")
    assert rig.wm.wt[big[0]] == 1 and rig.wm.wt[big[1]] == 0
    _same_sample(rig, 2000, "divide")
    rig.pool.weights_from_dedup(9, representatives=True)
    want.apply_weights(rig.wm, 9, du.REPRESENTATIVES)
    _same_weights(rig, "representatives")
    slot = _same_sample(rig, 2000, "representatives")
    assert rig.pool.weight_stats().total_weight == 9 * res.distinct and all(want.rep[int(s)] == int(s) for s in slot)
    dead = [s for s in range(rig.model.C) if s not in want.rep]
    assert dead and all(rig.wm.wt[s] == 1000 for s in dead)                      # dead slots are not assigned
    rig.pool.close()


def test_the_result_goes_stale_and_every_refusal(logic, runs):
    from alphazeroforhnefatafl_amd._lib import lib
    from alphazeroforhnefatafl_amd.abi import TaflPoolDedupCfg, TaflPoolDedupResult, TaflPoolDedupWeights
    ex, ta, ey, tb = runs
    rig = Rig(logic, 3000, weighting=4)
    L, h = lib(), rig.pool._h
    out = TaflPoolDedupResult()
    assert code(rig.pool.dedup) == INVALID_ARG                                   # live == 0
    assert code(rig.pool.gather_dedup, [0]) == INVALID_ARG and code(rig.pool.weights_from_dedup, 1) == INVALID_ARG
    rig.ingest(ex, ta)
    bad = TaflPoolDedupCfg(flags=0, key_bits=64)
    bad._reserved[3] = 1
    for cfg in (TaflPoolDedupCfg(flags=2, key_bits=64), TaflPoolDedupCfg(flags=0x80000001, key_bits=64), TaflPoolDedupCfg(flags=0, key_bits=65), bad):
        assert L.tafl_pool_dedup(h, C.byref(cfg), C.byref(out)) == UNSUPPORTED
    assert code(rig.pool.gather_dedup, [0]) == INVALID_ARG                       # a refused call leaves no result
    assert L.tafl_pool_dedup(h, C.byref(TaflPoolDedupCfg(flags=1, key_bits=64)), None) == 0        # out may be NULL
    for change in ("ingest", "trim", "clear"):
        rig.check(where=change)
        rig.pool.weights_from_dedup(3)
        if change == "ingest":
            rig.ingest(ey, tb)
        elif change == "trim":
            rig.trim(5)                                                         # (keeps everything: the result is dropped all the same)
        else:
            rig.pool.clear(); rig.model.clear()
        assert code(rig.pool.gather_dedup, [0]) == INVALID_ARG and code(rig.pool.weights_from_dedup, 3) == INVALID_ARG, change
        assert code(rig.pool.gather_dedup, dev_i32([0]), device=True) == INVALID_ARG, change
    rig.ingest(ex, ta)
    rig.check(True, where="after clear")
    wbad = TaflPoolDedupWeights(scale=1, flags=0)
    wbad._reserved[0] = 1
    for cfg in (TaflPoolDedupWeights(scale=1, flags=3), TaflPoolDedupWeights(scale=1, flags=4), wbad):
        assert L.tafl_pool_weights_from_dedup(h, C.byref(cfg)) == UNSUPPORTED
    assert L.tafl_pool_weights_from_dedup(h, None) == INVALID_ARG
    rig.pool.set_weighting(None)
    assert code(rig.pool.weights_from_dedup, 3) == INVALID_ARG                   # weighting off
    rig.pool.gather_dedup([rig.model.live_slots()[0]])                           # the result still stands
    assert rig.pool.stats().bad_slot == 3000 + 2 - rig.model.live               # (the device-route gathers of rig.check since the clear)
    rig.pool.close()


def test_device_bytes_before_during_and_after(logic, runs):
    ex, ta, *_ = runs
    rig = Rig(logic, 4096)
    rig.ingest(ex, ta)
    rig.pool.gather(rig.model.live_slots()[:300])                                # (the staging of the row calls exists before)
    before = rig.pool.stats().device_bytes
    res = rig.pool.dedup()
    assert res.device_bytes == du.device_bytes(4096) == 25 * 4096 + 24 * 8192 + 32 == rig.pool.stats().device_bytes - before
    assert rig.pool.dedup(True).device_bytes == res.device_bytes                 # allocated once
    rig.pool.gather_dedup(rig.model.live_slots()[:300])                          # host pointers: 16 bytes of staging per row
    assert rig.pool.stats().device_bytes - before == res.device_bytes + 16 * 300
    rig.pool.gather_dedup(dev_i32(rig.model.live_slots()[:900]), device=True)
    assert rig.pool.stats().device_bytes - before == res.device_bytes + 16 * 300
    rig.pool.free_dedup()
    assert rig.pool.stats().device_bytes == before
    assert code(rig.pool.gather_dedup, [0]) == INVALID_ARG
    rig.pool.free_dedup()                                                       # twice is fine
    assert rig.pool.dedup().device_bytes == res.device_bytes
    rig.pool.close()


@pytest.mark.parametrize("n, wb, rules", [(13, 256, "copenhagen"), (8, 128, "brandubh")])
def test_images_of_several_words_and_padding_bytes(n, wb, rules):
    """13x13: 169 tiles in 43 words, three padding bytes; 8x8: 64 tiles, no padding, an even side (no centre tile).  16 lanes from the
    start position, 12 moves, results set by hand (a quarter of the lanes drawn: zmean with draws); the ring wraps, so every live row has a
    copy.  (Groups that join different boards under a symmetry are the 7x7 workload's: twelve lanes rarely meet in mirrored positions.)"""
    from tests import board_sizes_util as bs
    rl = abi.rules.COPENHAGEN if rules == "copenhagen" else abi.rules.BRANDUBH
    lg = gpu_logic(rl, n, wb)
    ex, t = record(lg, bs.start_fen(n) if n == 8 else abi.boards.COPENHAGEN13, 16, 12, 16, 8, 11, cap=24, hand_set=True)
    T = qu.coverage(t)["taken"]
    assert T == 12 * 12 and (t.z[t.final != 0] == np.float32(1e-4)).any(), qu.coverage(t)
    rig = Rig(lg, T + T // 2, k=16)
    rig.ingest(ex, t); rig.ingest(ex, t)
    assert rig.model.written > rig.model.C
    raw, sym = du.Dedup(rig.model), du.Dedup(rig.model, True)
    assert raw.largest >= 12 and sym.distinct <= raw.distinct and sum(1 for v in sym.canon.values() if v) > 50      # (most images are folded under another symmetry)
    assert any(v not in (np.float32(1.0), np.float32(-1.0), np.float32(1e-4)) for v in raw.zm.values())      # mixed groups
    for symmetries in (False, True):
        want, res = rig.check(symmetries, where=(n, symmetries))
        assert res.collisions == 0
        rig.check(symmetries, key_bits=6, where=(n, symmetries, 6))
    rig.pool.close()


def test_the_other_calls_of_a_pool_are_what_they_were(logic, runs):
    """tafl_pool_sample, tafl_pool_gather and tafl_pool_sample_weighted of a pool after a de-duplication (and after its buffers were
    freed again) give the bytes of the same calls without it; two de-duplications of one pool leave the same bytes."""
    import torch
    ex, ta, ey, tb = runs
    outs = []
    for dedup in (False, True):
        rig = Rig(logic, 3000, weighting=7)
        rig.ingest(ex, ta); rig.ingest(ey, tb)
        if dedup:
            every = dev_i32(np.arange(3000))
            rig.pool.dedup(True)
            first = [t.cpu() for t in rig.pool.gather_dedup(every, device=True)]
            rig.pool.dedup(False); rig.pool.dedup(True)
            for a, b in zip(first, rig.pool.gather_dedup(every, device=True)):
                assert torch.equal(a, b.cpu())
        slots = rig.model.live_slots()[::3]
        got = [a.tobytes() for a in rig.pool.sample(700, SEED, STEP)] + [a.tobytes() for a in rig.pool.gather(slots, [s % 8 for s in slots])]
        got += [np.asarray(a).tobytes() for a in rig.pool.sample_weighted(700, SEED, STEP)]
        if dedup:
            rig.pool.free_dedup()
            got2 = [a.tobytes() for a in rig.pool.sample(700, SEED, STEP)]
            assert got2 == got[:len(got2)]
        outs.append(got)
        rig.pool.close()
    assert outs[0] == outs[1]
