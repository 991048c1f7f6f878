"""Training rows at every board size (DESIGN.md sections 12 and 19), CPU only: the workloads and the oracle-replay expectation of
tests/training_rows_util.py are proven here, on the host harness (tests/hostsim recording run, tests/hostsim_pool), so that
tests/test_gpu_training_rows.py judges only the kernels.  Per layout (9x9, 7x7 on the 128-bit word, 11x11, 13x13 preset and run-time
rules, 15x15): the expectation equals the harness's examples, it meets the coverage floors by itself, and the harness's pool (rows of
100+ words, Kp = 64, pools of 1 and 5 slots) equals pool_util.PoolModel.  The position with more than 256 legal plays meets its two
asserted counts through the oracle and through the harness.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from oracle import oracle as orc
from tests import pool_util as qu
from tests import training_rows_util as tu


@functools.lru_cache(maxsize=None)
def recorded(name, k):
    """(Recording, expected Table) of the layout through the harness; made once and left unchanged."""
    rec = tu.host_recorded(tu.wide_workload() if name == "wide" else tu.workload(name), k)
    return rec, tu.expected_table(rec)


def _check(pool, model, where):
    """The harness's pool against the model: the counters, every live row through read and gather under mixed symmetries."""
    st = pool.stats()
    for k, v in model.stats().items():
        assert st[k] == v, (where, k, st[k], v)
    slots = model.live_slots()
    assert len(set(slots)) == len(slots) == model.live
    sym = [(3 * i + 1) % 8 for i in range(len(slots))]
    rc, got_read = pool.read(slots)
    got_gather, bad = pool.gather(slots, sym)
    assert rc == 0 and bad == 0
    qu.check_rows(model, slots, sym, got_read, got_gather, where)
    return slots, sym, got_gather


@pytest.mark.parametrize("name", tu.NAMES)
def test_expectation_equals_the_harness_and_meets_the_floors(name):
    """The oracle replay of the returned plays gives the boards, sides, z and final the harness recorded (and ends in the states the run
    ended in: asserted inside expected_table).  The floors hold on the expectation alone: at least 50 taken and 5 open examples, 5 short
    lanes and one empty lane in the K = 64 object, and at least 5 overflowed examples in the K = 8 object of the same run."""
    rec, t = recorded(name, tu.K)
    small, ts = recorded(name, tu.K_SMALL)
    tu.assert_same_table(t, qu.host_table(rec.ex), name)
    tu.assert_same_table(ts, qu.host_table(small.ex), (name, "small"))
    assert bytes(rec.plays) == bytes(small.plays) and rec.ex.counts()[1]["overflowed"] == 0
    cov, covs = tu.summary(t), tu.summary(ts)
    print(name, "K=64", cov, "K=8", covs)
    for k, floor in qu.FLOORS.items():
        assert (covs if k == "overflow" else cov)[k] >= floor, (name, k, cov, covs)
    assert cov["overflow"] == 0 and covs["taken"] >= 1 and cov["widest"] > tu.K_SMALL
    es = np.asarray(t.valid(), np.int64)
    assert set(t.z[es].tolist()) == {0.0, 1.0, -1.0, float(np.float32(1e-4))} and set(t.side[es].tolist()) == {abi.ATTACKER, abi.DEFENDER}
    assert all(t.lens[g] == 0 for g in tu.OVER_AT_START) and all(t.lens[g] > 0 for g in tu.SPOT_LANES)


@pytest.mark.parametrize("name", tu.NAMES)
def test_host_pool_equals_the_model(name):
    """Ingest, read, gather and sample of the harness's pool with Kp = 64 (rows of 76 .. 128 words) against PoolModel fed with the
    expectation: a pool with room, pools of 1 and 5 slots (one ingest of T > C examples keeps the newest C), a second ingest that wraps
    them, and the K = 8 object whose overflowed examples are skipped."""
    rec, t = recorded(name, tu.K)
    small, ts = recorded(name, tu.K_SMALL)
    cov = qu.coverage(t)
    T, n = cov["taken"], t.n
    for Cp in (T + 9, 1, 5):
        pool, model = qu.HostPool(Cp, tu.K, n), qu.PoolModel(Cp, tu.K, n)
        assert pool.ingest(rec.ex) == model.ingest(t) == (T, cov["open"], cov["overflow"])
        slots, sym, got = _check(pool, model, (name, Cp))
        assert model.live == min(T, Cp) and model.source(slots).tolist() == sorted(model.source(slots).tolist())
        (boards, sides, pi, z, _fin), bad = rec.ex.gather(model.source(slots), sym)         # the rows of the source examples
        for nm, a, b in zip(("boards", "sides", "pi", "z"), got, (boards, sides, pi, z)):
            assert bad == 0 and a.tobytes() == b.tobytes(), (name, Cp, nm)
        assert pool.ingest(small.ex) == model.ingest(ts) == (qu.coverage(ts)["taken"], qu.coverage(ts)["open"], qu.coverage(ts)["overflow"])
        _check(pool, model, (name, Cp, "second"))
        assert model.written > Cp
        rc, rows, slot, sy = pool.sample(300, 9, 4, row_base=1000)
        want_slot, want_sym, _ = qu.draw_many(9, 4, 1000, 300, model.written, model.live, Cp)
        assert rc == 0 and np.array_equal(slot, want_slot) and np.array_equal(sy, want_sym)
        for a, b in zip(rows, model.expect_gather(slot, sy)):
            assert a.tobytes() == b.tobytes(), (name, Cp, "sample")


def test_the_wide_position_meets_its_counts():
    """More than 256 legal plays (the oracle's move generation), and with TAFL_MCTS_FLAG_FPU_INF and S = legal count + 8 more than 256
    visited root children: through the oracle's search on two lanes and through the harness on all of them.  The harness's examples
    equal the expectation, and its pool (rows of more than 300 words) equals the model under all eight symmetries."""
    count, w = tu.wide_legal_count(), tu.wide_workload()
    assert count > 256 and w.sims == count + 8 and tu.WIDE_K >= count
    kids, cnt, _ = orc.batch_mcts(w.logic(), w.start(), 2, w.wb, w.params(), 0, 512)
    assert list(cnt) == [count, count]
    rec, t = recorded("wide", tu.WIDE_K)
    tu.assert_same_table(t, qu.host_table(rec.ex), "wide")
    assert t.lens.tolist() == [1] * w.G and (t.nc[:tu.WIDE_CRAFTED] == count).all() and int(t.nc.max()) > 256 and not t.overflow.any()
    for g in range(2):
        assert [(kids[g * 512 + j].action, kids[g * 512 + j].visits) for j in range(count)] == list(zip(t.actions[g, :count].tolist(), t.visits[g, :count].tolist()))
    cov = tu.summary(t)
    print("wide", cov)
    assert cov["taken"] >= 48 and cov["open"] >= 5
    pool, model = qu.HostPool(cov["taken"] + 3, tu.WIDE_K, w.n), qu.PoolModel(cov["taken"] + 3, tu.WIDE_K, w.n)
    assert pool.ingest(rec.ex) == model.ingest(t) == (cov["taken"], cov["open"], 0)
    assert pool.raw().shape[1] > 300
    slots = model.live_slots()
    rc, got_read = pool.read(slots)
    for k in range(8):
        got, bad = pool.gather(slots, [k] * len(slots))
        assert rc == 0 and bad == 0
        qu.check_rows(model, slots, [k] * len(slots), got_read, got, ("wide", k))
