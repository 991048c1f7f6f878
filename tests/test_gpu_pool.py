"""The training pool on the device (include/taflhip.h tafl_pool_*): k_pool_count / k_pool_scan / k_pool_copy and
k_pool_rows against the Python restatements of tests/pool_util.py, computed from Examples.read / Examples.gather of the same examples
object.  Every comparison is exact.  The examples come from cheap rollout-mode runs (Brandubh, tafl_selfplay_record at S = 8, ply cap 64,
max_children 6 so that roots overflow) over games some random plies into the game, so that lanes end inside the run, stay open, or hold
nothing."""
import ctypes as C

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd._lib import TaflError
from tests import pool_util as qu

pytestmark = pytest.mark.gpu

N, K, SIMS, CAP = 7, 6, 8, 64
# (n_games, max_moves, moves played, modulus of the random plies before the run).  The ingest kernels work on tiles of 256 entries of the
# per-example arrays (4 waves), and k_pool_scan walks the tiles' counts 256 at a time with a carry:
#   small   216 entries: one partial tile (the run plays on after the buffer is full, so that most games end)
#   medium  13 200 entries: no power-of-two divisor, 52 tiles, tails in the wave, the tile and the scan's chunk
#   wide    66 000 entries: 258 tiles, the scan takes a second chunk of 256 tile counts (its only width limit: 65 536 entries per chunk)
SHAPES = {"small": (72, 3, 80, 90), "medium": (1100, 12, 12, 30), "wide": (5500, 12, 12, 30)}


@pytest.fixture(scope="module")
def logic():
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    lg = BatchedGameLogic(abi.rules.BRANDUBH, N, device=0)
    yield lg
    lg.close()


_CACHE = {}


def recorded(logic, shape, seed=8):
    """(Examples, its Table) of a recorded and finalized run of the shape; made once and left unchanged."""
    key = (shape, seed)
    if key not in _CACHE:
        G, max_moves, n_moves, mod = SHAPES[shape]
        b = logic.new_batch(G, abi.boards.BRANDUBH)
        b.random_advance(3, (C.c_uint32 * G)(*[(i * 5) % mod for i in range(G)]), 0)
        ex = logic.new_examples(G, max_moves, K)
        b.selfplay_record(ex, n_moves, SIMS, 1.0, seed, CAP, sample_seed=seed + 3, temp_moves=4, want_plays=False)
        ex.finalize(b)
        b.close()
        _CACHE[key] = (ex, qu.device_table(ex))
    return _CACHE[key]


def _stats(pool):
    st = pool.stats()
    return {k: getattr(st, k) for k in qu.STAT_NAMES}


def _check(pool, model, ex=None, where=""):
    """The device pool against the model: the counters; every live row through Pool.read and Pool.gather under mixed symmetries, against
    the numpy restatement and (ex: the object of the last ingest, if every live row is from it) against Examples.gather of the source."""
    st = _stats(pool)
    for k, v in model.stats().items():
        assert st[k] == v, (where, k, st[k], v)
    slots = model.live_slots()
    assert len(set(slots)) == len(slots) == model.live
    if not slots:
        return
    sym = np.asarray([(3 * i + s) % 8 for i, s in enumerate(slots)], np.uint8)
    got = pool.gather(slots, sym)
    qu.check_rows(model, slots, sym, pool.read(slots), got, where)
    if ex is not None:
        boards, sides, pi, z, fin = ex.gather(model.source(slots), sym)
        assert fin.all() and (z != 0).all()
        for name, a, b in zip(("boards", "sides", "pi", "z"), got, (boards, sides, pi, z)):
            assert a.tobytes() == b.tobytes(), (where, name)


@pytest.mark.parametrize("shape", ["small", "medium", "wide"])
def test_ingest_equals_the_serial_loop(logic, shape):
    """Coverage floors first (at least 50 taken, 5 open, 5 overflowed examples, 5 short lanes, one empty lane), then C above, equal to
    and below T, with rows wider than the examples once.  `wide` crosses the one width limit of the scan: k_pool_scan takes 256 tile
    counts (65 536 entries) per chunk and carries the sum into the next."""
    ex, t = recorded(logic, shape)
    cov = qu.assert_floors(t, shape)
    T = cov["taken"]
    assert t.G * t.max_moves > (65536 if shape == "wide" else 0)
    for Cp, Kp in ((T + 37, K + 3), (T, K), (max(1, T - 41), K)) if shape != "wide" else ((1500, K),):
        pool, model = logic.new_pool(Cp, Kp), qu.PoolModel(Cp, Kp, N)
        assert pool.ingest(ex) == model.ingest(t) == (T, cov["open"], cov["overflow"])
        _check(pool, model, ex, (shape, Cp))
        pool.close()


def test_two_ingests_wrap_the_ring_and_trim(logic):
    ex, ta = recorded(logic, "medium")
    ey, tb = recorded(logic, "small")
    Ta, Tb = qu.coverage(ta)["taken"], qu.coverage(tb)["taken"]
    Cp = Ta + Tb // 2
    pool, model = logic.new_pool(Cp, K + 1), qu.PoolModel(Cp, K + 1, N)
    assert pool.ingest(ex) == model.ingest(ta)
    assert pool.ingest(ey) == model.ingest(tb)
    _check(pool, model, None, "wrapped")
    assert model.written > Cp and sorted(model.live_slots()) == list(range(Cp)) and model.oldest_generation() == 1
    empty = logic.new_examples(5, 2, K)
    assert pool.ingest(empty) == model.ingest(qu.device_table(empty)) == (0, 0, 0)        # T = 0 is a generation
    assert pool.ingest(ey) == model.ingest(tb)
    _check(pool, model, None, "four generations")
    pool.trim(2); model.trim(2)
    _check(pool, model, ey, "keep 2")
    assert model.live == Tb and model.oldest_generation() == 4
    pool.trim(7); model.trim(7)
    _check(pool, model, ey, "keep 7")
    pool.clear(); model.clear()
    _check(pool, model, None, "cleared")
    assert _stats(pool)["bad_slot"] == 0
    empty.close(); pool.close()


def test_the_same_ingests_give_byte_identical_pools(logic):
    """No atomics hand out ranks: two fresh pools after the same two ingests hold the same bytes in every slot, and a device-pointer
    gather of all slots (dead ones included) returns the same tensors."""
    import torch
    ex, ta = recorded(logic, "medium")
    ey, _ = recorded(logic, "small")
    Cp = qu.coverage(ta)["taken"] - 100
    dev = torch.device("cuda", 0)
    slots = torch.arange(Cp + 1, dtype=torch.int32, device=dev)
    sym = (slots % 8).to(torch.uint8)
    outs = []
    for _ in range(2):
        pool = logic.new_pool(Cp, K)
        pool.ingest(ey); pool.ingest(ex)
        outs.append([t.cpu() for t in pool.gather(slots, sym, device=True)] + [pool.read(np.arange(Cp))])
        assert pool.stats().bad_slot == 1
        pool.close()
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0][4], outs[1][4]):
        assert np.array_equal(a, b)


def test_sample_is_the_stated_draw_and_the_gather_of_it(logic):
    """out_slot / out_sym equal the Python draw; the rows equal Pool.gather(out_slot, out_sym); device and host pointers give the same
    bytes; two ranks with row_base 0 and count reproduce one call of 2 * count.  count 257 is no multiple of anything in the launch,
    count 1 is one workgroup."""
    import torch
    ex, ta = recorded(logic, "medium")
    ey, tb = recorded(logic, "small")
    Cp = qu.coverage(ta)["taken"] - 57
    pool, model = logic.new_pool(Cp, K), qu.PoolModel(Cp, K, N)
    pool.ingest(ex); model.ingest(ta)
    pool.ingest(ey); model.ingest(tb)                              # (the ring has wrapped)
    seed, step = 0xFEDCBA9876543210, 12
    for count in (257, 1):
        for symmetries in (True, False):
            host = pool.sample(2 * count, seed, step, symmetries=symmetries)
            slot, sym, a = qu.draw_many(seed, step, 0, 2 * count, model.written, model.live, Cp, symmetries)
            assert np.array_equal(host[4], slot) and np.array_equal(host[5], sym) and a.max() < model.live
            for g, w in zip(host[:4], pool.gather(slot, sym)):
                assert g.tobytes() == w.tobytes()
            for g, w in zip(host[:4], model.expect_gather(slot, sym)):
                assert g.tobytes() == w.tobytes()
            ranks = [pool.sample(count, seed, step, row_base=k * count, symmetries=symmetries, device=True) for k in range(2)]
            for i in range(6):
                both = torch.cat([ranks[0][i], ranks[1][i]]).cpu().numpy()
                assert both.tobytes() == np.asarray(host[i]).astype(both.dtype).tobytes(), (count, symmetries, i)
    assert set(np.unique(pool.sample(257, seed, step)[5])) == set(range(8))
    pool.trim(1); model.trim(1)                                    # the draw follows the trimmed window
    assert model.live == qu.coverage(tb)["taken"] < Cp
    got = pool.sample(257, seed, step + 1)
    slot, sym, _ = qu.draw_many(seed, step + 1, 0, 257, model.written, model.live, Cp)
    assert np.array_equal(got[4], slot) and np.array_equal(got[5], sym) and set(int(s) for s in slot) <= set(model.live_slots())
    pool.close()


def test_errors(logic):
    import torch
    from alphazeroforhnefatafl_amd._lib import lib
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    INVALID_ARG, UNSUPPORTED = -1, -5
    ex, ta = recorded(logic, "small")
    T = qu.coverage(ta)["taken"]
    pool = logic.new_pool(T + 10, K)

    def code(fn, *a, **kw):
        with pytest.raises(TaflError) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(pool.sample, 4, 1, 2) == INVALID_ARG                                   # live == 0
    other = BatchedGameLogic(abi.rules.BRANDUBH, N, device=0)
    foreign = other.new_examples(8, 2, K)
    assert code(pool.ingest, foreign) == INVALID_ARG                                   # another context
    wide = logic.new_examples(8, 2, K + 1)
    assert code(pool.ingest, wide) == INVALID_ARG                                      # ex.max_children > Kp
    foreign.close(); other.close(); wide.close()
    assert _stats(pool)["ingests"] == 0
    pool.ingest(ex)
    out = [C.c_void_p()] * 6
    assert lib().tafl_pool_sample(pool._h, 1, 2, 0, 4, 2, *out, 0) == UNSUPPORTED      # unknown flags
    assert lib().tafl_pool_sample(pool._h, 1, 2, 0xFFFFFFFF, 4, 1, *out, 0) == INVALID_ARG
    assert code(pool.trim, 0) == INVALID_ARG
    for dead in (T, T + 9, T + 10, 0xFFFFFFFF):
        assert code(pool.gather, [0, dead]) == INVALID_ARG and code(pool.read, [dead]) == INVALID_ARG
    assert code(pool.gather, [0], [8]) == INVALID_ARG
    assert _stats(pool)["bad_slot"] == 0
    dev = torch.device("cuda", 0)
    slots = torch.tensor([T - 1, T, 0, -1], dtype=torch.int32, device=dev)            # (-1: slot 0xFFFFFFFF)
    sym = torch.tensor([9, 1, 2, 3], dtype=torch.uint8, device=dev)                    # (sym is taken modulo 8)
    got = [t.cpu().numpy() for t in pool.gather(slots, sym, device=True)]
    assert _stats(pool)["bad_slot"] == 2
    want = pool.gather([T - 1, 0], [1, 2])
    for g, w in zip(got, want):
        assert g[[0, 2]].tobytes() == w.tobytes() and not g[[1, 3]].any()
    pool.close()


def test_ingest_leaves_the_examples_as_they_were(logic):
    ex, t = recorded(logic, "medium")
    es = np.asarray(t.valid(), np.uint32)

    def snapshot():
        st = ex.stats()
        return ([a.tobytes() for a in ex.read(es)] + [a.tobytes() for a in ex.gather(es)] + [bytes(ex.counts()[0])],
                (st.dropped, st.overflowed, st.bad_index, st.device_bytes))

    before = snapshot()
    pool = logic.new_pool(300, K)
    pool.ingest(ex); pool.ingest(ex)
    assert snapshot() == before
    assert _stats(pool)["written"] == 2 * qu.coverage(t)["taken"]
    pool.close()


def test_guided_episodes_run_with_cut_episodes(logic):
    """A short play_guided_selfplay run with the stub net and episodes cut at 7 moves, from positions up to 85 random plies into the game: the cut episodes' examples (final = 0) and the
    lanes' open last episodes are skipped, every taken row has z != 0."""
    from alphazeroforhnefatafl_amd.mcts import MCTSArgs
    from alphazeroforhnefatafl_amd.selfplay import play_guided_selfplay
    from tests.guided_util import stub_batch
    G, A, LANE, CUT = 48, abi.action_size(N), 28, 7

    class Net:
        def predict_batch(self, boards, sides, waiting):
            self.keep = stub_batch(boards, sides, waiting, G, N, A, [g % 5 for g in range(G)])
            return self.keep

    b = logic.new_batch(G, abi.boards.BRANDUBH)
    b.random_advance(3, (C.c_uint32 * G)(*[(i * 5) % 90 for i in range(G)]), 0)
    ex = logic.new_examples(G, LANE, 64)
    episodes, stats, total, lost = play_guided_selfplay(b, ex, Net(), MCTSArgs(numMCTSSims=8, cpuct=1.0), LANE, episode_moves=CUT, sample_seed=3, temp_moves=2)
    assert stats.cut > 0 and lost == (0, 0)
    t = qu.device_table(ex)
    cov = qu.coverage(t)
    assert cov["open"] >= CUT * stats.cut and cov["taken"] > 0 and cov["overflow"] == 0
    pool, model = logic.new_pool(cov["taken"] + 3, 64), qu.PoolModel(cov["taken"] + 3, 64, N)
    assert pool.ingest(ex) == model.ingest(t) == (cov["taken"], cov["open"], 0)
    _check(pool, model, ex, "guided")
    z = pool.gather(model.live_slots())[3]
    assert (z != 0).all() and _stats(pool)["skipped_open"] == cov["open"]
    pool.close(); ex.close(); b.close()
