"""Training rows at every board size on the device (DESIGN.md sections 12 and 19): k_examples_gather, k_pool_count / k_pool_scan /
k_pool_copy and k_pool_rows on 9x9, 7x7 on the 128-bit word, 11x11, 13x13 (preset and run-time rules) and 15x15, against the
oracle-replay expectation of tests/training_rows_util.py, which uses neither kernel (tests/test_hostsim_training_rows.py proves the
workloads and that expectation on the CPU).  Rows of 76 .. 132 words (Kp = 64 and 67: several 32-word chunks, the chunk boundary inside
the board words at 13x13 and 15x15) and of 36 .. 72 words (Kp = 8: the last, partial chunk holds words that are never zero), pools below a wave / a tile / two tiles, samples and gathers above the 8 192-row grid cap, the
unaligned-pi instantiations of both row kernels, and roots with more than 256 children.  Every comparison is byte-exact."""
import ctypes as C

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from tests import pool_util as qu
from tests import training_rows_util as tu

pytestmark = pytest.mark.gpu

_LOGICS, _CACHE = {}, {}
ROWS = 4096
KP = (64, 67, tu.K_SMALL)
OUT_NAMES = ("boards", "sides", "pi", "z", "final")


def gpu_logic(name):
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    if name not in _LOGICS:
        rules, _, wb, n, _ = tu.LAYOUTS[name]
        _LOGICS[name] = BatchedGameLogic(rules, n, wb)
    return _LOGICS[name]


def recorded(name, k):
    """(Recording, expected Table) of the layout ("wide": the position with more than 256 legal plays) on the device; made once and left
    unchanged."""
    if (name, k) not in _CACHE:
        w = tu.wide_workload() if name == "wide" else tu.workload(name)
        rec = tu.device_recorded(gpu_logic(w.name), w, k)
        _CACHE[(name, k)] = (rec, tu.expected_table(rec))
    return _CACHE[(name, k)]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _same(got, want, where):
    for name, g, w in zip(OUT_NAMES, got, want):
        g, w = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (g, w))
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (where, name)


def _rows(t, count=ROWS, seed=4):
    """(index, sym) of `count` rows: all eight symmetries of every example of the lanes 0, 63, 64 and G - 1, then examples and
    symmetries drawn with a fixed seed."""
    es = np.asarray(t.valid(), np.uint32)
    spot = np.asarray([e for e in es if int(e) % t.G in tu.SPOT_LANES], np.uint32)
    assert spot.size >= len(tu.SPOT_LANES) and 8 * spot.size < count
    rng = np.random.default_rng(seed)
    more = count - 8 * spot.size
    return (np.concatenate([np.repeat(spot, 8), es[rng.integers(0, es.size, more)]]).astype(np.uint32),
            np.concatenate([np.tile(np.arange(8, dtype=np.uint8), spot.size), rng.integers(0, 8, more).astype(np.uint8)]))


def _check_gather(rec, t, idx, sym, where):
    """Examples.gather with host pointers == with device pointers == the expectation, in boards, sides, pi, z and final."""
    want = tu.expect_example_rows(t, idx, sym)
    _same(rec.ex.gather(idx, sym), want, (where, "host"))
    _same(rec.ex.gather(_dev(idx), _dev(sym), device=True), want, (where, "device"))
    k = min(512, idx.size)
    _same(rec.ex.gather(idx[:k]), rec.ex.gather(idx[:k], np.zeros(k, np.uint8)), (where, "sym = None"))
    _same(rec.ex.gather(_dev(idx[:k]), None, device=True), tu.expect_example_rows(t, idx[:k], np.zeros(k, np.uint8)), (where, "sym = None, device"))
    assert rec.ex.stats().bad_index == 0


def _stats(pool):
    st = pool.stats()
    return {k: getattr(st, k) for k in qu.STAT_NAMES}


def _check_pool(pool, model, rec=None, where="", syms=None):
    """The device pool against the model: the counters; every live row through Pool.read and Pool.gather (host and device pointers)
    under mixed symmetries (syms: under each of these for all rows) against the numpy restatement and (rec: the recording of the last
    ingest, if every live row is from it) against Examples.gather of the source examples."""
    st = _stats(pool)
    for k, v in model.stats().items():
        assert st[k] == v, (where, k, st[k], v)
    slots = model.live_slots()
    assert len(set(slots)) == len(slots) == model.live and slots
    got_read = pool.read(slots)
    for sym in [np.asarray([(3 * i + 1) % 8 for i in range(len(slots))], np.uint8)] if syms is None else [np.full(len(slots), k, np.uint8) for k in syms]:
        got = pool.gather(slots, sym)
        qu.check_rows(model, slots, sym, got_read, got, where)
        _same(pool.gather(_dev(np.asarray(slots, np.uint32)), _dev(sym), device=True), got, (where, "device"))
        if rec is not None:
            boards, sides, pi, z, fin = rec.ex.gather(model.source(slots), sym)
            assert fin.all() and (z != 0).all()
            _same(got, (boards, sides, pi, z), (where, "source"))
    assert _stats(pool)["bad_slot"] == 0


@pytest.mark.parametrize("name", tu.NAMES)
def test_gather_equals_the_oracle_replay(name):
    """4 096 rows of the K = 64 object (all eight symmetries of the examples of lanes 0, 63, 64 and G - 1 among them) and 512 of the
    K = 8 object, whose overflowed examples give all-zero policy rows.  The coverage floors are asserted on the expectation first."""
    rec, t = recorded(name, tu.K)
    small, ts = recorded(name, tu.K_SMALL)
    cov, covs = tu.summary(t), tu.summary(ts)
    print(name, "K=64", cov, "K=8", covs)
    for k, floor in qu.FLOORS.items():
        assert (covs if k == "overflow" else cov)[k] >= floor, (name, k, cov, covs)
    assert list(rec.ex.counts()[0]) == t.lens.tolist() == list(small.ex.counts()[0])
    assert rec.ex.stats().overflowed == 0 and small.ex.stats().overflowed == covs["overflow"] and rec.ex.stats().dropped == 0
    idx, sym = _rows(t)
    assert set(sym[:64].tolist()) == set(range(8))
    _check_gather(rec, t, idx, sym, name)
    idx, sym = _rows(ts, 512)
    assert ts.overflow[idx.astype(np.int64)].any()
    _check_gather(small, ts, idx, sym, (name, "small"))


@pytest.mark.parametrize("Kp", KP)
@pytest.mark.parametrize("name", tu.NAMES)
def test_pool_rows_of_several_chunks(name, Kp):
    """One ingest into a pool with room, rows wider than the examples for Kp = 67: (taken, open, overflow), every live row against the
    model and against Examples.gather of its source; then the K = 8 object, whose overflowed examples are skipped.  Kp = 8 takes the
    K = 8 object alone: rows of 36 .. 72 words whose last, partial chunk holds head words, board words or the first children."""
    rec, t = recorded(name, tu.K)
    small, ts = recorded(name, tu.K_SMALL)
    cov, covs = qu.coverage(t), qu.coverage(ts)
    glg = gpu_logic(name)
    Cp = cov["taken"] + covs["taken"] + 11
    pool, model = glg.new_pool(Cp, Kp), qu.PoolModel(Cp, Kp, t.n)
    if Kp >= tu.K:
        assert (t.n * t.n + 3) // 4 + 5 + Kp >= 76
        assert pool.ingest(rec.ex) == model.ingest(t) == (cov["taken"], cov["open"], 0)
        _check_pool(pool, model, rec, (name, Kp))
    assert pool.ingest(small.ex) == model.ingest(ts) == (covs["taken"], covs["open"], covs["overflow"])
    _check_pool(pool, model, None if Kp >= tu.K else small, (name, Kp, "K = 8"))
    pool.close()


@pytest.mark.parametrize("Cp", [1, 5, 300])
def test_pools_smaller_than_an_ingest(Cp):
    """C below a wave, below a tile and between one and two tiles, one ingest of T > 300 examples: the live slots hold the newest C
    rows; a second ingest wraps them."""
    name = "copenhagen11"
    rec, t = recorded(name, tu.K)
    small, ts = recorded(name, tu.K_SMALL)
    T = qu.coverage(t)["taken"]
    assert T > 300
    pool, model = gpu_logic(name).new_pool(Cp, tu.K), qu.PoolModel(Cp, tu.K, t.n)
    assert pool.ingest(rec.ex)[0] == model.ingest(t)[0] == T
    _check_pool(pool, model, rec, (name, Cp))
    taken = [e for e in t.valid() if t.final[e] and not t.overflow[e]]
    assert model.live == Cp and model.source(model.live_slots()).tolist() == taken[-Cp:]
    assert pool.ingest(small.ex) == model.ingest(ts)
    _check_pool(pool, model, small if qu.coverage(ts)["taken"] >= Cp else None, (name, Cp, "wrapped"))
    assert model.written == T + qu.coverage(ts)["taken"] > Cp
    pool.close()


def test_sample_and_gather_above_the_grid_cap():
    """count = 8 192 + 257: the host route launches two chunks (the second with row_base + 8 192), the device route one grid of 8 192
    workgroups that walks the rest.  out_slot / out_sym equal the Python draw, the rows equal Pool.gather of them and the model, the
    device route equals the host route, two ranks reproduce one call of 2 * count, and a gather of more than 8 192 slots with device
    pointers equals the one with host pointers."""
    import torch
    name = "tablut9"
    rec, t = recorded(name, tu.K)
    T = qu.coverage(t)["taken"]
    Cp = T - 7
    pool, model = gpu_logic(name).new_pool(Cp, tu.K), qu.PoolModel(Cp, tu.K, t.n)
    pool.ingest(rec.ex); model.ingest(t)
    pool.ingest(rec.ex); model.ingest(t)                              # (the ring has wrapped)
    seed, step, count = 0xFEDCBA9876543210, 12, 8192 + 257
    host = pool.sample(count, seed, step)
    slot, sym, a = qu.draw_many(seed, step, 0, 2 * count, model.written, model.live, Cp)
    assert np.array_equal(host[4], slot[:count]) and np.array_equal(host[5], sym[:count]) and a.max() < model.live
    _same(host[:4], pool.gather(slot[:count], sym[:count]), "gather of the draw")
    edge = np.r_[0:8, 8184:8200, count - 8:count]
    _same([x[edge] for x in host[:4]], model.expect_gather(slot[edge], sym[edge]), "model")
    dev = pool.sample(count, seed, step, device=True)
    for i in range(6):
        assert dev[i].cpu().numpy().tobytes() == np.asarray(host[i]).astype(dev[i].cpu().numpy().dtype).tobytes(), ("device route", i)
    both = pool.sample(2 * count, seed, step, device=True)
    ranks = [pool.sample(count, seed, step, row_base=k * count) for k in range(2)]
    assert np.array_equal(np.concatenate([ranks[0][4], ranks[1][4]]), slot) and np.array_equal(np.concatenate([ranks[0][5], ranks[1][5]]), sym)
    for i in range(6):
        one = both[i].cpu().numpy()
        assert np.concatenate([ranks[0][i], ranks[1][i]]).astype(one.dtype).tobytes() == one.tobytes(), ("ranks", i)
    _same(pool.gather(_dev(slot[:count]), _dev(sym[:count]), device=True), host[:4], "device gather")
    assert _stats(pool)["bad_slot"] == 0
    del both, dev
    torch.cuda.empty_cache()
    pool.close()


FILL = 7.0


def _unaligned_pi(glg, k, A, call):
    """`call(pi pointer)` writes k rows of A floats 4 bytes into a tensor that is longer by one float in front and 63 behind: the rows,
    after the floats around them were seen to keep their fill value."""
    import torch
    buf = torch.full((1 + k * A + 63,), FILL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    call(C.c_void_p(buf.data_ptr() + 4))
    glg.sync()
    out = buf.cpu().numpy()
    assert out[0] == FILL and (out[1 + k * A:] == FILL).all()
    return out[1:1 + k * A].reshape(k, A)


@pytest.mark.parametrize("kernel", ["examples_gather", "pool_gather", "pool_sample"])
@pytest.mark.parametrize("name", ["copenhagen11", "brandubh7_u128"])
def test_unaligned_pi_takes_the_scalar_store_loop(name, kernel):
    """The VEC = false instantiations of k_examples_gather and k_pool_rows (gather and draw), through the C-ABI directly: pi 4 bytes off
    a 16-byte boundary, 320 rows under mixed symmetries, byte-equal to the aligned call, nothing written outside the rows."""
    import torch
    from alphazeroforhnefatafl_amd._lib import check, lib
    rec, t = recorded(name, tu.K)
    glg = gpu_logic(name)
    n, A, k, vp = t.n, abi.action_size(t.n), 320, C.c_void_p
    idx, sym = _rows(t, k)
    d_idx, d_sym = _dev(idx), _dev(sym)
    boards, sides = torch.zeros((k, n, n), dtype=torch.uint8, device="cuda"), torch.zeros(k, dtype=torch.uint8, device="cuda")
    z, fin = torch.zeros(k, dtype=torch.float32, device="cuda"), torch.zeros(k, dtype=torch.uint8, device="cuda")
    if kernel == "examples_gather":
        pi = _unaligned_pi(glg, k, A, lambda p: check(lib().tafl_examples_gather(rec.ex._h, vp(d_idx.data_ptr()), vp(d_sym.data_ptr()), k, vp(boards.data_ptr()),
                                                                                    vp(sides.data_ptr()), p, vp(z.data_ptr()), vp(fin.data_ptr()), 1)))
        _same((boards, sides, pi, z, fin), rec.ex.gather(d_idx, d_sym, device=True), (name, kernel))
        return
    T = qu.coverage(t)["taken"]
    pool = glg.new_pool(T, tu.K)
    assert pool.ingest(rec.ex)[0] == T >= 50
    if kernel == "pool_gather":
        d_slots = _dev(np.asarray([(7 * i) % T for i in range(k)], np.uint32))
        pi = _unaligned_pi(glg, k, A, lambda p: check(lib().tafl_pool_gather(pool._h, vp(d_slots.data_ptr()), vp(d_sym.data_ptr()), k, vp(boards.data_ptr()),
                                                                                vp(sides.data_ptr()), p, vp(z.data_ptr()), 1)))
        _same((boards, sides, pi, z), pool.gather(d_slots, d_sym, device=True), (name, kernel))
    else:
        out_slot, out_sym = torch.zeros(k, dtype=torch.int32, device="cuda"), fin
        pi = _unaligned_pi(glg, k, A, lambda p: check(lib().tafl_pool_sample(pool._h, 5, 9, 33, k, abi.POOL_SAMPLE_SYM, vp(boards.data_ptr()), vp(sides.data_ptr()), p,
                                                                                vp(z.data_ptr()), vp(out_slot.data_ptr()), vp(out_sym.data_ptr()), 1)))
        want = pool.sample(k, 5, 9, row_base=33, device=True)
        _same((boards, sides, pi, z), want[:4], (name, kernel))
        assert torch.equal(out_slot, want[4]) and torch.equal(out_sym, want[5]) and set(out_sym.cpu().tolist()) == set(range(8))
    assert _stats(pool)["bad_slot"] == 0
    pool.close()


def _wide():
    """The recording of the position with more than 256 legal plays, after its two counts were asserted: the legal plays (oracle's move
    generation) and the children tafl_examples_read reports, so that the case cannot go quietly vacuous."""
    count = tu.wide_legal_count()
    assert count > 256
    rec, t = recorded("wide", tu.WIDE_K)
    es = np.asarray(t.valid(), np.uint32)
    nc = rec.ex.read(es)[0]
    assert es.size == rec.w.G and (nc[:tu.WIDE_CRAFTED] == count).all() and int(nc.max()) > 256 and rec.ex.stats().overflowed == 0
    cov = tu.summary(t)
    print("wide", cov)
    assert cov["taken"] >= 48 and cov["open"] >= 5 and cov["widest"] > 256
    return rec, t, es, cov


def test_gather_of_roots_with_more_than_256_children():
    """The crafted 15x15 position on 64 lanes + 6 ordinary lanes, one move with TAFL_MCTS_FLAG_FPU_INF and S = legal count + 8: every
    example under all eight symmetries, the second trip of the k += 256 loop of k_examples_gather."""
    rec, t, es, _ = _wide()
    _check_gather(rec, t, np.repeat(es, 8), np.tile(np.arange(8, dtype=np.uint8), es.size), "wide")


def test_pool_rows_of_roots_with_more_than_256_children():
    """The same examples in a pool with Kp = 340: rows of 404 words (12 chunks and a partial one that holds the last children) through
    k_pool_copy, and the second trip of the k += 256 loop of k_pool_rows, under all eight symmetries."""
    rec, t, _, cov = _wide()
    Cp = cov["taken"] + 3
    pool, model = gpu_logic(rec.w.name).new_pool(Cp, tu.WIDE_K), qu.PoolModel(Cp, tu.WIDE_K, t.n)
    assert (t.n * t.n + 3) // 4 + 5 + tu.WIDE_K > 300
    assert pool.ingest(rec.ex) == model.ingest(t) == (cov["taken"], cov["open"], 0)
    _check_pool(pool, model, rec, "wide", syms=range(8))
    pool.close()
