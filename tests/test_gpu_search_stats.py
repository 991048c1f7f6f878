"""Search statistics per training row (include/taflhip.h "search value and policy surprise") on a real MI355X:
k_gselfplay_record_stats behind the rounds of every guided self-play family and k_examples_gather_stats, through the C-ABI, against
the Python twins of tests/search_stats_util.py.  cq, cp and value bit for bit, surprise within 2^-23 |want| + 1e-10.  `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import _lib, abi
from oracle import oracle as orc
from tests import board_sizes_util as bsu
from tests import eval_symmetry_util as esu
from tests import noise_util as nu
from tests import search_stats_util as ssu

pytestmark = pytest.mark.gpu
G, S, K = 65, 24, 64
INVALID, UNSUPPORTED = -1, -5


@functools.lru_cache(maxsize=None)
def shape():
    return ssu.shape(orc, "copenhagen11", G)


def logic():
    rules, n, wb = shape()[:3]
    return bsu.gpu_logic(rules, n, wb)


@functools.lru_cache(maxsize=None)
def device(mode, stats=True):
    _rules, n, _wb, _lg, states, salts, over = shape()
    return ssu.device_run(logic(), n, states, salts, S, K, stats=stats, over=over, **ssu.MODES[mode])


@pytest.mark.parametrize("mode", list(ssu.MODES))
def test_a_run_records_what_the_twin_holds(mode):
    _rules, n, wb, lg, states, salts, over = shape()
    want = ssu.twin_run(orc, lg, states, wb, salts, nu.DeviceSide(logic(), n), S, **ssu.MODES[mode])
    ssu.assert_floors(want, over, mode)
    got = device(mode)
    st = got.ex.stats()
    assert st.dropped == 0 and st.overflowed == 0 and st.bad_index == 0
    ssu.assert_rows(got, want, mode)


@pytest.mark.parametrize("mode", ("plain", "solver"))
def test_the_recorder_changes_nothing_else(mode):
    on, off = device(mode), device(mode, False)
    assert on.plays == off.plays and on.states == off.states and on.moves == off.moves and on.lens == off.lens
    assert [[r.key()[:2] + r.key()[4:] for r in lane] for lane in on.rows] == [[r.key()[:2] + r.key()[4:] for r in lane] for lane in off.rows]
    assert on.z.tobytes() == off.z.tobytes() and on.fin.tobytes() == off.fin.tobytes()


@pytest.mark.parametrize("name", ("brandubh7", "copenhagen13", "side8"))
def test_the_other_board_sizes(name):
    """7 x 7 / u64 (G = 65, S = 32), 13 x 13 / u256 (G = 16) and side 8 on u128 (G = 16): a plain run of three moves."""
    rules, n, wb, lg, states, S_, _salts = esu.workload(orc, name)
    salts = [(3 * g + 1) % 256 for g in range(len(states))]
    glg = bsu.gpu_logic(rules, n, wb)
    want = ssu.twin_run(orc, lg, states, wb, salts, None, S_)
    got = ssu.device_run(glg, n, states, salts, S_, K)
    assert sum(len(lane) for lane in want) >= len(states)
    ssu.assert_rows(got, want, name)


def test_host_and_device_pointer_routes_and_bad_indices():
    import torch
    got = device("plain")
    ex, index = got.ex, got.index
    dev = torch.device("cuda", logic().device)
    for count in (1, 257):
        idx = [index[(7 * i) % len(index)] for i in range(count)]
        hv, hs = ex.gather_stats(idx)
        dv, ds = ex.gather_stats(torch.tensor(idx, dtype=torch.int32, device=dev), device=True)
        assert hv.tobytes() == dv.cpu().numpy().tobytes() and hs.tobytes() == ds.cpu().numpy().tobytes(), count
        for i, e in enumerate(idx):
            assert hv[i].tobytes() == np.float32(got.value[(e % G, e // G)]).tobytes()
    before = ex.stats().bad_index
    bad = [G * 3, -1, index[0], G * 3 + 5]
    dv, ds = ex.gather_stats(torch.tensor(bad, dtype=torch.int32, device=dev), device=True)
    assert ex.stats().bad_index == before + 3
    dv, ds = dv.cpu().numpy(), ds.cpu().numpy()
    assert not dv[[0, 1, 3]].any() and not ds[[0, 1, 3]].any() and dv[2].tobytes() == np.float32(got.value[(index[0] % G, index[0] // G)]).tobytes()
    with pytest.raises(_lib.TaflError):
        ex.gather_stats([G * 3])
    with pytest.raises(_lib.TaflError):
        ex.read_stats([G * 3])


def test_overflowed_examples_hold_no_statistics():
    _rules, n, _wb, _lg, states, salts, over = shape()
    got = ssu.device_run(logic(), n, states, salts, S, 4, over=over, max_moves=2, overflowing=True)
    st = got.ex.stats()
    assert st.overflowed > 0 and st.dropped > 0
    nc, ov, _pl, _mv, _a, _v = got.ex.read(got.index)
    q, p = got.ex.read_stats(got.index)
    for i, e in enumerate(got.index):
        if ov[i]:
            assert not q[i].any() and not p[i].any() and got.value[(e % G, e // G)] == 0 and got.surprise[(e % G, e // G)] == 0
    want = ssu.twin_run(orc, shape()[3], states, shape()[2], salts, None, S)
    for g in range(G):
        for j, r in enumerate(got.rows[g]):
            if len(want[g][j].visits) <= 4:
                assert r.key() == want[g][j].key(), (g, j)


def test_refusals_and_device_bytes():
    glg = logic()
    L = _lib.lib()
    plain, stats = glg.new_examples(G, 3, K), glg.new_examples(G, 3, K, search_stats=True)
    assert stats.stats().device_bytes == plain.stats().device_bytes + 8 * K * G * 3 + 4 * G
    with pytest.raises(_lib.TaflError):
        plain.gather_stats([0])
    with pytest.raises(_lib.TaflError):
        plain.read_stats([0])
    h = C.c_void_p()
    assert L.tafl_examples_create_ex(glg._h, G, 3, K, 2, C.byref(h)) == UNSUPPORTED
    b = glg.new_batch(G, abi.boards.COPENHAGEN)
    with pytest.raises(_lib.TaflError) as ei:
        b.selfplay_record(stats, 2, 8, 1.0, 8, 64, sample_seed=1, temp_moves=0, want_plays=False)
    assert ei.value.code == UNSUPPORTED
    b.selfplay_record(plain, 2, 8, 1.0, 8, 64, sample_seed=1, temp_moves=0, want_plays=False)


def test_a_run_under_an_evaluation_symmetry_records_the_plain_run():
    """SYM: the run latches tafl_eval_symmetry and is fed the conjugated network of tests/eval_symmetry_util.py, so the recorder behind
    the SYM rounds must leave what the plain twin holds - the priors indexed by the original action."""
    _rules, n, wb, lg, states, salts, over = shape()
    want = ssu.twin_run(orc, lg, states, wb, salts, None, S)
    got = ssu.device_run(logic(), n, states, salts, S, K, over=over, sym_seed=esu.SEED)
    assert got.syms == set(range(8))
    ssu.assert_rows(got, want, "sym")


# ---- the pool carries the two scalars ------------------------------------------------------------------------------------------------------
from tests import pool_weights_util as pwu  # noqa: E402

POOL_MOVES, POOL_C = 5, 300


@functools.lru_cache(maxsize=None)
def pool_want(moves=POOL_MOVES):
    _rules, _n, wb, lg, states, salts, _over = shape()
    return ssu.twin_run(orc, lg, states, wb, salts, None, S, n_moves=moves)


@functools.lru_cache(maxsize=None)
def pool_run(moves=POOL_MOVES):
    _rules, n, _wb, _lg, states, salts, over = shape()
    return ssu.device_run(logic(), n, states, salts, S, K, over=over, n_moves=moves)


def filled(weight=7):
    pool, want = logic().new_pool(POOL_C, K, search_stats=True), ssu.PoolExpectation(POOL_C)
    pool.set_weighting(weight); want.model.set_weighting(weight)
    for moves in (POOL_MOVES, 1):                                       # 325 rows (25 ranks dropped), then 65 that wrap
        taken = pool.ingest(pool_run(moves).ex)[0]
        assert taken == want.ingest(pool_want(moves)) == G * moves
    return pool, want


def dev_slots(slots):
    import torch
    return torch.tensor(np.asarray(slots, np.uint32).astype(np.int32), dtype=torch.int32, device=torch.device("cuda", logic().device))


def test_the_pool_holds_the_scalars_of_its_rows():
    """325 examples (one ingest tile plus a part) into 300 slots (ranks dropped), a second ingest of 65 that wraps, a trim; the pool's scalars
    per slot against the expectation and against tafl_examples_gather_stats of the source examples; both pointer routes; dead slots."""
    pool, want = filled()
    assert pool.stats().live == POOL_C
    slots = want.win.live_slots()
    v, s = pool.gather_stats(slots)
    want.check(slots, v, s, "two ingests")
    run = pool_run()
    ev, es = run.ex.gather_stats(run.index)                             # (ascending index = rank order; the first ingest's rows that are still live)
    order = sorted(run.index)
    src = {(r % POOL_C): run.index.index(e) for r, e in enumerate(order) if r >= 25 + 65}
    for slot, i in src.items():
        k = slots.index(slot)
        assert v[k].tobytes() == ev[i].tobytes() and s[k].tobytes() == es[i].tobytes(), slot
    for count in (1, 257):
        pick = [slots[(7 * i) % len(slots)] for i in range(count)]
        hv, hs = pool.gather_stats(pick)
        dv, ds = pool.gather_stats(dev_slots(pick), device=True)
        assert hv.tobytes() == dv.cpu().numpy().tobytes() and hs.tobytes() == ds.cpu().numpy().tobytes()
    pool.trim(1); want.win.trim(1)
    live = want.win.live_slots()
    v, s = pool.gather_stats(live)
    want.check(live, v, s, "after the trim")
    dead = [x for x in range(POOL_C) if x not in set(live)][:3] + [POOL_C, 2 ** 32 - 1]
    with pytest.raises(_lib.TaflError):
        pool.gather_stats(dead)
    before = pool.stats().bad_slot
    dv, ds = pool.gather_stats(dev_slots(dead + live[:2]), device=True)
    assert pool.stats().bad_slot == before + len(dead)
    dv, ds = dv.cpu().numpy(), ds.cpu().numpy()
    assert not dv[:len(dead)].any() and not ds[:len(dead)].any()
    want.check(live[:2], dv[len(dead):], ds[len(dead):], "beside dead slots")
    pool.close()


def test_weights_from_surprise_and_the_weighted_draw():
    pool, want = filled()
    pool.trim(2); want.win.trim(2)
    live = want.win.live_slots()
    read = np.zeros(POOL_C, np.float32)
    read[live] = pool.gather_stats(live)[1]
    want.check(live, pool.gather_stats(live)[0], read[live], "read back")
    every = dev_slots(list(range(POOL_C)))
    for base, per_nat, gen in ((3, 1000.0, 2), (11, 12345.678, 0), (5, 0.0, 1), (2 ** 32 - 16, 1e300, 2), (0, float("inf"), 0)):
        pool.weights_from_surprise(base, per_nat, gen)
        want.weights_from_surprise(read, base, per_nat, gen)
        got = pool.weights(every).cpu().numpy().view(np.uint32)
        assert got.tobytes() == want.model.get(range(POOL_C)).tobytes(), (base, per_nat, gen)
    assert max(want.model.wt) == pwu.MAXW
    pool.weights_from_surprise(9, 4000.0)
    want.weights_from_surprise(read, 9, 4000.0)
    out = pool.sample_weighted(500, 3, 9)
    ms, my, mw, mt, _ks = want.model.draw_many(3, 9, 0, 500)
    assert out[7] == mt and out[4].tobytes() == ms.tobytes() and out[5].tobytes() == my.tobytes() and out[6].tobytes() == mw.tobytes()
    pool.trim(1); want.win.trim(1)
    pool.weights_from_surprise(1, 1.0)
    want.weights_from_surprise(read, 1, 1.0)
    assert pool.weights(every).cpu().numpy().view(np.uint32).tobytes() == want.model.get(range(POOL_C)).tobytes()
    pool.close()


def test_what_the_pool_refuses_and_its_bytes():
    glg = logic()
    pool = glg.new_pool(POOL_C, K)
    base_bytes = pool.stats().device_bytes
    plain = glg.new_examples(G, 3, K)
    for call in (lambda: pool.weights_from_surprise(1, 1.0), lambda: pool.gather_stats([0])):
        with pytest.raises(_lib.TaflError) as ei:
            call()
        assert ei.value.code == INVALID
    pool.set_search_stats(True)
    assert pool.stats().device_bytes == base_bytes + 8 * POOL_C
    with pytest.raises(_lib.TaflError) as ei:
        pool.ingest(plain)
    assert ei.value.code == INVALID and pool.stats().ingests == 0
    with pytest.raises(_lib.TaflError):
        pool.weights_from_surprise(1, 1.0)                               # weighting off
    pool.set_weighting(1)
    pool.weights_from_surprise(1, 1.0)
    L = _lib.lib()
    for per_nat in (-0.5, float("nan")):
        with pytest.raises(_lib.TaflError) as ei:
            pool.weights_from_surprise(1, per_nat)
        assert ei.value.code == INVALID
    cfg = abi.TaflPoolSurpriseWeights(base=1, per_nat=1.0, flags=1)
    assert L.tafl_pool_weights_from_surprise(pool._h, C.byref(cfg)) == UNSUPPORTED
    for i in range(3):
        cfg = abi.TaflPoolSurpriseWeights(base=1, per_nat=1.0)
        cfg._reserved[i] = 1
        assert L.tafl_pool_weights_from_surprise(pool._h, C.byref(cfg)) == UNSUPPORTED
    pool.ingest(pool_run().ex)
    with pytest.raises(_lib.TaflError) as ei:
        pool.set_search_stats(False)
    assert ei.value.code == INVALID
    pool.clear()
    assert pool.stats().device_bytes >= base_bytes + 8 * POOL_C          # clear keeps the setting
    pool.gather_stats([])
    pool.set_search_stats(False)
    pool.set_weighting(None)
    off = glg.new_pool(POOL_C, K)
    assert off.ingest(pool_run().ex)[0] == G * POOL_MOVES               # a pool with the setting off ignores the arrays
    off.close(); pool.close()
