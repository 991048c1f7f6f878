"""Value targets from search values (include/taflhip.h "value targets") on a real MI355X: k_gselfplay_mark_boundary
behind the rounds of guided self-play families, k_examples_vt_stage, k_examples_vt_chain, the two gathers and the pool's pass, through the
C-ABI, against the Python twins of tests/value_targets_util.py: Brandubh 7 x 7 / u64, 65 lanes, S = 16, a lane budget of 20.  Everything
bit for bit.  `pytest -m gpu`."""
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import _lib
from oracle import oracle as orc
from tests import board_sizes_util as bsu
from tests import noise_util as nu
from tests import search_stats_util as ssu
from tests import solver_util as su
from tests import value_targets_util as vtu

pytestmark = pytest.mark.gpu
G, K = vtu.G, vtu.K
INVALID, UNSUPPORTED = -1, -5


@functools.lru_cache(maxsize=None)
def shape():
    return ssu.shape(orc, "brandubh7", G, vtu.MODULUS)


def logic():
    rules, n, wb = shape()[:3]
    return bsu.gpu_logic(rules, n, wb)


@functools.lru_cache(maxsize=None)
def expectation(mode):
    _rules, n, wb, lg, states, salts, _over = shape()
    return vtu.twin(orc, lg, states, wb, salts, nu.DeviceSide(logic(), n), **vtu.MODES[mode])


def record(mode, value_targets=True, K_=K, max_moves=vtu.BUDGET):
    _rules, n, _wb, _lg, states, salts, _over = shape()
    glg = logic()
    b = glg.new_batch(G)
    b.upload(states)
    ex = glg.new_examples(G, max_moves, K_, search_stats=True, value_targets=value_targets)
    m = vtu.MODES[mode]
    nz = nu.noise_cfg() if m.get("noise") else None
    cp = vtu.TaflPlayoutCap(vtu.CAP_SEED, vtu.FAST, vtu.FULL_PER, 0) if m.get("cap") else None
    su.device_solver(b, ex, n, salts, vtu.BUDGET, vtu.SEED, vtu.TEMP, n_sims=vtu.S, solver=bool(m.get("solver")), k=m.get("k"), cap=cp, episodes=True, base=vtu.BASE, stride=G,
                     episode_moves=m.get("episode_moves", 0), noise=nz)
    return ex, b


@functools.lru_cache(maxsize=None)
def device(mode):
    return record(mode)


def index_of(ex):
    lens, _tot = ex.counts()
    return vtu.index_of([min(x, ex.max_moves) for x in lens], G)


def code_of(call):
    with pytest.raises(_lib.TaflError) as err:
        call()
    return err.value.code


@pytest.mark.parametrize("mode", list(vtu.MODES))
def test_boundaries_and_targets_equal_the_twin(mode):
    (ex, _b), want = device(mode), expectation(mode)
    index = index_of(ex)
    assert len(index) == sum(len(lane) for lane in want.lanes)
    for lam in (0.0, 0.5, 1.0):
        exp = vtu.targets(want, lam)
        r = ex.value_targets(lam)
        assert (r.episodes_closed, r.episodes_unfinished, r.rows_with_target, r.rows_settled) == (exp.closed, exp.unfinished, exp.rows, 0), (mode, lam)
        t, kd, ee = ex.gather_targets(index)
        vtu.assert_targets(index, G, t, kd, ee, want, exp, (mode, lam))
        if lam == 1.0:                                            # closed episodes give z bit for bit
            _bd, _sd, _pi, z, _fin = ex.gather(index)
            assert all(np.float32(t[i]).tobytes() == np.float32(z[i]).tobytes() for i in range(len(index)) if kd[i] == 1) and (kd == 1).any()


def test_settling_staleness_and_both_pointer_routes():
    import torch
    _rules, n, _wb, _lg, _states, _salts, over = shape()
    ex, b = record("cut")
    want = expectation("cut")
    index = index_of(ex)
    assert code_of(lambda: ex.gather_targets(index)) == INVALID                   # no result yet
    exp = vtu.targets(want, 0.5, settle=True)
    before = ex.stats().device_bytes
    r = ex.value_targets(0.5, settle_unfinished=True)
    assert (r.episodes_closed, r.episodes_unfinished, r.rows_with_target, r.rows_settled) == (exp.closed, exp.unfinished, exp.rows, exp.settled) and exp.settled > 0
    _bd, _sd, _pi, z, fin = ex.gather(index)
    for count in (1, 257):
        idx = (index * 2)[:count]
        t, kd, ee = ex.gather_targets(idx)
        vtu.assert_targets(idx, G, t, kd, ee, want, exp, "host pointers", [z[index.index(e)] for e in idx], [fin[index.index(e)] for e in idx])
        dt, dk, de = ex.gather_targets(torch.tensor(idx, dtype=torch.int32, device="cuda:0"), device=True)
        assert dt.cpu().numpy().tobytes() == t.tobytes() and dk.cpu().numpy().tobytes() == kd.tobytes() and de.cpu().numpy().tobytes() == ee.tobytes()
    bad = [G * vtu.BUDGET, 0x7FFFFFFF]
    assert code_of(lambda: ex.gather_targets(bad + index[:1])) == INVALID
    seen = ex.stats().bad_index
    dt, dk, de = ex.gather_targets(torch.tensor(bad + index[:1], dtype=torch.int32, device="cuda:0"), device=True)
    assert ex.stats().bad_index == seen + 2 and not dt[:2].any() and not dk[:2].any() and not de[:2].any()
    for lam in (-0.5, 1.5, float("nan")):
        assert code_of(lambda: ex.value_targets(lam)) == INVALID
    # the pool: the setting, the refusals, vt and kind per slot past a wrap, both routes, dead slots
    glg = logic()
    pool = glg.new_pool(300, K, search_stats=True)
    base = pool.stats().device_bytes
    pool.set_value_targets(True)
    assert pool.stats().device_bytes - base == 5 * 300
    model = vtu.PoolModel(300)
    order = vtu.taken_order(want, exp)
    res = tuple(pool.ingest(ex))
    assert res[0] == len(order) > 300 and res[1] == 0
    model.ingest([(exp.vt[x], exp.kind[x]) for x in order])
    slots = model.live_slots()
    t, kd = pool.gather_targets(slots)
    model.check(slots, t, kd, "pool")
    for count in (1, 257):
        sl = [slots[(7 * i) % len(slots)] for i in range(count)]
        ht, hk = pool.gather_targets(sl)
        model.check(sl, ht, hk, ("pool, host pointers", count))
        dt, dk = pool.gather_targets(torch.tensor(sl, dtype=torch.int32, device="cuda:0"), device=True)
        assert dt.cpu().numpy().tobytes() == ht.tobytes() and dk.cpu().numpy().tobytes() == hk.tobytes(), count
    dt, dk = pool.gather_targets(torch.tensor(slots + [300], dtype=torch.int32, device="cuda:0"), device=True)
    assert dt[:-1].cpu().numpy().tobytes() == t.tobytes() and dk[:-1].cpu().numpy().tobytes() == kd.tobytes() and float(dt[-1]) == 0 and int(dk[-1]) == 0
    assert pool.stats().bad_slot == 1 and code_of(lambda: pool.gather_targets([300])) == INVALID
    # finalize marks the result stale: the readers and the ingest refuse it
    ob = glg.new_batch(G)
    ob.upload(over)
    ex.finalize(ob)
    assert code_of(lambda: ex.gather_targets(index)) == INVALID and code_of(lambda: pool.ingest(ex)) == INVALID
    ex.value_targets(1.0)
    assert tuple(pool.ingest(ex))[0] > 0
    assert ex.stats().device_bytes >= before                                     # (host-pointer gathers add their staging)
    ex.clear()
    assert code_of(lambda: ex.gather_targets([0])) == INVALID


def test_device_bytes_and_refusals():
    glg = logic()
    _rules, n, _wb, _lg, _states, _salts, _over = shape()
    plain, stats, both = glg.new_examples(G, 20, K), glg.new_examples(G, 20, K, search_stats=True), glg.new_examples(G, 20, K, search_stats=True, value_targets=True)
    E = G * 20
    assert both.stats().device_bytes - stats.stats().device_bytes == 6 * E + 32
    assert stats.stats().device_bytes - plain.stats().device_bytes == 8 * K * E + 4 * G
    assert code_of(lambda: glg.new_examples(G, 20, K, value_targets=True)) == UNSUPPORTED
    assert code_of(lambda: stats.value_targets(0.5)) == INVALID and code_of(lambda: stats.gather_targets([0])) == INVALID
    pool = glg.new_pool(64, K)
    assert code_of(lambda: pool.set_value_targets(True)) == INVALID               # needs the statistics
    assert code_of(lambda: pool.gather_targets([0])) == INVALID


def test_a_pool_with_the_setting_samples_what_one_without_it_samples():
    ex, _b = record("episodes")
    ex.value_targets(0.9, settle_unfinished=True)
    glg = logic()
    a, b = glg.new_pool(512, K, search_stats=True), glg.new_pool(512, K, search_stats=True, value_targets=True)
    for p in (a, b):
        p.set_weighting(3)
    assert tuple(a.ingest(ex))[0] == tuple(b.ingest(ex))[0] > 0
    slots = list(range(int(a.stats().live)))
    for p in (a, b):
        p.set_weights(slots[::3], [5 + (x % 11) for x in slots[::3]])
    same = lambda x, y: all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x, y))
    assert same(a.sample(200, 3, 1), b.sample(200, 3, 1))
    assert same(a.sample_weighted(200, 3, 2), b.sample_weighted(200, 3, 2))
    assert same(a.gather_stats(slots), b.gather_stats(slots)) and same(a.gather(slots), b.gather(slots))


# ---- runs driven here: other board sizes, an evaluation symmetry, K = 4, a plain run continued ------------------------------------------
def drive(b, ex, n, salts, n_sims, budget, episodes=True, episode_moves=0, move_base=0, base=vtu.BASE, sym_seed=None):
    """One run of `b` into `ex` with the stub network in host buffers (under sym_seed: eval_symmetry_util's conjugated network, so that
    the run must record what the plain run records)."""
    from alphazeroforhnefatafl_amd import abi
    from tests import eval_symmetry_util as esu
    from tests import gselfplay_util as gsu
    G_, A = b.n, abi.action_size(n)
    b.clear_solver(); b.clear_forced_playouts()
    if sym_seed is not None:
        b.set_eval_symmetry(sym_seed, 123456)
    if episodes:
        b.gselfplay_begin_episodes(ex, budget, n_sims, vtu.CPUCT, vtu.EDGES, game_id_base=base, sample_seed=vtu.SEED, temp_moves=vtu.TEMP, episode_moves=episode_moves, id_stride=G_)
    else:
        b.gselfplay_begin(ex, budget, n_sims, vtu.CPUCT, vtu.EDGES, game_id_base=base, sample_seed=vtu.SEED, temp_moves=vtu.TEMP, move_base=move_base)
    syms_seen = set()
    w = b.gselfplay_step()
    while w:
        boards, sides, waiting = b.gmcts_leaves()
        if sym_seed is not None:
            syms = b.gmcts_leaf_symmetry()
            syms_seen |= {syms[g] for g in range(G_) if waiting[g]}
            pri, val = esu.conjugated_rows(boards, sides, waiting, syms, G_, n, A, salts)
        else:
            pri, val = gsu.stub_rows(boards, sides, waiting, G_, n, A, salts)
        w = b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
    b.gselfplay_end()
    return syms_seen


def check_against(ex, want, G_, where, lams=(0.5,), Kmax=None, max_moves=None, ends=True):
    lens, _tot = ex.counts()
    index = vtu.index_of([min(x, ex.max_moves) for x in lens], G_)
    assert len(index) == sum(min(len(lane), max_moves or len(lane)) for lane in want.lanes), where
    for lam in lams:
        exp = vtu.targets(want, lam, Kmax=Kmax, max_moves=max_moves)
        r = ex.value_targets(lam)
        assert (r.episodes_closed, r.episodes_unfinished, r.rows_with_target, r.rows_settled) == (exp.closed, exp.unfinished, exp.rows, 0), (where, lam)
        t, kd, ee = ex.gather_targets(index)
        vtu.assert_targets(index, G_, t, kd, ee if ends else None, want, exp, (where, lam))
    return index, exp


@pytest.mark.parametrize("name", ("copenhagen13", "side8"))
def test_the_other_board_sizes(name):
    """13 x 13 / u256 and side 8 on u128 (G = 16, S = 12): an episodes run with a budget of six moves cut after two, so every lane reopens."""
    from tests import eval_symmetry_util as esu
    rules, n, wb, lg, states, S_, _salts = esu.workload(orc, name)
    G_ = len(states)
    salts = [(3 * g + 1) % 256 for g in range(G_)]
    glg = bsu.gpu_logic(rules, n, wb)
    want = vtu.twin(orc, lg, states, wb, salts, None, n_sims=S_, n_moves=6, episodes=True, episode_moves=2)
    assert want.cut >= G_ and sum(len(lane) for lane in want.lanes) >= 3 * G_
    b = glg.new_batch(G_)
    b.upload(states)
    ex = glg.new_examples(G_, 6, S_, search_stats=True, value_targets=True)
    drive(b, ex, n, salts, S_, 6, episode_moves=2)
    check_against(ex, want, G_, name, lams=(0.0, 0.5, 1.0))


def test_a_run_under_an_evaluation_symmetry():
    _rules, n, _wb, _lg, states, salts, _over = shape()
    glg = logic()
    b = glg.new_batch(G)
    b.upload(states)
    ex = glg.new_examples(G, vtu.BUDGET, K, search_stats=True, value_targets=True)
    seen = drive(b, ex, n, salts, vtu.S, vtu.BUDGET, episode_moves=5, sym_seed=77)
    assert len(seen) >= 4
    b.clear_eval_symmetry()
    check_against(ex, expectation("cut"), G, "eval symmetry", lams=(0.5, 1.0))


def test_examples_without_a_policy_take_no_part():
    """K = 4 and room for two examples per lane: an overflowed example has vt = 0, kind = 0 and the chain passes over it."""
    _rules, n, _wb, _lg, states, salts, _over = shape()
    glg = logic()
    b = glg.new_batch(G)
    b.upload(states)
    ex = glg.new_examples(G, 2, 4, search_stats=True, value_targets=True)
    drive(b, ex, n, salts, vtu.S, vtu.BUDGET)
    st = ex.stats()
    assert st.overflowed > 0 and st.dropped > 0
    want = expectation("episodes")
    # (a full lane's last example is marked by every later reopen, as the rule says: open_from stands at len; the marks are not compared)
    index, exp = check_against(ex, want, G, "K = 4", Kmax=4, max_moves=2, ends=False)
    assert exp.rows < len(index)
    assert [g for g in range(G) if (g, 1) in exp.kind and exp.kind[(g, 0)] == 0 and exp.kind[(g, 1)] != 0 and not want.lanes[g][0].ep_end]


def test_a_plain_run_continued_with_move_base_is_one_episode():
    from alphazeroforhnefatafl_amd import abi
    _rules, n, wb, lg, states, salts, _over = shape()
    glg = logic()
    b = glg.new_batch(G)
    b.upload(states)
    ex = glg.new_examples(G, 6, K, search_stats=True, value_targets=True)
    want = vtu.twin(orc, lg, states, wb, salts, None, n_moves=3)
    drive(b, ex, n, salts, vtu.S, 3, episodes=False)
    ex.value_targets(0.5)
    nxt = (abi.TaflState * G)(*b.download())
    want = vtu.twin(orc, lg, nxt, wb, salts, None, n_moves=3, move_base=3, into=want)
    drive(b, ex, n, salts, vtu.S, 3, episodes=False, move_base=3)
    assert code_of(lambda: ex.gather_targets([0])) == INVALID                     # the second run marked the result stale
    index, exp = check_against(ex, want, G, "two runs")
    assert exp.closed == 0 and exp.unfinished == sum(1 for lane in want.lanes if lane)
    assert not ex.gather_targets(index)[2].any()
