"""Forced playouts with policy target pruning in guided self-play (include/taflhip.h tafl_forced_playouts) on a
real MI355X: the rounds k_gselfplay_forced (plain / episodes, without / with root noise, without / with a playout cap) on the three preset
layouts in the shapes of tests/noise_util.setup - 72 lanes: a full wave, a partial one and the two crafted games -, S = 24, k = 2, against
the host harness (tests/hostsim_forced) on every lane and against the Python twin of tests/forced_util.py on ten spot lanes; the
counters, shards, latching, refusals and the Python front end.  Every comparison is exact except the row sum of a gathered policy.
`pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflEpisodeOpts, TaflForcedPlayouts, TaflForcedPlayoutsStats, TaflMatchOpts, TaflSelfplayOpts, TaflState
from oracle import oracle as orc
from tests import episodes_util as epu
from tests import forced_util as fu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import playout_cap_util as pcu
from tests.test_gpu_episodes import glg_of

pytestmark = pytest.mark.gpu

G, S, K = fu.G, fu.S, fu.K
RUN_MOVES, RUN_TEMP, RUN_SEED, RUN_IDS = 3, 2, 5, 1000
TINY, BUDGET = 2.0 ** -40, 6
SPOTS = list(fu.SPOTS)


def on_device(cfg, n_moves, seed, temp, k=K, cap=None, episodes=False, base=RUN_IDS, noise=None, states=None, salts=None, max_children=S):
    _rules, n, _wb, _lg, st, sa = nu.setup(orc, cfg)
    states, salts = st if states is None else states, sa if salts is None else salts
    glg = glg_of(cfg)
    b = glg.new_batch(len(states))
    b.upload(states)
    ex = glg.new_examples(len(states), n_moves, max_children)
    got = fu.device_forced(b, ex, n, salts, n_moves, seed, temp, k=k, cap=cap, episodes=episodes, base=base, stride=G if episodes else 0, noise=noise)
    es = ex.stats()
    assert got.stat_faults == 0 and (es.dropped, es.overflowed) == (0, 0)
    ex.close(); b.close()
    return got


def on_host(cfg, n_moves, seed, temp, k=K, cap=None, episodes=False, base=RUN_IDS, noise=None):
    rules, n, wb, _lg, states, salts = nu.setup(orc, cfg)
    ex = fu.HostExamples(n, G, n_moves, S)
    got = fu.host_forced(rules, n, wb, states, salts, n_moves, seed, temp, k=k, cap=cap, ex=ex, episodes=episodes, base=base, stride=G if episodes else 0, noise=noise)
    assert not any(got.faults) and got.stat_faults == 0
    return got


@functools.lru_cache(maxsize=None)
def plain_device(cfg):
    return on_device(cfg, RUN_MOVES, RUN_SEED, RUN_TEMP)


@pytest.mark.parametrize("cfg", fu.LAYOUTS)
def test_the_plain_run_equals_the_harness_and_the_twin(cfg):
    """Item 2: three moves, temp_moves = 2.  Every lane against the harness, counters included; ten spot lanes against the twin run."""
    _rules, _n, wb, lg, states, salts = nu.setup(orc, cfg)
    got = plain_device(cfg)
    fu.assert_same_lanes(got, on_host(cfg, RUN_MOVES, RUN_SEED, RUN_TEMP), cfg)
    want, tally = fu.twin_run(orc, lg, states, wb, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, 0, RUN_IDS, K, games=SPOTS)
    assert tally.forced_sims > 0 and tally.pruned_visits > 0 and tally.pruned_children > 0, cfg
    fu.assert_lanes_equal_run(got, want, RUN_MOVES, cfg, SPOTS)
    assert all(got.fp_stats) and got.fp_stats[3] == sum(got.moves) and got.sims == S * sum(got.moves)


def test_the_counters_equal_the_twins_tallies_on_every_lane():
    cfg = "brandubh7"
    _rules, _n, wb, lg, states, salts = nu.setup(orc, cfg)
    want, tally = fu.twin_run(orc, lg, states, wb, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, 0, RUN_IDS, K)
    got = plain_device(cfg)
    assert tally.draws_moved >= 1
    fu.assert_lanes_equal_run(got, want, RUN_MOVES, cfg)
    assert got.fp_stats == tally.stats() and got.sims == want.sims


@pytest.mark.parametrize("cfg", fu.LAYOUTS)
def test_a_tiny_k_prunes_without_forcing(cfg):
    """Item 3: k = 2^-40, temp_moves = 0: plays, states and simulations of the library's own run without the setting; the examples are
    the harness's and on the spot lanes the twin's."""
    _rules, n, wb, lg, states, salts = nu.setup(orc, cfg)
    got = on_device(cfg, RUN_MOVES, RUN_SEED, 0, k=TINY)
    off = on_device(cfg, RUN_MOVES, RUN_SEED, 0, k=None)
    assert off.fp_stats is None and got.plays == off.plays and got.states == off.states and got.sims == off.sims and got.moves == off.moves
    assert got.examples != off.examples and got.fp_stats[0] == 0 and got.fp_stats[1] > 0 and got.fp_stats[3] == sum(got.moves)
    fu.assert_same_lanes(got, on_host(cfg, RUN_MOVES, RUN_SEED, 0, k=TINY), cfg)
    want, tally = fu.twin_run(orc, lg, states, wb, salts, RUN_MOVES, RUN_SEED, 0, 0, RUN_IDS, TINY, games=SPOTS)
    assert tally.forced_sims == 0 and tally.pruned_visits > 0
    fu.assert_lanes_equal_run(got, want, RUN_MOVES, cfg, SPOTS)


@pytest.mark.parametrize("noisy", [True, False])
@pytest.mark.parametrize("cfg", fu.LAYOUTS)
def test_a_capped_episodes_run_equals_the_harness_and_the_composition(cfg, noisy):
    """Item 4: fast_sims = 6, half of the moves full.  Every lane against the harness; the spot lanes against the composition of forced
    twin moves (fed the device's eta) and uncapped unforced one-move runs."""
    _rules, n, _wb, _lg, _states, _salts = nu.setup(orc, cfg)
    noise = nu.noise_cfg() if noisy else None
    got = on_device(cfg, BUDGET, pcu.SSEED, pcu.TEMP, cap=fu.cap_cfg(32768), episodes=True, base=epu.IDS, noise=noise)
    host = on_host(cfg, BUDGET, pcu.SSEED, pcu.TEMP, cap=fu.cap_cfg(32768), episodes=True, base=epu.IDS, noise=noise)
    fu.assert_same_lanes(got, host, (cfg, noisy))
    assert got.cap_stats[0] == got.fp_stats[3] > 0 and got.cap_stats[1] > 0 and got.fp_stats[0] > 0
    want, tally = fu.capped_composition(orc, cfg, nu.DeviceSide(glg_of(cfg), n), 32768, noisy, lanes=SPOTS, budget=BUDGET)
    assert want.full > 0 and want.fast > 0 and tally.pruned_visits > 0
    pcu.assert_equal(got, want, (cfg, noisy, "composition"), games=SPOTS, predicts=False)


def test_every_move_full_and_every_move_fast():
    cfg = "brandubh7"
    noise = nu.noise_cfg()
    full = on_device(cfg, BUDGET, pcu.SSEED, pcu.TEMP, cap=fu.cap_cfg(65536), episodes=True, base=epu.IDS, noise=noise)
    free = on_device(cfg, BUDGET, pcu.SSEED, pcu.TEMP, episodes=True, base=epu.IDS, noise=noise)
    epu.assert_same(full, free, "every move full")
    assert full.cap_stats == (sum(full.moves), 0) and full.fp_stats == free.fp_stats and full.fp_stats[3] == sum(full.moves)
    fu.assert_same_lanes(full, on_host(cfg, BUDGET, pcu.SSEED, pcu.TEMP, cap=fu.cap_cfg(65536), episodes=True, base=epu.IDS, noise=noise), "every move full")
    fast = on_device(cfg, BUDGET, pcu.SSEED, pcu.TEMP, cap=fu.cap_cfg(0), episodes=True, base=epu.IDS, noise=noise)
    plain = on_device(cfg, BUDGET, pcu.SSEED, pcu.TEMP, k=None, cap=fu.cap_cfg(0), episodes=True, base=epu.IDS, noise=noise)
    epu.assert_same(fast, plain, "every move fast")
    assert fast.fp_stats == (0, 0, 0, 0) and fast.cap_stats == plain.cap_stats == (0, sum(fast.moves)) and sum(fast.moves) > 0


def test_two_shards_equal_the_whole_batch_with_ids_beyond_32_bits():
    cfg, base = "brandubh7", 2 ** 32 + 1000
    _rules, _n, _wb, _lg, states, salts = nu.setup(orc, cfg)
    noise = nu.noise_cfg()
    whole, total = on_device(cfg, RUN_MOVES, RUN_SEED, RUN_TEMP, base=base, noise=noise), [0, 0, 0, 0]
    for first, count in ((0, 35), (35, G - 35)):
        part = on_device(cfg, RUN_MOVES, RUN_SEED, RUN_TEMP, base=base + first, noise=noise, states=(TaflState * count)(*[states[first + g] for g in range(count)]),
                         salts=salts[first:first + count])
        for g in range(count):
            assert part.plays[g] == whole.plays[first + g] and part.states[g] == whole.states[first + g] and part.examples[g] == whole.examples[first + g], (first, g)
        total = [a + b for a, b in zip(total, part.fp_stats)]
    assert tuple(total) == whole.fp_stats
    assert on_device(cfg, RUN_MOVES, RUN_SEED, RUN_TEMP, base=1000, noise=noise).plays != whole.plays


def test_max_children_between_the_pruned_and_the_raw_count_overflows_nothing():
    cfg = "brandubh7"
    found = fu.searches(orc, cfg)
    raw = max(len(found[g][1]) for g in found)
    kept = max(sum(r[2] > 0 for r in found[g][1]) for g in found)
    assert kept < raw
    got = on_device(cfg, 1, RUN_SEED, 0, max_children=kept)              # (asserts that nothing overflowed)
    assert sum(got.moves) == got.fp_stats[3] > 0


def test_refusals_and_what_a_begin_latches():
    from alphazeroforhnefatafl_amd._lib import lib
    cfg = "brandubh7"
    _rules, n, _wb, _lg, states, salts = nu.setup(orc, cfg)
    glg = glg_of(cfg)
    count, A = 8, abi.action_size(n)
    sub = (TaflState * count)(*[states[g] for g in range(count)])
    b = glg.new_batch(count)
    b.upload(sub)
    ex = glg.new_examples(count, 3, S)
    L = lib()
    ok = TaflSelfplayOpts(RUN_SEED, 0, 0, 0)
    st = TaflForcedPlayoutsStats()

    def set_k(k, flags=0, reserved=None):
        f = TaflForcedPlayouts(k, flags)
        if reserved is not None:
            f._reserved[reserved] = 1
        return L.tafl_gselfplay_set_forced_playouts(b._h, C.byref(f))

    def run():
        b.upload(sub); ex.clear()
        b.gselfplay_begin(ex, 3, S, fu.CPUCT, 256, game_id_base=0, sample_seed=RUN_SEED, temp_moves=0)

    def drive():
        w = b.gselfplay_step()
        while w:
            boards, sides, waiting = b.gmcts_leaves()
            pri, val = gsu.stub_rows(boards, sides, waiting, count, n, A, salts[:count])
            w = b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        plays, moves = b.gselfplay_end()
        return [pcu.pu.play_tuple4(p) for p in plays], list(moves), gsu.device_examples(ex, count, n)[0]

    assert L.tafl_gselfplay_forced_playouts_stats(b._h, C.byref(st)) == -1 and L.tafl_gselfplay_set_forced_playouts(None, None) == -1
    assert [set_k(k) for k in (0.0, -1.0, float("nan"), float("inf"), 64.5)] == [-1] * 5                    # TAFL_ERR_INVALID_ARG
    assert set_k(2.0, flags=1) == -5 and all(set_k(2.0, reserved=i) == -5 for i in range(5))                # TAFL_ERR_UNSUPPORTED
    # nothing was set: a run is the run it was, and the stats call refuses, also after its end
    run()
    assert L.tafl_gselfplay_forced_playouts_stats(b._h, C.byref(st)) == -1
    assert set_k(2.0) == 0                                               # set after the begin: the open run is not affected
    off = drive()
    assert L.tafl_gselfplay_forced_playouts_stats(b._h, C.byref(st)) == -1
    run()
    b.clear_forced_playouts()                                           # a clear mid-run leaves the latched setting
    on = drive()
    fs = b.forced_playouts_stats()
    assert on != off and fs.forced_sims > 0 and fs.pruned_visits > 0 and fs.full_moves == sum(on[1])
    run()                                                               # NULL cleared it: this run is the first one again
    assert drive() == off and L.tafl_gselfplay_forced_playouts_stats(b._h, C.byref(st)) == -1
    # a rejected argument leaves the setting as it was
    assert set_k(2.0) == 0 and set_k(0.0) == -1
    run()
    assert drive() == on
    # the lock-step search ignores the setting: the children of the search without it
    def lockstep():
        b.upload(sub)
        return nu.DeviceSide(glg, n).search_on(b, salts[:count])[0]
    with_k = lockstep()
    b.clear_forced_playouts()
    assert lockstep() == with_k
    # a match is refused while the setting stands, and accepted after clearing
    assert set_k(2.0) == 0
    mo, eo = TaflMatchOpts(0, 0), TaflEpisodeOpts(0, 0, 0)
    b.upload(sub)
    assert L.tafl_gmatch_begin(b._h, S, 256, fu.CPUCT, C.byref(ok), 3, 0, None, C.byref(eo), None, C.byref(mo)) == -5
    b.clear_forced_playouts()
    assert L.tafl_gmatch_begin(b._h, S, 256, fu.CPUCT, C.byref(ok), 3, 0, None, C.byref(eo), None, C.byref(mo)) == 0
    b.gselfplay_end()
    ex.close(); b.close()


def test_python_front_end():
    """play_guided_selfplay with a small torch network on device pointers and forcedPlayoutsK from MCTSArgs; one gather over every
    recorded index: each row's entries equal n' / N' and the row sums to 1 within n_children * 2^-25.  play_match refuses the setting."""
    import torch
    from alphazeroforhnefatafl_amd import MCTSArgs, play_guided_selfplay, play_match
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    cfg = "brandubh7"
    _rules, side, _wb, _lg, states, _salts = nu.setup(orc, cfg)
    lg = glg_of(cfg)
    A, n, budget = lg.action_size, G, 8
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(8 * side * side, A + 1)).to(dev).eval()

    class DeviceNet:
        def __init__(self):
            self.boards = torch.empty((n, side, side), dtype=torch.uint8, device=dev)
            self.sides = torch.empty(n, dtype=torch.uint8, device=dev)
            self.waiting = torch.empty(n, dtype=torch.uint8, device=dev)
            self.keep = None

        def predict_batch(self, *_ptrs):
            with torch.no_grad():
                x = torch.stack([self.boards.float() / 35.0, (self.sides.float() / 8.0)[:, None, None].expand(-1, side, side)], 1)
                y = net(x)
                p, v = torch.softmax(y[:, :A], 1).contiguous(), torch.tanh(y[:, A]).contiguous()
            torch.cuda.synchronize()
            self.keep = (p, v)
            return p.data_ptr(), v.data_ptr()

    args = MCTSArgs(numMCTSSims=24, cpuct=1.25, dirichletAlpha=0.3, dirichletEpsilon=0.25, noiseSeed=9, forcedPlayoutsK=2.0)
    b = lg.new_batch(n)
    b.upload(states)
    ex = lg.new_examples(n, budget, 24)
    dn = DeviceNet()
    _eps, _est, total, lost = play_guided_selfplay(b, ex, dn, args, budget, game_id_base=RUN_IDS, sample_seed=3, temp_moves=2, device=True,
                                                   buffers=(dn.boards.data_ptr(), dn.sides.data_ptr(), dn.waiting.data_ptr()))
    fs, gs = b.forced_playouts_stats(), b.gmcts_stats()
    assert lost == (0, 0) and total == fs.full_moves > 0 and fs.forced_sims > 0 and fs.pruned_visits > 0 and gs.sims == 24 * fs.full_moves
    lens = list(ex.counts()[0])
    rows = np.array([j * n + g for g in range(n) for j in range(lens[g])], np.uint32)
    assert rows.size == total
    _boards, _sides, pi, _z, _fin = ex.gather(torch.from_numpy(rows.astype(np.int32)).to(dev), device=True)
    nc, _ov, played, _mv, acts, vis = ex.read(rows)
    pi = pi.cpu().numpy()
    assert int(vis.sum()) + fs.pruned_visits == 23 * total                 # (N' = sum n': what was pruned is gone from the stored visits)
    for i in range(rows.size):
        k = int(nc[i])
        a, v = acts[i, :k].astype(np.int64), vis[i, :k].astype(np.float64)
        assert k > 0 and (v > 0).all() and int(played[i]) in a.tolist(), i
        want = np.zeros(A, np.float32)
        want[a] = (v / v.sum()).astype(np.float32)
        assert (pi[i] == want).all(), i
        assert abs(float(pi[i].astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -25, i
    with pytest.raises(ValueError):
        play_match(b, (dn, dn), MCTSArgs(numMCTSSims=24, forcedPlayoutsK=2.0), budget)
    ex.close(); b.close()
