"""Playout cap randomization in guided self-play (include/taflhip.h tafl_playout_cap) on a real MI355X: the capped
rounds k_gselfplay_capped (plain / episodes, without / with root noise) on the three preset layouts, 72 lanes (a full wave and a partial
one), S = 16, fast_sims = 4, a quarter of the moves full - against the host harness's capped run (tests/hostsim_caps), against the
per-move composition of the library's own uncapped one-move runs on a second batch, at the two extremes, in two shards, the counters,
the refused arguments and the Python front end.  Every comparison is exact except the row sum of a gathered policy.  `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflEpisodeOpts, TaflMatchOpts, TaflPlayoutCap, TaflPlayoutCapStats, TaflSelfplayOpts, TaflState
from oracle import oracle as orc
from tests import episodes_util as epu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import playout_cap_util as pcu
from tests.test_gpu_episodes import glg_of

pytestmark = pytest.mark.gpu

G, S, FAST = pcu.G, pcu.S, pcu.FAST
LAYOUTS = list(pcu.SHAPES)


def on_device(cfg, episodes, cap, noise=None, states=None, salts=None, base=pcu.IDS, S_=S, with_ex=True):
    _rules, n, _wb, _lg, st, sa, _over, _S, budget = pcu.shape(orc, cfg)
    states, salts = st if states is None else states, sa if salts is None else salts
    glg = glg_of(cfg)
    b = glg.new_batch(len(states))
    b.upload(states)
    ex = glg.new_examples(len(states), budget, S_) if with_ex else None
    got = pcu.device_capped(b, ex, n, S_, salts, budget, cap, episodes, base=base, stride=G if episodes else 0, noise=noise)
    assert got.stat_faults == 0
    if ex is not None:
        es = ex.stats()
        assert (es.dropped, es.overflowed) == (0, 0)
        got.lens = list(ex.counts()[0])
        ex.close()
    b.close()
    return got


@functools.lru_cache(maxsize=None)
def capped(cfg, episodes, noisy=False):
    return on_device(cfg, episodes, pcu.cap_of(cfg), nu.noise_cfg() if noisy else None)


@functools.lru_cache(maxsize=None)
def composed(cfg, episodes, noisy=False):
    _rules, n, _wb, _lg, states, salts, over, _S, budget = pcu.shape(orc, cfg)
    route = pcu.device_route(glg_of(cfg), n, salts, FAST, nu.noise_cfg() if noisy else None)
    try:
        return pcu.composition(route, states, over, budget, pcu.CAP_SEED[cfg], pcu.FULL_PER, episodes, base=pcu.IDS, stride=G)
    finally:
        route.close()


@functools.lru_cache(maxsize=None)
def on_host(cfg, episodes):
    rules, n, wb, _lg, states, salts, _over, _S, budget = pcu.shape(orc, cfg)
    ex = pcu.HostExamples(n, G, budget, S)
    got = pcu.host_capped(rules, n, wb, states, S, salts, budget, pcu.cap_of(cfg), ex, episodes=episodes, base=pcu.IDS, stride=G if episodes else 0)
    assert not any(got.faults)
    return got


@pytest.mark.parametrize("episodes", [False, True])
@pytest.mark.parametrize("cfg", LAYOUTS)
def test_the_capped_run_equals_the_harness_and_the_composition(cfg, episodes):
    got = capped(cfg, episodes)
    host = on_host(cfg, episodes)
    pcu.assert_equal(got, host, (cfg, episodes, "host harness"))
    assert got.cap_stats == host.cap_stats and got.terminal_hits == host.terminal_hits
    want = composed(cfg, episodes)
    assert want.full > 0 and want.fast > 0 and (not episodes or cfg != "brandubh7" or 0 in want.closed)      # (on the expectation)
    pcu.assert_equal(got, want, (cfg, episodes, "device composition"))
    assert got.cap_stats == (want.full, want.fast)


@pytest.mark.parametrize("episodes", [False, True])
@pytest.mark.parametrize("cfg", LAYOUTS)
def test_the_noisy_capped_run_equals_the_device_composition(cfg, episodes):
    """The full route runs with root noise, the fast route without (the last bits of gamma are not portable to the host: section 14)."""
    got, want = capped(cfg, episodes, True), composed(cfg, episodes, True)
    assert want.plays != composed(cfg, episodes).plays
    pcu.assert_equal(got, want, (cfg, episodes, "noise"))
    assert got.cap_stats == (want.full, want.fast)


@pytest.mark.parametrize("episodes", [False, True])
@pytest.mark.parametrize("cfg", LAYOUTS)
def test_the_extremes(cfg, episodes):
    """full_per_65536 = 65536: the uncapped run in everything (noise, z, open_from's effect on finalize included).  full_per_65536 = 0
    with noise latched: the uncapped run at n_sims = fast_sims without noise and with ex = NULL, the examples object untouched."""
    ncfg = nu.noise_cfg()
    got, want = on_device(cfg, episodes, pcu.cap_of(cfg, 65536), ncfg), on_device(cfg, episodes, None, ncfg)
    pcu.assert_equal(got, want, (cfg, episodes, "all full"))
    assert got.cap_stats == (sum(got.moves), 0) and got.lens == want.lens and sum(got.lens) == sum(got.moves)
    assert (got.stats.terminal_hits, got.stats.predicts) == (want.stats.terminal_hits, want.stats.predicts)
    got, want = on_device(cfg, episodes, pcu.cap_of(cfg, 0), ncfg), on_device(cfg, episodes, None, None, S_=FAST, with_ex=False)
    pcu.assert_equal(got, want, (cfg, episodes, "all fast"))
    assert got.cap_stats == (0, sum(got.moves)) and got.lens == [0] * G and sum(got.moves) > 0
    assert (got.stats.terminal_hits, got.stats.predicts) == (want.stats.terminal_hits, want.stats.predicts)


@pytest.mark.parametrize("episodes", [False, True])
def test_two_shards_equal_the_whole(episodes):
    cfg = "brandubh7"
    states, salts = pcu.shape(orc, cfg)[4], pcu.shape(orc, cfg)[5]
    whole = capped(cfg, episodes)
    half, total, caps = G // 2, [0, 0, 0, 0], [0, 0]
    for first in (0, half):
        part = on_device(cfg, episodes, pcu.cap_of(cfg), states=(TaflState * half)(*[states[first + g] for g in range(half)]), salts=salts[first:first + half],
                         base=pcu.IDS + first)
        for g in range(half):
            assert part.plays[g] == whole.plays[first + g] and part.states[g] == whole.states[first + g], (first, g)
            assert part.examples[g] == whole.examples[first + g] and part.episodes[g] == whole.episodes[first + g], (first, g)
        total = [a + b for a, b in zip(total, part.counters)]
        caps = [a + b for a, b in zip(caps, part.cap_stats)]
    assert total == list(whole.counters) and tuple(caps) == whole.cap_stats


@pytest.mark.parametrize("episodes", [False, True])
@pytest.mark.parametrize("cfg", LAYOUTS)
def test_the_counters(cfg, episodes):
    """The invariants; the class counts of the expectation (the composition of uncapped harness runs on the CPU, classes by the rule
    restated in Python); both stats getters after tafl_gselfplay_end (device_capped reads them there)."""
    got = capped(cfg, episodes)
    full, fast = got.cap_stats
    assert full + fast == sum(got.moves) and sum(got.lens) == full
    assert got.stats.faults == 0 and got.sims == S * full + FAST * fast
    want = _host_composition(cfg, episodes)
    assert (full, fast) == (want.full, want.fast) and want.full > 0 and want.fast > 0


@functools.lru_cache(maxsize=None)
def _host_composition(cfg, episodes):
    rules, n, wb, _lg, states, salts, over, _S, budget = pcu.shape(orc, cfg)
    return pcu.composition(pcu.host_route(rules, n, wb, salts, FAST), states, over, budget, pcu.CAP_SEED[cfg], pcu.FULL_PER, episodes, base=pcu.IDS, stride=G)


def test_refusals_and_what_a_begin_latches():
    from alphazeroforhnefatafl_amd._lib import TaflError, lib
    cfg = "brandubh7"
    _rules, n, _wb, _lg, states, salts, _over, _S, _budget = pcu.shape(orc, cfg)
    glg = glg_of(cfg)
    count, A = 8, abi.action_size(n)
    sub = (TaflState * count)(*[states[g] for g in range(count)])
    b = glg.new_batch(count)
    b.upload(sub)
    ex = glg.new_examples(count, 6, S)
    L = lib()
    ok = TaflSelfplayOpts(pcu.SSEED, pcu.TEMP, 0, 0)

    def set_cap(fast, full_per, flags=0, reserved=None):
        cap = TaflPlayoutCap(7, fast, full_per, flags)
        if reserved is not None:
            cap._reserved[reserved] = 1
        return L.tafl_gselfplay_set_playout_cap(b._h, C.byref(cap))

    def begin(sims=S, episodes=False):
        if episodes:
            return L.tafl_gselfplay_begin_episodes(b._h, sims, 256, pcu.CPUCT, C.byref(ok), 6, 0, ex._h, C.byref(TaflEpisodeOpts(0, 0, 0)), None)
        return L.tafl_gselfplay_begin(b._h, sims, 256, pcu.CPUCT, C.byref(ok), 6, 0, ex._h)

    def no_run_to_step():
        with pytest.raises(TaflError) as ei:
            b.gselfplay_step()
        assert ei.value.code == -1

    def drive():
        w = b.gselfplay_step()
        while w:
            boards, sides, waiting = b.gmcts_leaves()
            pri, val = gsu.stub_rows(boards, sides, waiting, count, n, A, salts[:count])
            w = b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        b.gselfplay_end()

    # the stats call without a capped run
    st = TaflPlayoutCapStats()
    assert L.tafl_gselfplay_playout_cap_stats(b._h, C.byref(st)) == -1
    assert L.tafl_gselfplay_set_playout_cap(None, None) == -1
    # a setting that stands: fast_sims 8, every move fast; every rejected argument leaves it as it was
    assert set_cap(8, 0) == 0
    assert set_cap(1, 16384) == -1 and set_cap(0, 16384) == -1 and set_cap(65536, 16384) == -1 and set_cap(4, 65537) == -1       # TAFL_ERR_INVALID_ARG
    assert set_cap(4, 16384, flags=1) == -5 and all(set_cap(4, 16384, reserved=i) == -5 for i in range(3))                      # TAFL_ERR_UNSUPPORTED
    no_run_to_step()
    # at begin: fast_sims > n_sims, for both begins; no steppable run is left behind, not even the one that was open
    assert begin(sims=4) == -1 and begin(sims=4, episodes=True) == -1
    no_run_to_step()
    assert begin() == 0
    assert begin(sims=7) == -1
    no_run_to_step()
    assert L.tafl_gselfplay_playout_cap_stats(b._h, C.byref(st)) == -1
    # the setting that stood is the one a run latches: every move fast at 8 simulations
    b.upload(sub); ex.clear()
    assert begin() == 0
    drive()
    cs, gs = b.playout_cap_stats(), b.gmcts_stats()
    assert cs.full_moves == 0 and cs.fast_moves > 0 and gs.sims == 8 * cs.fast_moves and ex.counts()[1] == 0
    # a match is refused while a cap is set, and accepted after clearing
    mo, eo = TaflMatchOpts(0, 0), TaflEpisodeOpts(0, 0, 0)
    b.upload(sub)
    assert L.tafl_gmatch_begin(b._h, S, 256, pcu.CPUCT, C.byref(ok), 6, 0, None, C.byref(eo), None, C.byref(mo)) == -5
    b.clear_playout_cap()
    assert L.tafl_gmatch_begin(b._h, S, 256, pcu.CPUCT, C.byref(ok), 6, 0, None, C.byref(eo), None, C.byref(mo)) == 0
    b.gselfplay_end()
    # an uncapped run: the cap stats call is refused, also after its end
    b.upload(sub); ex.clear()
    assert begin() == 0
    assert L.tafl_gselfplay_playout_cap_stats(b._h, C.byref(st)) == -1
    # a cap set mid-run takes effect only at the next begin: this run stays uncapped and records every move
    assert set_cap(2, 0) == 0
    drive()
    assert L.tafl_gselfplay_playout_cap_stats(b._h, C.byref(st)) == -1
    moves = sum(b.gselfplay_end()[1])
    assert ex.counts()[1] == moves > 0 and b.gmcts_stats().sims == S * moves
    b.upload(sub); ex.clear()
    assert begin() == 0
    b.clear_playout_cap()                                               # and a clear mid-run leaves the latched cap
    drive()
    cs = b.playout_cap_stats()
    assert (cs.full_moves, ex.counts()[1]) == (0, 0) and b.gmcts_stats().sims == 2 * cs.fast_moves > 0
    # the lock-step search ignores the setting
    assert set_cap(2, 0) == 0
    b.upload(sub)
    b.gmcts_begin(S)
    w = b.gmcts_step(None, None, pcu.CPUCT, S)
    while w:
        boards, sides, waiting = b.gmcts_leaves()
        pri, val = gsu.stub_rows(boards, sides, waiting, count, n, A, salts[:count])
        w = b.gmcts_step(gsu.fptr(pri), gsu.fptr(val), pcu.CPUCT, S)
    ongoing = sum(1 for g in range(count) if sub[g].status == abi.ONGOING)
    assert b.gmcts_stats().sims == S * ongoing
    ex.close(); b.close()


def test_python_front_end():
    """play_guided_selfplay with a small torch network on device pointers and a cap from MCTSArgs; then a gather over every recorded
    index: every row belongs to a full move by playout_cap_is_full, its policy sums to 1 to float32 rounding, and final == 1 for the closed
    episodes.  play_match refuses fastSims."""
    import torch
    from alphazeroforhnefatafl_amd import MCTSArgs, play_guided_selfplay, play_match
    from alphazeroforhnefatafl_amd.mcts import playout_cap_is_full
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    cfg = "brandubh7"
    _rules, side, _wb, _lg, states, _salts, _over, _S, budget = pcu.shape(orc, cfg)
    lg = glg_of(cfg)
    A, n, cap_seed = lg.action_size, G, 12345
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

    args = MCTSArgs(numMCTSSims=16, cpuct=1.0, fastSims=4, fullMoveProb=0.25, capSeed=cap_seed)
    b = lg.new_batch(n)
    b.upload(states)
    ex = lg.new_examples(n, budget, 16)
    dn = DeviceNet()
    eps, est, total, lost = play_guided_selfplay(b, ex, dn, args, budget, game_id_base=pcu.IDS, sample_seed=3, temp_moves=2, device=True,
                                                 buffers=(dn.boards.data_ptr(), dn.sides.data_ptr(), dn.waiting.data_ptr()))
    cs, gs = b.playout_cap_stats(), b.gmcts_stats()
    assert lost == (0, 0) and total == cs.full_moves > 0 and cs.fast_moves > cs.full_moves and gs.sims == 16 * cs.full_moves + 4 * cs.fast_moves
    assert sum(eps) == est.attacker_wins + est.defender_wins + est.draws > 0 and est.cut == 0
    lens = list(ex.counts()[0])
    rows = np.array([j * n + g for g in range(n) for j in range(lens[g])], np.uint32)
    assert rows.size == total
    _boards, _sides, pi, z, fin = ex.gather(torch.from_numpy(rows.astype(np.int32)).to(dev), device=True)
    nc, _ov, _pl, mv, _acts, _vis = ex.read(rows)
    nct = torch.from_numpy(nc.astype(np.int64)).to(dev)
    assert bool((nct > 0).all()) and bool(((pi != 0).sum(1) == nct).all())
    assert bool(((pi.double().sum(1) - 1.0).abs() <= nct.double() * 2.0 ** -25).all())
    fin, z = fin.cpu().tolist(), z.cpu().tolist()
    # the episode and the move number of every move of a lane, by replaying its plays on the oracle from its opening (no cap on the
    # episode length here: an episode closes when its game is over)
    plays, moves = b.gselfplay_end()
    wb = pcu.shape(orc, cfg)[2]
    olg = pcu.shape(orc, cfg)[3]
    i = closed_rows = 0
    for g in range(n):
        st, k, m_ep, full_moves = orc.GameState.from_abi(states[g], wb), 0, 0, []
        for m in range(moves[g]):
            if playout_cap_is_full(cap_seed, pcu.IDS + k * n + g, m_ep, 16384):
                full_moves.append((k, m_ep))
            code, st, _eff = olg.do_play(plays[m * n + g], st)
            assert code == 0, (g, m)
            m_ep += 1
            if st.to_abi().status != abi.ONGOING and m + 1 < budget:
                st, k, m_ep = orc.GameState.from_abi(states[g], wb), k + 1, 0
        assert k == eps[g] and len(full_moves) == lens[g], (g, k, eps[g], len(full_moves), lens[g])
        for (ek, M) in full_moves:                                      # every gathered row belongs to a full move, in column order
            assert int(mv[i]) == M, (g, ek, M, int(mv[i]))
            if ek < eps[g]:
                assert fin[i] == 1 and z[i] != 0.0, (g, ek, M)
                closed_rows += 1
            i += 1
    assert i == total and closed_rows > 0 and sum(eps) > 0
    with pytest.raises(ValueError):
        play_match(b, (dn, dn), MCTSArgs(numMCTSSims=16, fastSims=4), budget)
    ex.close(); b.close()
