"""Match play (include/taflhip.h tafl_gmatch_*) on a real MI355X: the partition kernels k_gmatch_rank / k_gmatch_place,
the plane kernel k_gmatch_leaves, the round k_gmatch_round and the tally k_gmatch_tally on the three preset layouts, against the oracle
match loop on ten spot lanes and against the reference route (the existing tafl_gselfplay_begin_episodes loop on a second batch, row g of
its full-size priors answered by owner(g)'s evaluator) on all lanes; the structure of the two dense batches round by round; shards; the
device-pointer route through play_match; the refused arguments; no leak into a later run.  Every comparison is exact.  `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflEpisodeOpts, TaflMatchIo, TaflMatchOpts, TaflMatchStats, TaflSelfplayOpts, TaflState
from oracle import oracle as orc
from tests import episodes_util as epu
from tests import gselfplay_util as gsu
from tests import match_util as mu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

G, S, BUDGET = mu.G0, mu.S0, mu.BUDGET
_GLG = {}


def glg_of(cfg):
    if cfg not in _GLG:
        from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
        rules, fen, wb = pu.CONFIGS[cfg]
        _GLG[cfg] = BatchedGameLogic(rules, abi.fen_side_len(fen), wb)
    return _GLG[cfg]


def base_setup():
    return epu.setup(orc, "brandubh7", G, mu.MODULUS)


def on_device(cfg, states, route, budget, S_, **kw):
    """A route of match_util on a fresh batch and examples object of its own."""
    glg = glg_of(cfg)
    b = glg.new_batch(len(states))
    b.upload(states)
    ex = glg.new_examples(len(states), budget, S_)
    try:
        return route(b, ex, glg.side_len, S_, mu.CPUCT, budget=budget, sample_seed=mu.SSEED, temp_moves=mu.TEMP, **kw)
    finally:
        ex.close(); b.close()


def match_run(cfg, states, evaluate, budget, S_, **kw):
    return on_device(cfg, states, lambda b, ex, n, s, c, **k: mu.device_match(b, ex, n, s, c, evaluate, **k), budget, S_, **kw)


def reference_run(cfg, states, evaluate_full, budget, S_, **kw):
    return on_device(cfg, states, lambda b, ex, n, s, c, **k: mu.reference_route(b, ex, n, s, c, evaluate_full, **k), budget, S_, **kw)


@functools.lru_cache(maxsize=None)
def base_match(swap):
    _rules, n, _wb, _lg, states, _salts, _over = base_setup()
    return match_run("brandubh7", states, mu.stub_evaluate(n, mu.SALT), BUDGET, S, base=mu.IDS, stride=G, swap=swap)


@functools.lru_cache(maxsize=None)
def base_reference(swap):
    _rules, n, _wb, _lg, states, _salts, _over = base_setup()
    return reference_run("brandubh7", states, mu.stub_evaluate_full(n, mu.SALT), BUDGET, S, base=mu.IDS, stride=G, swap=swap)


@pytest.mark.parametrize("swap", [0, 1])
def test_the_base_setting_equals_the_reference_route(swap):
    want, _stats, _rounds, _lonely = base_reference(swap)
    wgames = mu.games_from_lanes(want, mu.IDS, swap)
    print("swap", swap, "reference route: games", wgames, "episodes", want.episodes, "sims", want.sims, "predicts", want.predicts)
    assert all(wgames[a][r] >= 2 for a in range(2) for r in range(2)) and sum(e >= 2 for e in want.episodes) >= 2      # (on the reference route)
    got, games, stats, _r = base_match(swap)
    mu.assert_equivalent(got, want, ("reference route", swap))
    assert games == wgames and stats.faults == 0
    assert [games[0][r] + games[1][r] for r in range(4)] == list(got.counters)


@pytest.mark.parametrize("swap", [0, 1])
def test_ten_spot_lanes_against_the_oracle_match_loop(swap):
    _rules, _n, wb, lg, states, _salts, _over = base_setup()
    ref = base_reference(swap)[0]
    closing = sorted(range(G), key=lambda g: -ref.episodes[g])[:6]
    spots = (closing + [g for g in (0, 1, 22, 23, 11, 12, 5, 6, 7, 9) if g not in closing])[:10]
    want, _games = mu.oracle_match(orc, lg, wb, states, states, S, mu.CPUCT, mu.SALT, BUDGET, mu.SSEED, mu.TEMP, mu.IDS, G, 0, swap, only=spots)
    assert sum(want.episodes[g] >= 1 for g in spots) >= 4
    epu.assert_same(base_match(swap)[0], want, ("oracle", swap), games=spots)


@pytest.mark.parametrize("cfg", ["copenhagen11", "copenhagen13"])
def test_other_presets_equal_the_reference_route(cfg):
    """70 lanes of the openings rule and two lanes that are over at the start, S = 8, budget 12."""
    _rules, n, _wb, _lg, st70, _salts, over = epu.setup(orc, cfg, 70, 500)
    states = (TaflState * 72)(*([st70[g] for g in range(70)] + [over, over]))
    kw = dict(base=mu.IDS, stride=72, swap=1)
    want, _stats, rounds, _lonely = reference_run(cfg, states, mu.stub_evaluate_full(n, mu.SALT), 12, 8, **kw)
    wgames = mu.games_from_lanes(want, mu.IDS, 1)
    print(cfg, "reference route: games", wgames, "rounds", rounds, "sims", want.sims)
    assert sum(states[g].status != abi.ONGOING for g in range(72)) >= 2 and want.sims > 0
    got, games, stats, _r = match_run(cfg, states, mu.stub_evaluate(n, mu.SALT), 12, 8, **kw)
    mu.assert_equivalent(got, want, cfg)
    assert games == wgames and stats.faults == 0


def device_states(cfg, count, modulus=60, seed=21):
    """The openings rule on the device: lane g = the start position advanced by (7 g) mod `modulus` random plies."""
    rules, fen, _wb = pu.CONFIGS[cfg]
    b = glg_of(cfg).new_batch(count, fen)
    b.random_advance(seed, (C.c_uint32 * count)(*[(7 * g) % modulus for g in range(count)]), 0)
    st = b.download()
    b.close()
    return st


@pytest.mark.parametrize("count", [773, 65, 1])
def test_partition_structure(count):
    """773 lanes: more than two workgroups of the partition kernels and a partial last wave; 65: a full wave and one lane; 1.  Two vectorised
    evaluators that differ.  Each round the two dense batches are checked against tafl_gmcts_leaves and the owner rule."""
    cfg, S_, budget = "brandubh7", 8, 12
    glg = glg_of(cfg)
    n, nn = glg.side_len, glg.side_len ** 2
    states = device_states(cfg, count)
    evaluate, evaluate_full = mu.vector_evaluators(n)
    kw = dict(base=mu.IDS, stride=count, swap=0)
    want, _stats, _rounds, lonely = reference_run(cfg, states, evaluate_full, budget, S_, **kw)
    print(count, "lanes: rounds with one evaluator idle on the reference route:", lonely, "episodes closed", sum(want.episodes))
    if count == 1:
        assert lonely > 0
    b = glg.new_batch(count)
    b.upload(states)
    ex = glg.new_examples(count, budget, S_)
    seen = {"lonely": 0}

    def each_round(counts, boards, sides, waiting, lanes):
        full_b, full_s, full_w = b.gmcts_leaves()
        full_b = np.frombuffer(full_b, np.uint8).reshape(count, nn)
        st, (eps, _es) = b.download(), b.gselfplay_episode_stats()
        assert counts[0] + counts[1] == b.gmcts_stats().waiting == sum(full_w)
        seen["lonely"] += (counts[0] == 0) != (counts[1] == 0)
        for e in range(2):
            mine = [g for g in range(count) if full_w[g] and mu.owner(mu.IDS, g, eps[g], 0, st[g].side_to_play) == e]
            assert lanes[e][:counts[e]].tolist() == mine, e
            assert waiting[e].tolist() == [1] * counts[e] + [0] * (count - counts[e]), e
            assert np.array_equal(boards[e][:counts[e]].reshape(counts[e], nn), full_b[mine]), e
            assert sides[e][:counts[e]].tolist() == [full_s[g] for g in mine], e

    got, games, stats, _r = mu.device_match(b, ex, n, S_, mu.CPUCT, evaluate, budget, mu.SSEED, mu.TEMP, each_round=each_round, **kw)
    ex.close(); b.close()
    assert seen["lonely"] == lonely
    mu.assert_equivalent(got, want, count)
    assert games == mu.games_from_lanes(want, mu.IDS, 0) and stats.faults == 0


def test_two_shards_equal_the_whole():
    _rules, n, _wb, _lg, states, _salts, _over = base_setup()
    whole, games, _stats, _r = base_match(0)
    half, total = G // 2, [[0] * 4, [0] * 4]
    for first in (0, half):
        sub = (TaflState * half)(*[states[first + g] for g in range(half)])
        part, pg, _s, _r2 = match_run("brandubh7", sub, mu.stub_evaluate(n, mu.SALT), BUDGET, S, base=mu.IDS + first, stride=G, swap=0)
        for g in range(half):
            assert part.plays[g] == whole.plays[first + g] and part.states[g] == whole.states[first + g], (first, g)
            assert part.examples[g] == whole.examples[first + g] and part.episodes[g] == whole.episodes[first + g], (first, g)
        total = [[a + c for a, c in zip(total[e], pg[e])] for e in range(2)]
    assert total == games


def test_device_pointer_route_through_play_match():
    """play_match with two torch modules whose inputs and outputs stay on the device, row_multiple = 64, == the same modules through host
    buffers (the same row counts, so the same shapes)."""
    import torch
    from alphazeroforhnefatafl_amd import MCTSArgs, play_match
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    cfg, count, budget, S_ = "brandubh7", 72, 20, 16
    states = epu.setup(orc, cfg, count, 60)[4]
    lg = glg_of(cfg)
    A, side = lg.action_size, lg.side_len
    mods = [torch.nn.Sequential(torch.nn.Conv2d(2, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(8 * side * side, A + 1)).to(dev).eval()
            for _ in range(2)]
    calls = {"device": [], "host": []}

    class Net:
        def __init__(self, e, route):
            self.e, self.route, self.keep = e, route, None

        def forward(self, boards_t, sides_t):
            calls[self.route].append((self.e, int(boards_t.shape[0])))
            with torch.no_grad():
                x = torch.stack([boards_t.float() / 35.0, (sides_t.float() / 8.0)[:, None, None].expand(-1, side, side)], 1)
                y = mods[self.e](x)
                return torch.softmax(y[:, :A], 1).contiguous(), torch.tanh(y[:, A]).contiguous()

    class DeviceNet(Net):
        def predict_batch(self, boards_t, sides_t, _waiting_t):
            p, v = self.forward(boards_t, sides_t)
            torch.cuda.synchronize()
            self.keep = (p, v)
            return p.data_ptr(), v.data_ptr()

    class HostNet(Net):
        def predict_batch(self, boards_, sides_, _waiting):
            p, v = self.forward(torch.from_numpy(boards_.copy()).to(dev), torch.from_numpy(sides_.copy()).to(dev))
            self.keep = (p.cpu().numpy(), v.cpu().numpy())
            return self.keep

    args = MCTSArgs(numMCTSSims=S_, cpuct=1.0)
    b1, b2 = lg.new_batch(count), lg.new_batch(count)
    b1.upload(states); b2.upload(states)
    ex1, ex2 = lg.new_examples(count, budget, S_), lg.new_examples(count, budget, S_)
    bufs = [(torch.zeros((count, side, side), dtype=torch.uint8, device=dev), torch.zeros(count, dtype=torch.uint8, device=dev),
             torch.zeros(count, dtype=torch.uint8, device=dev), torch.zeros(count, dtype=torch.int32, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    kw = dict(examples=None, episode_moves=7, swap=1, temp_moves=2, sample_seed=3, game_id_base=mu.IDS, row_multiple=64)
    kw1, kw2 = dict(kw, examples=ex1), dict(kw, examples=ex2)
    r1 = play_match(b1, [DeviceNet(0, "device"), DeviceNet(1, "device")], args, budget, device=True, buffers=bufs, **kw1)
    r2 = play_match(b2, [HostNet(0, "host"), HostNet(1, "host")], args, budget, **kw2)
    print(r1)
    assert calls["device"] == calls["host"] and {m for _e, m in calls["device"]} <= {64, 72}
    assert r1.games == r2.games and r1.games_played > 0 and r1.cut > 0
    assert r1.games_played == sum(r1.wins_as_attacker) + sum(r1.wins_as_defender) + r1.draws + r1.cut
    assert bytes(b1.download()) == bytes(b2.download())
    assert epu.device_examples(ex1, count, side)[0] == epu.device_examples(ex2, count, side)[0]
    eps, es = b1.gselfplay_episode_stats()
    assert [r1.games[0][r] + r1.games[1][r] for r in range(4)] == [es.attacker_wins, es.defender_wins, es.draws, es.cut] and sum(eps) == r1.games_played
    for x in (ex1, ex2, b1, b2):
        x.close()


def test_refused_arguments_and_what_closes_a_run():
    from alphazeroforhnefatafl_amd._lib import TaflError, lib
    _rules, n, _wb, _lg, states, _salts, _over = base_setup()
    glg = glg_of("brandubh7")
    count, A, nn = 8, abi.action_size(n), n * n
    first = (TaflState * count)(*[states[g] for g in range(count)])
    b = glg.new_batch(count)
    b.upload(first)
    L = lib()
    ok, eo = TaflSelfplayOpts(mu.SSEED, 0, 0, 0), TaflEpisodeOpts(0, 0, 0)

    def begin(mo, opts=ok, episode=eo):
        return L.tafl_gmatch_begin(b._h, S, 256, mu.CPUCT, C.byref(opts), 4, 0, None, C.byref(episode) if episode is not None else None, None, C.byref(mo) if mo is not None else None)

    assert begin(TaflMatchOpts(2, 0)) == -1                                                      # swap = 2: TAFL_ERR_INVALID_ARG
    assert begin(TaflMatchOpts(0, 1)) == -5                                                      # flags: TAFL_ERR_UNSUPPORTED
    bad = TaflMatchOpts(0, 0)
    bad._reserved[5] = 1
    assert begin(bad) == -5
    assert begin(None) == -1 and begin(TaflMatchOpts(0, 0), episode=None) == -1
    assert begin(TaflMatchOpts(0, 0), opts=TaflSelfplayOpts(mu.SSEED, 0, 3, 0)) == -1           # what the episodes begin rejects
    assert begin(TaflMatchOpts(0, 0), episode=TaflEpisodeOpts(0, 0, 1)) == -5
    b.set_root_noise(0.3, 0.25, 7)
    assert begin(TaflMatchOpts(0, 0)) == -5                                                      # noise set
    b.clear_root_noise()
    # match calls on a batch without a run, and on a plain episodes run
    io, cnt, st = TaflMatchIo(), (C.c_uint32 * 2)(), TaflMatchStats()
    none2 = (C.c_void_p * 2)()

    def match_calls_fail():
        assert L.tafl_gmatch_leaves(b._h, C.byref(io), 0, cnt) == -1
        assert L.tafl_gmatch_step(b._h, none2, none2, 0) == -1
        assert L.tafl_gmatch_get_stats(b._h, C.byref(st)) == -1
    match_calls_fail()
    b.gselfplay_begin_episodes(None, 4, S, mu.CPUCT, sample_seed=mu.SSEED)
    match_calls_fail()
    assert b.gselfplay_step() == count                                                           # the plain run is alive
    b.gselfplay_end()

    evaluate = mu.stub_evaluate(n, mu.SALT)

    def open_match():
        b.upload(first)
        b.gmatch_begin(None, 4, S, mu.CPUCT, sample_seed=mu.SSEED)
        counts, boards, sides, _waiting, _lanes = b.gmatch_leaves()
        assert sum(counts) == count
        ev = [evaluate(e, counts[e], boards[e], sides[e]) for e in range(2)]
        return [gsu.fptr(p) for p, _v in ev], [gsu.fptr(v) for _p, v in ev], ev

    def fails(call, code=-1):
        with pytest.raises(TaflError) as ei:
            call()
        assert ei.value.code == code

    pri, val, _keep = open_match()
    b.gmatch_step(pri, val)
    fails(lambda: b.gmatch_step(pri, val))                                                       # a step without leaves
    # cap too small: TAFL_ERR_CAPACITY, the counts come back, nothing is written
    counts, _b, _s, _w, _l = b.gmatch_leaves()
    e = 0 if counts[0] else 1
    small = np.full((2, count * nn), 0xEE, np.uint8)
    flags = np.full((2, count), 0xEE, np.uint8)
    rows = np.full((2, count), 0xEEEEEEEE, np.uint32)
    io2 = TaflMatchIo()
    for k in range(2):
        io2.boards[k], io2.sides[k], io2.waiting[k], io2.lanes[k], io2.cap[k] = small[k].ctypes.data, flags[k].ctypes.data, flags[k].ctypes.data, rows[k].ctypes.data, count
    io2.cap[e] = counts[e] - 1
    assert L.tafl_gmatch_leaves(b._h, C.byref(io2), 0, cnt) == -7 and (cnt[0], cnt[1]) == counts
    assert bool((small == 0xEE).all()) and bool((flags == 0xEE).all()) and bool((rows == 0xEEEEEEEE).all())
    assert L.tafl_gmatch_step(b._h, none2, none2, 0) == -1                                       # that call does not count as leaves
    b.gmatch_leaves()
    with pytest.raises(TaflError):
        b.gselfplay_step(pri[0], val[0])                                                         # tafl_gselfplay_step on a match run
    # what closes an episodes run closes a match run
    pri, val, _keep = open_match()
    b.upload(first)                                                                              # a write to the batch states
    fails(lambda: b.gmatch_step(pri, val))
    fails(lambda: b.gmatch_leaves())
    pri, val, _keep = open_match()
    b.gmcts_begin(8)
    fails(lambda: b.gmatch_step(pri, val))
    pri, val, _keep = open_match()
    b.gselfplay_end()
    fails(lambda: b.gmatch_step(pri, val))
    b.gmatch_stats(); b.gselfplay_episode_stats()                                                # still readable after the end
    b.upload(first)
    b.gselfplay_begin_episodes(None, 2, S, mu.CPUCT)                                             # an episodes run follows: no match stats
    fails(lambda: b.gmatch_stats())
    b.close()


def test_no_leak_into_a_later_episodes_run():
    """An episodes run after a match run on the same batch and examples object (cleared) leaves what it leaves on fresh ones."""
    rules, n, _wb, _lg, states, salts, _over = base_setup()
    glg = glg_of("brandubh7")
    budget = 20

    def episodes_on(b, ex):
        b.upload(states)
        got, over, stats = epu.device_episodes(b, ex, n, S, mu.CPUCT, salts, budget, mu.SSEED, mu.TEMP, base=mu.IDS, stride=G)
        assert stats.faults == 0 and not any(any(o) for o in over)
        return got

    fresh_b, fresh_ex = glg.new_batch(G), glg.new_examples(G, budget, S)
    want = episodes_on(fresh_b, fresh_ex)
    assert sum(want.episodes) >= 3
    b, ex = glg.new_batch(G), glg.new_examples(G, budget, S)
    b.upload(states)
    _got, games, _stats, _r = mu.device_match(b, ex, n, S, mu.CPUCT, mu.stub_evaluate(n, mu.SALT), budget, mu.SSEED, mu.TEMP, base=mu.IDS, stride=G, swap=1)
    assert sum(map(sum, games)) >= 3
    ex.clear()
    epu.assert_same(episodes_on(b, ex), want, "episodes after a match")
    for x in (fresh_ex, fresh_b, ex, b):
        x.close()
