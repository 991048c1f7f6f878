"""Guided self-play in episodes (include/taflhip.h tafl_gselfplay_begin_episodes) on a real MI355X: the episodes
kernels k_gselfplay_episodes (without and with noise) and k_gselfplay_reopen on the three preset layouts, 70 + 2 lanes (a full wave and a partial one),
against the concatenation of plain runs (tests/episodes_util.reference) made by the library's own tafl_gselfplay_begin on a second batch,
ten spot lanes against the oracle loop, shards, the device-pointer route with a torch network and a gather across episodes, the refused
arguments and the Python front end.  Every comparison is exact except the row sum of a gathered policy.  `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflEpisodeOpts, TaflSelfplayOpts, TaflState
from oracle import oracle as orc
from tests import episodes_util as epu
from tests import gselfplay_util as gsu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

G = 72
# per layout: (modulus of the openings rule, S, lane budget) - chosen on the host harness so that games end inside the budget
SHAPES = {"brandubh7": (60, 16, 20), "copenhagen11": (500, 16, 12), "copenhagen13": (500, 16, 20)}
_GLG = {}


def glg_of(cfg):
    if cfg not in _GLG:
        from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
        rules, fen, wb = pu.CONFIGS[cfg]
        _GLG[cfg] = BatchedGameLogic(rules, abi.fen_side_len(fen), wb)
    return _GLG[cfg]


def shape(cfg):
    modulus, S, budget = SHAPES[cfg]
    return epu.setup(orc, cfg, G, modulus) + (S, budget)


def run_on_device(cfg, states, salts, base, stride, episode_moves=0, openings=None, noise=None):
    _rules, n, _wb, _lg, _st, _sa, _over, S, budget = shape(cfg)
    glg = glg_of(cfg)
    b = glg.new_batch(len(states))
    b.upload(states)
    ob = None
    if openings is not None:
        ob = glg.new_batch(len(states))
        ob.upload(openings)
    ex = glg.new_examples(len(states), budget, S)
    got, over, stats = epu.device_episodes(b, ex, n, S, epu.CPUCT, salts, budget, epu.SSEED, epu.TEMP, base=base, stride=stride, episode_moves=episode_moves, openings=ob,
                                            noise=noise)
    if ob is not None:
        ob.close()
    assert stats.faults == 0 and not any(any(o) for o in over)
    es = ex.stats()
    assert (es.dropped, es.overflowed) == (0, 0)
    return got, b, ex


@functools.lru_cache(maxsize=None)
def whole(cfg, episode_moves=0):
    _rules, _n, _wb, _lg, states, salts, _over, _S, _budget = shape(cfg)
    got, b, ex = run_on_device(cfg, states, salts, epu.IDS, G, episode_moves)
    ex.close(); b.close()
    return got


@functools.lru_cache(maxsize=None)
def plain_concatenation(cfg, episode_moves=0):
    _rules, n, _wb, _lg, states, salts, over, S, budget = shape(cfg)
    return epu.reference(epu.device_plain(glg_of(cfg), n, S, epu.CPUCT, salts, epu.SSEED, epu.TEMP), states, states, over, budget, episode_moves, epu.IDS, G)


@pytest.mark.parametrize("cfg", list(SHAPES))
def test_episodes_equal_the_concatenation_of_plain_runs(cfg):
    states = shape(cfg)[4]
    want = plain_concatenation(cfg)
    ongoing = [g for g in range(G) if states[g].status == abi.ONGOING]
    print(cfg, "episodes", want.episodes, "counters", want.counters, "sims", want.sims, "predicts", want.predicts)
    assert sum(want.episodes[g] >= 1 for g in ongoing) >= 2 and len(ongoing) < G and any(want.budget_cut)      # (on the reference route)
    assert any(want.episodes[g] for g in range(64)) or cfg != "brandubh7"
    epu.assert_same(whole(cfg), want, cfg)


@pytest.mark.parametrize("cfg", list(SHAPES))
def test_an_episode_cap(cfg):
    want = plain_concatenation(cfg, 5)
    assert want.counters[3] >= G // 2
    got = whole(cfg, 5)
    epu.assert_same(got, want, (cfg, "episode_moves = 5"))
    g = next(g for g in range(G) if want.capped[g])
    col = got.examples[g]
    assert any(col[j][0][5] == 4 and col[j][1:] == (0.0, 0) and col[j + 1][0][5] == 0 for j in range(len(col) - 1))


@pytest.mark.parametrize("cfg", list(SHAPES))
def test_episodes_with_root_noise(cfg):
    """alpha 0.3, epsilon 0.25 (k_gselfplay_episodes<NL, W, true>): the expectation is the concatenation of the library's noisy plain runs,
    which tests/test_gpu_root_noise.py pins against the twin; the noise is keyed by the episode's game id and move number."""
    from tests import noise_util as nu
    _rules, n, _wb, _lg, states, salts, over, S, budget = shape(cfg)
    ncfg = nu.noise_cfg()
    want = epu.reference(epu.device_plain(glg_of(cfg), n, S, epu.CPUCT, salts, epu.SSEED, epu.TEMP, noise=ncfg), states, states, over, budget, 0, epu.IDS, G)
    print(cfg, "noisy episodes", want.episodes, "counters", want.counters)
    assert want.plays != plain_concatenation(cfg).plays
    if cfg == "brandubh7":
        assert sum(e >= 1 for e in want.episodes) >= 2 and any(e >= 2 for e in want.episodes)      # (on the reference route)
    got, b, ex = run_on_device(cfg, states, salts, epu.IDS, G, noise=ncfg)
    ex.close(); b.close()
    epu.assert_same(got, want, (cfg, "noise"))


@pytest.mark.parametrize("cfg", list(SHAPES))
def test_ten_spot_lanes_against_the_oracle_loop(cfg):
    _rules, _n, wb, lg, states, salts, over, S, budget = shape(cfg)
    want_all = plain_concatenation(cfg)
    closing = [g for g in range(G) if want_all.episodes[g]]
    spots = (closing + [g for g in (0, 1, 63, 64, 65, 70, 71, 30, 31, 32) if g not in closing])[:10]
    want = epu.reference(epu.oracle_plain(orc, lg, wb, S, epu.CPUCT, salts, epu.SSEED, epu.TEMP), states, states, over, budget, 0, epu.IDS, G, only=spots)
    epu.assert_same(whole(cfg), want, (cfg, "oracle"), games=spots)


def test_two_shards_equal_the_whole():
    cfg = "brandubh7"
    states, salts = shape(cfg)[4], shape(cfg)[5]
    got = whole(cfg)
    total = [0, 0, 0, 0]
    for first in (0, G // 2):
        count = G // 2
        part, b, ex = run_on_device(cfg, (TaflState * count)(*[states[first + g] for g in range(count)]), salts[first:first + count], epu.IDS + first, G)
        ex.close(); b.close()
        for g in range(count):
            assert part.plays[g] == got.plays[first + g] and part.states[g] == got.states[first + g], (first, g)
            assert part.examples[g] == got.examples[first + g] and part.episodes[g] == got.episodes[first + g], (first, g)
        total = [a + c for a, c in zip(total, part.counters)]
    assert total == got.counters


def test_openings_from_another_batch_and_finalize():
    """The openings are another batch (the states rotated by five lanes; writing it after the begin changes nothing); then finalize
    leaves the closed episodes as they are and settles the open tails."""
    cfg = "brandubh7"
    _rules, n, _wb, _lg, states, salts, over, S, budget = shape(cfg)
    openings = (TaflState * G)(*[states[(g + 5) % G] for g in range(G)])
    want = epu.reference(epu.device_plain(glg_of(cfg), n, S, epu.CPUCT, salts, epu.SSEED, epu.TEMP), states, openings, over, budget, 0, epu.IDS, G)
    assert [g for g in range(G) if want.episodes[g] and openings[g].status != abi.ONGOING] and [g for g in range(G) if want.episodes[g] and openings[g].status == abi.ONGOING]
    got, b, ex = run_on_device(cfg, states, salts, epu.IDS, G, openings=openings)
    epu.assert_same(got, want, "openings")
    ex.finalize(b)
    after, _ = epu.device_examples(ex, G, n)
    settled = 0
    for g in range(G):
        col = got.examples[g]
        starts = [j for j, (f, _z, _fin) in enumerate(col) if f[5] == 0]
        tail = starts[-1] if len(starts) == got.episodes[g] + 1 else len(col)          # (no cap here: every episode but an open last one is closed)
        assert all(fin == 1 for _f, _z, fin in col[:tail]) and all(fin == 0 for _f, _z, fin in col[tail:]), g
        assert after[g][:tail] == col[:tail], g
        assert after[g][tail:] == [(f,) + epu.outcome(got.states[g], f[1]) for f, _z, _fin in col[tail:]], g
        settled += any(fin for _f, _z, fin in after[g][tail:])
    print("lanes whose open tail finalize settled:", settled)
    ex.close(); b.close()


def test_device_pointer_route_and_a_gather_across_episodes():
    """play_guided_selfplay with a torch network whose inputs and outputs stay on the device == the same network through host buffers;
    then a device gather over every row of the lanes that played several episodes: z and final as the run and finalize wrote them, every
    row with n_children > 0 sums to 1 within n_children * 2^-25."""
    import torch
    from alphazeroforhnefatafl_amd import MCTSArgs, play_guided_selfplay
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    cfg = "brandubh7"
    _rules, side, _wb, _lg, states, _salts, _over, S, budget = shape(cfg)
    lg = glg_of(cfg)
    A, n = lg.action_size, G
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(8 * side * side, A + 1)).to(dev).eval()

    class Net:
        def forward(self, boards_t, sides_t):
            with torch.no_grad():
                x = torch.stack([boards_t.float() / 35.0, (sides_t.float() / 8.0)[:, None, None].expand(-1, side, side)], 1)
                y = net(x)
                return torch.softmax(y[:, :A], 1).contiguous(), torch.tanh(y[:, A]).contiguous()

    class DeviceNet(Net):
        def __init__(self):
            self.boards = torch.empty((n, side, side), dtype=torch.uint8, device=dev)
            self.sides = torch.empty(n, dtype=torch.uint8, device=dev)
            self.waiting = torch.empty(n, dtype=torch.uint8, device=dev)
            self.keep = None

        def predict_batch(self, *_ptrs):
            p, v = self.forward(self.boards, self.sides)
            torch.cuda.synchronize()
            self.keep = (p, v)
            return p.data_ptr(), v.data_ptr()

    class HostNet(Net):
        def predict_batch(self, boards_, sides_, waiting):
            bt = torch.frombuffer(bytearray(bytes(boards_)), dtype=torch.uint8).reshape(n, side, side).to(dev)
            st = torch.frombuffer(bytearray(bytes(sides_)), dtype=torch.uint8).to(dev)
            p, v = self.forward(bt, st)
            p, v = p.cpu().numpy(), v.cpu().numpy()
            self.keep = (p, v)
            return p.ctypes.data_as(C.POINTER(C.c_float)), v.ctypes.data_as(C.POINTER(C.c_float))

    args = MCTSArgs(numMCTSSims=S, cpuct=1.0)
    b1, b2 = lg.new_batch(n), lg.new_batch(n)
    b1.upload(states); b2.upload(states)
    ex1, ex2 = lg.new_examples(n, budget, S), lg.new_examples(n, budget, S)
    dn = DeviceNet()
    r1 = play_guided_selfplay(b1, ex1, dn, args, budget, episode_moves=7, game_id_base=epu.IDS, sample_seed=3, temp_moves=2, device=True,
                              buffers=(dn.boards.data_ptr(), dn.sides.data_ptr(), dn.waiting.data_ptr()))
    r2 = play_guided_selfplay(b2, ex2, HostNet(), args, budget, episode_moves=7, game_id_base=epu.IDS, sample_seed=3, temp_moves=2)
    eps = list(r1[0])
    c1 = (r1[1].attacker_wins, r1[1].defender_wins, r1[1].draws, r1[1].cut)
    assert eps == list(r2[0]) and c1 == (r2[1].attacker_wins, r2[1].defender_wins, r2[1].draws, r2[1].cut) and r1[2:] == r2[2:]
    assert sum(c1) == sum(eps) and c1[3] > 0 and r1[3] == (0, 0)
    assert bytes(b1.download()) == bytes(b2.download())
    e1, _ = epu.device_examples(ex1, n, side)
    assert e1 == epu.device_examples(ex2, n, side)[0]
    several = [g for g in range(n) if eps[g] >= 2]
    assert several
    rows = np.array([j * n + g for g in several for j in range(len(e1[g]))], np.uint32)
    _boards, _sides, pi, z, fin = ex1.gather(torch.from_numpy(rows.astype(np.int32)).to(dev), device=True)
    nc = torch.from_numpy(ex1.read(rows)[0].astype(np.int64)).to(dev)
    assert bool((nc > 0).all()) and bool(((pi != 0).sum(1) == nc).all())
    assert bool(((pi.double().sum(1) - 1.0).abs() <= nc.double() * 2.0 ** -25).all())
    want = [e1[g][j][1:] for g in several for j in range(len(e1[g]))]
    assert list(zip(z.cpu().tolist(), fin.cpu().tolist())) == want
    # a lane's column: move_no returns to 0 at every episode boundary, a cut episode (7 moves) is not final, a closed one is
    for g in several:
        starts = [j for j, (f, _z, _fin) in enumerate(e1[g]) if f[5] == 0]
        assert len(starts) in (eps[g], eps[g] + 1) and starts[0] == 0
    for x in (ex1, ex2, b1, b2):
        x.close()


def test_refused_arguments_and_what_closes_a_run():
    from alphazeroforhnefatafl_amd._lib import TaflError, lib
    cfg = "brandubh7"
    _rules, n, _wb, _lg, states, salts, _over, S, _budget = shape(cfg)
    glg = glg_of(cfg)
    count, A = 8, abi.action_size(n)
    b = glg.new_batch(count)
    b.upload((TaflState * count)(*[states[g] for g in range(count)]))
    ex = glg.new_examples(count, 4, S)
    L = lib()

    def begin(opts, eo, openings=None, sims=S, moves=4, x=ex):
        return L.tafl_gselfplay_begin_episodes(b._h, sims, 256, epu.CPUCT, C.byref(opts), moves, 0, x._h, C.byref(eo) if eo is not None else None, openings)

    ok = TaflSelfplayOpts(epu.SSEED, 0, 0, 0)
    assert begin(TaflSelfplayOpts(epu.SSEED, 0, 3, 0), TaflEpisodeOpts(0, 0, 0)) == -1           # move_base != 0: TAFL_ERR_INVALID_ARG
    assert begin(ok, None) == -1
    assert begin(ok, TaflEpisodeOpts(0, 0, 1)) == -5                                             # TAFL_ERR_UNSUPPORTED
    bad = TaflEpisodeOpts(0, 0, 0)
    bad._reserved[2] = 1
    assert begin(ok, bad) == -5
    other = glg.new_batch(count + 1)
    assert begin(ok, TaflEpisodeOpts(0, 0, 0), other._h) == -1
    big = glg_of("copenhagen11").new_batch(count)
    assert begin(ok, TaflEpisodeOpts(0, 0, 0), big._h) == -1
    assert begin(ok, TaflEpisodeOpts(0, 0, 0), sims=0) == -1 and begin(ok, TaflEpisodeOpts(0, 0, 0), moves=0) == -1 and begin(ok, TaflEpisodeOpts(0, 0, 0), sims=65536) == -1
    wrong_ex, fresh = glg.new_examples(count + 1, 4, S), glg.new_batch(count)
    assert begin(ok, TaflEpisodeOpts(0, 0, 0), x=wrong_ex) == -1
    with pytest.raises(TaflError):
        fresh.gselfplay_episode_stats()                                                          # no episodes run on that batch
    for x in (other, big, wrong_ex, fresh):
        x.close()

    def open_run():
        b.gselfplay_begin_episodes(ex, 4, S, epu.CPUCT, sample_seed=epu.SSEED)
        assert b.gselfplay_step() == count
        boards, sides, waiting = b.gmcts_leaves()
        return gsu.stub_rows(boards, sides, waiting, count, n, A, salts[:count])

    def step_fails(pri, val):
        with pytest.raises(TaflError) as ei:
            b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        assert ei.value.code == -1

    pri, val = open_run()
    b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
    pri, val = open_run()
    b.upload((TaflState * count)(*[states[g] for g in range(count)]))                             # a write to the batch states
    step_fails(pri, val)
    pri, val = open_run()
    b.gmcts_begin(8)
    step_fails(pri, val)
    pri, val = open_run()
    b.gselfplay_end()
    step_fails(pri, val)
    b.gselfplay_episode_stats()                                                                  # still readable after the end
    b.gselfplay_begin(ex, 2, S, epu.CPUCT)                                                       # a plain run follows: no episode stats
    with pytest.raises(TaflError):
        b.gselfplay_episode_stats()
    ex.close(); b.close()
