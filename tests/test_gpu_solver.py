"""Exact win/loss proofs in guided self-play (include/taflhip.h tafl_solver) on a real MI355X: the rounds
k_gselfplay_solver (plain / episodes, without / with root noise, a playout cap and forced playouts) on the endgame set of
tests/solver_util.py - 72 Brandubh lanes, the last four plies of 18 random games, S = 24 - against the host harness
(tests/hostsim_solver) on every lane and against the Python twin on ten spot lanes; the crafted lanes of the three layouts as 8-lane
batches; opening positions, where the setting changes nothing; latching, refusals and the Python front end.  Every comparison is exact
except the row sum of a gathered policy.  Arenas are sized so that nothing overflows.  `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflEpisodeOpts, TaflMatchOpts, TaflSelfplayOpts, TaflSolver, TaflSolverStats, TaflState
from oracle import oracle as orc
from tests import episodes_util as epu
from tests import forced_util as fu
from tests import gselfplay_util as gsu
from tests import noise_util as nu
from tests import playout_cap_util as pcu
from tests import solver_util as su
from tests.test_gpu_episodes import glg_of

pytestmark = pytest.mark.gpu

G, S, K = su.G, su.S, fu.K
RUN_MOVES, RUN_TEMP, RUN_SEED, RUN_IDS = 3, 2, 5, 1000
BUDGET = 6
SPOTS = list(su.SPOTS)


def on_device(cfg, states, salts, n_moves, seed, temp, n_sims=S, max_children=S, **kw):
    n = abi.fen_side_len(pcu.pu.CONFIGS[cfg][1])
    glg = glg_of(cfg)
    b = glg.new_batch(len(states))
    b.upload(states)
    ex = glg.new_examples(len(states), n_moves, max_children)
    got = su.device_solver(b, ex, n, salts, n_moves, seed, temp, n_sims=n_sims, **kw)
    es = ex.stats()
    assert got.stat_faults == 0 and (es.dropped, es.overflowed) == (0, 0)
    ex.close(); b.close()
    return got


def on_host(cfg, states, salts, n_moves, seed, temp, n_sims=S, max_children=S, **kw):
    rules, _fen, wb = pcu.pu.CONFIGS[cfg]
    n = abi.fen_side_len(pcu.pu.CONFIGS[cfg][1])
    ex = su.HostExamples(n, len(states), n_moves, max_children)
    got = su.host_solver(rules, n, wb, states, salts, n_moves, seed, temp, n_sims=n_sims, ex=ex, **kw)
    assert not any(got.faults) and got.stat_faults == 0
    return got


@functools.lru_cache(maxsize=None)
def plain_device():
    _rules, _n, _wb, _lg, states, salts = su.endgame(orc)
    return on_device("brandubh7", states, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, base=RUN_IDS)


def test_the_plain_run_equals_the_harness_and_the_twin():
    """Three moves, temp_moves = 2, nothing else set.  Every lane against the harness, counters included; ten spot lanes against the twin
    run; the simulations run and skipped add up to the budgets of the searches."""
    _rules, _n, wb, lg, states, salts = su.endgame(orc)
    got = plain_device()
    su.assert_same_lanes(got, on_host("brandubh7", states, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, base=RUN_IDS), "plain")
    want, tally = su.twin_run(orc, lg, states, wb, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, 0, RUN_IDS, S, games=SPOTS)
    assert tally.root_won >= 1 and tally.skipped_sims > 0 and tally.pruned_visits > 0, tally.stats()
    fu.assert_lanes_equal_run(got, want, RUN_MOVES, "plain", SPOTS)
    sv = dict(zip(su.STATS, got.sv_stats))
    assert sv["root_won"] >= 6 and sv["nodes_won"] >= 15 and sv["moves"] == sum(got.moves)
    assert got.sims + sv["skipped_sims"] == S * sv["moves"]          # (every search of these lanes ends in a move)


@pytest.mark.parametrize("episodes,noisy,capped,forced", [(False, True, False, True), (True, False, True, False), (True, True, False, False), (True, True, True, True)])
def test_every_composition_equals_the_harness(episodes, noisy, capped, forced):
    """The four instantiations of the layout with the settings they take at run time: every lane, every counter."""
    _rules, _n, _wb, _lg, states, salts = su.endgame(orc)
    kw = dict(k=K if forced else None, cap=fu.cap_cfg(32768) if capped else None, noise=nu.noise_cfg() if noisy else None, episodes=episodes,
              base=epu.IDS, stride=G if episodes else 0)
    got = on_device("brandubh7", states, salts, BUDGET, pcu.SSEED, pcu.TEMP, **kw)
    host = on_host("brandubh7", states, salts, BUDGET, pcu.SSEED, pcu.TEMP, **kw)
    su.assert_same_lanes(got, host, (episodes, noisy, capped, forced))
    sv = dict(zip(su.STATS, got.sv_stats))
    assert sv["root_won"] > 0 and sv["skipped_sims"] > 0 and sv["moves"] == sum(got.moves)
    if capped:
        assert sum(got.cap_stats) == sv["moves"] and got.cap_stats[1] > 0
    if forced:
        assert got.fp_stats[0] > 0 and got.fp_stats[3] == (got.cap_stats[0] if capped else sv["moves"])


def test_the_full_composition_equals_the_twins_on_the_spot_lanes():
    """Episodes, root noise, a cap (fast_sims 6, half of the moves full) and forced playouts: the spot lanes against the composition of
    solver twin moves, fed the device's eta."""
    rules, n, _wb, _lg, states, salts = su.endgame(orc)
    got = on_device("brandubh7", states, salts, BUDGET, pcu.SSEED, pcu.TEMP, k=K, cap=fu.cap_cfg(32768), noise=nu.noise_cfg(), episodes=True, base=epu.IDS, stride=G)
    want, tally = su.capped_composition(orc, nu.DeviceSide(glg_of("brandubh7"), n), 32768, True, K, lanes=SPOTS, budget=BUDGET)
    assert want.full > 0 and want.fast > 0 and tally.root_won > 0
    pcu.assert_equal(got, want, "composition", games=SPOTS, predicts=False)


@pytest.mark.parametrize("cfg", nu.LAYOUTS)
def test_the_crafted_lanes(cfg):
    """8-lane batches under the flat predictor: LOST roots on every layout, a WON root through a depth-1 LOST node on Brandubh, a win in
    one on the larger boards; the pruned root block, the example and the counters against the harness and the twin."""
    _rules, _n, wb, lg, states, salts, sims = su.crafted(orc, cfg)
    distinct = 3 if cfg == "brandubh7" else 2
    found = su.searches(orc, ("crafted", cfg), lg, states, wb, salts, sims, games=range(distinct))
    assert su.LOST in [found[g][0].root.proof for g in found] and su.WON in [found[g][0].root.proof for g in found]
    for s in sorted(set(sims)):
        got = on_device(cfg, states, salts, 1, RUN_SEED, 0, n_sims=s, max_children=512)
        host = on_host(cfg, states, salts, 1, RUN_SEED, 0, n_sims=s, max_children=512, kids=True)
        su.assert_same_lanes(got, host, (cfg, s))
        mine = [g for g in range(8) if sims[g] == s]
        twin = {g: found[g % distinct] for g in mine}
        su.assert_search_equals_twin(host, twin, mine, (cfg, s))
        for g in mine:                                              # (the device leaves what the harness leaves: its example is the twin's)
            assert got.examples[g] == host.examples[g] and got.plays[g] == host.plays[g]
        if len(mine) == 8:
            assert got.sv_stats == tuple(sum(getattr(twin[g][2], name) for g in mine) for name in su.STATS)
            assert got.sims + got.sv_stats[2] == s * 8


def test_on_opening_positions_the_setting_changes_nothing():
    """noise_util.setup's 70 opening positions reach no terminal: the run is byte for byte the run without the setting, and every counter that
    can change a run (proven roots, skipped simulations, pruned visits and children) is 0."""
    _rules, _n, _wb, _lg, states, salts = nu.setup(orc, "brandubh7")
    states, salts = (TaflState * nu.G_PLAIN)(*[states[g] for g in range(nu.G_PLAIN)]), salts[:nu.G_PLAIN]      # (the two crafted games are late ones)
    on = on_device("brandubh7", states, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, base=RUN_IDS)
    off = on_device("brandubh7", states, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, base=RUN_IDS, solver=False)
    epu.assert_same(on, off, "openings")
    assert off.sv_stats is None and on.sims == off.sims and on.predicts == off.predicts
    sv = dict(zip(su.STATS, on.sv_stats))
    assert [sv[name] for name in ("root_won", "root_lost", "skipped_sims", "pruned_visits", "pruned_children")] == [0] * 5 and sv["moves"] == sum(on.moves) > 0
    # (one lane proves a node two plies down WON, which no selection meets again: the harness, which the CPU tests hold to the twin, counts it too)
    assert on.sv_stats == on_host("brandubh7", states, salts, RUN_MOVES, RUN_SEED, RUN_TEMP, base=RUN_IDS).sv_stats and sv["nodes_won"] + sv["nodes_lost"] <= 2


def test_refusals_and_what_a_begin_latches():
    from alphazeroforhnefatafl_amd._lib import lib
    _rules, n, _wb, _lg, states, salts = su.endgame(orc)
    glg = glg_of("brandubh7")
    count, A = 8, abi.action_size(n)
    sub = (TaflState * count)(*[states[g] for g in range(count)])
    b = glg.new_batch(count)
    b.upload(sub)
    ex = glg.new_examples(count, 3, S)
    L = lib()
    ok = TaflSelfplayOpts(RUN_SEED, 0, 0, 0)
    st = TaflSolverStats()

    def set_it(flags=0, reserved=None):
        f = TaflSolver(flags)
        if reserved is not None:
            f._reserved[reserved] = 1
        return L.tafl_gselfplay_set_solver(b._h, C.byref(f))

    def run():
        b.upload(sub); ex.clear()
        b.gselfplay_begin(ex, 3, S, su.CPUCT, 256, game_id_base=0, sample_seed=RUN_SEED, temp_moves=0)

    def drive():
        w = b.gselfplay_step()
        while w:
            boards, sides, waiting = b.gmcts_leaves()
            pri, val = gsu.stub_rows(boards, sides, waiting, count, n, A, salts[:count])
            w = b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        plays, moves = b.gselfplay_end()
        return [pcu.pu.play_tuple4(p) for p in plays], list(moves), gsu.device_examples(ex, count, n)[0], b.gmcts_stats().sims

    assert L.tafl_gselfplay_solver_stats(b._h, C.byref(st)) == -1
    assert set_it(flags=1) == -5 and all(set_it(reserved=i) == -5 for i in range(7))      # TAFL_ERR_UNSUPPORTED, and nothing is set:
    run()
    assert L.tafl_gselfplay_solver_stats(b._h, C.byref(st)) == -1
    assert set_it() == 0                                                 # set after the begin: the open run is not affected
    off = drive()
    assert L.tafl_gselfplay_solver_stats(b._h, C.byref(st)) == -1
    run()
    b.clear_solver()                                                    # a clear mid-run leaves the latched setting
    on = drive()
    ss = b.solver_stats()
    assert on != off and ss.root_won > 0 and ss.skipped_sims > 0 and ss.moves == sum(on[1]) and on[3] + ss.skipped_sims == S * ss.moves
    run()                                                               # NULL cleared it: this run is the first one again
    assert drive() == off and L.tafl_gselfplay_solver_stats(b._h, C.byref(st)) == -1
    assert set_it() == 0 and set_it(flags=2) == -5                      # a rejected argument leaves the setting as it was
    run()
    assert drive() == on

    def lockstep():                                                     # the lock-step search ignores the setting
        b.upload(sub)
        return nu.DeviceSide(glg, n).search_on(b, salts[:count])[0]
    with_it = lockstep()
    b.clear_solver()
    assert lockstep() == with_it
    assert set_it() == 0                                                # a match is refused while the setting stands, and accepted after clearing
    mo, eo = TaflMatchOpts(0, 0), TaflEpisodeOpts(0, 0, 0)
    b.upload(sub)
    assert L.tafl_gmatch_begin(b._h, S, 256, su.CPUCT, C.byref(ok), 3, 0, None, C.byref(eo), None, C.byref(mo)) == -5
    b.clear_solver()
    assert L.tafl_gmatch_begin(b._h, S, 256, su.CPUCT, C.byref(ok), 3, 0, None, C.byref(eo), None, C.byref(mo)) == 0
    b.gselfplay_end()
    ex.close(); b.close()


def test_python_front_end():
    """play_guided_selfplay with a small torch network on device pointers and MCTSArgs(solver=True) on the endgame set: the simulations
    run and skipped add up to S per move, and every gathered row sums to 1 within n_children * 2^-25.  play_match refuses the setting."""
    import torch
    from alphazeroforhnefatafl_amd import MCTSArgs, play_guided_selfplay, play_match
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    _rules, side, _wb, _lg, states, _salts = su.endgame(orc)
    lg = glg_of("brandubh7")
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

    args = MCTSArgs(numMCTSSims=24, cpuct=1.25, solver=True)
    b = lg.new_batch(n)
    b.upload(states)
    ex = lg.new_examples(n, budget, 24)
    dn = DeviceNet()
    _eps, _est, total, lost = play_guided_selfplay(b, ex, dn, args, budget, game_id_base=RUN_IDS, sample_seed=3, temp_moves=2, device=True,
                                                   buffers=(dn.boards.data_ptr(), dn.sides.data_ptr(), dn.waiting.data_ptr()))
    ss, gs = b.solver_stats(), b.gmcts_stats()
    assert gs.faults == 0 and lost == (0, 0) and total == ss.moves > 0
    assert gs.sims + ss.skipped_sims == 24 * ss.moves
    lens = list(ex.counts()[0])
    rows = np.array([j * n + g for g in range(n) for j in range(lens[g])], np.uint32)
    assert rows.size == total
    _boards, _sides, pi, _z, _fin = ex.gather(torch.from_numpy(rows.astype(np.int32)).to(dev), device=True)
    nc, _ov, played, _mv, acts, vis = ex.read(rows)
    pi = pi.cpu().numpy()
    for i in range(rows.size):
        k = int(nc[i])
        a, v = acts[i, :k].astype(np.int64), vis[i, :k].astype(np.float64)
        assert k > 0 and (v > 0).all() and int(played[i]) in a.tolist(), i
        assert abs(float(pi[i].astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -25, i
    with pytest.raises(ValueError):
        play_match(b, (dn, dn), MCTSArgs(numMCTSSims=24, solver=True), budget)
    ex.close(); b.close()
