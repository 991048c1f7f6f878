"""Dirichlet noise at the root of a guided search (include/taflhip.h tafl_root_noise) on a real MI355X: the noisy
instantiations of k_gmcts_step / k_gselfplay_step, k_root_noise_eval and k_gmcts_root_priors on the three preset layouts against the twin
of tests/noise_util.py fed the device's own eta, eta by its exact properties and against numpy's Dirichlet sampler, and the rules of the
setting: errors, latching, clearing, device pointers.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflRootNoise, TaflState
from oracle import oracle as orc
from tests import noise_util as nu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

_SIDES = {}


def side(cfg):
    if cfg not in _SIDES:
        from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
        rules, fen, wb = pu.CONFIGS[cfg]
        n = abi.fen_side_len(fen)
        _SIDES[cfg] = nu.DeviceSide(BatchedGameLogic(rules, n, wb), n)
    return _SIDES[cfg]


@pytest.mark.parametrize("cfg", nu.LAYOUTS)
def test_lockstep_search_equals_the_twin(cfg):
    P = nu.check_lockstep(side(cfg), orc, cfg)
    nu.check_extremes(side(cfg), orc, cfg, P)


@pytest.mark.parametrize("cfg", nu.LAYOUTS)
def test_guided_selfplay_equals_the_twin_loop(cfg):
    nu.check_selfplay(side(cfg), orc, cfg)


@pytest.mark.parametrize("cfg", nu.LAYOUTS)
def test_only_the_root_is_mixed(cfg):
    broken, of = nu.check_only_the_root(side(cfg), orc, cfg)
    print(f"{cfg}: noise at depth 1 as well breaks {broken} of {of} games")


@pytest.mark.parametrize("cfg", nu.LAYOUTS)
def test_eta_properties(cfg):
    nu.check_eta_properties(side(cfg), orc, cfg)


@pytest.mark.parametrize("cfg,alpha,ks", [("copenhagen11", 1.0, True), ("copenhagen11", 0.3, True), ("copenhagen11", 0.03, False), ("brandubh7", 0.3, True)])
def test_eta_is_dirichlet(cfg, alpha, ks):
    nu.check_eta_distribution(side(cfg), orc, cfg, alpha, ks)


def test_bad_settings_are_refused():
    from alphazeroforhnefatafl_amd._lib import TaflError, lib
    _rules, _n, _wb, _lg, states, salts = nu.setup(orc, "brandubh7")
    sd = side("brandubh7")
    b = sd._batch(states)
    for alpha, eps in ((0.0, 0.25), (-1.0, 0.25), (float("inf"), 0.25), (float("nan"), 0.25), (0.3, 0.0), (0.3, -0.5), (0.3, 1.5), (0.3, float("nan"))):
        for call in (lambda: b.set_root_noise(alpha, eps, 1), lambda: b.root_noise_eval(alpha, eps, 1)):
            with pytest.raises(TaflError) as ei:
                call()
            assert ei.value.code == -1, (alpha, eps)                       # TAFL_ERR_INVALID_ARG
    out = (C.c_double * (b.n * sd.A))()
    for bad in (TaflRootNoise(0.3, 0.25, 1, 0, 0, 1, 0), TaflRootNoise(0.3, 0.25, 1, 0, 0, 0, 1)):
        assert lib().tafl_gmcts_set_root_noise(b._h, C.byref(bad)) == -5   # TAFL_ERR_UNSUPPORTED
        assert lib().tafl_root_noise_eval(b._h, C.byref(bad), C.cast(out, C.c_void_p), 0) == -5
    # none of the refused settings took hold: the search is the noise-free one
    plain = sd.search(states, salts, None)
    got = sd.search_on(b, salts)
    assert got[0] == plain[0] and got[1].tobytes() == plain[1].tobytes()
    # a retained tree takes no noise
    b.set_root_noise(nu.ALPHA, nu.EPSILON, nu.NOISE_SEED)
    with pytest.raises(TaflError) as ei:
        b.gmcts_begin(nu.S, nu.EDGES, keep=True)
    assert ei.value.code == -5
    b.clear_root_noise()
    b.gmcts_begin(nu.S, nu.EDGES, keep=True)
    b.close()


def test_the_setting_is_latched_at_begin():
    """A change during a search takes effect at the next begin; the same for a run."""
    cfg = "brandubh7"
    _rules, n, _wb, _lg, states, salts = nu.setup(orc, cfg)
    sd = side(cfg)
    G, A = len(states), sd.A
    want_kids, want_pri, _ = nu.noisy_search(sd, orc, cfg)
    plain_kids, plain_pri, _ = sd.search(states, salts, None)
    b = sd._batch(states)
    b.set_root_noise(nu.ALPHA, nu.EPSILON, nu.NOISE_SEED)
    b.gmcts_begin(nu.S, nu.EDGES)
    b.clear_root_noise()                                                   # before the roots are expanded: the search keeps its noise
    w = b.gmcts_step(None, None, nu.CPUCT, nu.S)
    flip = 0
    while w:
        boards, sides, waiting = b.gmcts_leaves()
        pri, val = nu.gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
        w = b.gmcts_step(nu.gsu.fptr(pri), nu.gsu.fptr(val), nu.CPUCT, nu.S)
        flip += 1
        if flip == 2:
            b.set_root_noise(1.0, 1.0, 3)
        if flip == 3:
            b.clear_root_noise()
    kids, cnt = b.gmcts_root_children(512)
    assert nu._kids_of(kids, cnt, G, 512) == want_kids
    assert np.frombuffer(b.gmcts_root_priors(), np.float64).tobytes() == want_pri.tobytes()
    got = sd.search_on(b, salts)                                           # the next begin: cleared
    assert got[0] == plain_kids and got[1].tobytes() == plain_pri.tobytes()
    # a run: set after tafl_gselfplay_begin, the run stays noise-free; the next run has it
    ex = sd.glg.new_examples(G, nu.RUN_MOVES, nu.S)
    b.upload(states)
    b.gselfplay_begin(ex, nu.RUN_MOVES, nu.S, nu.CPUCT, nu.EDGES, game_id_base=nu.RUN_IDS, sample_seed=nu.RUN_SEED, temp_moves=nu.RUN_TEMP, move_base=nu.RUN_BASE)
    b.set_root_noise(nu.ALPHA, nu.EPSILON, nu.NOISE_SEED)
    w = b.gselfplay_step()
    while w:
        boards, sides, waiting = b.gmcts_leaves()
        pri, val = nu.gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
        w = b.gselfplay_step(nu.gsu.fptr(pri), nu.gsu.fptr(val))
    plays, moves = b.gselfplay_end()
    quiet = sd.run(states, salts, None, nu.RUN_MOVES, nu.RUN_SEED, nu.RUN_TEMP, nu.RUN_BASE, nu.RUN_IDS)
    assert [[pu.play_tuple4(plays[m * G + g]) for g in range(G)] for m in range(nu.RUN_MOVES)] == quiet.plays and list(moves) == quiet.moves
    noisy = nu.whole_run(sd, orc, cfg)
    assert noisy.plays != quiet.plays
    b.upload(states)
    ex.clear()
    run, _over, _stats = nu.gsu.device_run(b, ex, n, nu.S, nu.CPUCT, salts, nu.RUN_MOVES, nu.RUN_SEED, nu.RUN_TEMP, move_base=nu.RUN_BASE, base=nu.RUN_IDS, edges_per_node=nu.EDGES)
    assert run.plays == noisy.plays and run.states == noisy.states and run.examples == noisy.examples
    ex.close(); b.close()


@pytest.mark.parametrize("cfg", nu.LAYOUTS)
def test_cleared_noise_is_the_oracle_search(cfg):
    """After clear_root_noise a search equals orc.GameLogic.gmcts (gm_search) exactly: children, visits, Qsa bits, root priors."""
    _rules, n, wb, lg, states, salts = nu.setup(orc, cfg)
    sd = side(cfg)
    b = sd._batch(states)
    b.set_root_noise(nu.ALPHA, nu.EPSILON, nu.NOISE_SEED)
    noisy = sd.search_on(b, salts)
    b.clear_root_noise()
    kids, pri, _cnt = sd.search_on(b, salts)
    b.close()
    assert noisy[0] == nu.noisy_search(sd, orc, cfg)[0]
    for g in range(len(states)):
        st = orc.GameState.from_abi(states[g], wb)
        okids, _ns, opri, _ocnt = lg.gmcts(st, nu.S, nu.CPUCT, nu.predictor(sd.A, salts[g]), wb)
        assert kids[g] == [(a, v, nu.qbits(q)) for (_p, a, v, q) in okids], (cfg, g)
        if states[g].status == abi.ONGOING:
            assert pri[g].tobytes() == np.array(opri, np.float64).tobytes(), (cfg, g)
        else:
            assert not pri[g].any()


def test_device_pointer_route():
    """tafl_root_noise_eval and tafl_gmcts_root_priors into torch tensors == the host route."""
    import torch
    cfg = "copenhagen11"
    _rules, _n, _wb, _lg, states, salts = nu.setup(orc, cfg)
    sd = side(cfg)
    G = len(states)
    dev = torch.device("cuda:0")
    b = sd._batch(states)
    eta_t = torch.full((G, sd.A), -1.0, dtype=torch.float64, device=dev)
    b.root_noise_eval(nu.ALPHA, nu.EPSILON, nu.NOISE_SEED, out_device_ptr=eta_t.data_ptr())
    sd.glg.sync()
    assert eta_t.cpu().numpy().tobytes() == nu.eta_rows(sd, orc, cfg).tobytes()
    b.set_root_noise(nu.ALPHA, nu.EPSILON, nu.NOISE_SEED)
    _kids, pri, _ = sd.search_on(b, salts)
    pri_t = torch.full((G, sd.A), -1.0, dtype=torch.float64, device=dev)
    b.gmcts_root_priors(out_device_ptr=pri_t.data_ptr())
    sd.glg.sync()
    assert pri_t.cpu().numpy().tobytes() == pri.tobytes() == nu.noisy_search(sd, orc, cfg)[1].tobytes()
    b.close()


def test_python_front_ends_honour_the_args():
    """GuidedMCTS.search_all and play_guided_episodes set the noise MCTSArgs asks for, and clear it when dirichletEpsilon is 0."""
    from alphazeroforhnefatafl_amd import GuidedMCTS, MCTSArgs, play_guided_episodes
    cfg = "brandubh7"
    _rules, n, _wb, _lg, states, salts = nu.setup(orc, cfg)
    sd = side(cfg)
    G, A = len(states), sd.A

    class Net:
        def predict_batch(self, boards, sides, waiting):
            self.keep = nu.gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
            return nu.gsu.fptr(self.keep[0]), nu.gsu.fptr(self.keep[1])

    on = MCTSArgs(numMCTSSims=nu.S, cpuct=nu.CPUCT, dirichletAlpha=nu.ALPHA, dirichletEpsilon=nu.EPSILON, noiseSeed=nu.NOISE_SEED)
    off = MCTSArgs(numMCTSSims=nu.S, cpuct=nu.CPUCT)
    b = sd._batch(states)
    GuidedMCTS(b, Net(), on, edges_per_node=nu.EDGES).search_all()
    assert np.frombuffer(b.gmcts_root_priors(), np.float64).tobytes() == nu.noisy_search(sd, orc, cfg)[1].tobytes()
    GuidedMCTS(b, Net(), off, edges_per_node=nu.EDGES).search_all()
    assert np.frombuffer(b.gmcts_root_priors(), np.float64).tobytes() == sd.search(states, salts, None)[1].tobytes()
    on.game_id_base = nu.RUN_IDS
    ex = sd.glg.new_examples(G, nu.RUN_MOVES, nu.S)
    play_guided_episodes(b, ex, Net(), on, nu.RUN_MOVES, sample_seed=nu.RUN_SEED, temp_moves=nu.RUN_TEMP, edges_per_node=nu.EDGES, move_base=nu.RUN_BASE)
    want = nu.whole_run(sd, orc, cfg)
    assert [bytes(s) for s in b.download()] == want.states
    got, _over = nu.gsu.device_examples(ex, G, n)
    assert got == want.examples
    ex.close(); b.close()
