"""Dirichlet noise at the root of a guided search (include/taflhip.h tafl_root_noise) on the host harness
(tests/hostsim_noise: the per-game functions of tafl_guided.hpp compiled for the CPU) against the twin of tests/noise_util.py, and the
eta rows by their exact properties and against numpy's Dirichlet sampler.  The same checks run on the device in test_gpu_root_noise.py."""
import pytest

from alphazeroforhnefatafl_amd import abi
from oracle import oracle as orc
from tests import noise_util as nu
from tests import parity_util as pu

_SIDES = {}


def side(cfg):
    if cfg not in _SIDES:
        rules, fen, wb = pu.CONFIGS[cfg]
        _SIDES[cfg] = nu.HostSide(rules, abi.fen_side_len(fen), wb)
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
