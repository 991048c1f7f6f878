"""The value-only playout (tafl_core.hpp: ValueOnly - repetition tracker on packed records) on the host, next to the keeping path, on
run-time Consts and on the constexpr Consts of the presets: value, status, reason, winner
and plies of every playout against the CPU oracle, over inputs that make the tracker matter (tests/value_only_util.py).  The in-place
playouts of the same states pin the keeping path: the states they leave must be the oracle's byte for byte.

Condition on the inputs, checked on the oracle's results alone: at least 32 playouts per ruleset end by repetition - Copenhagen and Brandubh
lose by it, Tablut draws.  (13x13 Copenhagen shares its ruleset with the 11x11 board and is held to what its smaller search aims for.)"""
import ctypes as C
import os
import subprocess

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflRolloutResult, TaflRules, TaflState
from tests import parity_util as pu
from tests import rare_workloads as rw
from tests import value_only_util as vu

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_value_only")
_LIB = None
POLICIES = {"keep": 0, "value_only": 1}


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_value_only.so"))
        P, u8, u32, u64, i32 = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int
        L.hsv_rollout.restype = i32
        L.hsv_rollout.argtypes = [P(TaflRules), u8, u32, i32, i32, i32, P(TaflState), u32, u64, u32, u32, u64, P(TaflRolloutResult)]
        L.hsv_random_advance.restype = i32
        L.hsv_random_advance.argtypes = [P(TaflRules), u8, u32, i32, P(TaflState), u32, u64, P(u32), u64]
        _LIB = L
    return _LIB


class Engine:
    """Adapter for rare_workloads._compare_rollouts."""

    def __init__(self, cfg, policy, preset):
        self.cfg, self.policy, self.preset = cfg, POLICIES[policy], int(preset)
        self.rules = cfg.rules.to_c()
        self.dense13 = int(cfg.n == 13 and cfg.wb == 256)
        self.label = f"host-sim {policy} ({'preset' if preset else 'run-time'} Consts)"

    def rollout(self, states, G, seed, sim, cap, base):
        mine = pu.clone_states(states, G)
        out = (TaflRolloutResult * G)()
        rc = lib().hsv_rollout(C.byref(self.rules), self.cfg.n, self.cfg.wb, self.policy, self.preset, self.dense13, mine, G, seed, sim, cap, base, out)
        assert rc == 0, (self.label, rc)
        return out, mine

    def random_advance(self, states, G, seed, plies, base):
        mine = pu.clone_states(states, G)
        rc = lib().hsv_random_advance(C.byref(self.rules), self.cfg.n, self.cfg.wb, self.preset, mine, G, seed, plies, base)
        assert rc == 0, (self.label, rc)
        return mine


def _consts(cfg):
    return (False, True) if cfg.preset else (False,)


@pytest.mark.parametrize("name", list(vu.CONFIGS))
def test_inputs_end_by_repetition_often_enough(name):
    floor = vu.FLOOR if name != "copenhagen13" else vu.WANTED[name][0]
    got = vu.repetition_endings(name, vu.CPU_CAP)
    assert got >= floor, (name, got, floor)
    want_status = abi.WIN if vu.CONFIGS[name].rules.repetition_rule[1] else abi.DRAW
    assert all(t[1] == want_status for t in vu.expectations(name, vu.CPU_CAP)[vu.G_FULL][2][vu.SEED] if vu.is_repetition(t)), name
    assert vu.workload(name)[2] >= vu.WANTED.get(name, vu.WANTED[None])[1], name           # near misses: same first ply, another tracker


@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("name", list(vu.CONFIGS))
def test_playouts_equal_the_oracle(name, policy):
    cfg = vu.CONFIGS[name]
    states, G, want = vu.expectations(name, vu.CPU_CAP)[vu.G_FULL]
    for preset in _consts(cfg):
        rw._compare_rollouts(Engine(cfg, policy, preset), cfg, states, G, want, vu.CPU_CAP, vu.BASE, f"{name} rollout")


@pytest.mark.parametrize("name", list(vu.CONFIGS))
def test_longer_playouts_equal_the_oracle(name):
    """The cap of the device test: the counters of both sides run on for 80 plies behind the crafted start."""
    cfg = vu.CONFIGS[name]
    states, G, want = vu.expectations(name, vu.GPU_CAP)[65]
    for preset in _consts(cfg):
        for policy in ("value_only", "keep"):
            rw._compare_rollouts(Engine(cfg, policy, preset), cfg, states, G, want, vu.GPU_CAP, vu.BASE, f"{name} rollout, cap {vu.GPU_CAP}")


@pytest.mark.parametrize("name", [n for n in vu.CONFIGS])
def test_in_place_playouts_leave_the_oracles_states(name):
    cfg = vu.CONFIGS[name]
    states = vu.workload(name)[0]
    want = vu.advance_expectation(name)
    for preset in _consts(cfg):
        eng = Engine(cfg, "keep", preset)
        got = eng.random_advance(states, vu.G_FULL, rw.ADVANCE_SEED, vu.advance_plies(vu.G_FULL), rw.ADVANCE_BASE)
        g = pu.first_state_diff(want, got, vu.G_FULL)
        assert g < 0, f"{eng.label} {name} random_advance: game {g} ({g % 7 + 1} plies) from\n{pu.describe_state(states[g], cfg.wb)}\n" \
                      f"oracle\n{pu.describe_state(want[g], cfg.wb)}\nengine\n{pu.describe_state(got[g], cfg.wb)}"
