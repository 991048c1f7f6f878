"""The exact pre-filters of the playout ply on the host (tests/hostsim_filters): for every position along in-place playouts,
  filter false  =>  full test false
for the far-tile filter of the king capture (Engine::captures; rule (i), strong-by-throne beside the throne, and rule (ii), far tile
hostile), the exit-fort candidate test (Fast::fort_candidate: flanks, then the inner lines) against Engine::exit_fort, and the enclosure
filter of Fast::ply_of against the flood and security test.  The king-capture block sits behind its filter, so a second build of the same
source (-DTAFL_FILTER_PROBE) runs the block whatever the filter says and reports both.  Both builds must leave the oracle's states byte for
byte: the plain build is the filtered ply, the probe build the unfiltered one.

Inputs: the crafted rare-rule positions of tests/rare_workloads.py (enclosure, shieldwall, sparse endgames, exit forts, random boards),
positions with the king ringed by attackers but for one tile that an attacker can reach, positions with the king on each of the four
edges, next to each corner and next to the throne between flanking defenders, and playouts from the start position - under Copenhagen
11x11, Brandubh 7x7, Tablut 9x9 (strong by the throne) and Copenhagen with a weak, armed king (the far-tile filter is in force under
the two Copenhagen rulesets; under the other two every adjacency goes in, tafl_core.hpp).

The property is empty unless the full tests say yes often enough.  What the ORACLE alone says for these inputs (in-place playouts, the
state it leaves and the state one ply before; floors below, at least 50 each):
  exit fort 194, enclosed 123, king captured under the two rulesets of the far-tile filter (they have rule (ii) alone) 117, king captured
  beside his throne under a strong-by-throne ruleset (rule (i) decides there) 156
and the full tests of the walk itself, which sees every position on the way: exit fort 196, enclosed 123, rule (ii) 383 (65 of them under
the far-tile filter), rule (i) 176.  The whole file takes 7 s once the two libraries are built (a minute).
"""
import ctypes as C
import os
import subprocess
import functools

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflRules, TaflState
from oracle import oracle as orc
from tests import parity_util as pu
from tests.filters_util import CONFIGS, edge_king_spots, workload

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_filters")
_LIBS = {}
RULES = ("king (i)", "king (ii)", "exit fort", "enclosed")
SEED, BASE = 5, 11
FLOOR = 50


def lib(probe):
    if probe not in _LIBS:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libhostsim_filters_probe.so" if probe else "libhostsim_filters.so"))
        P, u8, u32, u64 = C.POINTER, C.c_uint8, C.c_uint32, C.c_uint64
        L.hsf_walk.restype = C.c_int
        L.hsf_walk.argtypes = [P(TaflRules), u8, u32, P(TaflState), u32, u64, P(u32), u64, P(u64)]
        assert L.hsf_probe_build() == int(probe)
        _LIBS[probe] = L
    return _LIBS[probe]


def _advance(name, plies):
    cfg = CONFIGS[name]
    states, G, _, _ = workload(name)
    out = pu.clone_states(states, G)
    orc.batch_random_advance(orc.GameLogic(cfg.rules, cfg.n), out, G, cfg.wb, SEED, (C.c_uint32 * G)(*plies), BASE)
    return out


@functools.lru_cache(maxsize=None)
def oracle_states(name):
    """What the oracle's in-place playouts leave, and for the games they ended the state one ply before the end."""
    _, G, plies, _ = workload(name)
    final = _advance(name, plies)
    ended = [g for g in range(G) if final[g].status != abi.ONGOING and final[g].turn > 0]
    before = _advance(name, [final[g].turn - 1 if final[g].status != abi.ONGOING and final[g].turn > 0 else 0 for g in range(G)])
    return final, before, ended


def _king_tile(st, wb):
    a, d = abi.state_words(st, wb)
    return (d >> (wb - 4)) & 15, (a >> (wb - 4)) & 15


def oracle_counts():
    """{rule: positions in which the oracle says yes}"""
    out = dict.fromkeys(RULES, 0)
    for name, cfg in CONFIGS.items():
        final, before, ended = oracle_states(name)
        sbt = cfg.rules.king_strength == abi.STRONG_BY_THRONE
        t = cfg.n // 2
        for g in ended:
            if final[g].status != abi.WIN:
                continue
            if final[g].reason == abi.EXIT_FORT:
                out["exit fort"] += 1
            elif final[g].reason == abi.ENCLOSED:
                out["enclosed"] += 1
            elif final[g].reason == abi.KING_CAPTURED:
                kr, kc = _king_tile(before[g], cfg.wb)
                if sbt:
                    out["king (i)"] += abs(kr - t) + abs(kc - t) == 1          # beside his throne: rule (i) is the one that decides
                else:
                    out["king (ii)"] += 1                                      # these rulesets have rule (ii) alone
    return out


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

def test_inputs_hold_the_king_on_every_edge_by_the_corners_and_by_the_throne():
    for name, cfg in CONFIGS.items():
        states, G, _, _ = workload(name)
        have = {_king_tile(states[g], cfg.wb) for g in range(G)}
        assert set(edge_king_spots(cfg.n)) <= have, (name, sorted(set(edge_king_spots(cfg.n)) - have))


def test_the_oracle_says_yes_often_enough():
    got = oracle_counts()
    print(got)
    for rule in RULES:
        assert got[rule] >= FLOOR, (rule, got)


def _walk(name, probe):
    cfg = CONFIGS[name]
    states, G, plies, _ = workload(name)
    mine = pu.clone_states(states, G)
    counts = (C.c_uint64 * 16)()
    r = cfg.rules.to_c()
    rc = lib(probe).hsf_walk(C.byref(r), cfg.n, cfg.wb, mine, G, SEED, (C.c_uint32 * G)(*plies), BASE, counts)
    assert rc == 0, (name, rc)
    return mine, {rule: tuple(counts[4 * i:4 * i + 4]) for i, rule in enumerate(RULES)}


@pytest.mark.parametrize("probe", [False, True], ids=["filtered ply", "probe build"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_no_filter_says_no_to_a_yes_and_the_ply_is_the_oracles(name, probe):
    cfg = CONFIGS[name]
    states, G, plies, spans = workload(name)
    got, counts = _walk(name, probe)
    print(name, "probe" if probe else "plain", "(tested, filter true, full true, filter false and full true):", counts)
    for rule, (_tested, _filt, _full, broken) in counts.items():
        assert broken == 0, (name, rule, counts[rule])
    if probe:                                   # the block reports only in the probe build: every attacker ply with the king on the board
        assert counts["king (ii)"][0] > 0 and counts["king (i)"][0] == counts["king (ii)"][0], (name, counts)
    want = oracle_states(name)[0]
    g = pu.first_state_diff(want, got, G)
    assert g < 0, f"{name} game {g} ({[k for k, (a, b) in spans.items() if a <= g < b]}, {plies[g]} plies) from\n{pu.describe_state(states[g], cfg.wb)}\n" \
                  f"oracle\n{pu.describe_state(want[g], cfg.wb)}\nhost-sim\n{pu.describe_state(got[g], cfg.wb)}"


def test_the_full_tests_say_yes_in_the_walk_as_often_as_the_oracle():
    """The walk sees every position the oracle's playouts pass through, so its full tests say yes at least where the oracle ended a game."""
    total = dict.fromkeys(RULES, 0)
    for name in CONFIGS:
        for rule, c in _walk(name, True)[1].items():
            total[rule] += c[2]
    want = oracle_counts()
    print(total, want)
    for rule in ("exit fort", "enclosed"):
        assert total[rule] >= want[rule] >= FLOOR, (rule, total, want)
    assert total["king (i)"] >= want["king (i)"] >= FLOOR and total["king (ii)"] >= want["king (ii)"] >= FLOOR, (total, want)
