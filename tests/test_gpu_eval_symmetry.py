"""A random board symmetry per leaf evaluation (include/taflhip.h tafl_eval_symmetry) on a real MI355X: the SYM
rounds of tafl_gmcts_sym.hip, k_gmcts_leaves and k_gmcts_leaf_symmetry against the oracle's guided search run with the wrapped predictor
of tests/eval_symmetry_util.py, the self-play families by conjugation, and the rules of the setting.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflEpisodeOpts, TaflEvalSymmetry, TaflMatchOpts, TaflSelfplayOpts, TaflState
from oracle import oracle as orc
from tests import board_sizes_util as bsu
from tests import eval_symmetry_util as su

pytestmark = pytest.mark.gpu
UNSUPPORTED = -5


def batch_of(name, states=None):
    rules, n, wb, _lg, st, _S, _salts = su.workload(orc, name)
    st = st if states is None else states
    return bsu.gpu_batch(rules, n, wb, st, len(st))


@pytest.mark.parametrize("name", ("copenhagen11", "brandubh7", "copenhagen13", "side8"))
def test_lockstep_search_equals_the_wrapped_oracle(name):
    """Root children bit for bit, stats.sims, stats.predicts and faults == 0 against lg.gmcts with predict'."""
    _rules, n, _wb, _lg, states, S, salts = su.workload(orc, name)
    on, tally, off = su.expectation(orc, name)
    G = len(states)
    b = batch_of(name)
    b.set_eval_symmetry(su.SEED, su.BASE)
    kids, st = su.device_search(b, n, S, salts)
    b.close()
    for g in range(G):
        assert kids[g] == on[g][0], (name, "children", g)
    assert (st.sims, st.predicts, st.terminal_hits) == tuple(sum(on[g][1][i] for g in range(G)) for i in range(3)), name
    assert st.faults == 0
    differ = sum(on[g][0] != off[g][0] for g in range(G))
    print(f"{name}: {tally.leaves} leaves, draws {tally.draws}, all-masked {tally.all_masked}, {differ} of {G} games differ from the unwrapped search")
    assert differ > G // 2 and all(tally.draws), name


def test_first_round_every_game_at_its_root():
    """tafl_gmcts_leaf_symmetry equals the Python rule on the downloaded states; the boards are the transformed board_to_matrix; sides
    and waiting are as with the setting off; a second context at game_id_base + 32 gives the same draws; the device-pointer route
    equals the host-pointer route."""
    import torch
    _rules, n, wb, _lg, states, S, _salts = su.workload(orc, "copenhagen11")
    G = len(states)
    b = batch_of("copenhagen11")
    b.gmcts_begin(S, su.EDGES)
    assert b.gmcts_step(None, None, su.CPUCT, S) == G
    boards0, sides0, waiting0 = b.gmcts_leaves()
    assert not any(b.gmcts_leaf_symmetry())                                       # the setting is off
    b.set_eval_symmetry(su.SEED, su.BASE)
    b.gmcts_begin(S, su.EDGES)
    assert b.gmcts_step(None, None, su.CPUCT, S) == G
    boards, sides, waiting = b.gmcts_leaves()
    syms = list(b.gmcts_leaf_symmetry())
    got = b.download()
    gs = [orc.GameState.from_abi(got[g], wb) for g in range(G)]
    assert syms == [su.draw_of(orc, gs[g], su.SEED, su.BASE + g) for g in range(G)]
    assert set(syms) == set(range(8))
    shown = np.frombuffer(bytes(boards), np.uint8).reshape(G, n, n)
    plain = np.frombuffer(bytes(boards0), np.uint8).reshape(G, n, n)
    for g in range(G):
        want = su.transform(np.array(gs[g].board_to_matrix(), np.uint8), syms[g])
        assert (shown[g] == want).all() and (plain[g] == np.array(gs[g].board_to_matrix(), np.uint8)).all(), g
    assert bytes(sides) == bytes(sides0) and bytes(waiting) == bytes(waiting0) == bytes([1] * G)
    # the device-pointer route
    dev = torch.device("cuda", 0)
    tb, ts, tw, ty = (torch.full((k,), 0xAA, dtype=torch.uint8, device=dev) for k in (G * n * n, G, G, G))
    b.gmcts_leaves(tb.data_ptr(), ts.data_ptr(), tw.data_ptr())
    b.gmcts_leaf_symmetry(ty.data_ptr())
    torch.cuda.synchronize()
    assert bytes(tb.cpu().numpy()) == bytes(boards) and bytes(ts.cpu().numpy()) == bytes(sides) and bytes(tw.cpu().numpy()) == bytes(waiting)
    assert ty.cpu().tolist() == syms
    b.close()
    # independence of the sharding: the second half of the games alone, under its own base
    half = (TaflState * (G - 32))(*[states[g] for g in range(32, G)])
    b2 = batch_of("copenhagen11", half)
    b2.set_eval_symmetry(su.SEED, su.BASE + 32)
    b2.gmcts_begin(S, su.EDGES)
    assert b2.gmcts_step(None, None, su.CPUCT, S) == G - 32
    assert list(b2.gmcts_leaf_symmetry()) == syms[32:]
    b2.close()


_RUNS = {}


def selfplay(variant, episodes, sym_seed=None, conjugated=False):
    key = (variant, episodes, sym_seed, conjugated)
    if key not in _RUNS:
        rules, n, wb, _lg, states, _S, salts = su.workload(orc, "copenhagen11")
        _RUNS[key] = su.device_selfplay(bsu.gpu_logic(rules, n, wb), states, n, salts, variant, episodes, sym_seed, conjugated)
    return _RUNS[key]


@pytest.mark.parametrize("episodes", (False, True), ids=("per_pace", "episodes"))
@pytest.mark.parametrize("variant", su.VARIANTS)
def test_selfplay_families_by_conjugation(variant, episodes):
    """The run with the setting on and the conjugated stub equals the run with it off and the plain stub: plays, moves, states, every
    example field, the counters and the episode stats; all eight symmetries appear in the getter during the on-run."""
    off, seen_off = selfplay(variant, episodes)
    on, seen_on = selfplay(variant, episodes, su.SEED, True)
    assert seen_off == {0} and seen_on == set(range(8)), (seen_off, seen_on)
    assert off["stats"][3] == 0 and off["stats"][0] > 0 and sum(off["moves"]) > 0
    for key in off:
        assert on[key] == off[key], (variant, episodes, key)
    assert set(on) == set(off)
    if episodes:
        assert min(off["episodes"][0]) >= 1                                       # every lane closed or cut an episode and reopened


def test_selfplay_with_the_plain_stub_differs():
    """One on-run with the plain stub differs from the off-run in more than half of the games."""
    off, _ = selfplay("plain", False)
    on, seen = selfplay("plain", False, su.SEED, False)
    G = len(off["moves"])
    assert seen == set(range(8)) and on["stats"][3] == 0
    differ = sum([on["plays"][m * G + g] for m in range(su.SP_MOVES)] != [off["plays"][m * G + g] for m in range(su.SP_MOVES)] or
                 on["examples"][g] != off["examples"][g] for g in range(G))
    print(f"{differ} of {G} games differ")
    assert differ > G // 2


def test_contract():
    """Set then clear equals never set; a change between begin and the first step does not affect the running search; non-zero flags or
    reserved words and a match while set are refused."""
    from alphazeroforhnefatafl_amd._lib import lib
    _rules, n, _wb, _lg, states, S, salts = su.workload(orc, "brandubh7")
    on, _tally, off = su.expectation(orc, "brandubh7")
    G = len(states)
    b = batch_of("brandubh7")
    b.set_eval_symmetry(su.SEED, su.BASE)
    b.clear_eval_symmetry()
    kids, st = su.device_search(b, n, S, salts)
    assert all(kids[g] == off[g][0] for g in range(G)) and st.faults == 0
    # latched at the begin: clearing (or another seed) before the first step changes nothing
    b.set_eval_symmetry(su.SEED, su.BASE)
    b.gmcts_begin(S, su.EDGES)
    b.clear_eval_symmetry()
    kids, st = su.device_search(b, n, S, salts, begin=False)
    assert all(kids[g] == on[g][0] for g in range(G)) and st.faults == 0
    b.gmcts_begin(S, su.EDGES)
    b.set_eval_symmetry(su.SEED + 1, su.BASE)
    kids, st = su.device_search(b, n, S, salts, begin=False)
    assert all(kids[g] == off[g][0] for g in range(G)) and st.faults == 0
    # refused settings leave the setting as it was (SEED + 1 is set)
    for bad in (TaflEvalSymmetry(1, 0, 1), TaflEvalSymmetry(1, 0, 0, (1, 0, 0)), TaflEvalSymmetry(1, 0, 0, (0, 0, 1))):
        assert lib().tafl_gmcts_set_eval_symmetry(b._h, C.byref(bad)) == UNSUPPORTED
    b.set_eval_symmetry(su.SEED, su.BASE)
    bad = TaflEvalSymmetry(99, 5, 7)
    assert lib().tafl_gmcts_set_eval_symmetry(b._h, C.byref(bad)) == UNSUPPORTED
    kids, st = su.device_search(b, n, S, salts)
    assert all(kids[g] == on[g][0] for g in range(G))
    # a match refuses the setting
    o, eo, mo = TaflSelfplayOpts(1, 0, 0, 0), TaflEpisodeOpts(0, 0, 0), TaflMatchOpts(0, 0)
    assert lib().tafl_gmatch_begin(b._h, 8, su.EDGES, su.CPUCT, C.byref(o), 4, 0, None, C.byref(eo), None, C.byref(mo)) == UNSUPPORTED
    b.clear_eval_symmetry()
    assert lib().tafl_gmatch_begin(b._h, 8, su.EDGES, su.CPUCT, C.byref(o), 4, 0, None, C.byref(eo), None, C.byref(mo)) == 0
    b.close()


def test_keep_tree_by_conjugation():
    """KEEP_TREE (the oracle's guided search has no entry point that continues a tree with a predictor, so by conjugation): a search, an
    advance along the most visited child and a continued search, on 16 games - the setting on with the conjugated stub equals the
    setting off with the plain stub, and the continued search draws symmetries for its new leaves."""
    _rules, n, _wb, _lg, states, S, salts = su.workload(orc, "copenhagen13")
    G = len(states)
    results = []
    for on in (False, True):
        b = batch_of("copenhagen13")
        if on:
            b.set_eval_symmetry(su.SEED, su.BASE)
        net = su.conjugated_net(G, n, salts) if on else None
        b.gmcts_begin(S, su.EDGES, keep=True)
        first, _ = su.device_search(b, n, S, salts, begin=False, net=net)
        b.gmcts_advance(None)
        b.gmcts_begin(S, su.EDGES, keep=True)
        rounds = []
        second, st = su.device_search(b, n, S, salts, rounds_out=rounds, begin=False, net=net)
        assert st.faults == 0
        results.append((first, second, bytes(b.download()), st.sims, st.predicts))
        seen = {r[3][g] for r in rounds for g in range(G) if r[2][g]}
        assert (len(seen) >= 4) if on else seen == {0}, seen
        b.close()
    assert results[0] == results[1]
    assert any(results[0][1][g] != results[0][0][g] for g in range(G))
