"""Device replay of tests/golden/mcts_reuse_golden.json: the reference's src/mcts.py with ONE MCTS object across a script of searches and
moves (tests/golden/make_mcts_reuse_golden.py), replayed with keep-searches and tafl_mcts_advance / tafl_gmcts_advance.  After every
search the root children (action, Nsa, Qsa bits), the probs at temp 1, the tree size (the reference's Es keys below the root) and, in
guided mode, the predict calls must match exactly; after every advance, the kept tree size."""
import json
import os

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflState
from tests import guided_util as gu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "mcts_reuse_golden.json")) as f:
    GOLD = json.load(f)
_LOGICS = {}


def _batch(case, G):
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    key = (case["rules"], case["side_len"], case["word_bits"])
    if key not in _LOGICS:
        _LOGICS[key] = BatchedGameLogic(abi.rules.BY_NAME[case["rules"]], case["side_len"], case["word_bits"])
    b = _LOGICS[key].new_batch(G)
    st = TaflState.from_buffer_copy(bytes.fromhex(case["state_hex"]))
    b.upload((TaflState * G)(*[st] * G))
    return b


def _kids(kids, cnt, g, width):
    return [[kids[g * width + j].action, kids[g * width + j].visits, float(kids[g * width + j].q).hex()] for j in range(cnt[g])]


def _probs(flat, g, A):
    row = np.frombuffer(flat, dtype=np.float64)[g * A:(g + 1) * A]
    return [[int(i), float(row[i]).hex()] for i in np.nonzero(row)[0]]


def _advance(b, step, games, slots, guided):
    if step["how"] == "best":
        acts = None
    else:
        acts = [step["action"] if g in slots else abi.ACTION_NONE for g in range(games)]
    plays, eff = (b.gmcts_advance if guided else b.mcts_advance)(acts)
    return plays, eff


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_rollout_scripts_match_the_reference(case):
    # the case's game sits in slot 1 (its global id is the case's game id), beside two other games (same position, other ids)
    G, slot, W = 3, 1, 256
    b = _batch(case, G)
    base = case["game_id"] - slot
    n, A = case["side_len"], abi.action_size(case["side_len"])
    for i, step in enumerate(case["steps"]):
        if step["op"] == "search":
            b.mcts_run(step["n_sims"], case["cpuct"], case["seed"], case["max_plies"], game_id_base=base, sim_offset=step["sim_offset"], keep=True)
            kids, cnt = b.mcts_root_children(W)
            got = _kids(kids, cnt, slot, W)
            assert got == step["root_children"], (case["name"], i)
            assert sum(k[1] for k in got) == step["root_ns"]
            assert b.mcts_tree_nodes()[slot] == step["subtree_states"], (case["name"], i)
            if step["probs_temp1_nonzero"]:
                assert _probs(b.mcts_policy(1.0), slot, A) == [list(x) for x in step["probs_temp1_nonzero"]]
            assert b.mcts_stats().faults == 0
        else:
            plays, eff = _advance(b, step, G, {slot}, guided=False)
            assert abi.action_encode(n, plays[slot]) == step["action"] and eff[slot].code == 0
            assert (eff[slot].status != abi.ONGOING) == step["ended"]
            # the reference has no entry for a child no search reached; the device's fresh root is one node without statistics
            assert b.mcts_tree_nodes()[slot] == max(1, step["kept_states"]), (case["name"], i)


@pytest.mark.parametrize("case", GOLD["guided_cases"], ids=[c["name"] for c in GOLD["guided_cases"]])
def test_guided_scripts_match_the_reference(case):
    G, W = 3, 600                                        # the case in every slot: every slot must match
    b = _batch(case, G)
    n, A = case["side_len"], abi.action_size(case["side_len"])
    salts = [case["salt"]] * G
    for i, step in enumerate(case["steps"]):
        if step["op"] == "search":
            S = step["n_sims"]
            b.gmcts_begin(S, 256, keep=True)
            w = b.gmcts_step(None, None, case["cpuct"], S)
            while w:
                pri, val = gu.stub_batch(*b.gmcts_leaves(), G, n, A, salts)
                w = b.gmcts_step(pri, val, case["cpuct"], S)
            kids, cnt = b.gmcts_root_children(W)
            probs = b.gmcts_policy(1.0)
            nodes = b.gmcts_tree_nodes()
            for g in range(G):
                assert _kids(kids, cnt, g, W) == step["root_children"], (case["name"], i, g)
                assert nodes[g] == step["subtree_states"], (case["name"], i, g)
                if step["probs_temp1_nonzero"]:
                    assert _probs(probs, g, A) == [list(x) for x in step["probs_temp1_nonzero"]]
            st = b.gmcts_stats()
            assert st.predicts == G * step["predict_calls"] and st.faults == 0, (case["name"], i)
        else:
            plays, eff = _advance(b, step, G, set(range(G)), guided=True)
            for g in range(G):
                assert abi.action_encode(n, plays[g]) == step["action"] and eff[g].code == 0
            assert list(b.gmcts_tree_nodes()) == [max(1, step["kept_states"])] * G, (case["name"], i)
