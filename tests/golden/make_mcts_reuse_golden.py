#!/usr/bin/env python3
"""Generates tests/golden/mcts_reuse_golden.json by running the REFERENCE's own src/mcts.py across a script of moves.

Runs only in the build container (needs /root/reference; the output is data).  It reuses the adaptor of make_mcts_golden.py (game
methods on our CPU oracle, states keyed by their move path) with ONE `MCTS` object per case, kept across every step of its script, as an
alpha-zero-general episode keeps it: the Board path runs from the position the case starts at, so the root after move a has key "a", and
the tables (Qsa, Nsa, Ns, Ps, Es, Vs) persist.  Steps:
  search  n_sims [sim_offset]   getActionProb(root, temp=1) = n_sims more search(root) calls (a terminal root: the calls alone; the
                                reference's probs divide by zero there)
  advance best | unvisited | ending | a
                                the root becomes child (root, a): the most visited root child (first maximum), the lowest legal action
                                no search has taken yet, the lowest legal action that ends the game, or the action a
After every search: root Ns, root children (a, Nsa, Qsa.hex()), the nonzero probs at temp 1, predict calls during the search, and the
subtree size = the Es keys under the root's path (every state the searches reached below it, terminal or not).  After every advance: the
action and the kept subtree size.  Evaluators: RolloutNet (sim word = (sim_offset + state_hash) mod 2^32: include/taflhip.h "leaf key")
and StubNet (tests/stub_net.py).

Usage:  python tests/golden/make_mcts_reuse_golden.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_mcts_golden as mg  # noqa: E402  (imports the reference's src/mcts.py and the oracle)
from make_mcts_golden import Args, Board, StubNet, TaflGame, abi, orc, ref_mcts  # noqa: E402
from stub_net import matrix_bytes_of, stub_predict  # noqa: E402


class RolloutNet(mg.RolloutNet):
    """predict of the random-rollout mode with the run's sim_offset: one playout keyed by (seed, game id, sim_offset + leaf key)."""

    def __init__(self, game, seed, game_id, max_plies):
        super().__init__(game, seed, game_id, max_plies)
        self.sim_offset = 0
        self.calls = 0

    def predict(self, b):
        self.calls += 1
        sim = (self.sim_offset + self.game.logic.state_hash(b.state)) & 0xFFFFFFFF
        r = self.game.logic.rollout(b.state, self.seed, self.game_id, sim, self.max_plies)
        return np.ones(self.game.getActionSize(), dtype=np.float64), float(r.value)


CASES = [
    dict(name="brandubh_continue_then_moves", rules="brandubh", fen=abi.boards.BRANDUBH, side="starting", cpuct=1.0, seed=0, game_id=1,
         max_plies=256, script=[["search", 120], ["search", 80], ["advance", "best"], ["search", 200], ["advance", "best"], ["search", 200],
                                ["advance", "best"], ["search", 200], ["advance", "best"], ["search", 200]]),
    dict(name="copenhagen_midgame_300", rules="copenhagen", fen=None, advance=dict(seed=1, game_id=37, plies=37), side="starting", cpuct=1.0,
         seed=7, game_id=37, max_plies=512, script=[["search", 300], ["advance", "best"], ["search", 300], ["advance", "best"], ["search", 300],
                                                    ["advance", "best"], ["search", 300]]),
    dict(name="copenhagen_start_sim_offsets", rules="copenhagen", fen=abi.boards.COPENHAGEN, side="starting", cpuct=1.5, seed=2, game_id=5,
         max_plies=512, script=[["search", 64, 0], ["advance", "best"], ["search", 64, 64], ["advance", "best"], ["search", 96, 128]]),
    dict(name="copenhagen_unvisited_child", rules="copenhagen", fen=abi.boards.COPENHAGEN, side="starting", cpuct=1.0, seed=3, game_id=2,
         max_plies=512, script=[["search", 32], ["advance", "unvisited"], ["search", 48], ["advance", "best"], ["search", 48]]),
    dict(name="brandubh_move_ends_game", rules="brandubh", fen="7/7/3t3/2t4/7/6K/3t3", side="D", cpuct=1.0, seed=4, game_id=3,
         max_plies=128, script=[["search", 150], ["advance", "ending"], ["search", 20]]),
    dict(name="tablut_moves_150", rules="tablut", fen=abi.boards.TABLUT, side="starting", cpuct=1.0, seed=3, game_id=1, max_plies=300,
         script=[["search", 150], ["advance", "best"], ["search", 150], ["advance", "best"], ["search", 150]]),
    dict(name="copenhagen13_moves_48", rules="copenhagen", fen=abi.boards.COPENHAGEN13, side="starting", cpuct=1.0, seed=9, game_id=1,
         max_plies=256, script=[["search", 48], ["advance", "best"], ["search", 48], ["advance", "best"], ["search", 48]]),
]
GUIDED_CASES = [
    dict(name="guided_brandubh_continue_then_moves", rules="brandubh", fen=abi.boards.BRANDUBH, side="starting", cpuct=1.0, salt=1,
         script=[["search", 150], ["search", 100], ["advance", "best"], ["search", 200], ["advance", "best"], ["search", 200]]),
    dict(name="guided_copenhagen_midgame", rules="copenhagen", fen=None, advance=dict(seed=1, game_id=37, plies=37), side="starting",
         cpuct=2.5, salt=3, script=[["search", 150], ["advance", "best"], ["search", 150], ["advance", "best"], ["search", 150]]),
    dict(name="guided_copenhagen_unvisited", rules="copenhagen", fen=abi.boards.COPENHAGEN, side="starting", cpuct=1.0, salt=2,
         script=[["search", 40], ["advance", "unvisited"], ["search", 40]]),
    dict(name="guided_copenhagen13", rules="copenhagen", fen=abi.boards.COPENHAGEN13, side="starting", cpuct=1.0, salt=6,
         script=[["search", 60], ["advance", "best"], ["search", 60]]),
    dict(name="guided_masked_root", rules="brandubh", fen=abi.boards.BRANDUBH, side="starting", cpuct=1.0, salt=None,
         script=[["search", 90], ["advance", "best"], ["search", 90]]),
]


def start_state(c):
    rules = abi.rules.BY_NAME[c["rules"]]
    side = rules.starting_side if c["side"] == "starting" else (abi.ATTACKER if c["side"] == "A" else abi.DEFENDER)
    fen = c["fen"] or abi.boards.COPENHAGEN
    n = abi.fen_side_len(fen)
    wb = abi.word_bits_for(n)
    logic = orc.GameLogic(rules, n)
    st = orc.GameState(fen, side, wb)
    if c.get("advance"):
        a = c["advance"]
        st = logic.random_advance(st, a["seed"], a["game_id"], a["plies"])
    return logic, st, n, wb


def subtree(m, key):
    return sum(1 for s in m.Es if s == key or (key == "" and s != "") or s.startswith(key + ","))


def play_script(c, game, net, m, root):
    steps = []
    A = game.getActionSize()
    for step in c["script"]:
        s = game.stringRepresentation(root)
        if step[0] == "search":
            n_sims = step[1]
            if isinstance(net, RolloutNet):
                net.sim_offset = step[2] if len(step) > 2 else 0
            calls0 = net.calls
            m.args.numMCTSSims = n_sims
            if game.getGameEnded(root, 1) != 0:
                for _ in range(n_sims):
                    m.search(root)
                probs = []
            else:
                probs = m.getActionProb(root, temp=1)
            kids = [[a, int(m.Nsa[(s, a)]), float(m.Qsa[(s, a)]).hex()] for a in range(A) if (s, a) in m.Nsa]
            steps.append(dict(op="search", n_sims=n_sims, sim_offset=step[2] if len(step) > 2 else 0, root_ns=int(m.Ns.get(s, 0)),
                              root_children=kids, probs_temp1_nonzero=[(i, float(p).hex()) for i, p in enumerate(probs) if p != 0],
                              predict_calls=net.calls - calls0, subtree_states=subtree(m, s)))
        else:
            how = step[1]
            if how == "best":
                counts = [m.Nsa[(s, a)] if (s, a) in m.Nsa else 0 for a in range(A)]
                a = int(np.argmax(counts))
            elif how == "ending":                              # the lowest legal action that ends the game
                valid = game.getValidMoves(root, 1)
                a = next(x for x in range(A) if valid[x] and game.getGameEnded(game.getNextState(root, 1, x)[0], 1) != 0)
            elif how == "unvisited":
                valid = game.getValidMoves(root, 1)
                a = next(x for x in range(A) if valid[x] and (s, x) not in m.Nsa)
            else:
                a = int(how)
            root, _ = game.getNextState(root, 1, a)
            steps.append(dict(op="advance", how=how, action=a, kept_states=subtree(m, game.stringRepresentation(root)),
                              ended=bool(game.getGameEnded(root, 1) != 0)))
    return steps


def run_case(c):
    logic, st, n, wb = start_state(c)
    game = TaflGame(logic, n)
    net = RolloutNet(game, c["seed"], c["game_id"], c["max_plies"])
    m = ref_mcts.MCTS(game, net, Args(1, c["cpuct"]))
    out = dict(c)
    out.update(fen=st.to_fen(), side_to_play=int(st.side_to_play), state_hex=bytes(st.to_abi()).hex(), word_bits=wb, side_len=n,
               steps=play_script(c, game, net, m, Board(st, ())))
    return out


def run_guided_case(c):
    logic, st, n, wb = start_state(c)
    game = TaflGame(logic, n)
    salt = c["salt"]
    if salt is None:      # a salt for which the ROOT gets all-zero priors: the workaround branch at the root (mcts.py:91-98)
        mb = matrix_bytes_of(st.board_to_matrix())
        salt = next(x for x in range(256) if not stub_predict(mb, int(st.side_to_play), game.getActionSize(), x)[0].any())
    net = StubNet(game, salt)
    m = ref_mcts.MCTS(game, net, Args(1, c["cpuct"]))
    out = dict(c)
    out.update(salt=salt, fen=st.to_fen(), side_to_play=int(st.side_to_play), state_hex=bytes(st.to_abi()).hex(), word_bits=wb, side_len=n,
               steps=play_script(c, game, net, m, Board(st, ())))
    return out


def main():
    res = dict(_comment="Generated by tests/golden/make_mcts_reuse_golden.py: the reference's src/mcts.py with ONE MCTS object per case "
                        "across a script of searches and moves (states keyed by their move path from the case's start). Qsa/probs are float.hex().",
               cases=[run_case(c) for c in CASES], guided_cases=[run_guided_case(c) for c in GUIDED_CASES])
    with open(os.path.join(HERE, "mcts_reuse_golden.json"), "w") as f:
        json.dump(res, f, separators=(",", ":"))
    for c in res["cases"] + res["guided_cases"]:
        print(c["name"], [(s["op"], s.get("subtree_states", s.get("kept_states")), s.get("ended", "")) for s in c["steps"]])


if __name__ == "__main__":
    main()
