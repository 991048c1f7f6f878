"""Subtree reuse (TAFL_MCTS_FLAG_KEEP_TREE): how much of a search survives into the next one, and what it costs.

An 8-move loop over 65 536 Copenhagen games from the start position: search, then the most visited play - with keep (tafl_mcts_advance
+ keep-search) and without (tafl_mcts_play_best + fresh search).  Rollout mode at S = 64 and S = 256; guided mode with a free evaluator
(device-resident random priors, value 0: the network costs nothing, so the numbers are the engine's own).  Per configuration: sims/s of
the searches, the time of the move step per move (advance + re-root with keep; play_best or tafl_step without), kept nodes per move
(mean / p50 / max over games), playouts consumed or predicts per move, and the device memory the batch holds.  One warm-up loop,
then `--repeats` timed loops; the spread is min..max of the loops' sims/s.

    python tools/measure_reuse.py [--games 65536] [--moves 8] [--repeats 2] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alphazeroforhnefatafl_amd import abi  # noqa: E402
from alphazeroforhnefatafl_amd.abi import TaflPlay  # noqa: E402


def loop_rollout(lg, fen, G, S, moves, keep):
    b = lg.new_batch(G, fen)
    t_search, t_move, sims, playouts, kept = 0.0, 0.0, 0, [], []
    for m in range(moves):
        t0 = time.perf_counter()
        b.mcts_run(S, 1.0, 1, 512, sim_offset=m * S, keep=keep)
        t_search += time.perf_counter() - t0
        st = b.mcts_stats()
        sims += st.sims
        playouts.append(st.rollouts)
        t0 = time.perf_counter()
        if keep:
            b.mcts_advance(None, want_results=False)           # (synchronises: it reads back its consistency check)
        else:
            b.mcts_play_best(want_results=False)
            b.logic.sync()
        t_move += time.perf_counter() - t0
        if keep:
            kept.append(np.frombuffer(b.mcts_tree_nodes(), dtype=np.uint32).astype(np.int64) - 1)   # (the kept root itself not counted)
    return b, sims / t_search, playouts, kept, 1e3 * t_move / moves


def loop_guided(lg, fen, G, S, moves, keep, torch):
    A, side = lg.action_size, lg.side_len
    dev = torch.device("cuda:0")
    bt = torch.empty((G, side, side), dtype=torch.uint8, device=dev)
    st_ = torch.empty(G, dtype=torch.uint8, device=dev)
    wt = torch.empty(G, dtype=torch.uint8, device=dev)
    pri = torch.rand((G, A), dtype=torch.float32, device=dev)
    val = torch.zeros(G, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b = lg.new_batch(G, fen)
    t_search, t_move, sims, predicts, kept = 0.0, 0.0, 0, [], []
    for m in range(moves):
        t0 = time.perf_counter()
        b.gmcts_begin(S, 256, keep=keep)
        w = b.gmcts_step(None, None, 1.0, S)
        while w:
            b.gmcts_leaves(bt.data_ptr(), st_.data_ptr(), wt.data_ptr())
            w = b.gmcts_step(pri.data_ptr(), val.data_ptr(), 1.0, S, device=True)
        t_search += time.perf_counter() - t0
        gs = b.gmcts_stats()
        sims += gs.sims
        predicts.append(gs.predicts)
        t0 = time.perf_counter()
        if keep:
            b.gmcts_advance(None, want_results=False)
        else:
            # a loop without reuse, as a host runs it today: the most visited play (first maximum of the root visits) with tafl_step
            v = np.frombuffer(b.gmcts_root_visits(), dtype=np.uint32).reshape(G, A)
            b.do_play((TaflPlay * G)(*[abi.action_decode(side, int(x)) for x in v.argmax(axis=1)]), want_effects=False)
        t_move += time.perf_counter() - t0
        if keep:
            kept.append(np.frombuffer(b.gmcts_tree_nodes(), dtype=np.uint32).astype(np.int64) - 1)
    return b, sims / t_search, predicts, kept, 1e3 * t_move / moves


def summary(kept):
    if not kept:
        return None
    k = np.concatenate(kept)
    return {"mean": round(float(k.mean()), 2), "p50": float(np.median(k)), "max": int(k.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--moves", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from alphazeroforhnefatafl_amd import BatchedGameLogic, boards, rules
    lg = BatchedGameLogic(rules.COPENHAGEN, 11, 128)
    fen, G = boards.COPENHAGEN, a.games
    rows = []
    for mode, S in (("rollout", 64), ("rollout", 256), ("guided", 64)):
        for keep in (False, True):
            runs = []
            for rep in range(a.repeats + 1):                    # repeat 0 warms up
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                if mode == "rollout":
                    b, rate, per_move, kept, move_ms = loop_rollout(lg, fen, G, S, a.moves, keep)
                else:
                    b, rate, per_move, kept, move_ms = loop_guided(lg, fen, G, S, a.moves, keep, torch)
                held = free0 - torch.cuda.mem_get_info()[0]
                b.close()
                if rep:
                    runs.append((rate, per_move, kept, held, move_ms))
            rates = [r[0] for r in runs]
            row = {"mode": mode, "S": S, "keep": keep, "games": G, "moves": a.moves,
                   "sims_per_s_M": round(float(np.median(rates)) / 1e6, 2), "spread_M": [round(min(rates) / 1e6, 2), round(max(rates) / 1e6, 2)],
                   ("playouts_per_move" if mode == "rollout" else "predicts_per_move"): runs[-1][1],
                   "kept_nodes_per_move": summary(runs[-1][2]), "device_bytes_held": int(runs[-1][3]),
                   "move_ms": round(float(np.median([r[4] for r in runs])), 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
