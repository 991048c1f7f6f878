"""Self-play that records training examples (tafl_selfplay_record / tafl_examples_gather): what recording costs and how fast minibatches
are served.

65 536 Copenhagen games from the start position, S = 64, cap 512, 8 moves per run:
  * tafl_selfplay_run (untouched by the feature: the baseline) against tafl_selfplay_record with K = 64 and temp_moves = 0 (same
    positions, so the two lines compare) and temp_moves = 8 (other positions: quoted on its own); whole-call wall time and the union of
    the tree / playout kernel times (HIP events), one warm-up, `--repeats` timed runs, min..max;
  * the host loop the recording run replaces (mcts_run + mcts_policy_device + encode_boards + tafl_step per move, dense float64 pi left
    on the device), for the record;
  * k_examples_gather with device pointers: HIP events around each launch, one warm-up, `--launches` timed launches, min..max, for 4 096
    and 65 536 rows with identity and mixed symmetries, against bytes written / the achievable HBM bandwidth (6.3 TB/s).

    python tools/measure_examples.py [--games 65536] [--moves 8] [--repeats 3] [--launches 10] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alphazeroforhnefatafl_amd import abi  # noqa: E402
from alphazeroforhnefatafl_amd._lib import check, lib  # noqa: E402
from alphazeroforhnefatafl_amd.engine import KC_MCTS_ROLLOUT, KC_MCTS_TREE, BatchedGameLogic  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def timed_runs(lg, fen, G, S, cap, moves, repeats, fn):
    """Wall time of `repeats` runs after one warm-up (event timing off), then one more run with the library's HIP-event spans on: the
    time with at least one tree / playout kernel in flight."""
    wall = []
    for r in range(repeats + 1):
        b = lg.new_batch(G, fen)
        lg.sync()
        t0 = time.perf_counter()
        fn(b)
        lg.sync()
        dt = time.perf_counter() - t0
        sims = b.mcts_stats().sims
        b.close()
        if r:                                                   # the first run warms up
            wall.append(dt)
    b = lg.new_batch(G, fen)
    lg.sync()
    lg.timing_enable(True)
    lg.timing_reset()
    fn(b)
    lg.sync()
    tu, _ = lg.timing_get_union(KC_MCTS_TREE)
    ru, _ = lg.timing_get_union(KC_MCTS_ROLLOUT)
    lg.timing_enable(False)
    b.close()
    return {"sims": int(sims), "wall_ms": [1e3 * min(wall), 1e3 * max(wall)], "ms_per_move": [1e3 * min(wall) / moves, 1e3 * max(wall) / moves],
            "msims_per_s": [sims / max(wall) / 1e6, sims / min(wall) / 1e6], "tree_union_ms": tu, "playout_union_ms": ru}


def host_loop(lg, fen, G, S, cap, moves, repeats, torch):
    A, n = lg.action_size, lg.side_len
    pi = torch.empty((G, A), dtype=torch.float64, device="cuda:0")
    boards = torch.empty((G, n, n), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    wall = []
    for r in range(repeats + 1):
        b = lg.new_batch(G, fen)
        lg.sync()
        t0 = time.perf_counter()
        for m in range(moves):
            b.mcts_run(S, 1.0, 2, cap, sim_offset=m * S)
            b.mcts_policy_device(1.0, pi.data_ptr())
            b.encode_boards(boards.data_ptr())
            plays, _ = b.mcts_best_play()                       # the host chooses (here: the most visited play) and steps
            b.do_play(plays, want_effects=False)
        lg.sync()
        if r:
            wall.append(time.perf_counter() - t0)
        b.close()
    return {"wall_ms": [1e3 * min(wall), 1e3 * max(wall)], "ms_per_move": [1e3 * min(wall) / moves, 1e3 * max(wall) / moves]}


def gather_rates(lg, ex, G, moves, launches, torch):
    A, n = lg.action_size, lg.side_len
    out = []
    rng = np.random.default_rng(1)
    for rows in (4096, 65536):
        idx = torch.from_numpy((rng.integers(0, moves, rows) * G + rng.integers(0, G, rows)).astype(np.int32)).cuda()
        boards = torch.empty((rows, n, n), dtype=torch.uint8, device="cuda:0")
        sides = torch.empty(rows, dtype=torch.uint8, device="cuda:0")
        pi = torch.empty((rows, A), dtype=torch.float32, device="cuda:0")
        z = torch.empty(rows, dtype=torch.float32, device="cuda:0")
        fin = torch.empty(rows, dtype=torch.uint8, device="cuda:0")
        for label, sym in (("identity", None), ("mixed", torch.from_numpy(rng.integers(0, 8, rows).astype(np.uint8)).cuda())):
            torch.cuda.synchronize()
            stream = torch.cuda.ExternalStream(lib().tafl_ctx_stream(lg._h))
            us = []
            for k in range(launches + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                check(lib().tafl_examples_gather(ex._h, C.c_void_p(idx.data_ptr()), C.c_void_p(sym.data_ptr()) if sym is not None else None, rows,
                                                 C.c_void_p(boards.data_ptr()), C.c_void_p(sides.data_ptr()), C.c_void_p(pi.data_ptr()),
                                                 C.c_void_p(z.data_ptr()), C.c_void_p(fin.data_ptr()), 1))
                e1.record(stream)
                e1.synchronize()
                if k:
                    us.append(1e3 * e0.elapsed_time(e1))
            written = rows * (4 * A + n * n + 6)
            out.append({"rows": rows, "sym": label, "us": [min(us), max(us)], "bytes_written": written,
                        "gb_per_s": [written / max(us) / 1e3, written / min(us) / 1e3],
                        "fraction_of_hbm": [written / (max(us) * 1e-6) / HBM_ACHIEVABLE, written / (min(us) * 1e-6) / HBM_ACHIEVABLE]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--moves", type=int, default=8)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--cap", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    G, S, cap, moves = a.games, a.sims, a.cap, a.moves
    lg = BatchedGameLogic(abi.rules.COPENHAGEN, 11, 128)
    fen = abi.boards.COPENHAGEN
    res = {"games": G, "sims": S, "cap": cap, "moves": moves}
    res["selfplay_run"] = timed_runs(lg, fen, G, S, cap, moves, a.repeats, lambda b: b.selfplay_run(moves, S, 1.0, 2, cap, want_plays=False))
    ex = lg.new_examples(G, moves, 64)

    def rec(temp):
        def f(b):
            ex.clear()
            b.selfplay_record(ex, moves, S, 1.0, 2, cap, sample_seed=11, temp_moves=temp, want_plays=False)
        return f
    res["record_temp0"] = timed_runs(lg, fen, G, S, cap, moves, a.repeats, rec(0))
    res["record_temp8"] = timed_runs(lg, fen, G, S, cap, moves, a.repeats, rec(moves))
    res["examples_device_bytes"] = int(ex.stats().device_bytes)
    res["examples_total"] = int(ex.counts()[1])
    res["host_loop"] = host_loop(lg, fen, G, S, cap, moves, a.repeats, torch)
    res["gather"] = gather_rates(lg, ex, G, moves, a.launches, torch)
    for k, v in res.items():
        print(k, json.dumps(v))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
