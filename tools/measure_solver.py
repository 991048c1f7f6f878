#!/usr/bin/env python3
"""Exact win/loss proofs in guided self-play on one MI355X (tafl_gselfplay_set_solver): 65 536 lanes of Brandubh
moved to mixed late positions with tafl_random_advance (lane g: (7 g) mod `--spread` random plies, the lanes whose game that ends stay
idle), one episodes run of `--moves` moves per lane at S = 64 with a free evaluator (constant priors, value 0), timed with the setting
off and on in one process.  Off is the yardstick: it launches k_gselfplay_episodes, whose resource usage is the parent commit's.

One warm-up and `--runs` timed runs per setting.  Per setting one record with the min..max over the runs of: the step kernels' device
time per round (HIP events on the library's stream), rounds a lane waits per move it makes (the sum over the rounds of the lanes that
wait for the evaluator, by the moves made: the evaluator rows a move costs), wall seconds; and the rounds of the run, the simulations
run, skipped and the eight counters of the last run.  (The rounds of a run are set by its slowest lane, and every round evaluates the
whole batch, so they fall only when every lane saves simulations.)  `--spread 5 --moves 2` gives opening positions, where nothing is
proven and both settings do the same work: the like-for-like cost of the solver kernel.  The records are printed and written as one JSON document to `--out`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--moves", type=int, default=8)
    ap.add_argument("--edges-per-node", type=int, default=128)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--spread", type=int, default=60)
    ap.add_argument("--commit", default="", help="written into the document")
    ap.add_argument("--out", default="", help="where the JSON document goes (nothing is written without it)")
    args = ap.parse_args()
    import torch
    from alphazeroforhnefatafl_amd import BatchedGameLogic, boards, rules
    from alphazeroforhnefatafl_amd._lib import lib
    dev = torch.device("cuda:0")
    n, side, S, moves, epn = args.games, 7, args.sims, args.moves, args.edges_per_node
    lg = BatchedGameLogic(rules.BRANDUBH, side)
    A = lg.action_size
    stream = torch.cuda.ExternalStream(lib().tafl_ctx_stream(lg._h))
    bt = torch.empty((n, side, side), dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    wt = torch.empty(n, dtype=torch.uint8, device=dev)
    bufs = (bt.data_ptr(), st.data_ptr(), wt.data_ptr())
    torch.manual_seed(0)
    p = torch.rand((n, A), dtype=torch.float32, device=dev)
    v = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    plies = (C.c_uint32 * n)(*[(7 * g) % args.spread for g in range(n)])
    start = lg.new_batch(n, boards.BRANDUBH)
    start.random_advance(21, plies, 0)
    openings = start.download()
    start.close()
    doc = {"lanes": n, "board": "brandubh7", "spread": args.spread, "sims_per_move": S, "lane_budget": moves, "edges_per_node": epn, "runs": args.runs,
           "evaluator": "constant_priors", "commit": args.commit, "settings": []}
    for name, on in (("off", False), ("on", True)):
        b = lg.new_batch(n)
        ms_round, rounds_move, secs, last = [], [], [], None
        for i in range(1 + args.runs):
            b.upload(openings)
            bt.zero_(); st.zero_(); wt.zero_()
            if on:
                b.set_solver()
            else:
                b.clear_solver()
            rounds, waiting, pairs = 0, 0, []
            lg.sync(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.gselfplay_begin_episodes(None, moves, S, 1.0, epn, sample_seed=1)
            w = b.gselfplay_step()
            while w:
                rounds += 1; waiting += w
                b.gmcts_leaves(*bufs)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                w = b.gselfplay_step(p.data_ptr(), v.data_ptr(), device=True)
                e1.record(stream)
                pairs.append((e0, e1))
            _plays, made = b.gselfplay_end(want_plays=False)
            lg.sync(); torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            made = int(sum(made))
            if i:
                ms_round.append(sum(a.elapsed_time(c) for a, c in pairs) / max(1, rounds))
                rounds_move.append(waiting / max(1, made))
                secs.append(dt)
            last = (b.gmcts_stats(), rounds, made)
        gs, rounds, made = last
        rec = {"setting": name, "rounds": rounds, "moves": made, "sims": gs.sims, "faults": gs.faults,
               "step_ms_per_round_min": min(ms_round), "step_ms_per_round_max": max(ms_round),
               "waiting_rounds_per_move_min": min(rounds_move), "waiting_rounds_per_move_max": max(rounds_move),
               "seconds_min": min(secs), "seconds_max": max(secs), "sims_per_move": gs.sims / max(1, made)}
        if on:
            ss = b.solver_stats()
            rec.update({k: getattr(ss, k) for k in ("root_won", "root_lost", "skipped_sims", "nodes_won", "nodes_lost", "pruned_visits", "pruned_children", "moves")})
            rec["skipped_fraction"] = ss.skipped_sims / max(1, gs.sims + ss.skipped_sims)
        doc["settings"].append(rec)
        print(json.dumps(rec), flush=True)
        b.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
