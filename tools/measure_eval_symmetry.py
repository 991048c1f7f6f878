#!/usr/bin/env python3
"""What a random board symmetry per leaf evaluation (include/taflhip.h tafl_eval_symmetry) costs the library's share
of a guided round on one MI355X: 65 536 Copenhagen 11x11 games, S simulations per root, a free evaluator (a constant float32 prior
tensor and zero values resident in HBM, as the engine-only mode of tools/measure_guided.py), so that the time of a round is
k_gmcts_step (or k_gmcts_step_sym) + k_gmcts_leaves and the host's two calls.

Each repetition times `--searches` whole searches (a host clock around work that ends in a stream synchronise: every step returns the
waiting count) after one untimed search that allocates the arena and loads the code objects.  `--modes off,on` alternates the setting
inside one process and one build, `--reps` times; `--modes off` runs on a build without the feature too, which is how the parent
commit's figure is taken.  Prints one JSON line per (repetition, mode) and, with --out, appends them to that file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--edges-per-node", type=int, default=192)
    ap.add_argument("--searches", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from alphazeroforhnefatafl_amd import BatchedGameLogic, GuidedMCTS, MCTSArgs, boards, rules
    if not torch.cuda.is_available():
        raise SystemExit("measure_eval_symmetry: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    n, side = args.games, 11
    lg = BatchedGameLogic(rules.COPENHAGEN, side)
    A = lg.action_size
    bt = torch.zeros((n, side, side), dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    wt = torch.zeros(n, dtype=torch.uint8, device=dev)
    bufs = (bt.data_ptr(), st.data_ptr(), wt.data_ptr())

    class Const:
        def __init__(self):
            torch.manual_seed(0)
            self.p = torch.rand((n, A), dtype=torch.float32, device=dev)
            self.v = torch.zeros(n, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()

        def predict_batch(self, *_):
            return self.p.data_ptr(), self.v.data_ptr()

    net = Const()
    b = lg.new_batch(n, boards.COPENHAGEN)
    modes = args.modes.split(",")

    def searcher(mode):
        a = MCTSArgs(numMCTSSims=args.sims, cpuct=1.0)
        if mode == "on":
            a.evalSymmetry, a.symmetrySeed = True, 0x5EED
        return GuidedMCTS(b, net, a, edges_per_node=args.edges_per_node, device=True, buffers=bufs)

    def one_search(m):
        b.reset_fen(boards.COPENHAGEN, rules.COPENHAGEN.starting_side)
        m.search_all()

    for mode in modes:                                           # untimed: the arena, the code objects of both kernel families
        one_search(searcher(mode))
    lg.sync(); torch.cuda.synchronize()
    for rep in range(args.reps):
        for mode in modes:
            m = searcher(mode)
            lg.sync(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.searches):
                one_search(m)
            lg.sync(); torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            s = b.gmcts_stats()                                  # (of the last search)
            row = {"label": args.label, "mode": mode, "rep": rep, "games": n, "sims_per_root": args.sims, "searches": args.searches, "seconds": round(dt, 4),
                   "rounds": m.rounds, "ms_per_round": round(1e3 * dt / max(1, m.rounds), 4), "predicts_last_search": s.predicts, "faults": s.faults}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
