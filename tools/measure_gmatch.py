#!/usr/bin/env python3
"""Match play on one MI355X (tafl_gmatch_*): 65 536 Copenhagen 11x11 lanes from the openings of section 15's
measurement (the start position advanced by (7 g) mod 500 random plies, seed 21), S = 64 simulations per move, a lane budget of 32 moves,
one warm-up and `--runs` timed runs per route, in one process.

  A  match       gmatch_begin; { gmatch_leaves; evaluator e on its own count_e rows (rounded up to --row-multiple); gmatch_step } with
                 device pointers: what this library now offers.
  B  both_full   what the parent commit allows without a per-round download: gselfplay_begin_episodes; { gmcts_leaves; BOTH evaluators on
                 the full batch; torch.where blends the rows by a FIXED mask (lane parity); gselfplay_step }.  That mask is not the true
                 owner - the host cannot know the owner without downloading the states - so B's games are not a match: B is a lower
                 bound on the parent's cost per round, not a result.

with two evaluator pairs: two constant-prior evaluators resident in HBM (what the library costs per round) and two instances of the fp16
conv network of tools/measure_gselfplay.py with different weights.  One JSON line per (pair, route): min..max seconds, rounds, the mean
rows per network call, the device time per round of the leaves call(s) and of the step from events on the library's stream, and for
route A the tally.  The time of the partition and plane kernels comes from a trace of its own:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/measure_gmatch.py --no-conv --runs 1 --routes A
(the rows k_gmatch_rank, k_gmatch_place, k_gmatch_leaves of OUT/*_kernel_stats.csv: total time / calls)."""
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
    ap.add_argument("--moves", type=int, default=32, help="the lane budget")
    ap.add_argument("--edges-per-node", type=int, default=256)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spread", type=int, default=500)
    ap.add_argument("--row-multiple", type=int, default=32768, help="route A: a network sees its rows rounded up to this; every distinct shape costs the conv "
                    "library a kernel search of its own (minutes in all at 4096), so the default leaves two: half the batch and all of it")
    ap.add_argument("--routes", default="AB")
    ap.add_argument("--no-conv", action="store_true", help="only the constant-prior pair")
    ap.add_argument("--no-const", action="store_true", help="only the conv pair")
    args = ap.parse_args()
    import numpy as np
    import torch
    from alphazeroforhnefatafl_amd import BatchedGameLogic, abi, boards, rules
    from alphazeroforhnefatafl_amd._lib import lib
    dev = torch.device("cuda:0")
    n, side, S, moves, epn, mult = args.games, 11, args.sims, args.moves, args.edges_per_node, args.row_multiple
    lg = BatchedGameLogic(rules.COPENHAGEN, side)
    A = lg.action_size
    stream = torch.cuda.ExternalStream(lib().tafl_ctx_stream(lg._h))
    # evaluator e's dense batch (route A); route B uses evaluator 0's buffers as the full batch
    bufs = [(torch.zeros((n, side, side), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
             torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(2)]
    ptrs = [tuple(t.data_ptr() for t in bufs[e]) + (n,) for e in range(2)]
    parity = (torch.arange(n, device=dev) & 1).bool()

    class Const:
        def __init__(self, e):
            torch.manual_seed(10 + e)
            self.p = torch.rand((n, A), dtype=torch.float32, device=dev)
            self.v = torch.full((n,), 0.25 - 0.5 * e, dtype=torch.float32, device=dev)

        def predict(self, boards_t, sides_t):
            m = boards_t.shape[0]
            return self.p[:m], self.v[:m]

    class Conv:
        def __init__(self, e):
            torch.manual_seed(e)
            c = args.channels
            self.body = torch.nn.Sequential(torch.nn.Conv2d(2, c, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(c, c, 3, padding=1), torch.nn.ReLU(),
                                            torch.nn.Conv2d(c, 20, 1)).to(dev).eval().half()
            self.vhead = torch.nn.Linear(20 * side * side, 1).to(dev).eval().half()

        def predict(self, boards_t, sides_t):
            m = boards_t.shape[0]
            with torch.no_grad():
                x = torch.stack([boards_t.half() / 35.0, (sides_t.half() / 8.0)[:, None, None].expand(-1, side, side)], 1)
                y = self.body(x)                                   # [m, 20, 11, 11]: one logit per (tile, slot) = the action layout
                p = torch.softmax(y.permute(0, 2, 3, 1).reshape(m, A).float(), 1).contiguous()
                v = torch.tanh(self.vhead(y.reshape(m, -1))).float().reshape(m).contiguous()
            return p, v

    class Rounds:
        def __init__(self):
            self.rounds, self.calls, self.rows, self.pairs = 0, 0, 0, {"leaves": [], "step": []}

        def timed(self, what, fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            out = fn()
            b.record(stream)
            self.pairs[what].append((a, b))
            return out

        def ms(self, what):
            torch.cuda.synchronize()
            return sum(a.elapsed_time(b) for a, b in self.pairs[what])

    def route_a(b, nets, r):
        b.clear_root_noise()
        b.gmatch_begin(None, moves, S, 1.0, epn, sample_seed=1)
        keep = None
        while True:
            counts = r.timed("leaves", lambda: b.gmatch_leaves(ptrs))
            if not (counts[0] or counts[1]):
                break
            r.rounds += 1
            pp, vv, keep = [None, None], [None, None], []
            for e in range(2):
                if counts[e]:
                    m = min(n, -(-counts[e] // mult) * mult)
                    p, v = nets[e].predict(bufs[e][0][:m], bufs[e][1][:m])
                    keep.append((p, v))
                    pp[e], vv[e] = p.data_ptr(), v.data_ptr()
                    r.calls += 1; r.rows += m
            torch.cuda.synchronize()
            r.timed("step", lambda: b.gmatch_step(pp, vv, device=True))
        b.gselfplay_end(want_plays=False)
        return b.gmcts_stats().sims

    def route_b(b, nets, r):
        b.clear_root_noise()
        b.gselfplay_begin_episodes(None, moves, S, 1.0, epn, sample_seed=1)
        w = b.gselfplay_step()
        full = ptrs[0][:3]
        while w:
            r.rounds += 1
            r.timed("leaves", lambda: b.gmcts_leaves(*full))
            p0, v0 = nets[0].predict(bufs[0][0], bufs[0][1])
            p1, v1 = nets[1].predict(bufs[0][0], bufs[0][1])
            p = torch.where(parity[:, None], p1, p0)
            v = torch.where(parity, v1, v0)
            r.calls += 2; r.rows += 2 * n
            torch.cuda.synchronize()
            w = r.timed("step", lambda: b.gselfplay_step(p.data_ptr(), v.data_ptr(), device=True))
        b.gselfplay_end(want_plays=False)
        return b.gmcts_stats().sims

    plies = (C.c_uint32 * n)(*[(7 * g) % args.spread for g in range(n)])
    start = lg.new_batch(n, boards.COPENHAGEN)
    start.random_advance(21, plies, 0)
    openings = start.download()
    over0 = int(np.count_nonzero(np.frombuffer(openings, np.uint8).reshape(n, C.sizeof(abi.TaflState))[:, abi.TaflState.status.offset]))
    start.close()
    pairs = ([] if args.no_const else [("constant_priors", [Const(0), Const(1)])]) + ([] if args.no_conv else [("torch_conv_fp16", [Conv(0), Conv(1)])])
    for name, nets in pairs:
        for m in sorted({min(n, k * mult) for k in range(1, -(-n // mult) + 1)} | {n}):      # kernel selection of every shape the routes use
            for net in nets:
                net.predict(bufs[0][0][:m], bufs[0][1][:m])
            torch.cuda.synchronize()
            print(f"{name}: warmed {m} rows", file=sys.stderr, flush=True)
        for route, fn in (("A_match", route_a), ("B_both_full", route_b)):
            if route[0] not in args.routes:
                continue
            b = lg.new_batch(n)
            secs, last = [], None
            for i in range(1 + args.runs):                           # (the first run allocates the arena and is not reported)
                b.upload(openings)
                r = Rounds()
                lg.sync(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                sims = fn(b, nets, r)
                lg.sync(); torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if i:
                    secs.append(dt)
                last = (sims, r)
                print(f"{name} {route} run {i}: {dt:.3f} s, {r.rounds} rounds", file=sys.stderr, flush=True)
            sims, r = last
            eps, est = b.gselfplay_episode_stats()
            line = {"evaluators": name, "route": route, "lanes": n, "lanes_over_at_the_start": over0, "spread": args.spread, "sims_per_move": S, "lane_budget": moves,
                    "edges_per_node": epn, "row_multiple": mult if route[0] == "A" else None, "seconds_min": round(min(secs), 3), "seconds_max": round(max(secs), 3),
                    "sims": sims, "rounds": r.rounds, "network_calls": r.calls, "rows_per_network_call": r.rows / max(1, r.calls),
                    "rows_per_round": r.rows / max(1, r.rounds), "leaves_ms_per_round": r.ms("leaves") / max(1, r.rounds), "step_ms_per_round": r.ms("step") / max(1, r.rounds),
                    "episodes_closed_or_cut": int(sum(eps)), "attacker_wins": est.attacker_wins, "defender_wins": est.defender_wins, "draws": est.draws, "cut": est.cut}
            if route[0] == "A":
                line["games"] = [[int(x) for x in row] for row in b.gmatch_stats().games]
            else:
                line["note"] = "the blend mask is lane parity, not the owner: these games are not a match; a lower bound on the parent's cost per round"
            print(json.dumps(line), flush=True)
            b.close()


if __name__ == "__main__":
    main()
