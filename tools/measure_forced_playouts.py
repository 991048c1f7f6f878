#!/usr/bin/env python3
"""Forced playouts with policy target pruning in guided self-play on one MI355X (tafl_gselfplay_set_forced_playouts, DESIGN.md section
18): the workload of tools/measure_playout_cap.py - 65 536 lanes of 11x11 Copenhagen from openings spread over the game, a lane budget of
`--moves` moves, S simulations per full move, recording into an examples object, constant priors and a small fp16 conv network - timed
four ways in one process:

  off             no setting: the kernels a run launched before (the yardstick of what the forced kernel costs)
  cap_on          the playout cap of section 17 alone (fast_sims = `--fast`, full_per_65536 = `--full-per`)
  forced          k = `--k` with root noise 0.3 / 0.25, no cap
  forced+cap_on   both, with the same noise

One warm-up and `--runs` timed runs per line; one JSON line each with rounds, min..max seconds, evaluations, moves and recorded examples
per second, the mean fraction of the lanes that wait per round, the step's device time per round from events on the library's stream,
and for the forced lines the four counters with their shares: forced simulations per full-move simulation, pruned visits per recorded
visit, children pruned per example."""
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
    ap.add_argument("--fast", type=int, default=16)
    ap.add_argument("--full-per", type=int, default=16384)
    ap.add_argument("--k", type=float, default=2.0)
    ap.add_argument("--commit", default="", help="written into every line")
    ap.add_argument("--moves", type=int, default=32)
    ap.add_argument("--edges-per-node", type=int, default=256)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spread", type=int, default=500, help="lane g starts from the start position advanced by (7 g) mod SPREAD random plies")
    ap.add_argument("--no-conv", action="store_true", help="only the constant-prior evaluator")
    args = ap.parse_args()
    import torch
    from alphazeroforhnefatafl_amd import BatchedGameLogic, boards, rules
    from alphazeroforhnefatafl_amd._lib import lib
    dev = torch.device("cuda:0")
    n, side, S, moves, epn = args.games, 11, args.sims, args.moves, args.edges_per_node
    lg = BatchedGameLogic(rules.COPENHAGEN, side)
    A = lg.action_size
    stream = torch.cuda.ExternalStream(lib().tafl_ctx_stream(lg._h))
    bt = torch.empty((n, side, side), dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    wt = torch.empty(n, dtype=torch.uint8, device=dev)
    bufs = (bt.data_ptr(), st.data_ptr(), wt.data_ptr())

    class Const:
        def __init__(self):
            self.p = torch.rand((n, A), dtype=torch.float32, device=dev)
            self.v = torch.zeros(n, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()

        def predict_batch(self, *_):
            return self.p.data_ptr(), self.v.data_ptr()

    class Conv:
        def __init__(self):
            torch.manual_seed(0)
            c = args.channels
            self.body = torch.nn.Sequential(torch.nn.Conv2d(2, c, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(c, c, 3, padding=1), torch.nn.ReLU(),
                                            torch.nn.Conv2d(c, 20, 1)).to(dev).eval().half()
            self.vhead = torch.nn.Linear(20 * side * side, 1).to(dev).eval().half()
            self.keep = None

        def predict_batch(self, *_):
            with torch.no_grad():
                x = torch.stack([bt.half() / 35.0, (st.half() / 8.0)[:, None, None].expand(-1, side, side)], 1)
                y = self.body(x)
                p = torch.softmax(y.permute(0, 2, 3, 1).reshape(n, A).float(), 1).contiguous()
                v = torch.tanh(self.vhead(y.reshape(n, -1))).float().reshape(n).contiguous()
            torch.cuda.synchronize()
            self.keep = (p, v)
            return p.data_ptr(), v.data_ptr()

    plies = (C.c_uint32 * n)(*[(7 * g) % args.spread for g in range(n)])
    start = lg.new_batch(n, boards.COPENHAGEN)
    start.random_advance(21, plies, 0)
    openings = start.download()
    start.close()
    ex = lg.new_examples(n, moves, S)
    routes = (("off", None, 0.0), ("cap_on", args.full_per, 0.0), ("forced", None, args.k), ("forced+cap_on", args.full_per, args.k))
    nets = [("constant_priors", Const())] + ([] if args.no_conv else [("torch_conv_fp16", Conv())])
    for name, net in nets:
        for _ in range(3):
            net.predict_batch()
        for route, full_per, k in routes:
            b = lg.new_batch(n)
            secs, last = [], None
            for i in range(1 + args.runs):
                b.upload(openings)
                ex.clear()
                bt.zero_(); st.zero_(); wt.zero_()
                if k:
                    b.set_root_noise(0.3, 0.25, 7)
                    b.set_forced_playouts(k)
                else:
                    b.clear_root_noise()
                    b.clear_forced_playouts()
                if full_per is None:
                    b.clear_playout_cap()
                else:
                    b.set_playout_cap(args.fast, full_per / 65536.0, 1)
                rounds, waiting, pairs = 0, 0, []
                lg.sync(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.gselfplay_begin_episodes(ex, moves, S, 1.0, epn, sample_seed=1)
                w = b.gselfplay_step()
                while w:
                    rounds += 1; waiting += w
                    b.gmcts_leaves(*bufs)
                    p, v = net.predict_batch()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    w = b.gselfplay_step(p, v, device=True)
                    e1.record(stream)
                    pairs.append((e0, e1))
                _plays, made = b.gselfplay_end(want_plays=False)
                lg.sync(); torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if i:
                    secs.append(dt)
                last = (b.gmcts_stats().sims, rounds, waiting, sum(a.elapsed_time(c) for a, c in pairs), int(sum(made)))
            sims, rounds, waiting, ms, made = last
            total, es = ex.counts()[1], ex.stats()
            eps, est = b.gselfplay_episode_stats()
            closed = int(sum(eps))
            line = {"evaluator": name, "route": route, "lanes": n, "spread": args.spread, "sims_per_full_move": S, "fast_sims": args.fast if full_per is not None else None,
                    "full_per_65536": full_per, "lane_budget": moves, "edges_per_node": epn, "rounds": rounds, "seconds_min": round(min(secs), 3),
                    "seconds_max": round(max(secs), 3), "evaluations": sims, "moves": made, "evaluations_per_move": sims / max(1, made),
                    "evaluations_per_sec_best": sims / min(secs), "evaluations_per_sec_worst": sims / max(secs), "episodes_closed_or_cut": closed,
                    "episodes_per_sec_best": closed / min(secs), "episodes_per_sec_worst": closed / max(secs), "examples": total,
                    "examples_per_sec_best": total / min(secs), "examples_per_sec_worst": total / max(secs), "dropped": es.dropped, "overflowed": es.overflowed,
                    "attacker_wins": est.attacker_wins, "defender_wins": est.defender_wins, "draws": est.draws, "cut": est.cut,
                    "mean_fraction_waiting": waiting / max(1, rounds) / n, "step_ms_per_round": ms / max(1, rounds), "step_ms_total": ms}
            if full_per is not None:
                cs = b.playout_cap_stats()
                line.update({"full_moves": cs.full_moves, "fast_moves": cs.fast_moves})
            if k:
                fs = b.forced_playouts_stats()
                line.update({"k": k, "root_noise": [0.3, 0.25], "forced_sims": fs.forced_sims, "pruned_visits": fs.pruned_visits, "pruned_children": fs.pruned_children,
                             "full_moves": fs.full_moves, "forced_sims_per_full_move_sim": fs.forced_sims / max(1, S * fs.full_moves),
                             "pruned_visits_per_recorded_visit": fs.pruned_visits / max(1, (S - 1) * fs.full_moves - fs.pruned_visits),
                             "children_pruned_per_example": fs.pruned_children / max(1, total)})
            line.update({"moves_per_sec_best": made / min(secs), "moves_per_sec_worst": made / max(secs), "commit": args.commit})
            print(json.dumps(line), flush=True)
            b.close()


if __name__ == "__main__":
    main()
