#!/usr/bin/env python3
"""Guided self-play on one MI355X: the own-pace run (tafl_gselfplay_*) against the host loop it replaces, in one
process: 11x11 Copenhagen from the start position, S simulations per move, `--moves` moves.

  own_pace    gselfplay_begin; { gmcts_leaves; network; gselfplay_step } until nothing waits; gselfplay_end
  lock_step   per move: gmcts_begin; { gmcts_leaves; network; gmcts_step } until nothing waits; gmcts_root_visits to the host; the most
              visited action per game with numpy; tafl_step - existing entry points only

with two evaluators (tools/measure_guided.py): constant priors resident in HBM (what the library costs per round) and a small fp16 conv
network.  Both routes play the most visited move (temp_moves = 0), so they play the same games.  One warm-up and `--runs` timed runs per
line; one JSON line each with min..max seconds, evaluated simulations per second, rounds per move, the mean fraction of the games that
wait per round (the evaluator's batch fill) and the step's device time per round from events on the library's stream (they bracket the
8-byte counter memset, the step kernel and the 8-byte read-back of a round).

`--noise ALPHA EPS` mixes Dirichlet(ALPHA) noise into every root's priors with weight EPS (tafl_root_noise), seed 1:
the own-pace run keys it by its own move numbers, the lock-step loop sets the move number before each search, so both still play the
same games.

`--episodes` measures the run in episodes (tafl_gselfplay_begin_episodes) instead: the lanes start from openings with
terminal nodes in reach - the start position advanced by random plies spread over 0 .. `--spread` (tafl_random_advance, seed 21) - with a
lane budget of `--moves` moves (32 in DESIGN.md), and two routes are timed with each evaluator:

  plain      gselfplay_begin with n_moves = the budget: a lane whose game ends idles until the run is over (the parent's route)
  episodes   gselfplay_begin_episodes with the same budget: a lane whose game ends starts its next game from its opening in place

Both record into an examples object (max_children = S).  Per line also: recorded examples and examples per second, and for the episodes
route the episodes closed and the result counters.  The per-round cost of k_gselfplay_reopen comes from a trace of its own:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/measure_gselfplay.py --episodes --no-conv --runs 1
(the kernel's row of OUT/*_kernel_stats.csv: total time / calls)."""
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
    ap.add_argument("--edges-per-node", type=int, default=256)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-conv", action="store_true", help="only the constant-prior evaluator")
    ap.add_argument("--episodes", action="store_true", help="the run in episodes against the plain run, from openings spread over the game (DESIGN.md section 15)")
    ap.add_argument("--spread", type=int, default=500, help="--episodes: lane g starts from the start position advanced by (7 g) mod SPREAD random plies")
    ap.add_argument("--noise", type=float, nargs=2, metavar=("ALPHA", "EPS"), help="Dirichlet noise at every root (default: off)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from alphazeroforhnefatafl_amd import BatchedGameLogic, abi, boards, rules
    from alphazeroforhnefatafl_amd._lib import lib
    from alphazeroforhnefatafl_amd.abi import TaflPlay
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
                y = self.body(x)                                   # [n, 20, 11, 11]: one logit per (tile, slot) = the action layout
                logits = y.permute(0, 2, 3, 1).reshape(n, A).float()
                p = torch.softmax(logits, 1).contiguous()
                v = torch.tanh(self.vhead(y.reshape(n, -1))).float().reshape(n).contiguous()
            torch.cuda.synchronize()
            self.keep = (p, v)
            return p.data_ptr(), v.data_ptr()

    class Rounds:
        """rounds, waiting games summed over the rounds, and an event pair per step"""

        def __init__(self):
            self.rounds, self.waiting, self.pairs = 0, 0, []

        def timed(self, step):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            w = step()
            b.record(stream)
            self.pairs.append((a, b))
            return w

        def step_ms(self):
            torch.cuda.synchronize()
            return sum(a.elapsed_time(b) for a, b in self.pairs)

    def noise(b, move_no=0):
        if args.noise:
            b.set_root_noise(args.noise[0], args.noise[1], 1, 0, move_no)
        else:
            b.clear_root_noise()

    def own_pace(b, net, r):
        noise(b)
        b.gselfplay_begin(None, moves, S, 1.0, epn)
        w = b.gselfplay_step()
        while w:
            r.rounds += 1; r.waiting += w
            b.gmcts_leaves(*bufs)
            p, v = net.predict_batch()
            w = r.timed(lambda: b.gselfplay_step(p, v, device=True))
        b.gselfplay_end(want_plays=False)
        return b.gmcts_stats().sims

    m1 = side - 1

    def plays_of(actions):
        """abi.action_decode for a vector of dense actions, as a TaflPlay array"""
        sq, slot = np.divmod(actions.astype(np.int64), 2 * m1)
        r, c = np.divmod(sq, side)
        vert = slot < m1
        disp = np.where(slot < m1 - r, slot + 1, np.where(vert, -(slot - (m1 - r) + 1), np.where(slot < m1 + (m1 - c), slot - m1 + 1, -(slot - m1 - (m1 - c) + 1))))
        out = np.empty((actions.size, 4), np.uint8)
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = r, c, np.where(vert, abi.VERTICAL, abi.HORIZONTAL), disp.astype(np.int8).view(np.uint8)
        return (TaflPlay * actions.size).from_buffer(out)

    def lock_step(b, net, r):
        sims = 0
        for m in range(moves):
            noise(b, m)
            b.gmcts_begin(S, epn)
            w = b.gmcts_step(None, None, 1.0, S)
            while w:
                r.rounds += 1; r.waiting += w
                b.gmcts_leaves(*bufs)
                p, v = net.predict_batch()
                w = r.timed(lambda: b.gmcts_step(p, v, 1.0, S, device=True))
            sims += b.gmcts_stats().sims
            visits = np.frombuffer(b.gmcts_root_visits(), np.uint32).reshape(n, A)       # the read-back per move
            b.do_play(plays_of(visits.argmax(1)), want_effects=True)
        return sims

    def fill(b, net, r, begin):
        """the step loop of a recording run opened by `begin`; returns the evaluated simulations"""
        noise(b)
        begin()
        w = b.gselfplay_step()
        while w:
            r.rounds += 1; r.waiting += w
            b.gmcts_leaves(*bufs)
            p, v = net.predict_batch()
            w = r.timed(lambda: b.gselfplay_step(p, v, device=True))
        b.gselfplay_end(want_plays=False)
        return b.gmcts_stats().sims

    nets = [("constant_priors", Const())] + ([] if args.no_conv else [("torch_conv_fp16", Conv())])
    if args.episodes:
        plies = (C.c_uint32 * n)(*[(7 * g) % args.spread for g in range(n)])
        start = lg.new_batch(n, boards.COPENHAGEN)
        start.random_advance(21, plies, 0)
        openings = start.download()
        over0 = int(np.count_nonzero(np.frombuffer(openings, np.uint8).reshape(n, C.sizeof(abi.TaflState))[:, abi.TaflState.status.offset]))
        start.close()
        ex = lg.new_examples(n, moves, S)
        for name, net in nets:
            for _ in range(3):
                net.predict_batch()
            for route in ("plain", "episodes"):
                b = lg.new_batch(n)
                secs, last = [], None
                for i in range(1 + args.runs):
                    b.upload(openings)
                    ex.clear()
                    bt.zero_(); st.zero_(); wt.zero_()
                    r = Rounds()
                    begin = (lambda: b.gselfplay_begin(ex, moves, S, 1.0, epn, sample_seed=1)) if route == "plain" else \
                            (lambda: b.gselfplay_begin_episodes(ex, moves, S, 1.0, epn, sample_seed=1))
                    lg.sync(); torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sims = fill(b, net, r, begin)
                    lg.sync(); torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if i:
                        secs.append(dt)
                    last = (sims, r, r.step_ms())
                sims, r, ms = last
                total = ex.counts()[1]
                es = ex.stats()
                line = {"evaluator": name, "route": route, "lanes": n, "lanes_over_at_the_start": over0, "spread": args.spread, "sims_per_move": S, "lane_budget": moves,
                        "edges_per_node": epn, "noise": args.noise, "seconds_min": round(min(secs), 3), "seconds_max": round(max(secs), 3), "sims": sims,
                        "sims_per_sec_best": sims / min(secs), "sims_per_sec_worst": sims / max(secs), "examples": total,
                        "examples_per_sec_best": total / min(secs), "examples_per_sec_worst": total / max(secs), "dropped": es.dropped, "overflowed": es.overflowed,
                        "rounds": r.rounds, "mean_fraction_waiting": r.waiting / max(1, r.rounds) / n, "step_ms_per_round": ms / max(1, r.rounds), "step_ms_total": ms}
                if route == "episodes":
                    eps, est = b.gselfplay_episode_stats()
                    line.update({"episodes_closed_or_cut": int(sum(eps)), "attacker_wins": est.attacker_wins, "defender_wins": est.defender_wins, "draws": est.draws, "cut": est.cut})
                print(json.dumps(line), flush=True)
                b.close()
        return
    final = {}
    for name, net in nets:
        for _ in range(3):
            net.predict_batch()                                  # MIOpen / hipBLASLt kernel selection happens on the first calls
        for route, fn in (("own_pace", own_pace), ("lock_step", lock_step)):
            b = lg.new_batch(n, boards.COPENHAGEN)
            secs, last = [], None
            for i in range(1 + args.runs):                       # (the first run allocates the arena and is not reported)
                b.reset_fen(boards.COPENHAGEN, rules.COPENHAGEN.starting_side)
                bt.zero_(); st.zero_(); wt.zero_()
                r = Rounds()
                lg.sync(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                sims = fn(b, net, r)
                lg.sync(); torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if i:
                    secs.append(dt)
                last = (sims, r, r.step_ms())
            sims, r, ms = last
            final[(name, route)] = bytes(b.download())
            print(json.dumps({"evaluator": name, "route": route, "games": n, "sims_per_move": S, "moves": moves, "edges_per_node": epn, "noise": args.noise,
                              "seconds_min": round(min(secs), 3), "seconds_max": round(max(secs), 3), "sims": sims,
                              "sims_per_sec_best": sims / min(secs), "sims_per_sec_worst": sims / max(secs),
                              "rounds": r.rounds, "rounds_per_move": r.rounds / moves, "mean_fraction_waiting": r.waiting / max(1, r.rounds) / n,
                              "step_ms_per_round": ms / max(1, r.rounds), "step_ms_total": ms}), flush=True)
            b.close()
        print(json.dumps({"evaluator": name, "same_final_states": final[(name, "own_pace")] == final[(name, "lock_step")]}), flush=True)


if __name__ == "__main__":
    main()
